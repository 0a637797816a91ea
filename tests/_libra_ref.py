"""numpy float32 / integer restatements of the Libra R-CNN entries (include/mxdet.h), operation for operation:
the Balanced Feature Pyramid's gather / scatter and their adjoints, the IoU-balanced sampler on oracle.box_iou / oracle.encode
/ the oracle's sample key, and Balanced L1 on oracle.logf with the box-head loss entry's reduction order. bf16 tensors are
float32 arrays holding bf16 values."""
import math

import numpy as np

from oracle import oracle

F = np.float32


# ---- Balanced Feature Pyramid ---------------------------------------------------------------------
def pool_window(o, n_in, n_out):
    """[lo, hi) of adaptive-pool output o along an axis."""
    return (o * n_in) // n_out, -((-(o + 1) * n_in) // n_out)


def nearest_src(n_out, n_in):
    return (np.arange(n_out) * n_in) // n_out


def adaptive_max_pool(x, oh, ow):
    """x [N,H,W,C] -> (max [N,oh,ow,C], (ay, ax) [N,oh,ow,C] the arg-maximum's position; ties: first in row-major order)."""
    N, H, W, C = x.shape
    out = np.zeros((N, oh, ow, C), F)
    ay = np.zeros((N, oh, ow, C), np.int64)
    ax = np.zeros((N, oh, ow, C), np.int64)
    for oy in range(oh):
        y0, y1 = pool_window(oy, H, oh)
        for ox in range(ow):
            x0, x1 = pool_window(ox, W, ow)
            win = x[:, y0:y1, x0:x1, :].reshape(N, -1, C)
            a = np.argmax(win, axis=1)                      # first maximum
            out[:, oy, ox, :] = np.take_along_axis(win, a[:, None, :], 1)[:, 0, :]
            ay[:, oy, ox, :] = y0 + a // (x1 - x0)
            ax[:, oy, ox, :] = x0 + a % (x1 - x0)
    return out, (ay, ax)


def nearest_resize(x, oh, ow):
    return x[:, nearest_src(oh, x.shape[1])][:, :, nearest_src(ow, x.shape[2])]


def gather_fwd(P, r):
    """B = bf16((((g_0 + g_1) + ...) + g_{L-1}) / L); returns (B, args) with args[l] the pool arg-maxima of level l < r."""
    h, w = P[r].shape[1:3]
    acc, args = None, {}
    for l, p in enumerate(P):
        if l < r:
            g, args[l] = adaptive_max_pool(p, h, w)
        elif l == r:
            g = p
        else:
            g = nearest_resize(p, h, w)
        acc = g.astype(F) if acc is None else (acc + g).astype(F)
    return oracle.round_bf16(acc / F(len(P))), args


def scatter_fwd(P, Rf, r):
    """Q_l = bf16(P_l + s_l); returns (Q, args) with args[l] the pool arg-maxima of level l > r."""
    Q, args = [], {}
    for l, p in enumerate(P):
        H, W = p.shape[1:3]
        if l < r:
            s = nearest_resize(Rf, H, W)
        elif l == r:
            s = Rf
        else:
            s, args[l] = adaptive_max_pool(Rf, H, W)
        Q.append(oracle.round_bf16((p + s).astype(F)))
    return Q, args


def _add_at_argmax(acc, arg, oy, ox, term):
    ay, ax = arg
    n, c = np.meshgrid(np.arange(acc.shape[0]), np.arange(acc.shape[3]), indexing="ij")
    acc[n, ay[:, oy, ox, :], ax[:, oy, ox, :], c] += term           # one target per (n, c): no repeated index


def scatter_bwd(dQ, r, args):
    """dRf = bf16(sum_l adj(s_l)(dQ_l)): one fp32 sum, levels in order, contributing pixels in row-major order."""
    N, h, w, C = dQ[r].shape
    acc = np.zeros((N, h, w, C), F)
    for l, d in enumerate(dQ):
        H, W = d.shape[1:3]
        if l == r:
            acc += d
            continue
        sy, sx = nearest_src(H, h), nearest_src(W, w)
        for Y in range(H):
            for X in range(W):
                if l < r:
                    acc[:, sy[Y], sx[X], :] += d[:, Y, X, :]
                else:
                    _add_at_argmax(acc, args[l], Y, X, d[:, Y, X, :])
    return oracle.round_bf16(acc)


def gather_bwd(dQ, dB, r, args):
    """dP_l = bf16(dQ_l + adj(g_l)(dB / L)): terms divided first, summed in row-major order of the contributing cells."""
    L = F(len(dQ))
    N, h, w, C = dB.shape
    out = []
    for l, d in enumerate(dQ):
        H, W = d.shape[1:3]
        acc = np.zeros(d.shape, F)
        if l == r:
            acc += (dB / L).astype(F)
        else:
            sy, sx = nearest_src(h, H), nearest_src(w, W)
            for oy in range(h):
                for ox in range(w):
                    term = (dB[:, oy, ox, :] / L).astype(F)
                    if l < r:
                        _add_at_argmax(acc, args[l], oy, ox, term)
                    else:
                        acc[:, sy[oy], sx[ox], :] += term
        out.append(oracle.round_bf16((d + acc).astype(F)))
    return out


# ---- IoU-balanced sampler -------------------------------------------------------------------------
def bin_edges(bg_lo, bg_hi, K):
    """e_j = bg_lo + (bg_hi - bg_lo) * (j / K), j = 1..K-1, one fp32 operation each."""
    span = F(bg_hi) - F(bg_lo)
    return [F(F(bg_lo) + F(span * F(F(j) / F(K)))) for j in range(1, K)]


def proposal_target_balanced(rois, num_rois, gt, R, fg_fraction, fg_thresh, bg_hi, bg_lo, num_classes, stds, seed, step,
                             image_offset, num_bins, stats=None):
    """mxdet_proposal_target_balanced (class-specific targets, means 0). stats (a list): one dict per image with the bins'
    candidate counts, what each gave and the top-up."""
    rois, gt = np.asarray(rois, F), np.asarray(gt, F)
    N, S = rois.shape[:2]
    D = 4 * num_classes
    o_rois, o_lab = np.zeros((N, R, 5), F), np.full((N, R), -1, np.int32)
    o_tgt, o_wgt = np.zeros((N, R, D), F), np.zeros((N, R, D), F)
    o_m, o_nfg = np.full((N, R), -1, np.int32), np.zeros((N,), np.int32)
    max_fg = int(F(fg_fraction) * F(R))
    edges = bin_edges(bg_lo, bg_hi, num_bins)
    for n in range(N):
        o_rois[n, :, 0] = n
        nr = min(max(int(num_rois[n]), 0), S)
        valid = [g for g in range(gt.shape[1]) if gt[n, g, 4] >= 0]
        boxes = np.concatenate([rois[n, :nr, 1:5], gt[n, valid, :4]], 0).reshape(-1, 4)
        nc = boxes.shape[0]
        if valid:
            iou = oracle.box_iou(boxes, gt[n, valid, :4])
            best, bi = iou.max(1), np.array(valid)[iou.argmax(1)]          # argmax: the first maximum
        else:
            best, bi = np.zeros((nc,), F), np.full((nc,), -1)
        fg = [i for i in range(nc) if best[i] >= F(fg_thresh) and bi[i] >= 0]
        bg = [i for i in range(nc) if i not in set(fg) and F(bg_lo) <= best[i] < F(bg_hi)]
        image = image_offset + n
        key = lambda stream: (lambda i: (oracle.sample_key(seed, step, image, stream, i), i))  # noqa: E731
        fg_sel = sorted(sorted(fg, key=key(2))[:max_fg])
        nfg = len(fg_sel)
        want = max(R - nfg, 0)
        per = want // num_bins
        bins = [[] for _ in range(num_bins)]
        for i in bg:
            bins[sum(1 for e in edges if best[i] >= e)].append(i)
        chosen, gave = [], []
        for b in bins:
            take = sorted(b, key=key(3))[:per]
            gave.append(len(take))
            chosen += take
        rest = sorted([i for i in bg if i not in set(chosen)], key=key(3))[:want - len(chosen)]
        if stats is not None:
            stats.append(dict(nfg=nfg, want=want, per=per, counts=[len(b) for b in bins], gave=gave, top_up=len(rest),
                              edges=edges, best=best))
        bg_sel = sorted(chosen + rest)
        o_nfg[n] = nfg
        for s, i in enumerate(fg_sel + bg_sel):
            o_rois[n, s, 1:] = boxes[i]
            o_m[n, s] = bi[i]
            if s < nfg:
                g = gt[n, bi[i]]
                cls = int(g[4])
                o_lab[n, s] = cls
                t = oracle.encode(boxes[i], g[:4])
                o_tgt[n, s, 4 * cls:4 * cls + 4] = (t - F(0)) / np.asarray(stds, F)
                o_wgt[n, s, 4 * cls:4 * cls + 4] = 1
            else:
                o_lab[n, s] = 0
    return o_rois, o_lab, o_tgt, o_wgt, o_m, o_nfg


def sampler_inputs(seed=0, S=300, G=4, N=2, jitter=0.6, num_rois=None):
    """Proposals scattered around the ground truth of conftest.synth_gt images (400 x 600): each is a ground-truth box moved and
    resized by up to `jitter` of its size, so the IoUs spread over [0, 1]. Returns (rois [N,S,5], num_rois [N], gt [N,G,5])."""
    from conftest import synth_gt
    rng = np.random.default_rng(seed)
    gt = synth_gt(rng, N, G, 400, 600, g_lo=2, g_hi=G)
    rois = np.zeros((N, S, 5), F)
    for n in range(N):
        valid = gt[n][gt[n, :, 4] >= 0]
        base = valid[rng.integers(0, len(valid), S), :4]
        size = np.stack([base[:, 2] - base[:, 0], base[:, 3] - base[:, 1]] * 2, 1)
        rois[n, :, 1:] = base + rng.uniform(-jitter, jitter, (S, 4)).astype(F) * size
        rois[n, :, 3:] = np.maximum(rois[n, :, 3:], rois[n, :, 1:3] + 1)
        rois[n, :, 0] = n
    num = np.array([S, S - 17] * N, np.int32)[:N] if num_rois is None else np.asarray(num_rois, np.int32)
    return rois, num, gt


# ---- Balanced L1 ------------------------------------------------------------------------------------
def bl1_b(alpha, gamma):
    return F(math.exp(float(gamma) / float(alpha)) - 1.0)


def _bl1_log(a, beta, b):
    t = F(b * a)
    t = F(t / beta)
    t = F(t + F(1))
    return oracle.logf(t)


def balanced_l1(d, alpha, gamma, beta, b):
    """(L, dL/dd) of float32 differences d, in the kernel's operation order."""
    d = np.asarray(d, F)
    alpha, gamma, beta, b = F(alpha), F(gamma), F(beta), F(b)
    a = np.abs(d)
    inner = a < beta
    lg = _bl1_log(np.where(inner, a, F(0)), beta, b)
    p = F(F(b * a) + F(1))
    q = F(F(F(alpha / b) * p) * lg)
    L_in = F(q - F(alpha * a))
    L_out = F(F(F(gamma * a) + F(gamma / b)) - F(alpha * beta))
    m = np.where(inner, F(alpha * lg), gamma).astype(F)
    g = np.where(d > 0, m, np.where(d < 0, -m, F(0))).astype(F)
    return np.where(inner, L_in, L_out).astype(F), g


def _xor_tree(v):
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[lane ^ off]).astype(F)
    return v[0]


def _down_tree(v):
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        src = np.where(lane + off < 64, v[np.minimum(lane + off, 63)], v)
        v = (v + src).astype(F)
    return v[0]


def finalize(partial):
    """finalize_kernel on one component: 256 threads stride the partials, fixed tree per wave, waves in order."""
    acc = np.zeros((256,), F)
    for i, p in enumerate(partial):
        acc[i % 256] = F(acc[i % 256] + F(p))
    s = F(0)
    for wv in range(4):
        s = F(s + _down_tree(acc[64 * wv:64 * wv + 64]))
    return s


def rcnn_reg_balanced(pred, labels, tgt, wgt, alpha, gamma, beta, b, reg_weight, norm, loss_scale, bf16=False):
    """The regression half of mxdet_rcnn_loss_balanced: (loss_out[1], grad_reg [R,reg_dim] float32 -- bf16 values if bf16)."""
    pred, tgt, wgt = np.asarray(pred, F), np.asarray(tgt, F), np.asarray(wgt, F)
    R, D = tgt.shape
    assert D <= 64
    on = (wgt != 0) & (np.asarray(labels)[:, None] > 0)
    d = ((pred - tgt).astype(F) * wgt).astype(F)
    L, g = balanced_l1(d, alpha, gamma, beta, b)
    rw, norm, ls = F(reg_weight), F(norm), F(loss_scale)
    grad = np.where(on, F(F(F(F(g * rw) * wgt) * norm) * ls), F(0)).astype(F)
    if bf16:
        grad = oracle.round_bf16(grad)
    partial = []
    for r in range(R):
        lanes = np.zeros((64,), F)
        lanes[:D] = np.where(on[r], L[r], F(0))
        partial.append(F(F(rw * _xor_tree(lanes)) * norm))
    return finalize(partial), grad
