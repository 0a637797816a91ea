"""References of the distribution box head (integral decode, box loss, quality, DFL; DESIGN.md 5k, include/mxdet.h).
No tests here.

  * float64 torch autograd written from the definition: torch.softmax, F.cross_entropy, the corner form of
    tests/test_iou_loss_cases_cpu.py's iou_loss64 (absolute coordinates, torch.maximum / torch.minimum); the quality q and
    the DFL target y are DETACHED. Nothing from include/mxdet_math.h. `mistake` names one deliberate error, for the
    sensitivity test only.
  * a numpy float32 restatement in the kernel's operation order (oracle.expf / oracle.logf, centre-relative corners, the
    gradient by hand): a CPU stand-in that measures the float32 error and builds exact detection cases, never a reference.
"""
import numpy as np

import _quality_loss_ref as Q
import test_iou_loss_cases_cpu as T

KINDS = T.KINDS
CLS_KINDS = ("focal", "qfl", "vfl")
EPS = 0.1                                    # the published epsilon of the DFL target's upper clamp


def O():
    return T.O()


# ---------------------------------------------------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------------------------------------------------
def iou_corners64(p, g, kind):
    """(L, inter / union) [n] float64 tensors of predicted corners p [n,4] against ground truth g [n,4]: iou_loss64 without
    its decode ("+1" lengths, centre 0.5 (p1 + p2))."""
    import torch
    zero = torch.zeros((), dtype=torch.float64)
    il, cl, gl, pl, e2 = [], [], [], [], 0.0
    for k in (0, 1):
        p1, p2, g1, g2 = p[:, k], p[:, 2 + k], g[:, k], g[:, 2 + k]
        il.append(torch.maximum(torch.minimum(p2, g2) - torch.maximum(p1, g1) + 1.0, zero))
        cl.append(torch.maximum(p2, g2) - torch.minimum(p1, g1) + 1.0)
        gl.append(g2 - g1 + 1.0)
        pl.append(p2 - p1 + 1.0)
        e2 = e2 + (0.5 * (p1 + p2) - (g1 + 0.5 * (gl[k] - 1.0))) ** 2
    inter = il[0] * il[1]
    union = pl[0] * pl[1] + gl[0] * gl[1] - inter
    L = 1.0 - inter / union
    if kind == "giou":
        L = L + (cl[0] * cl[1] - union) / (cl[0] * cl[1])
    elif kind == "diou":
        L = L + e2 / (cl[0] ** 2 + cl[1] ** 2)
    else:
        assert kind == "iou"
    return L, inter / union


def centres64(b):
    return 0.5 * (b[:, 0] + b[:, 2]), 0.5 * (b[:, 1] + b[:, 3])


def decode64(b, x, R, s):
    """(corners [n,4], E [n,4]) float64 tensors: the integral decode of logits x [n,4,R+1] at boxes b."""
    import torch
    k = torch.arange(R + 1, dtype=torch.float64)
    E = (torch.softmax(x, dim=-1) * k).sum(-1)
    cx, cy = centres64(b)
    return torch.stack([cx - s * E[:, 0], cy - s * E[:, 1], cx + s * E[:, 2], cy + s * E[:, 3]], dim=1), E


def targets64(b, g, R, s, mistake=None):
    """y [n,4] float64 tensor (no gradient): clamp(dist / s, 0, R - eps)."""
    import torch
    cx, cy = centres64(b)
    dist = torch.stack([cx - g[:, 0], cy - g[:, 1], g[:, 2] - cx, g[:, 3] - cy], dim=1)
    y = dist if mistake == "stride" else dist / s
    return torch.clamp(y, 0.0, R - (0.01 if mistake == "eps" else EPS)).detach()


def rows64(b, g, x, R, s, kind, mistake=None):
    """Unweighted per-row terms as float64 tensors: L [n], DFL [n] (the mean of the four sides), q [n] (detached)."""
    import torch
    import torch.nn.functional as F
    n = x.shape[0]
    p, _ = decode64(b, x, R, s)
    L, q = iou_corners64(p, g, kind)
    y = targets64(b, g, R, s, mistake)
    yl = torch.floor(y)
    flat = x.reshape(n * 4, R + 1)
    ce_l = F.cross_entropy(flat, yl.reshape(-1).long(), reduction="none").reshape(n, 4)
    ce_r = F.cross_entropy(flat, yl.reshape(-1).long() + 1, reduction="none").reshape(n, 4)
    dfl = ((yl + 1.0 - y) * ce_l + (y - yl) * ce_r).sum(1) * (1.0 if mistake == "quarter" else 0.25)
    return L, dfl, (q if mistake == "q_attached" else q.detach())


def ref_rows(b, g, x, R, s, kind, reg_weight, dfl_weight, mistake=None):
    """mxdet_box_dist_loss in float64: x [n,4(R+1)] -> loss_box [n], loss_dfl [n], quality [n], grad [n,4(R+1)] (numpy)."""
    n = np.shape(x)[0]
    xx = T._t64(np.asarray(x, np.float64).reshape(n, 4, R + 1), True)
    L, dfl, q = rows64(T._t64(b), T._t64(g), xx, R, float(s), kind, mistake)
    lb, ld = reg_weight * L, dfl_weight * dfl
    (lb.sum() + ld.sum()).backward()
    return lb.detach().numpy(), ld.detach().numpy(), q.detach().numpy(), xx.grad.numpy().reshape(n, 4 * (R + 1))


def level_positives(A, cls_labels, matched, G, level_offset, n_lvl):
    lab = np.asarray(cls_labels)[:, level_offset:level_offset + n_lvl]
    m = np.asarray(matched)[:, level_offset:level_offset + n_lvl]
    n_i, a_i = np.nonzero((lab > 0) & (m >= 0) & (m < G))
    return lab, m, n_i, a_i


def ref_level(cls, reg, A, Cc, cls_labels, anchors, matched, gt_boxes, level_offset, cls_loss, alpha, gamma, kind, R, s,
              reg_weight, dfl_weight, num_fg, loss_scale, mistake=None):
    """mxdet_retina_loss_level_dfl in float64: loss [3] (class, box, DFL), grad_cls, grad_reg (zeros in the padding), q
    [N,n_lvl], the per-anchor terms before normalisation, unit = loss_scale / max(1, num_fg)."""
    import torch
    from test_loss_cases_cpu import _focal_terms
    N, H, W, ldr = reg.shape
    n_lvl, nb, G = H * W * A, R + 1, np.shape(gt_boxes)[1]
    lab, m, n_i, a_i = level_positives(A, cls_labels, matched, G, level_offset, n_lvl)
    inv = 1.0 / max(1, int(num_fg))
    xr = T._t64(np.asarray(reg, np.float64)[..., :4 * nb * A].reshape(N, n_lvl, 4, nb), True)
    z = T._t64(np.asarray(cls, np.float64)[..., :A * Cc].reshape(N, n_lvl, Cc), True)
    q = torch.zeros((N, n_lvl), dtype=torch.float64)
    per_box, per_dfl = np.zeros((N, n_lvl)), np.zeros((N, n_lvl))
    lb = ld = torch.zeros((), dtype=torch.float64)
    if len(n_i):
        ni, ai = torch.from_numpy(n_i), torch.from_numpy(a_i)
        L, dfl, qq = rows64(T._t64(np.asarray(anchors)[level_offset + a_i]), T._t64(np.asarray(gt_boxes)[n_i, m[n_i, a_i], :4]),
                            xr[ni, ai], R, float(s), kind, mistake)
        q = q.index_put((ni, ai), qq)
        per_box[n_i, a_i], per_dfl[n_i, a_i] = reg_weight * L.detach().numpy(), dfl_weight * dfl.detach().numpy()
        lb, ld = reg_weight * L.sum(), dfl_weight * dfl.sum()
    labt = torch.from_numpy(lab.astype(np.int64))
    if cls_loss == "focal":
        lc = _focal_terms(z, labt, Cc, alpha, gamma)
        per_cls = None
    else:
        onehot = (labt[..., None] == torch.arange(1, Cc + 1)).to(torch.float64)
        y = onehot * q[..., None]
        valid = (labt >= 0).to(torch.float64)[..., None]
        if mistake != "q_attached":
            assert not y.requires_grad
            elems = Q.cls_elems64(z, y, cls_loss, alpha, gamma) * valid
        else:                                                      # cls_elems64 asserts the detachment: inline its QFL line
            import torch.nn.functional as F
            assert cls_loss == "qfl"
            bce = -y * F.logsigmoid(z) - (1.0 - y) * F.logsigmoid(-z)
            elems = (y - torch.sigmoid(z)).abs().pow(gamma) * bce * valid
        per_cls = elems.sum(2).detach().numpy()
        lc = elems.sum()
    ((lc + lb + ld) * inv + 0.0 * (xr.sum() + z.sum())).backward()
    gcls, greg = np.zeros(cls.shape), np.zeros(reg.shape)
    gcls[..., :A * Cc] = (z.grad.numpy() * loss_scale).reshape(N, H, W, A * Cc)
    greg[..., :4 * nb * A] = (xr.grad.numpy() * loss_scale).reshape(N, H, W, 4 * nb * A)
    return {"loss": np.array([float(lc.detach()), float(lb.detach()), float(ld.detach())]) * inv, "grad_cls": gcls, "grad_reg": greg,
            "q": q.detach().numpy(),
            "per_box": per_box, "per_dfl": per_dfl, "per_cls": per_cls, "unit": inv * loss_scale, "nfg": len(n_i),
            "n_valid": int((lab >= 0).sum())}


# ---------------------------------------------------------------------------------------------------------------------
# float32 restatement
# ---------------------------------------------------------------------------------------------------------------------
def _u(fn, x):
    u, inv = np.unique(np.asarray(x, np.float32), return_inverse=True)
    return fn(u)[inv].reshape(np.shape(x)).astype(np.float32)


def expect_fp32(x):
    """x [..., R+1] float32 -> (E, m, Z, e) in the order of dist_expect: Z and S from 0, k ascending; E = S / Z."""
    f = np.float32
    x = np.asarray(x, f)
    m = x.max(axis=-1)
    e = _u(O().expf, x - m[..., None])
    Z, S = np.zeros(m.shape, f), np.zeros(m.shape, f)
    for k in range(x.shape[-1]):
        Z = Z + e[..., k]
        S = S + f(k) * e[..., k]
    E = S / Z
    assert E.dtype == f
    return E, m, Z, e


def decode_fp32(b, x, s, im_hw=None):
    """Corners [n,4] float32 of mxdet_retina_detect_dfl: (cx - s E_l, cy - s E_t, cx + s E_r, cy + s E_b), clipped to the
    image when im_hw = (h, w) is given. x [n,4,R+1]."""
    f = np.float32
    b, s = np.asarray(b, f), f(s)
    E = expect_fp32(x)[0]
    cx, cy = f(0.5) * (b[:, 0] + b[:, 2]), f(0.5) * (b[:, 1] + b[:, 3])
    out = np.stack([cx - s * E[:, 0], cy - s * E[:, 1], cx + s * E[:, 2], cy + s * E[:, 3]], axis=1)
    if im_hw is not None:
        mx, my = f(im_hw[1]) - f(1.0), f(im_hw[0]) - f(1.0)
        out[:, 0::2] = np.minimum(np.maximum(out[:, 0::2], f(0.0)), mx)
        out[:, 1::2] = np.minimum(np.maximum(out[:, 1::2], f(0.0)), my)
    assert out.dtype == f
    return out


def _step(a, b):
    return np.where(a > b, 1.0, np.where(a == b, 0.5, 0.0)).astype(np.float32)


def rows_fp32(b, g, x, R, s, kind, reg_weight, dfl_weight, mistake=None):
    """dist_box_quad + box_iou_core for every row, float32: loss_box, loss_dfl, quality [n], grad [n,4(R+1)]."""
    f = np.float32
    n = np.shape(x)[0]
    b, g, s = np.asarray(b, f), np.asarray(g, f), f(s)
    x = np.asarray(x, f).reshape(n, 4, R + 1)
    one, half, zero = f(1.0), f(0.5), f(0.0)
    E, m, Z, e = expect_fp32(x)
    cx, cy = half * (b[:, 0] + b[:, 2]), half * (b[:, 1] + b[:, 3])
    c = (cx, cy)
    g1 = [g[:, k] - c[k] for k in (0, 1)]
    g2 = [g[:, 2 + k] - c[k] for k in (0, 1)]
    p1 = [-(s * E[:, k]) for k in (0, 1)]
    p2 = [s * E[:, 2 + k] for k in (0, 1)]
    pl = [p2[k] - p1[k] + one for k in (0, 1)]
    pc = [half * (p1[k] + p2[k]) for k in (0, 1)]
    gl, il, cl, a1, a2, st = ([None, None] for _ in range(6))
    for k in (0, 1):
        gl[k] = g2[k] - g1[k] + one
        a1[k], a2[k] = _step(p1[k], g1[k]), _step(g2[k], p2[k])
        r = np.minimum(p2[k], g2[k]) - np.maximum(p1[k], g1[k]) + one
        st[k] = _step(r, zero)
        il[k] = np.maximum(r, zero)
        cl[k] = np.maximum(p2[k], g2[k]) - np.minimum(p1[k], g1[k]) + one
    inter = il[0] * il[1]
    uni = pl[0] * pl[1] + gl[0] * gl[1] - inter
    L = one - inter / uni
    q = inter / uni
    iu2 = one / (uni * uni)
    dI, dA = -(uni + inter) * iu2, inter * iu2
    gc, gp = [np.zeros(n, f), np.zeros(n, f)], [np.zeros(n, f), np.zeros(n, f)]
    if kind == "giou":
        Cc = cl[0] * cl[1]
        ic = one / Cc
        L = L + (Cc - uni) * ic
        dI, dA = dI + ic, dA - ic
        dC = uni * ic * ic
        gc = [dC * cl[1], dC * cl[0]]
    elif kind == "diou":
        e0, e1 = pc[0] - half * (g1[0] + g2[0]), pc[1] - half * (g1[1] + g2[1])
        rho, iD = e0 * e0 + e1 * e1, one / (cl[0] * cl[0] + cl[1] * cl[1])
        L = L + rho * iD
        qq = f(-2.0) * rho * iD * iD
        gc = [qq * cl[0], qq * cl[1]]
        gp = [f(2.0) * e0 * iD, f(2.0) * e1 * iD]
    dE, dist = np.zeros((n, 4), f), np.zeros((n, 4), f)
    for k in (0, 1):
        gi = dI * il[1 - k] * st[k]
        d2 = gi * a2[k] + gc[k] * (one - a2[k])
        d1 = -(gi * a1[k] + gc[k] * (one - a1[k]))
        da = dA * pl[1 - k]
        dE[:, k] = -(s * (d1 + half * gp[k] - da))
        dE[:, 2 + k] = s * (d2 + half * gp[k] + da)
        dist[:, k], dist[:, 2 + k] = -g1[k], g2[k]
    ymax = f(R) - f(0.01 if mistake == "eps" else EPS)
    y = dist if mistake == "stride" else dist / s
    y = np.minimum(np.maximum(y, zero), ymax).astype(f)
    yl = y.astype(np.int64)
    ylf = yl.astype(f)
    wl, wr = ylf + one - y, y - ylf
    lse = m + _u(O().logf, Z)
    xl = np.take_along_axis(x, yl[..., None], axis=-1)[..., 0]
    xr = np.take_along_axis(x, yl[..., None] + 1, axis=-1)[..., 0]
    dfl = wl * (lse - xl) + wr * (lse - xr)
    dsum = ((dfl[:, 0] + dfl[:, 1]) + dfl[:, 2]) + dfl[:, 3]
    quarter = one if mistake == "quarter" else f(0.25)
    rw, dw = f(reg_weight), f(dfl_weight)
    ks = np.arange(R + 1)
    p = e / Z[..., None]
    t = np.where(ks == yl[..., None], wl[..., None], zero).astype(f) + np.where(ks == yl[..., None] + 1, wr[..., None], zero).astype(f)
    kE = ks.astype(f) - (zero if mistake == "k_not_k_minus_E" else E[..., None])
    grad = (rw * dE)[..., None] * (p * kE) + (dw * quarter) * (p - t)
    out = (rw * L, dw * quarter * dsum, q, grad.reshape(n, 4 * (R + 1)))
    assert all(a.dtype == f for a in out)
    return out


def level_fp32(reg, A, cls_labels, anchors, matched, gt_boxes, level_offset, kind, R, s, reg_weight, dfl_weight):
    """(per-anchor box loss, per-anchor DFL, q [N,n_lvl]; d / d logits [N,n_lvl,4(R+1)]) float32, before normalisation."""
    N, H, W, _ = reg.shape
    n_lvl, nb = H * W * A, R + 1
    lab, m, n_i, a_i = level_positives(A, cls_labels, matched, np.shape(gt_boxes)[1], level_offset, n_lvl)
    out = [np.zeros((N, n_lvl), np.float32) for _ in range(3)] + [np.zeros((N, n_lvl, 4 * nb), np.float32)]
    if len(n_i):
        x = np.asarray(reg, np.float32)[..., :4 * nb * A].reshape(N, n_lvl, 4 * nb)[n_i, a_i]
        r = rows_fp32(np.asarray(anchors)[level_offset + a_i], np.asarray(gt_boxes)[n_i, m[n_i, a_i], :4], x, R, s, kind,
                      reg_weight, dfl_weight)
        for o, v in zip(out, r):
            o[n_i, a_i] = v
    return out


# ---------------------------------------------------------------------------------------------------------------------
# test-time detection
# ---------------------------------------------------------------------------------------------------------------------
def candidate_anchors(gidx, base, H, W, strides, A, Cn):
    """gidx [R] (global (anchor, class) index, -1 padding) -> (level, cell, anchor, anchor box [R,4] float32 built as the
    kernels build it: base + (float)(x * stride))."""
    offs = np.cumsum([0] + [h * w * A * Cn for h, w in zip(H, W)])
    g = np.maximum(np.asarray(gidx, np.int64), 0)
    lvl = np.searchsorted(offs, g, side="right") - 1
    local = g - offs[lvl]
    cell, a = local // (A * Cn), (local % (A * Cn)) // Cn
    Wl, sl = np.asarray(W)[lvl], np.asarray(strides)[lvl]
    sx, sy = ((cell % Wl) * sl).astype(np.float32), ((cell // Wl) * sl).astype(np.float32)
    bb = np.stack([np.asarray(base[l], np.float32)[ai] for l, ai in zip(lvl, a)])
    box = np.stack([bb[:, 0] + sx, bb[:, 1] + sy, bb[:, 2] + sx, bb[:, 3] + sy], axis=1).astype(np.float32)
    return lvl, cell, a, box


def detect_ref(oracle, cls_logits, dist, base, H, W, strides, im_info, Cn, R, pre_n, score_thresh, nms_thresh, max_det,
               method="hard", sigma=0.5, cap=4096, decode=None):
    """mxdet_retina_detect_dfl composed from the oracle's selection / merge / NMS and the decode of this module.
    cls_logits[l] [N, H*W*A*Cn]; dist[l] [N, H*W, A, 4, R+1] float32. decode: None = decode_fp32 (the kernel's bits), or
    "f64" = the float64 decode (clipped), for the general-logit case. Returns (dets [N,max_det,6], num [N])."""
    import ctypes as C
    import _soft_nms_ref as S
    A = np.shape(base[0])[0]
    N = cls_logits[0].shape[0]
    exp_b = [np.repeat(np.ascontiguousarray(b, np.float32), Cn, axis=0) for b in base]
    zero_d = [np.zeros((N, h * w * A * Cn, 4), np.float32) for h, w in zip(H, W)]
    post = min(len(cls_logits) * pre_n, cap)
    rois, logit, gidx, num = oracle.proposal(cls_logits, zero_d, exp_b, H, W, strides, im_info, pre_n, post, 2.0, 0.0)
    L = oracle.lib()
    L.oracle_sigmoid.restype = C.c_float
    L.oracle_sigmoid.argtypes = [C.c_float]
    prob = np.array([[L.oracle_sigmoid(float(z)) for z in row] for row in logit], np.float32)
    cls = (gidx % Cn + 1).astype(np.int32)
    boxes = np.zeros((N, post, 4), np.float32)
    for n in range(N):
        k = int(num[n])
        cls[n, k:] = 0
        if k == 0:
            continue
        lvl, cell, a, ab = candidate_anchors(gidx[n, :k], base, H, W, strides, A, Cn)
        x = np.stack([dist[l][n, c, ai] for l, c, ai in zip(lvl, cell, a)])
        sl = np.asarray(strides, np.float32)[lvl]
        for s in np.unique(sl):
            pick = np.flatnonzero(sl == s)
            if decode == "f64":
                p = decode64(T._t64(ab[pick]), T._t64(x[pick]), R, float(s))[0].numpy()
                p[:, 0::2] = np.clip(p[:, 0::2], 0.0, float(im_info[n, 1]) - 1.0)
                p[:, 1::2] = np.clip(p[:, 1::2], 0.0, float(im_info[n, 0]) - 1.0)
                boxes[n, pick] = p
            else:
                boxes[n, pick] = decode_fp32(ab[pick], x[pick], s, (im_info[n, 0], im_info[n, 1]))
    if method == "hard":
        return oracle.class_nms_topk(boxes, prob, cls, num, Cn, score_thresh, nms_thresh, max_det) + (boxes, num)
    dets, nd = np.zeros((N, max_det, 6), np.float32), np.zeros((N,), np.int32)
    for n in range(N):
        rows = []
        for c in range(1, Cn + 1):
            cand = np.flatnonzero((cls[n] == c) & (prob[n] > np.float32(score_thresh)))
            sel, ssc = S.soft_nms_list(oracle, boxes[n][cand], prob[n, cand], cand, S.METHODS[method], nms_thresh, sigma,
                                       score_thresh, max_det)
            rows += [(ssc[k], int(cand[j]), c, boxes[n][cand[j]], prob[n, cand[j]]) for k, j in enumerate(sel)]
        dets[n], nd[n], _ = S.merge_image(rows, max_det)
    return dets, nd, boxes, num
