"""Libra R-CNN without a GPU: the references of tests/_libra_ref.py pinned against float64 torch (Balanced Feature Pyramid),
the C oracle (sampler with one bin) and hand-computed answers; Balanced L1's continuity, gradient and constant; option
validation in the model / builder / config; the entries' host argument checks."""
import ctypes as C
import glob
import math
import os

import numpy as np
import pytest

import _libra_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PYRAMIDS = {"exact": [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)], "overlap": [(25, 34), (13, 17), (7, 9), (4, 5), (2, 3)]}
BF16_VALUES = np.array([-2.0, -0.75, -0.5, 0.0, 0.25, 0.5, 1.0, 1.5, 3.0], np.float32)      # few values: ties inside windows


def _pyramid(rng, sizes, N=2, C=8):
    return [rng.choice(BF16_VALUES, (N, h, w, C)).astype(np.float32) for h, w in sizes]


def _t64(x, grad=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).double().requires_grad_(grad)


def _np(t):
    return t.detach().numpy().transpose(0, 2, 3, 1)


def _gather64(P, r):
    import torch.nn.functional as Fn
    hw = tuple(P[r].shape[2:])
    g = [Fn.adaptive_max_pool2d(p, hw) if l < r else (p if l == r else Fn.interpolate(p, size=hw, mode="nearest"))
         for l, p in enumerate(P)]
    return sum(g) / len(P)


def _scatter64(P, Rf, r):
    import torch.nn.functional as Fn
    out = []
    for l, p in enumerate(P):
        hw = tuple(p.shape[2:])
        s = Fn.interpolate(Rf, size=hw, mode="nearest") if l < r else (Rf if l == r else Fn.adaptive_max_pool2d(Rf, hw))
        out.append(p + s)
    return out


# One bf16 rounding of an exact value v: |bf16(v) - v| <= 2^-8 |v| (8 significand bits, round to nearest: half an ulp). The references sum in
# fp32 first: n terms t_i (each possibly a rounded quotient) accumulate an error of at most n * 2^-24 * sum|t_i| =: e32, and
# the bf16 rounding then acts on a value within e32 of v. So |ref - v| <= 2^-8 (|v| + e32) + e32. The forward sums L = 5 terms,
# a backward element at most 25 (a 5 x 5 block of fine pixels, or 5 x 5 overlapping windows), plus the gradient it is added to.
def _bound(v, sum_abs, n):
    e32 = n * 2.0 ** -24 * sum_abs
    return 2.0 ** -8 * (np.abs(v) + e32) + e32


@pytest.mark.parametrize("name,r", [("exact", 2), ("overlap", 2), ("overlap", 0), ("overlap", 4)])
def test_bfp_reference_against_float64_torch(name, r):
    import torch
    rng = np.random.default_rng(3)
    P = _pyramid(rng, PYRAMIDS[name])
    L = len(P)
    # ---- forward ----
    B, args_g = ref.gather_fwd(P, r)
    P64 = [_t64(p, True) for p in P]
    B64 = _gather64(P64, r)
    sum_abs = _np(_gather64([_t64(np.abs(p)) for p in P], r)) * L        # max|x| >= |max x|: an upper bound on sum_l |g_l|
    assert np.all(np.abs(B - _np(B64)) <= _bound(_np(B64), sum_abs, L + 1))
    Rf = oracle_round(rng.normal(size=B.shape).astype(np.float32))
    Q, args_s = ref.scatter_fwd(P, Rf, r)
    Rf64 = _t64(Rf, True)
    Q64 = _scatter64(P64, Rf64, r)
    mass = _scatter64([_t64(np.abs(p)) for p in P], _t64(np.abs(Rf)), r)
    for q, q64, m_ in zip(Q, Q64, mass):
        assert np.all(np.abs(q - _np(q64)) <= _bound(_np(q64), _np(m_), 2))
    # ---- backward, stage by stage (each stage rounds once) ----
    dQ = [oracle_round(rng.normal(size=p.shape).astype(np.float32)) for p in P]
    dRf = ref.scatter_bwd(dQ, r, args_s)
    want, = torch.autograd.grad(Q64, Rf64, [_t64(d) for d in dQ], retain_graph=True)
    mass, = torch.autograd.grad(Q64, Rf64, [_t64(np.abs(d)) for d in dQ])          # the adjoint has coefficients 0 / 1
    assert np.all(np.abs(dRf - _np(want)) <= _bound(_np(want), _np(mass), 25 * L))
    dB = oracle_round(rng.normal(size=B.shape).astype(np.float32))
    dP = ref.gather_bwd(dQ, dB, r, args_g)
    want = torch.autograd.grad(B64, P64, _t64(dB), retain_graph=True)
    mass = torch.autograd.grad(B64, P64, _t64(np.abs(dB)))
    for d, q, w_, m_ in zip(dP, dQ, want, mass):
        v = q.astype(np.float64) + _np(w_)
        assert np.all(np.abs(d - v) <= _bound(v, np.abs(q) + _np(m_), 26))
    # ties occurred, and in the overlapping pyramid a window shares pixels with its neighbour
    if name == "overlap":
        assert ref.pool_window(0, 25, 7)[1] > ref.pool_window(1, 25, 7)[0]


def oracle_round(x):
    from oracle import oracle
    return oracle.round_bf16(x)


def test_bfp_tie_inside_an_overlapping_window_by_hand():
    """1-D in spirit: a 1 x 5 map pooled to 1 x 3. Windows [0,2), [1,4), [3,5): pixel 1 lies in windows 0 and 1. With the
    values (1, 3, 3, 0, 2) window 0 takes pixel 1, window 1 ties between pixels 1 and 2 and takes the FIRST (pixel 1), window 2
    takes pixel 4. So the adjoint sends dy0 + dy1 to pixel 1 and nothing to pixel 2."""
    assert [ref.pool_window(o, 5, 3) for o in range(3)] == [(0, 2), (1, 4), (3, 5)]
    x = np.array([1, 3, 3, 0, 2], np.float32).reshape(1, 1, 5, 1)
    out, (ay, ax) = ref.adaptive_max_pool(x, 1, 3)
    assert out.ravel().tolist() == [3, 3, 2] and ax.ravel().tolist() == [1, 1, 4] and ay.ravel().tolist() == [0, 0, 0]
    # as a two-level pyramid refined at the coarse level (r = 1): B = (pool(P0) + P1) / 2; dP0 = dQ0 + adj(dB / 2)
    P = [x, np.array([1, -1, 0], np.float32).reshape(1, 1, 3, 1)]
    B, args = ref.gather_fwd(P, 1)
    assert B.ravel().tolist() == [2.0, 1.0, 1.0]
    dQ = [np.zeros_like(P[0]), np.zeros_like(P[1])]
    dB = np.array([2, 4, 8], np.float32).reshape(1, 1, 3, 1)
    dP = ref.gather_bwd(dQ, dB, 1, args)
    assert dP[0].ravel().tolist() == [0, 3, 0, 0, 4] and dP[1].ravel().tolist() == [1, 2, 4]
    # ... and the scatter at r = 0 of the same map: Q1 = P1 + pool(Rf); dRf collects dQ1 at the arg-maxima
    Q, args_s = ref.scatter_fwd([np.zeros_like(x), np.zeros((1, 1, 3, 1), np.float32)], x, 0)
    assert Q[1].ravel().tolist() == [3, 3, 2] and Q[0].ravel().tolist() == [1, 3, 3, 0, 2]
    dRf = ref.scatter_bwd([np.zeros_like(x), dB], 0, args_s)
    assert dRf.ravel().tolist() == [0, 6, 0, 0, 8]


def test_index_rules_are_torchs_on_both_pyramids():
    import torch
    import torch.nn.functional as Fn
    for sizes in PYRAMIDS.values():
        for a in sizes:
            for b in sizes:
                x = torch.arange(a[0] * a[1], dtype=torch.float64).reshape(1, 1, *a)
                want = Fn.interpolate(x, size=b, mode="nearest")[0, 0].numpy()
                got = ref.nearest_resize(x.numpy().transpose(0, 2, 3, 1), *b)[0, :, :, 0]
                assert np.array_equal(got, want), (a, b)
                if a[0] >= b[0] and a[1] >= b[1]:
                    _, idx = Fn.adaptive_max_pool2d(-x, b, return_indices=True)       # -x: the window's first element wins
                    lo = np.array([[ref.pool_window(oy, a[0], b[0])[0] * a[1] + ref.pool_window(ox, a[1], b[1])[0]
                                    for ox in range(b[1])] for oy in range(b[0])])
                    assert np.array_equal(idx[0, 0].numpy(), lo), (a, b)


# ---- sampler ----------------------------------------------------------------------------------------
KW = dict(R=64, fg_fraction=0.25, fg_thresh=0.5, bg_hi=0.5, bg_lo=0.0, num_classes=81, stds=(0.1, 0.1, 0.2, 0.2))


def test_sampler_reference_with_one_bin_is_the_oracle(oracle):
    rois, num, gt = ref.sampler_inputs()
    for step in (0, 5):
        got = ref.proposal_target_balanced(rois, num, gt, seed=3, step=step, image_offset=2, num_bins=1, **KW)
        want = oracle.proposal_target(rois, num, gt, R=64, seed=3, step=step, image_offset=2)
        for g, w_, name in zip(got, want, ("rois", "labels", "tgt", "wgt", "matched", "nfg")):
            assert np.array_equal(g, w_), name


def test_bin_edges_and_membership():
    e = ref.bin_edges(0.0, 0.5, 3)
    assert [float(v) for v in e] == [float(np.float32(0.5) * (np.float32(1) / np.float32(3))),
                                    float(np.float32(0.5) * (np.float32(2) / np.float32(3)))]
    assert ref.bin_edges(0.0, 0.5, 1) == [] and ref.bin_edges(0.1, 0.5, 2)[0] == np.float32(0.1) + np.float32(0.4) * np.float32(0.5)


def test_quota_and_top_up_arithmetic_by_hand(oracle):
    """One ground truth (0,0,99,99) and hand-placed proposals (x1,0,x1+99,99): IoU = (100 - x1) / (100 + x1). R = 8 and no
    foreground quota (fg_fraction 0): want = 8, three bins with edges 1/6 and 1/3, per = 2. Bin 2 holds one candidate, bin 1
    none, bin 0 eight: the bins give 2 + 0 + 1, the top-up takes 5 more of bin 0's remaining six, by key."""
    xs = [100, 101, 102, 103, 104, 105, 106, 107, 45]        # IoU 0 (eight times, disjoint) and 55 / 145 = 0.379 > 1/3
    rois = np.array([[[0, x, 0, x + 99, 99] for x in xs]], np.float32)
    gt = np.array([[[0, 0, 99, 99, 7]]], np.float32)
    stats = []
    kw = dict(KW, R=8, fg_fraction=0.0)
    out = ref.proposal_target_balanced(rois, [9], gt, seed=1, step=0, image_offset=0, num_bins=3, stats=stats, **kw)
    s = stats[0]
    assert (s["nfg"], s["want"], s["per"]) == (0, 8, 2) and s["counts"] == [8, 0, 1] and s["gave"] == [2, 0, 1]
    assert s["top_up"] == 5
    labels = out[1][0]
    assert (labels == 0).all() and out[5][0] == 0
    # eight of the nine proposals: the one left out is the bin-0 candidate with the largest key; ascending candidate order
    keys = sorted((oracle.sample_key(1, 0, 0, 3, i), i) for i in range(8))
    kept = sorted([i for _, i in keys[:7]] + [8])
    assert np.array_equal(out[0][0][:, 1], np.array([xs[i] for i in kept], np.float32))
    # want = 7 is not divisible by 3 either: per = 2, the same bins, top-up 4
    stats = []
    ref.proposal_target_balanced(rois, [9], gt, seed=1, step=0, image_offset=0, num_bins=3, stats=stats, **dict(kw, R=7))
    assert (stats[0]["per"], stats[0]["gave"], stats[0]["top_up"]) == (2, [2, 0, 1], 4)
    # fewer candidates than wanted: padding
    out = ref.proposal_target_balanced(rois, [9], gt, seed=1, step=0, image_offset=0, num_bins=3, **dict(kw, R=16))
    assert (out[1][0][:9] == 0).all() and (out[1][0][9:] == -1).all() and (out[4][0][9:] == -1).all()       # the GT box is foreground


def test_the_ground_truth_box_is_a_candidate_too(oracle):
    """Candidates are the proposals followed by the valid ground truth: with a foreground quota the GT box itself (IoU 1) is
    the one foreground RoI."""
    rois = np.array([[[0, 100, 0, 199, 99]]], np.float32)
    gt = np.array([[[0, 0, 99, 99, 7]]], np.float32)
    out = ref.proposal_target_balanced(rois, [1], gt, seed=1, step=0, image_offset=0, num_bins=2, **dict(KW, R=4))
    assert out[5][0] == 1 and out[1][0].tolist() == [7, 0, -1, -1] and out[0][0][0].tolist() == [0, 0, 0, 99, 99]


# ---- Balanced L1 ------------------------------------------------------------------------------------
def _bl1_64(d, alpha, gamma, beta):
    b = math.exp(gamma / alpha) - 1.0
    a = np.abs(d)
    return np.where(a < beta, alpha / b * (b * a + 1) * np.log(b * a / beta + 1) - alpha * a, gamma * a + gamma / b - alpha * beta)


def test_balanced_l1_constant_continuity_and_gradient(oracle):
    assert ref.bl1_b(0.5, 1.5) == np.float32(math.e ** 3 - 1)
    for alpha, gamma, beta in ((0.5, 1.5, 1.0), (0.25, 1.0, 0.5), (1.0, 2.0, 0.11)):
        b = ref.bl1_b(alpha, gamma)
        below = np.nextafter(np.float32(beta), np.float32(0))
        L, g = ref.balanced_l1(np.array([below, beta, -below, -beta], np.float32), alpha, gamma, beta, b)
        scale = float(gamma * beta + gamma / b)
        assert abs(float(L[0]) - float(L[1])) <= 8 * np.finfo(np.float32).eps * scale            # value continuous at a = beta
        assert abs(float(g[0]) - float(g[1])) <= 8 * np.finfo(np.float32).eps * gamma            # gradient too: alpha ln(b + 1) = gamma
        assert L[2] == L[0] and L[3] == L[1] and g[2] == -g[0] and g[3] == -g[1]
        d = np.array([-3.0, -1.2 * beta, -0.7 * beta, -0.01, 0.003, 0.4 * beta, 0.999 * beta, 1.5 * beta, 7.0], np.float32)
        L, g = ref.balanced_l1(d, alpha, gamma, beta, b)
        d64 = d.astype(np.float64)
        assert np.allclose(L, _bl1_64(d64, alpha, gamma, beta), rtol=2e-5, atol=2e-6)
        h = 1e-6
        fd = (_bl1_64(d64 + h, alpha, gamma, beta) - _bl1_64(d64 - h, alpha, gamma, beta)) / (2 * h)
        # The closed-form gradient alpha * log(b a / beta + 1) is the paper's; it is the derivative of L exactly when beta = 1
        # (the published setting). Otherwise d/da L = that + alpha * ((b a + 1) / (b a + beta) - 1) inside the knee: the entry
        # keeps the closed form (include/mxdet.h), and this is the documented difference.
        a64 = np.abs(d64)
        extra = np.where(a64 < beta, alpha * ((float(b) * a64 + 1) / (float(b) * a64 + beta) - 1), 0.0) * np.sign(d64)
        assert beta != 1.0 or not extra.any()
        assert np.allclose(g + extra, fd, rtol=2e-5, atol=2e-6)
    L, g = ref.balanced_l1(np.zeros(2, np.float32), 0.5, 1.5, 1.0, ref.bl1_b(0.5, 1.5))
    assert L.tolist() == [0, 0] and g.tolist() == [0, 0]


def test_host_b_is_the_reference_b():
    from mxdetection_amd.core.loss import balanced_l1_b
    for a, g in ((0.5, 1.5), (0.25, 1.0), (1.0, 2.0)):
        assert balanced_l1_b(a, g) == float(ref.bl1_b(a, g))


# ---- options ------------------------------------------------------------------------------------------
def test_option_validation_in_the_model():
    from mxdetection_amd.models import FasterRCNN, RetinaNet
    bad = [dict(sampler="iou_balanced", ohem=True), dict(reg_loss="balanced_l1", ohem=True), dict(sampler="libra"),
           dict(sampler="iou_balanced", sampler_bins=0), dict(sampler="iou_balanced", sampler_bins=9),
           dict(sampler_bins=2.0), dict(sampler_bins=True), dict(reg_loss="balanced_l1", bl1_alpha=0),
           dict(reg_loss="balanced_l1", bl1_gamma=-1.0), dict(bl1_beta=float("inf")), dict(bl1_beta="1"), dict(neck="pafpn"),
           dict(neck="bfp", bfp_refine="non_local"), dict(reg_loss="balanced_l1", reg_loss_weight=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            FasterRCNN("cpu", **kw)
    with pytest.raises(ValueError, match="iou_balanced.*ohem"):
        FasterRCNN("cpu", sampler="iou_balanced", ohem=True)
    with pytest.raises(ValueError, match="balanced_l1.*ohem"):
        FasterRCNN("cpu", reg_loss="balanced_l1", ohem=True)
    with pytest.raises(ValueError, match="balanced_l1.*box head"):
        RetinaNet("cpu", reg_loss="balanced_l1")
    with pytest.raises(TypeError):
        RetinaNet("cpu", neck="bfp")


def test_option_validation_in_the_builder_and_config():
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils.config import load_config
    for key in ("network.neck=bfp", "network.sampler=iou_balanced", "network.reg_loss=balanced_l1"):
        cfg = load_config(None, ["network.type=retinanet", key])
        with pytest.raises(ValueError, match=key.split("=")[0].split(".")[1] if "reg_loss" not in key else "balanced_l1"):
            build_detector(cfg, "cpu")
    for o in (["network.sampler=iou_balanced", "network.ohem=true"], ["network.reg_loss=balanced_l1", "network.ohem=true"],
              ["network.sampler=iou_balanced", "network.sampler_bins=12"], ["network.reg_loss=balanced_l1", "network.bl1_beta=0"],
              ["network.neck=bfp", "network.bfp_refine=attention"]):
        with pytest.raises(ValueError):
            build_detector(load_config(None, o), "cpu")
    with pytest.raises(KeyError):
        load_config(None, ["network.sampler_bin=3"])


def test_configs_load():
    from mxdetection_amd.utils.config import default_config, load_config
    cfg = load_config(os.path.join(ROOT, "configs", "libra_faster_rcnn_r50_fpn.yaml"))
    net = cfg.network
    assert (net.neck, net.bfp_refine, net.sampler, net.sampler_bins) == ("bfp", "conv", "iou_balanced", 3)
    assert (net.reg_loss, net.reg_loss_weight, net.bl1_alpha, net.bl1_gamma, net.bl1_beta) == ("balanced_l1", 1.0, 0.5, 1.5, 1.0)
    d = default_config().network
    new = ("neck", "bfp_refine", "sampler", "sampler_bins", "bl1_alpha", "bl1_gamma", "bl1_beta")
    assert [d[k] for k in new] == ["fpn", "conv", "random", 3, 0.5, 1.5, 1.0]
    others = [p for p in sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml"))) if "libra" not in os.path.basename(p)]
    assert len(others) >= 19
    for p in others:
        net = load_config(p).network
        assert [net[k] for k in new] == [d[k] for k in new], p
        assert net.reg_loss != "balanced_l1"


# ---- the entries' host checks (no launch, no GPU) ---------------------------------------------------
def test_entries_refuse_bad_arguments_before_any_launch():
    from mxdetection_amd import _lib
    lib = _lib.load()
    f4 = (C.c_float * 4)(0, 0, 0, 0)
    one = C.c_void_p(16)                  # never dereferenced: the checks come first
    for bins in (0, -1, 9):
        rc = lib.mxdet_proposal_target_balanced(one, one, 8, one, 1, 4, 8, 0.25, 0.5, 0.5, 0.0, 81, 0, f4, f4, 0, 0, None, 0, bins,
                                                one, one, one, one, one, one, None)
        assert rc == -1 and b"num_bins" in lib.mxdet_last_error()
    rc = lib.mxdet_proposal_target_balanced(None, one, 8, one, 1, 4, 8, 0.25, 0.5, 0.5, 0.0, 81, 0, f4, f4, 0, 0, None, 0, 3,
                                            one, one, one, one, one, one, None)
    assert rc == -1 and b"null" in lib.mxdet_last_error()
    for bad in ((0.0, 1.5, 1.0, 19.0, 1.0), (0.5, 1.5, -1.0, 19.0, 1.0), (0.5, 1.5, 1.0, 0.0, 1.0), (0.5, 1.5, 1.0, 19.0, 0.0)):
        rc = lib.mxdet_rcnn_loss_balanced(one, one, 0, 64, 64, one, one, one, 4, 5, 20, *bad, 1.0, 1.0, one, one, one, one, 1 << 20,
                                          None)
        assert rc == -1 and b"positive" in lib.mxdet_last_error()
    rc = lib.mxdet_rcnn_loss_balanced(one, one, 0, 64, 8, one, one, one, 4, 5, 20, 0.5, 1.5, 1.0, 19.0, 1.0, 1.0, 1.0, one, one, one,
                                      one, 1 << 20, None)
    assert rc == -2
    d = _lib.BfpDescT()

    def desc(L=5, r=2, N=2, Cc=8, sizes=PYRAMIDS["overlap"]):
        d.num_levels, d.refine_level, d.N, d.C = L, r, N, Cc
        for l, (h, w) in enumerate(sizes):
            d.H[l], d.W[l] = h, w
            d.feat[l], d.out[l] = 16, 16
        return d
    assert lib.mxdet_bfp_workspace_bytes(desc()) > 0
    for kw in (dict(L=1), dict(L=7), dict(r=-1), dict(r=5), dict(N=0), dict(Cc=12), dict(Cc=0),
               dict(sizes=[(25, 34), (13, 0), (7, 9), (4, 5), (2, 3)]), dict(sizes=[(200, 34), (13, 17), (7, 9), (4, 5), (2, 3)])):
        assert lib.mxdet_bfp_workspace_bytes(desc(**kw)) == 0, kw
        for fn in (lib.mxdet_bfp_gather_fwd, lib.mxdet_bfp_scatter_fwd, lib.mxdet_bfp_scatter_bwd, lib.mxdet_bfp_gather_bwd):
            assert fn(d, one, one, 1 << 30, None) == -2, kw
    desc()
    for fn in (lib.mxdet_bfp_gather_fwd, lib.mxdet_bfp_scatter_fwd, lib.mxdet_bfp_scatter_bwd, lib.mxdet_bfp_gather_bwd):
        assert fn(d, one, one, 16, None) == -3 and b"workspace" in lib.mxdet_last_error()
        assert fn(d, None, one, 1 << 30, None) == -1 and fn(d, one, None, 1 << 30, None) == -1
        assert fn(None, one, one, 1 << 30, None) == -1
    d.feat[3] = None
    assert lib.mxdet_bfp_gather_fwd(d, one, one, 1 << 30, None) == -1 and b"level pointer" in lib.mxdet_last_error()
