"""The Libra R-CNN entries on the GPU, bit for bit against tests/_libra_ref.py: the IoU-balanced sampler's quota, top-up, empty
bin, padding, exact-edge and multi-candidate-per-thread paths; Balanced L1 in the box-head loss entry below, at and above the
knee for f32 and bf16 column views; the Balanced Feature Pyramid's four entries on exact and overlapping pool windows at three
refine levels, with ties, their adjoint identities and run-to-run bits."""
import functools

import numpy as np
import pytest

import _libra_ref as ref

pytestmark = pytest.mark.gpu

KW = dict(R=64, fg_fraction=0.25, fg_thresh=0.5, bg_hi=0.5, bg_lo=0.0, num_classes=81, stds=(0.1, 0.1, 0.2, 0.2))
NAMES = ("rois", "labels", "tgt", "wgt", "matched", "nfg")


def _sample(rois, num, gt, num_bins, seed=3, step=2, image_offset=0, step_dev=None, **kw):
    import torch
    from mxdetection_amd.core import bbox as B
    kw = dict(KW, **kw)
    out = B.sample_rois(torch.from_numpy(rois).cuda(), torch.from_numpy(np.asarray(num, np.int32)).cuda(),
                        torch.from_numpy(gt).cuda(), kw["R"], kw["fg_fraction"], kw["fg_thresh"], kw["bg_hi"], kw["bg_lo"],
                        kw["num_classes"], False, (0.0, 0.0, 0.0, 0.0), kw["stds"], seed, step, image_offset, step_dev,
                        num_bins=num_bins)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check(rois, num, gt, num_bins, seed=3, step=2, image_offset=0, **kw):
    stats = []
    want = ref.proposal_target_balanced(rois, num, gt, seed=seed, step=step, image_offset=image_offset, num_bins=num_bins,
                                        stats=stats, **dict(KW, **kw))
    got = _sample(rois, num, gt, num_bins, seed, step, image_offset, **kw)
    for g, w, name in zip(got, want, NAMES):
        assert np.array_equal(g, w), name
    return stats, got


def test_one_bin_is_the_uniform_sampler_bit_for_bit(hip):
    rois, num, gt = ref.sampler_inputs(seed=1)
    for step in (0, 7):
        a, b = _sample(rois, num, gt, None, step=step), _sample(rois, num, gt, 1, step=step)
        for x, y, name in zip(a, b, NAMES):
            assert np.array_equal(x, y), name
    _check(rois, num, gt, 1)


# jitter 1.5: few proposals near the ground truth -- the top bin holds 4-5 candidates for a quota of 20, the rest is topped up;
# jitter 3.0: the top bin is empty; 5 and 7 bins: want = 48 is no multiple; 30 / 12 proposals: fewer candidates than wanted
@pytest.mark.parametrize("case", ["quota", "top_up", "empty_bin", "five_bins", "seven_bins", "padding", "stride_1500"])
def test_sampler_paths(hip, case):
    kw, K = {"quota": (dict(jitter=0.6), 3), "top_up": (dict(jitter=1.5), 3), "empty_bin": (dict(jitter=3.0), 3),
             "five_bins": (dict(jitter=0.6), 5), "seven_bins": (dict(jitter=0.6), 7),
             "padding": (dict(jitter=0.6, num_rois=[30, 12]), 3), "stride_1500": (dict(jitter=0.6, S=1500), 3)}[case]
    rois, num, gt = ref.sampler_inputs(seed=1, **kw)
    stats, got = _check(rois, num, gt, K)
    for s in stats:
        print(case, {k: v for k, v in s.items() if k not in ("best", "edges")})
        if case == "quota":
            assert s["gave"] == [s["per"]] * 3 and s["top_up"] == 0
        if case == "top_up":
            assert min(s["counts"]) > 0 and s["gave"][2] == s["counts"][2] < s["per"] and s["top_up"] > 0
        if case == "empty_bin":
            assert s["counts"][2] == 0 and s["top_up"] > s["per"]
        if case in ("five_bins", "seven_bins"):
            assert s["want"] % K and s["top_up"] == s["want"] - K * s["per"]
        if case == "padding":
            assert sum(s["counts"]) < s["want"] and s["top_up"] == 0
    if case == "padding":
        labels = got[1]
        assert (labels[:, -1] == -1).all() and (got[4][labels == -1] == -1).all() and not got[0][labels == -1][:, 1:].any()
    if case == "stride_1500":
        assert rois.shape[1] + gt.shape[1] > 1024          # more candidates than the workgroup has threads


def test_image_without_ground_truth(hip):
    """Every IoU is 0: all candidates are background of bin 0; the other bins give nothing and the top-up fills the batch."""
    rois, num, gt = ref.sampler_inputs(seed=2)
    gt[1, :, :] = -1
    stats, got = _check(rois, num, gt, 3)
    s = stats[1]
    assert s["nfg"] == 0 and s["counts"] == [int(num[1]), 0, 0] and s["gave"] == [21, 0, 0] and s["top_up"] == 43
    assert (got[1][1] == 0).all() and (got[4][1] == -1).all() and got[5][1] == 0


def test_iou_exactly_on_an_edge_belongs_to_the_upper_bin(hip):
    """Two bins on [0, 0.5): the edge is 0.25. Ground truth (0,0,99,99) and the proposal (60,0,159,99) overlap in 40 x 100 of
    a union of 160 x 100: IoU = 4000 / 16000 = 0.25 in fp32 exactly, so a box pair attains the edge. With want = 4, per = 2
    the upper bin holds that proposal and one at IoU 0.3 (x1 = 54: 46 / 154 < 0.3; x1 = 53: 47 / 153 = 0.307): both are taken
    whatever their keys, which would not hold were the edge candidate counted below."""
    xs = [60, 53] + [100 + 3 * i for i in range(12)]               # twelve disjoint proposals: IoU 0
    rois = np.array([[[0, x, 0, x + 99, 99] for x in xs]] * 2, np.float32)
    rois[1, :, 0] = 1
    gt = -np.ones((2, 4, 5), np.float32)
    gt[:, 0] = [0, 0, 99, 99, 5]
    for seed in (0, 1, 2):
        stats, got = _check(rois, [14, 14], gt, 2, seed=seed, R=4, fg_fraction=0.0)
        for n, s in enumerate(stats):
            assert s["best"][0] == s["edges"][0] == np.float32(0.25)
            assert s["counts"] == [12, 2] and s["gave"] == [2, 2] and s["top_up"] == 0
            assert got[0][n][:2, 1].tolist() == [60.0, 53.0]


def test_step_dev_against_step(hip):
    import torch
    rois, num, gt = ref.sampler_inputs(seed=4, jitter=1.5)
    want = _sample(rois, num, gt, 3, step=11, image_offset=5)
    dev = torch.tensor([11], dtype=torch.int32).cuda()
    got = _sample(rois, num, gt, 3, step=0, image_offset=5, step_dev=dev)
    other = _sample(rois, num, gt, 3, step=0, image_offset=5)
    for g, w, name in zip(got, want, NAMES):
        assert np.array_equal(g, w), name
    assert not np.array_equal(other[0], want[0])


def test_bad_num_bins(hip):
    from mxdetection_amd import _lib
    rois, num, gt = ref.sampler_inputs(seed=1)
    for k in (0, 9, -3, 2.5):
        with pytest.raises((ValueError, _lib.MxdetError)):
            _sample(rois, num, gt, k)


# ---- Balanced L1 ------------------------------------------------------------------------------------
R_, NC, RD, LD = 130, 5, 20, 64
BL1 = (0.5, 1.5, 1.0)


@functools.lru_cache(maxsize=None)
def _loss_inputs():
    """One [R, 64] buffer: class logits in columns 0..4, box deltas in 5..24. Differences of the first rows are exact in bf16:
    0, below / at / above beta = 1 on both sides."""
    rng = np.random.default_rng(5)
    labels = rng.integers(1, NC, R_).astype(np.int32)
    labels[[3, 40, 129]] = -1
    labels[[4, 41, 128]] = 0
    tgt = np.zeros((R_, RD), np.float32)
    wgt = np.zeros((R_, RD), np.float32)
    buf = ref.oracle.round_bf16(rng.normal(size=(R_, LD)).astype(np.float32))
    special = np.array([0.0, 0.25, -0.25, 0.75, 1.0, -1.0, 1.5, -3.0, 0.5, -0.5, 2.0, 0.125], np.float32)
    for r in range(R_):
        c0 = 4 * max(int(labels[r]), 0)
        tgt[r, c0:c0 + 4] = rng.choice(np.array([0.0, 0.5, -0.25], np.float32), 4)
        wgt[r, c0:c0 + 4] = 1.0 if r % 7 else 0.5
        if r < 24:
            buf[r, NC + c0:NC + c0 + 4] = tgt[r, c0:c0 + 4] + special[(4 * r + np.arange(4)) % len(special)]
    wgt[50, :] = 0                                    # a foreground row with nothing to regress
    return labels, tgt, wgt, buf


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_balanced_l1_in_the_box_head_loss(hip, dtype):
    import torch
    from mxdetection_amd.core import loss as L
    labels, tgt, wgt, buf = _loss_inputs()
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    o = torch.from_numpy(buf).cuda().to(td)
    lab, t, w = torch.from_numpy(labels).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(wgt).cuda()
    ws = L.loss_workspace(R_, "cuda")
    norm, scale, rw = 1.0 / R_, 4.0, 1.5
    grads, losses = [], []
    for balanced in (False, True):
        g = torch.full((R_, LD), 7.0, dtype=td, device="cuda")
        loss = torch.zeros(2, device="cuda")
        if balanced:
            L.rcnn_loss_balanced(o, o[:, NC:], lab, t, w, NC, RD, LD, LD, *BL1, rw, norm, scale, g, g[:, NC:], loss, ws)
        else:
            L.rcnn_loss(o, o[:, NC:], lab, t, w, NC, RD, LD, LD, 1.0, norm, scale, g, g[:, NC:], loss, ws)
        torch.cuda.synchronize()
        grads.append(g.float().cpu().numpy())
        losses.append(loss.cpu().numpy())
    # the class half is mxdet_rcnn_loss's, bit for bit; columns past reg_dim are untouched
    assert losses[1][0] == losses[0][0] and np.array_equal(grads[1][:, :NC], grads[0][:, :NC])
    assert (grads[1][:, NC + RD:] == 7.0).all()
    b = ref.bl1_b(BL1[0], BL1[1])
    want_loss, want_grad = ref.rcnn_reg_balanced(buf[:, NC:NC + RD], labels, tgt, wgt, *BL1, b, rw, norm, scale, bf16=dtype == "bf16")
    got = grads[1][:, NC:NC + RD]
    assert np.array_equal(got, want_grad)
    assert losses[1][1] == want_loss
    assert not got[labels <= 0].any() and not got[50].any() and not grads[1][labels < 0][:, :NC].any()
    d = (buf[:24, NC:NC + RD] - tgt[:24]) * wgt[:24]
    on = wgt[:24] != 0
    assert (np.abs(d[on]) == 1.0).any() and (np.abs(d[on]) > 1.0).any() and (d[on] == 0).any() and (np.abs(d[on]) < 1.0).any()
    assert not got[:24][on & (d == 0) & (labels[:24, None] > 0)].any()
    assert want_loss > 0 and losses[1][1] != losses[0][1]


# ---- Balanced Feature Pyramid -------------------------------------------------------------------------
PYRAMIDS = {"exact": [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)], "overlap": [(25, 34), (13, 17), (7, 9), (4, 5), (2, 3)]}
VALUES = np.array([-2.0, -0.75, -0.5, 0.0, 0.25, 0.5, 1.0, 1.5, 3.0], np.float32)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).cuda()


def _host(t):
    return t.float().cpu().numpy()


U = 2.0 ** -8 * (1 + 2.0 ** -7)      # one bf16 rounding relative to the ROUNDED magnitude


@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("name,r", [("exact", 2), ("overlap", 2), ("overlap", 0), ("overlap", 4)])
def test_bfp_entries(hip, name, r, C):
    import torch
    from mxdetection_amd.ops.bfp import BfpPlan
    rng = np.random.default_rng(11)
    N, sizes = 2, PYRAMIDS[name]
    shapes = [(N, h, w, C) for h, w in sizes]
    P = [rng.choice(VALUES, s).astype(np.float32) for s in shapes]
    Rf = rng.choice(VALUES, shapes[r]).astype(np.float32)
    dQ = [rng.choice(VALUES, s).astype(np.float32) for s in shapes]
    dB = rng.choice(VALUES, shapes[r]).astype(np.float32)
    plan = BfpPlan(shapes, r, "cuda")
    new = lambda s: torch.full(s, 9.0, dtype=torch.bfloat16, device="cuda")    # noqa: E731
    # ---- forward ----
    want_B, args_g = ref.gather_fwd(P, r)
    dP_ = [_dev(p) for p in P]
    B = plan.gather_forward(dP_, new(shapes[r]))
    assert np.array_equal(_host(B), want_B)
    want_Q, args_s = ref.scatter_fwd(P, Rf, r)
    Q = plan.scatter_forward(dP_, _dev(Rf), [new(s) for s in shapes])
    for l in range(len(P)):
        assert np.array_equal(_host(Q[l]), want_Q[l]), l
    if r > 0:     # ties inside the first pool window of the finest level
        y1, x1 = ref.pool_window(0, sizes[0][0], sizes[r][0])[1], ref.pool_window(0, sizes[0][1], sizes[r][1])[1]
        win = P[0][:, :y1, :x1, :].reshape(N, -1, C)
        assert ((win == win.max(1, keepdims=True)).sum(1) > 1).any()
    # ---- backward: bits, twice ----
    want_dRf = ref.scatter_bwd(dQ, r, args_s)
    want_dP = ref.gather_bwd(dQ, dB, r, args_g)
    for run in range(2):
        d_ = [_dev(d) for d in dQ]
        dRf = plan.scatter_backward(d_, new(shapes[r]))
        assert np.array_equal(_host(dRf), want_dRf), run
        out = plan.gather_backward(d_, _dev(dB), [new(s) for s in shapes])
        for l in range(len(P)):
            assert np.array_equal(_host(out[l]), want_dP[l]), (run, l)
            assert np.array_equal(_host(d_[l]), dQ[l])                       # out of place: the input is intact
        plan.gather_backward(d_, _dev(dB))                                    # in place over dQ
        for l in range(len(P)):
            assert np.array_equal(_host(d_[l]), want_dP[l]), (run, l)
    # ---- adjoint identities in float64 ----
    # gather: with the arg-maxima fixed it is linear and homogeneous, J P = B before rounding; J^T dB = dP at dQ = 0.
    # Each side carries one bf16 rounding per element: |<B, dB> - <P, dP>| <= U (sum|B||dB| + sum|P||dP|)
    zeros = lambda: [_dev(np.zeros(s, np.float32)) for s in shapes]    # noqa: E731
    adj = [_host(t).astype(np.float64) for t in plan.gather_backward(zeros(), _dev(dB))]
    Bg = _host(B).astype(np.float64)
    lhs, rhs = (Bg * dB).sum(), sum((p * a).sum() for p, a in zip(P, adj))
    assert abs(lhs - rhs) <= U * ((np.abs(Bg) * np.abs(dB)).sum() + sum((np.abs(p) * np.abs(a)).sum() for p, a in zip(P, adj)))
    # scatter: at P = 0, Q_l = s_l(Rf) exactly (a selection of bf16 values); <Q, dQ> = <Rf, dRf> up to dRf's rounding
    Qz = [_host(t).astype(np.float64) for t in plan.scatter_forward(zeros(), _dev(Rf), [new(s) for s in shapes])]
    dRf64 = _host(plan.scatter_backward([_dev(d) for d in dQ], new(shapes[r]))).astype(np.float64)
    lhs, rhs = sum((q * d).sum() for q, d in zip(Qz, dQ)), (Rf * dRf64).sum()
    assert abs(lhs - rhs) <= U * (np.abs(Rf) * np.abs(dRf64)).sum()
    torch.cuda.synchronize()


def test_bfp_bad_arguments(hip):
    from mxdetection_amd import _lib
    from mxdetection_amd.ops.bfp import BfpPlan
    good = [(2, h, w, 8) for h, w in PYRAMIDS["overlap"]]
    for shapes, r in ((good[:1], 0), (good, 5), (good, -1), ([(2, h, w, 12) for h, w in PYRAMIDS["overlap"]], 2),
                      ([(2, 200, 34, 8)] + good[1:], 2)):
        with pytest.raises(_lib.MxdetError):
            BfpPlan(shapes, r, "cuda")
