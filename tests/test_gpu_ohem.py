"""The OHEM entries on the device (include/mxdet.h, csrc/ohem.hip) against tests/_ohem_ref.py: mxdet_ohem_select's integer
outputs exactly, at pool sizes that reach one and several rank workgroups and sizes that are no multiple of 64 or 256, with
padding, an empty image, all-equal scores, a block of duplicate boxes, no dedup and a NaN score; mxdet_ohem_roi_score bit for bit
against the existing loss entry called on a row alone and against float64 within LOSS_RTOL; mxdet_ohem_gather against indexing
the pool."""
import functools

import numpy as np
import pytest

import _ohem_ref as ref
import test_iou_loss_cases_cpu as TI
import test_loss_cases_cpu as T
from conftest import synth_boxes

pytestmark = pytest.mark.gpu

NC, LD = 81, 448
REG_LOSSES = ("smooth_l1", "iou", "giou", "diou")
STDS, SIGMA, REG_WEIGHT = (0.1, 0.1, 0.2, 0.2), 1.0, 10.0


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# select
SELECT_CASES = [
    # full: the reference must fill all R slots of every image AND suppress at least one candidate
    dict(id="P64-N1-R16", P=64, N=1, R=16, nms=0.7, full=True),
    dict(id="P333-N3-R16", P=333, N=3, R=16, nms=0.7, full=True),
    dict(id="P1100-N3-R64", P=1100, N=3, R=64, nms=0.7, full=True),
    dict(id="P1100-N1-R128-nms0.5", P=1100, N=1, R=128, nms=0.5, full=True),
    dict(id="P333-N3-R16-few-and-none", P=333, N=3, R=16, nms=0.7, full=False, few=True),
    dict(id="P333-N1-R16-equal-scores", P=333, N=1, R=16, nms=0.7, full=True, equal=True),
    dict(id="P64-N1-R16-duplicates", P=64, N=1, R=16, nms=0.7, full=True, dup=True),
    dict(id="P333-N3-R16-no-nms", P=333, N=3, R=16, nms=1.0, full=False),
    dict(id="P64-N1-R16-nan", P=64, N=1, R=16, nms=0.7, full=True, nan=True),
]


@functools.lru_cache(maxsize=None)
def _select_data(cid):
    c = next(c for c in SELECT_CASES if c["id"] == cid)
    N, P = c["N"], c["P"]
    rng = np.random.default_rng(sum(map(ord, cid)))
    rois = np.zeros((N, P, 5), np.float32)
    labels = np.zeros((N, P), np.int32)
    score = np.zeros((N, P), np.float32)
    for n in range(N):
        # most boxes are jitters of a few objects, so that NMS has something to do
        objs = synth_boxes(rng, 6, im_h=256, im_w=320)
        b = objs[rng.integers(0, 6, P)] + rng.uniform(-5, 5, (P, 4)).astype(np.float32)
        far = rng.random(P) < 0.5
        b[far] = synth_boxes(rng, int(far.sum()), im_h=256, im_w=320)
        rois[n, :, 0], rois[n, :, 1:] = n, b
        u = rng.random(P)
        labels[n] = np.where(u < 0.2, rng.integers(1, NC, P), np.where(u < 0.9, 0, -1))
        s = rng.gamma(2.0, 1.0, P).astype(np.float32)
        s[rng.random(P) < 0.3] = np.float32(0.75)              # ties among unequal scores
        score[n] = s
    if c.get("few"):
        labels[0, 10:] = -1                                    # 10 slots, fewer candidates than R
        labels[1, :] = -1                                      # an image without candidates
    if c.get("equal"):
        score[:] = np.float32(1.5)
    if c.get("dup"):
        x = 12.0 * np.arange(P, dtype=np.float32)
        rois[0, :, 1:] = np.stack([x, np.zeros(P, np.float32), x + 9, np.full(P, 9, np.float32)], 1)      # disjoint
        rois[0, 10:50, 1:] = np.array([30, 40, 130, 160], np.float32)                                     # 40 copies of one box
        labels[0] = np.where(np.arange(P) % 3 == 0, 7, 0)
        score[0, 10:50] += 10.0                                # ... that lead the order
    if c.get("nan"):
        score[0, 37] = np.nan
        labels[0, 37] = 0
    score[labels < 0] = -1.0
    want = ref.select(score, labels, rois, c["R"], c["nms"])
    return c, score, labels, rois, want


def test_select_cases_are_what_they_are_named():
    full = 0
    for c in SELECT_CASES:
        _, score, labels, rois, (sel, num_sel, num_fg, sup) = _select_data(c["id"])
        cand = (labels >= 0).sum(1)
        if c["full"]:
            assert (num_sel == c["R"]).all() and sup.sum() >= 1 and (cand > c["R"]).all(), c["id"]
            full += 1
        if c.get("few"):
            assert cand[0] < c["R"] and num_sel[0] == cand[0] and cand[1] == 0 and num_sel[1] == 0 and (sel[1] == -1).all()
        if c.get("dup"):
            assert np.isin(sel[0], np.arange(10, 50)).sum() == 1 and sup[0] >= 39
        if c.get("nan"):
            assert 37 in sel[0]
        if c["nms"] >= 1.0:
            assert sup.sum() == 0
        if not c.get("few"):
            assert (num_fg >= 1).any() and (num_fg < num_sel).any()          # both groups of the output order are in use
    assert 2 * full >= len(SELECT_CASES)
    assert {c["P"] for c in SELECT_CASES} == {64, 333, 1100} and {c["N"] for c in SELECT_CASES} == {1, 3}


@pytest.mark.parametrize("cid", [c["id"] for c in SELECT_CASES])
def test_select(hip, cid):
    import torch
    from mxdetection_amd.core import bbox as B
    c, score, labels, rois, (w_sel, w_num, w_fg, sup) = _select_data(cid)
    if c["full"]:      # conditioned on the inputs: the reference fills every slot and NMS removes something
        assert (w_num == c["R"]).all() and sup.sum() >= 1
    runs = []
    for _ in range(2):
        sel, num_sel, num_fg = B.ohem_select(_t(score), _t(labels), _t(rois), c["R"], c["nms"])
        torch.cuda.synchronize()
        runs.append((sel.cpu().numpy(), num_sel.cpu().numpy(), num_fg.cpu().numpy()))
    for got in runs:
        assert np.array_equal(got[0], w_sel), (got[0], w_sel)
        assert np.array_equal(got[1], w_num) and np.array_equal(got[2], w_fg)


def test_select_refuses_bad_arguments(hip):
    from mxdetection_amd.core import bbox as B
    _, score, labels, rois, _ = _select_data("P64-N1-R16")
    with pytest.raises(hip.MxdetError, match="R must be >= 1"):
        B.ohem_select(_t(score), _t(labels), _t(rois), 0, 0.7)
    with pytest.raises(hip.MxdetError, match="nms_thresh"):
        B.ohem_select(_t(score), _t(labels), _t(rois), 16, 0.0)
    import torch
    with pytest.raises(hip.MxdetError, match="workspace"):
        B.ohem_select(_t(score), _t(labels), _t(rois), 16, 0.7, workspace=torch.empty((256,), dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
# gather
@pytest.mark.parametrize("cid", ["P333-N3-R16-few-and-none", "P1100-N3-R64"])
@pytest.mark.parametrize("with_targets", [True, False])
def test_gather(hip, cid, with_targets):
    import torch
    from mxdetection_amd.core import bbox as B
    c, score, labels, rois, (sel, num_sel, _, _) = _select_data(cid)
    N, P, R, D = c["N"], c["P"], c["R"], 4 * NC
    rng = np.random.default_rng(5)
    matched = rng.integers(0, 8, (N, P)).astype(np.int32)
    tgt = rng.standard_normal((N, P, D)).astype(np.float32)
    wgt = (rng.random((N, P, D)) < 0.1).astype(np.float32)
    SENT = 12345.0
    out = (torch.full((N, R, 5), SENT, device="cuda"), torch.full((N, R), 77, dtype=torch.int32, device="cuda"),
           torch.full((N, R, D), SENT, device="cuda") if with_targets else None,
           torch.full((N, R, D), SENT, device="cuda") if with_targets else None,
           torch.full((N, R), 77, dtype=torch.int32, device="cuda"))
    got = B.ohem_gather(_t(sel), _t(rois), _t(labels), _t(matched), _t(tgt) if with_targets else None,
                        _t(wgt) if with_targets else None, out=out)
    torch.cuda.synchronize()
    want = ref.gather(sel, rois, labels, matched, tgt if with_targets else None, wgt if with_targets else None)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert np.array_equal(g.cpu().numpy(), w)
    # what "indexing the pool by sel" and "padding rows as proposal-target writes them" mean, spelled out once
    g_rois, g_lab, g_t, g_w, g_m = [None if g is None else g.cpu().numpy() for g in got]
    for n in range(N):
        k = int(num_sel[n])
        assert np.array_equal(g_rois[n, :k], rois[n, sel[n, :k]]) and np.array_equal(g_lab[n, :k], labels[n, sel[n, :k]])
        assert np.array_equal(g_rois[n, k:], np.tile(np.array([n, 0, 0, 0, 0], np.float32), (R - k, 1)))
        assert (g_lab[n, k:] == -1).all() and (g_m[n, k:] == -1).all()
        if with_targets:
            assert np.array_equal(g_t[n, :k], tgt[n, sel[n, :k]]) and not g_t[n, k:].any() and not g_w[n, k:].any()
    if cid.endswith("few-and-none"):
        assert int(num_sel[0]) < R and int(num_sel[1]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# score
SCORE_ROWS, SCORE_N, SCORE_G = 203, 2, 8          # rows: no multiple of the four rows of a workgroup


@functools.lru_cache(maxsize=None)
def _score_data(bf16):
    rng = np.random.default_rng(11 + int(bf16))
    R, N, G = SCORE_ROWS, SCORE_N, SCORE_G
    o = np.zeros((R, LD), np.float32)
    o[:, :NC] = rng.standard_normal((R, NC)) * 2.0
    o[:, NC:5 * NC] = rng.standard_normal((R, 4 * NC)) * 0.5
    if bf16:
        o = T.bf16r(o)
    u = rng.random(R)
    labels = np.where(u < 0.45, rng.integers(1, NC, R), np.where(u < 0.9, 0, -1)).astype(np.int32)
    gt = -np.ones((N, G, 5), np.float32)
    gt[:, :, :4] = synth_boxes(rng, N * G, im_h=256, im_w=320).reshape(N, G, 4)
    gt[:, :, 4] = rng.integers(1, NC, (N, G))
    img = rng.integers(0, N, R)
    matched = rng.integers(0, G, R).astype(np.int32)
    rois = np.zeros((R, 5), np.float32)
    rois[:, 0] = img
    rois[:, 1:] = gt[img, matched, :4] + rng.uniform(-8, 8, (R, 4)).astype(np.float32)
    rois[:, 3:] = np.maximum(rois[:, 3:], rois[:, 1:3] + 4)
    matched[labels <= 0] = np.where(rng.random((labels <= 0).sum()) < 0.5, -1, matched[labels <= 0])
    tgt = np.zeros((R, 4 * NC), np.float32)
    wgt = np.zeros((R, 4 * NC), np.float32)
    for r in np.flatnonzero(labels > 0):
        tgt[r, 4 * labels[r]:4 * labels[r] + 4] = rng.standard_normal(4) * 1.5
        wgt[r, 4 * labels[r]:4 * labels[r] + 4] = 1.0
    return o, labels, rois, matched, gt, tgt, wgt


def _score_fp64(reg_loss, o, labels, rois, matched, gt, tgt, wgt):
    z = o[:, :NC].astype(np.float64)
    d = o[:, NC:5 * NC].astype(np.float64)
    R = len(labels)
    lab = np.maximum(labels, 0)
    mx = z.max(1)
    ce = mx + np.log(np.exp(z - mx[:, None]).sum(1)) - z[np.arange(R), lab]
    reg = np.zeros(R)
    fg = np.flatnonzero(labels > 0)
    if reg_loss == "smooth_l1":
        x = np.abs((d - tgt) * wgt)
        s2 = SIGMA * SIGMA
        reg[fg] = np.where(x < 1.0 / s2, 0.5 * s2 * x * x, x - 0.5 / s2).sum(1)[fg]
    else:
        cols = 4 * labels[fg][:, None] + np.arange(4)[None]
        g = gt[rois[fg, 0].astype(np.int64), matched[fg], :4]
        L, _ = TI.ref_rows(rois[fg, 1:], g, o[fg[:, None], NC + cols], STDS, reg_loss)
        reg[fg] = REG_WEIGHT * L
    return np.where(labels >= 0, ce + reg, -1.0)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("reg_loss", REG_LOSSES)
def test_score(hip, reg_loss, bf16):
    import torch
    from mxdetection_amd.core import loss as L
    o, labels, rois, matched, gt, tgt, wgt = _score_data(bf16)
    R = SCORE_ROWS
    dt = torch.bfloat16 if bf16 else torch.float32
    x = _t(o).to(dt)
    assert torch.equal(x.float().cpu(), torch.from_numpy(o))                   # the device holds exactly these logits
    d_lab, d_rois, d_m, d_gt, d_tgt, d_wgt = _t(labels), _t(rois), _t(matched), _t(gt), _t(tgt), _t(wgt)
    iou = reg_loss != "smooth_l1"
    kw = dict(rois=d_rois, matched_gt=d_m, gt_boxes=d_gt, stds=STDS, reg_weight=REG_WEIGHT) if iou else \
        dict(bbox_targets=d_tgt, bbox_weights=d_wgt, sigma=SIGMA)
    before = x.clone()
    score = L.ohem_roi_score(x, x[:, NC:], d_lab, NC, 4 * NC, LD, LD, reg_loss, **kw)
    torch.cuda.synchronize()
    assert torch.equal(x, before)                                              # read-only
    got = score.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (R,)
    assert (got[labels < 0] == -1.0).all() and (labels < 0).sum() >= 8
    # fp64, every row
    want = _score_fp64(reg_loss, o, labels, rois, matched, gt, tgt, wgt)
    valid = labels >= 0
    err = np.abs(got[valid] - want[valid]) / want[valid]
    print("ohem score %s %s: max rel err %.3e (bound %.1e), %d fg rows" % (reg_loss, dt, err.max(), T.LOSS_RTOL, (labels > 0).sum()))
    assert (want[valid] > 0).all() and err.max() <= T.LOSS_RTOL
    # bit-identical to the existing entry on the row alone (R = 1, norm = 1, loss_scale = 1), 32 rows of every kind
    rows = np.concatenate([np.flatnonzero(labels > 0)[:20], np.flatnonzero(labels == 0)[:12]])
    assert len(rows) == 32
    ws = L.loss_workspace(1, "cuda")
    out = torch.zeros((2,), dtype=torch.float32, device="cuda")
    g = torch.zeros((1, LD), dtype=dt, device="cuda")
    for r in rows:
        r = int(r)
        xr = x[r:r + 1]
        if iou:
            L.rcnn_loss_iou(xr, xr[:, NC:], d_lab[r:r + 1], d_rois[r:r + 1], d_m[r:r + 1], d_gt, NC, 4 * NC, LD, LD, reg_loss, STDS,
                            REG_WEIGHT, 1.0, 1.0, g, g[:, NC:], out, ws)
        else:
            L.rcnn_loss(xr, xr[:, NC:], d_lab[r:r + 1], d_tgt[r:r + 1], d_wgt[r:r + 1], NC, 4 * NC, LD, LD, SIGMA, 1.0, 1.0, g,
                        g[:, NC:], out, ws)
        parts = out.cpu().numpy()
        alone = np.float32(parts[0]) + np.float32(parts[1])
        assert alone.view(np.uint32) == got[r].view(np.uint32), (r, parts, got[r])
        assert labels[r] == 0 or parts[1] > 0
