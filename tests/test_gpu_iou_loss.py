"""The IoU / GIoU / DIoU box-loss entries (csrc/losses.hip, retina_loss.hip) on the case tables of tests/test_iou_loss_cases_cpu.py.

For every case: gradients against the float64 autograd reference after division by `unit` (ATOL_GRAD of the stds setting, as
measured in the CPU module, plus one bf16 step 2^-8 * |ref| for bf16 outputs), per-box losses within ATOL_LOSS, summed
losses within LOSS_RTOL of the float64 sum plus ATOL_LOSS per summed box (exactly 0 where no box contributes), the class
half bit-identical to the smooth-L1 entries on the same inputs, a second run bit-identical to the first, and the written
extents: every output is an interior slice of a sentinel-filled buffer.
"""
import numpy as np
import pytest

import test_iou_loss_cases_cpu as T
from test_gpu_losses import SENT, Guarded, _bits, _np, _t

pytestmark = pytest.mark.gpu


def _grad_ok(what, got, ref, unit, atol, bf16):
    got, ref = np.asarray(got, np.float64) / unit, np.asarray(ref, np.float64) / unit
    err = np.abs(got - ref)
    bound = atol + (T.BF16_STEP * np.abs(ref) if bf16 else 0.0)
    print("%s: max |got-ref|/unit = %.3e (atol %.3e), max excess over the bound = %.3e"
          % (what, float(err.max()) if err.size else 0.0, atol, float(np.max(err - bound)) if err.size else 0.0))
    return bool(np.all(err <= bound))


def _sum_ok(what, got, ref, scale, nfg):
    """|got - ref| <= LOSS_RTOL |ref| + nfg boxes * ATOL_LOSS * scale (scale = reg_weight * norm); 0 stays 0."""
    got, ref = float(got), float(ref)
    print("%s: got %.9g ref %.9g (%d boxes)" % (what, got, ref, nfg))
    return got == 0.0 if nfg == 0 else abs(got - ref) <= T.LOSS_RTOL * abs(ref) + nfg * T.ATOL_LOSS * scale


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("c", T.PRIM_CASES, ids=T.ids(T.PRIM_CASES))
def test_box_iou_loss(hip, c, kind, bf):
    import torch
    from mxdetection_amd.core import loss as L
    d, ref = T.prim_data(c), T.prim_ref(c, kind)
    n, ld = c["n"], 7                                                     # deltas are columns 2..5 of a 7-column buffer
    dt = torch.bfloat16 if bf else torch.float32
    box, gt = _t(d["box"]), _t(d["gt"])
    w = None if d["w"] is None else _t(d["w"])
    wide = np.full((n, ld), 3.0, np.float32)
    wide[:, 2:6] = d["d"]
    x = _t(wide, dt)
    runs = []
    for _ in range(2):
        g, loss = Guarded((n, ld), dt), Guarded((n,), torch.float32)
        L.box_iou_loss(box, gt, x[:, 2:6], kind, d["stds"], w, float(c["gs"]), loss.view, g.view[:, 2:6])
        torch.cuda.synchronize()
        assert g.outside_intact() and loss.outside_intact()
        assert bool((g.view[:, :2] == SENT).all()) and bool((g.view[:, 6:] == SENT).all())      # columns 4 .. ld: untouched
        runs.append((g.view[:, 2:6].clone(), loss.view.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    g, loss = runs[0]
    assert not bool((g == SENT).any()) and not bool((loss == SENT).any())
    err = np.abs(_np(loss) - ref["loss"])
    print("per-box loss: max error %.3e (atol %.3e)" % (err.max(), T.ATOL_LOSS))
    wmax = 1.0 if d["w"] is None else max(1.0, float(d["w"].max()))
    assert np.all(err <= T.ATOL_LOSS * wmax)
    assert _grad_ok("grad_deltas", _np(g), ref["grad"], ref["unit"] * wmax, T.ATOL_GRAD[c["stds"]], bf)
    if c["name"] == "identical":
        assert not loss.any()
    if c["name"] == "clamped_dw":
        assert not g[:, 2].any() and g[:, 3].all()
    if c["name"] == "disjoint" and kind == "iou":
        assert not g.any() and float(loss[0]) == 1.0
    if d["w"] is not None:
        z = torch.from_numpy(d["w"] == 0).cuda()
        assert not loss[z].any() and not g[z].any()


def test_box_iou_loss_of_nothing(hip):
    import torch
    from mxdetection_amd.core import loss as L
    e = torch.empty((0, 4), dtype=torch.float32, device="cuda")
    loss, g = L.box_iou_loss(e, e, e, "giou")
    torch.cuda.synchronize()
    assert loss.shape == (0,) and g.shape == (0, 4)


# ---------------------------------------------------------------------------------------------------------------------
def _run_rcnn(c, d, kind, iou=True):
    """One launch on the fused 448-column buffer (grad_cls / grad_reg are column views); rows beyond R are guard rows."""
    import torch
    from mxdetection_amd.core import loss as L
    nc, R, ld = c["nc"], c["R"], T.RCNN_LD
    rd = 4 * nc
    dt = torch.bfloat16 if c["bf"] else torch.float32
    fused = np.full((R, ld), 7.0, np.float32)
    fused[:, :nc], fused[:, nc:nc + rd] = d["cls"], d["reg"]
    x = _t(fused, dt)
    g, out = Guarded((R, ld), dt), Guarded((2,), torch.float32)
    ws = L.loss_workspace(R, "cuda")
    lab = _t(d["labels"])
    if iou:
        L.rcnn_loss_iou(x, x[:, nc:], lab, _t(d["rois"]), _t(d["matched"]), _t(d["gt"]), nc, rd, ld, ld, kind, T.STDS[T.RCNN_STDS],
                        T.RCNN_WEIGHT, d["norm"], float(c["ls"]), g.view, g.view[:, nc:], out.view, ws)
    else:
        zeros = torch.zeros((R, rd), dtype=torch.float32, device="cuda")
        L.rcnn_loss(x, x[:, nc:], lab, zeros, zeros, nc, rd, ld, ld, 1.0, d["norm"], float(c["ls"]), g.view, g.view[:, nc:], out.view, ws)
    torch.cuda.synchronize()
    assert g.outside_intact() and out.outside_intact()                   # rows beyond R and the words around loss_out
    assert bool((g.view[:, nc + rd:] == SENT).all())                      # padding columns: untouched
    assert not bool((g.view[:, :nc + rd] == SENT).any())
    return g.view[:, :nc].clone(), g.view[:, nc:nc + rd].clone(), out.view.clone()


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("c", T.RCNN_CASES, ids=T.ids(T.RCNN_CASES))
def test_rcnn_loss_iou(hip, c, kind):
    import torch
    d, ref = T.rcnn_data(c), T.rcnn_ref(c, kind)
    gc, gr, out = _run_rcnn(c, d, kind)
    gc2, gr2, out2 = _run_rcnn(c, d, kind)
    assert torch.equal(gc, gc2) and torch.equal(gr, gr2) and torch.equal(out, out2)
    oc, _, oout = _run_rcnn(c, d, kind, iou=False)                        # the class half of mxdet_rcnn_loss: the same bits
    assert torch.equal(gc, oc) and torch.equal(out[0], oout[0])
    assert abs(float(out[0]) - ref["loss"][0]) <= T.LOSS_RTOL * abs(ref["loss"][0])
    assert _sum_ok("rcnn reg loss", out[1], ref["loss"][1], T.RCNN_WEIGHT * d["norm"], ref["nfg"])
    assert _grad_ok("rcnn grad_reg", _np(gr), ref["grad_reg"], ref["unit_reg"], T.ATOL_GRAD[T.RCNN_STDS], c["bf"])
    lab = torch.from_numpy(d["labels"]).cuda()
    assert not gr[lab <= 0].any()
    if c["mix"] == "all_bg":
        assert not gr.any() and float(out[1]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
def _run_retina(c, d, kind, iou=True):
    import torch
    from mxdetection_amd.core import loss as L
    N, H, W, A, Cc = c["shape"]
    ldc, ldr = T.retina_ld(c)
    bf = torch.bfloat16
    cls, reg = _t(d["cls"], bf), _t(d["reg"], bf)
    gc, gr = Guarded((N, H, W, ldc), bf), Guarded((N, H, W, ldr), bf)
    nparts = L.retina_loss_num_partials(N, H, W, A)
    part, out = Guarded((2 * nparts,), torch.float32), Guarded((2,), torch.float32)
    num_fg = torch.tensor([T.retina_num_fg(c)], dtype=torch.int32, device="cuda")
    lab = _t(d["cls_labels"])
    if iou:
        L.retina_loss_level_iou(cls, reg, A, Cc, lab, _t(d["anchors"]), _t(d["matched"]), _t(d["gt"]), c["off"], T.RETINA_ALPHA,
                                T.RETINA_GAMMA, kind, T.STDS[T.RETINA_STDS], c["rw"], num_fg, float(c["ls"]), gc.view, gr.view, part.view)
    else:
        tgt = torch.zeros((N, d["A_total"], 4), dtype=torch.float32, device="cuda")
        L.retina_loss_level(cls, reg, A, Cc, lab, tgt, c["off"], T.RETINA_ALPHA, T.RETINA_GAMMA, 3.0, num_fg, float(c["ls"]), gc.view,
                            gr.view, part.view)
    L.loss_finalize(part.view, nparts, 2, out.view)
    torch.cuda.synchronize()
    for t in (gc, gr, part, out):
        assert t.outside_intact()
    assert bool((gc.view[..., A * Cc:] == SENT).all()) and bool((gr.view[..., 4 * A:] == SENT).all())
    assert not bool((part.view == SENT).any()) and not bool((gr.view[..., :4 * A] == SENT).any())
    return gc.view[..., :A * Cc].clone(), gr.view[..., :4 * A].clone(), part.view.clone(), out.view.clone()


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("c", T.RETINA_CASES, ids=T.ids(T.RETINA_CASES))
def test_retina_loss_level_iou(hip, c, kind):
    import torch
    d, ref = T.retina_data(c), T.retina_ref(c, kind)
    N, H, W, A, Cc = c["shape"]
    assert T.retina_iou_route(c)[1] == (c["form"] == "vec")
    gc, gr, part, out = _run_retina(c, d, kind)
    again = _run_retina(c, d, kind)
    assert all(torch.equal(a, b) for a, b in zip((gc, gr, part, out), again))
    oc, _, opart, oout = _run_retina(c, d, kind, iou=False)               # the focal half of mxdet_retina_loss_level: the same bits
    assert np.array_equal(_bits(gc), _bits(oc)) and torch.equal(part[0::2], opart[0::2]) and torch.equal(out[0], oout[0])
    inv = ref["unit"] / c["ls"]
    assert abs(float(out[0]) - ref["loss"][0]) <= T.LOSS_RTOL * abs(ref["loss"][0])
    assert _sum_ok("retina box loss", out[1], ref["loss"][1], c["rw"] * inv, ref["nfg"])
    assert _grad_ok("retina grad_reg", _np(gr), ref["grad_reg"][..., :4 * A], ref["unit_reg"], T.ATOL_GRAD[T.RETINA_STDS], True)
    n_lvl = H * W * A
    bg = torch.from_numpy(d["cls_labels"][:, c["off"]:c["off"] + n_lvl] <= 0).cuda()
    assert not gr.reshape(N, n_lvl, 4)[bg].any()
