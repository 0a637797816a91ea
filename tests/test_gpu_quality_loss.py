"""The quality-aware class-loss entries (mxdet_quality_focal_loss, mxdet_retina_loss_level_quality in csrc/losses.hip / retina_loss.hip) on the
case tables of tests/test_quality_loss_cases_cpu.py.

For every case: class gradients against the float64 autograd reference after division by inv * loss_scale (ATOL_CLS_GRAD as
measured in the CPU module, plus one bf16 step 2^-8 * |ref| for bf16 outputs), the summed class loss within LOSS_RTOL of the
float64 sum plus ATOL_CLS_LOSS per summed anchor, the box half (grad_reg, partial[2i+1]) bit-identical to
mxdet_retina_loss_level_iou on the same inputs, a second run bit-identical to the first, and the written extents: every
output is an interior slice of a sentinel-filled buffer.
"""
import numpy as np
import pytest

import test_iou_loss_cases_cpu as T
import test_quality_loss_cases_cpu as QT
from test_gpu_losses import SENT, Guarded, _bits, _np, _t

pytestmark = pytest.mark.gpu


def _grad_ok(what, got, ref, unit, bf16):
    got, ref = np.asarray(got, np.float64) / unit, np.asarray(ref, np.float64) / unit
    err = np.abs(got - ref)
    bound = QT.ATOL_CLS_GRAD + (QT.BF16_STEP * np.abs(ref) if bf16 else 0.0)
    print("%s: max |got-ref|/unit = %.3e (atol %.3e), max excess over the bound = %.3e"
          % (what, float(err.max()) if err.size else 0.0, QT.ATOL_CLS_GRAD, float(np.max(err - bound)) if err.size else 0.0))
    return bool(np.all(err <= bound))


def _sum_ok(what, got, ref, inv, n_anchors):
    """|got - ref| <= LOSS_RTOL |ref| + n anchors * ATOL_CLS_LOSS * inv; nothing summed gives exactly 0."""
    got, ref = float(got), float(ref)
    print("%s: got %.9g ref %.9g (%d anchors)" % (what, got, ref, n_anchors))
    return got == 0.0 if n_anchors == 0 else abs(got - ref) <= QT.LOSS_RTOL * abs(ref) + n_anchors * QT.ATOL_CLS_LOSS * inv


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", QT.PRIM_CASES, ids=QT.ids(QT.PRIM_CASES))
def test_quality_focal_loss(hip, c, bf):
    import torch
    from mxdetection_amd import _lib
    from mxdetection_amd.core import loss as L
    d, ref = QT.prim_data(c), QT.prim_ref(c)
    n, Cc = c["n"], c["C"]
    dt = torch.bfloat16 if bf else torch.float32
    x, lab, q = _t(d["x"], dt), _t(d["labels"]), _t(d["q"])
    lib = _lib.load()
    runs = []
    for _ in range(2):
        g, loss = Guarded((n, Cc), dt), Guarded((1,), torch.float32)
        ws = L.loss_workspace(n, "cuda")
        L.check(lib.mxdet_quality_focal_loss(L.ptr(x), L._DT[dt], L.ptr(lab), L.ptr(q), n, Cc, L.CLS_LOSS_KINDS[c["cls_loss"]], c["alpha"],
                                             c["gamma"], float(c["gs"]), L.ptr(loss.view), L.ptr(g.view), L.ptr(ws), ws.numel(),
                                             L.stream_ptr()), "quality_focal_loss")
        torch.cuda.synchronize()
        assert g.outside_intact() and loss.outside_intact() and not bool((g.view == SENT).any())
        runs.append((g.view.clone(), loss.view.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    g, loss = runs[0]
    w_loss, w_grad = L.quality_focal_loss(x, lab, q, c["cls_loss"], c["alpha"], c["gamma"], float(c["gs"]))       # the wrapper: the same bits
    assert torch.equal(w_loss, loss) and torch.equal(w_grad, g)
    n_valid = int((d["labels"] >= 0).sum())
    assert _sum_ok("primitive loss", loss[0], ref["loss"], ref["unit"] / c["gs"], n_valid)
    assert _grad_ok("primitive grad", _np(g), ref["grad"], ref["unit"], bf)
    ign = torch.from_numpy(d["labels"] < 0).cuda()
    assert not g[ign].any()
    if c["name"] == "all_bg":
        assert float(loss[0]) > 0.0 and ref["unit"] == c["gs"]                       # normaliser max(1, 0)


def test_quality_focal_loss_defaults_and_nothing(hip):
    import torch
    from mxdetection_amd.core import loss as L
    c = next(x for x in QT.PRIM_CASES if x["id"].startswith("n65-C8-vfl"))
    d = QT.prim_data(c)
    x, lab, q = _t(d["x"]), _t(d["labels"]), _t(d["q"])
    a = L.quality_focal_loss(x, lab, q, "vfl", grad_scale=float(c["gs"]))               # None = alpha 0.75, gamma 2
    b = L.quality_focal_loss(x, lab, q, "vfl", 0.75, 2.0, float(c["gs"]))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for dt in (torch.float32, torch.bfloat16):
        e = torch.empty((0, 8), dtype=dt, device="cuda")
        loss, g = L.quality_focal_loss(e, torch.empty((0,), dtype=torch.int32, device="cuda"), torch.empty((0,), device="cuda"), "qfl")
        torch.cuda.synchronize()
        assert g.shape == (0, 8) and float(loss[0]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
def _run_level(c, d, entry="quality", gt=None):
    import torch
    from mxdetection_amd.core import loss as L
    N, H, W, A, Cc = c["shape"]
    ldc, ldr = QT.retina_ld(c)
    bf = torch.bfloat16
    cls, reg = _t(d["cls"], bf), _t(d["reg"], bf)
    gc, gr = Guarded((N, H, W, ldc), bf), Guarded((N, H, W, ldr), bf)
    nparts = L.retina_loss_num_partials(N, H, W, A)
    part, out = Guarded((2 * nparts,), torch.float32), Guarded((2,), torch.float32)
    nfg = torch.tensor([QT.num_fg(c)], dtype=torch.int32, device="cuda")
    lab = _t(d["cls_labels"])
    gt = _t(d["gt"]) if gt is None else gt
    if entry == "quality":
        L.retina_loss_level_quality(cls, reg, A, Cc, lab, _t(d["anchors"]), _t(d["matched"]), gt, c["off"], c["cls_loss"], c["alpha"],
                                    c["gamma"], c["kind"], QT.STDS, c["rw"], nfg, float(c["ls"]), gc.view, gr.view, part.view)
    elif entry == "iou":
        L.retina_loss_level_iou(cls, reg, A, Cc, lab, _t(d["anchors"]), _t(d["matched"]), gt, c["off"], T.RETINA_ALPHA, T.RETINA_GAMMA,
                                c["kind"], QT.STDS, c["rw"], nfg, float(c["ls"]), gc.view, gr.view, part.view)
    L.loss_finalize(part.view, nparts, 2, out.view)
    torch.cuda.synchronize()
    for t in (gc, gr, part, out):
        assert t.outside_intact()
    assert bool((gc.view[..., A * Cc:] == SENT).all()) and bool((gr.view[..., 4 * A:] == SENT).all())       # padding columns: untouched
    assert not bool((part.view == SENT).any()) and not bool((gr.view[..., :4 * A] == SENT).any())
    assert not bool((gc.view[..., :A * Cc] == SENT).any())
    return gc.view[..., :A * Cc].clone(), gr.view[..., :4 * A].clone(), part.view.clone(), out.view.clone()


@pytest.mark.parametrize("c", QT.CASES, ids=QT.ids(QT.CASES))
def test_retina_loss_level_quality(hip, c):
    import torch
    d, ref = QT.level_data(c), QT.level_ref(c)
    N, H, W, A, Cc = c["shape"]
    assert QT.quality_route(c)[1] == (c["form"] == "vec")
    gc, gr, part, out = _run_level(c, d)
    again = _run_level(c, d)
    assert all(torch.equal(a, b) for a, b in zip((gc, gr, part, out), again))
    _, igr, ipart, iout = _run_level(c, d, "iou")                          # the box half of mxdet_retina_loss_level_iou: the same bits
    assert np.array_equal(_bits(gr), _bits(igr)) and torch.equal(part[1::2], ipart[1::2]) and torch.equal(out[1], iout[1])
    assert _sum_ok("class loss", out[0], ref["loss"], ref["inv"], ref["n_valid"])
    assert _grad_ok("grad_cls", _np(gc), ref["grad_cls"][..., :A * Cc], ref["unit"], True)
    n_lvl = H * W * A
    lv = d["cls_labels"][:, c["off"]:c["off"] + n_lvl]
    ign = torch.from_numpy(lv < 0).cuda()
    assert not gc.reshape(N, n_lvl, Cc)[ign].any()
    if c["name"] == "coco_bg":
        assert not gr.any() and float(out[1]) == 0.0 and float(out[0]) > 0.0
    elif n_lvl > 8 and c["cls_loss"] == "vfl":                            # q == 0 in its own column: the negatives' sign
        col = lv[0, QT.SPECIAL["miss"]] - 1
        assert float(gc.reshape(N, n_lvl, Cc)[0, QT.SPECIAL["miss"], col]) > 0.0
        assert float(gc.reshape(N, n_lvl, Cc)[0, QT.SPECIAL["hit"], lv[0, QT.SPECIAL["hit"]] - 1]) < 0.0


def test_qfl_without_foreground_is_the_focal_negatives(hip):
    """Every label <= 0: QFL(beta = 2) = sigma^2 * (-log(1 - sigma)) = the focal entry's negatives / (1 - alpha), within one
    bf16 step (the spacing of bf16 at the value). alpha = 1/2 here: the division is then exact in bf16, so the two outputs
    differ by the float32 rounding of two forms of one formula, i.e. by at most one step where that crosses a rounding tie."""
    import torch
    from mxdetection_amd.core import loss as L
    c = next(x for x in QT.CASES if x["name"] == "coco_bg" and x["cls_id"] == "qfl2")
    d = QT.level_data(c)
    N, H, W, A, Cc = c["shape"]
    gc, _, part, out = _run_level(c, d)
    ldc, ldr = QT.retina_ld(c)
    bf = torch.bfloat16
    fc, fr = torch.zeros((N, H, W, ldc), dtype=bf, device="cuda"), torch.zeros((N, H, W, ldr), dtype=bf, device="cuda")
    nparts = L.retina_loss_num_partials(N, H, W, A)
    fpart = torch.zeros((2 * nparts,), device="cuda")
    tgt = torch.zeros((N, d["A_total"], 4), device="cuda")
    alpha = 0.5
    L.retina_loss_level(_t(d["cls"], bf), _t(d["reg"], bf), A, Cc, _t(d["cls_labels"]), tgt, c["off"], alpha, 2.0, 3.0,
                        torch.zeros((1,), dtype=torch.int32, device="cuda"), float(c["ls"]), fc, fr, fpart)
    torch.cuda.synchronize()
    want = _np(fc[..., :A * Cc]) / (1.0 - alpha)
    got = _np(gc)
    valid = np.repeat(d["cls_labels"][:, c["off"]:c["off"] + H * W * A].reshape(N, H, W, A) >= 0, Cc, axis=3)
    assert np.all(want[valid] > 0) and not want[~valid].any() and not got[~valid].any()
    step = np.where(valid, 2.0 ** (np.floor(np.log2(np.where(valid, want, 1.0))) - 7), 0.0)
    print("QFL vs focal negatives: largest difference in bf16 steps %.3g" % float(np.max(np.abs(got - want)[valid] / step[valid])))
    assert np.all(np.abs(got - want) <= step)
    fsum, qsum = float(fpart[0::2].double().sum()) / (1.0 - alpha), float(part[0::2].double().sum())
    assert abs(fsum - qsum) <= 1e-5 * abs(fsum)


def test_graph_replay_follows_new_ground_truth(hip):
    """Captured once, replayed after gt_boxes was overwritten: the eager result of the new boxes (the quality is computed
    inside the kernel from what gt_boxes holds at replay)."""
    import torch
    from mxdetection_amd.core import loss as L
    c = next(x for x in QT.CASES if x["id"] == "coco-vec-vfl-giou-ls512-nfgtrue")
    d = QT.level_data(c)
    N, H, W, A, Cc = c["shape"]
    gt_b = d["gt"].copy()
    gt_b[..., :4] = T.jitter(np.random.default_rng(5), d["gt"][..., :4].reshape(-1, 4)).reshape(N, -1, 4)
    want = [_run_level(c, d, gt=_t(g)) for g in (d["gt"], gt_b)]
    assert not torch.equal(want[0][0], want[1][0]) and not torch.equal(want[0][1], want[1][1])
    ldc, ldr = QT.retina_ld(c)
    bf = torch.bfloat16
    cls, reg, lab, anchors, matched = _t(d["cls"], bf), _t(d["reg"], bf), _t(d["cls_labels"]), _t(d["anchors"]), _t(d["matched"])
    gt = _t(d["gt"])
    gc, gr = torch.zeros((N, H, W, ldc), dtype=bf, device="cuda"), torch.zeros((N, H, W, ldr), dtype=bf, device="cuda")
    nparts = L.retina_loss_num_partials(N, H, W, A)
    part, out = torch.zeros((2 * nparts,), device="cuda"), torch.zeros((2,), device="cuda")
    nfg = torch.tensor([QT.num_fg(c)], dtype=torch.int32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap):
        graph.capture_begin(capture_error_mode="thread_local")
        L.retina_loss_level_quality(cls, reg, A, Cc, lab, anchors, matched, gt, c["off"], c["cls_loss"], c["alpha"], c["gamma"], c["kind"],
                                    QT.STDS, c["rw"], nfg, float(c["ls"]), gc, gr, part)
        L.loss_finalize(part, nparts, 2, out)
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(cap)
    for g, w in ((d["gt"], want[0]), (gt_b, want[1]), (d["gt"], want[0])):
        gt.copy_(torch.from_numpy(g))
        gc.fill_(3.0)
        part.fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gc[..., :A * Cc], w[0]) and torch.equal(gr[..., :4 * A], w[1]) and torch.equal(part, w[2]) and torch.equal(out, w[3])
