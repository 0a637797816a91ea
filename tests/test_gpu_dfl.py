"""The distribution box head's entries (mxdet_box_dist_loss, mxdet_retina_loss_level_dfl in csrc/losses.hip / retina_loss.hip,
mxdet_retina_detect_dfl in csrc/postprocess.hip) on the case tables of tests/test_dfl_cases_cpu.py.

Losses: per row / per element against the float64 autograd reference within the bounds measured in the CPU module (plus one
bf16 step 2^-8 |ref| for bf16 outputs), the summed losses within LOSS_RTOL of the float64 sum plus the per-row bound per
summed anchor, padding channels and everything outside the outputs keeping a sentinel, the class half bit-identical to
mxdet_retina_loss_level_quality / _iou on the same inputs. Detection: bit for bit against the reference composed from the
oracle's selection / NMS / merge and the _dfl_ref decode where the decode is exact, within ATOL_DECODE otherwise.
"""
import numpy as np
import pytest

import _dfl_ref as D
import test_dfl_cases_cpu as DT
from test_gpu_losses import SENT, Guarded, _bits, _np, _t

pytestmark = pytest.mark.gpu


def _close(what, got, ref, atol, unit=1.0, bf16=False):
    got, ref = np.asarray(got, np.float64) / unit, np.asarray(ref, np.float64) / unit
    err = np.abs(got - ref)
    bound = atol + (DT.BF16_STEP * np.abs(ref) if bf16 else 0.0)
    print("%s: max |got-ref|/unit = %.3e (atol %.3e), max excess over the bound = %.3e"
          % (what, float(err.max()) if err.size else 0.0, atol, float(np.max(err - bound)) if err.size else 0.0))
    return bool(np.all(err <= bound))


def _sum_ok(what, got, ref, atol_row, inv, n_rows):
    got, ref = float(got), float(ref)
    print("%s: got %.9g ref %.9g (%d rows)" % (what, got, ref, n_rows))
    return got == 0.0 if n_rows == 0 else abs(got - ref) <= DT.LOSS_RTOL * abs(ref) + n_rows * atol_row * inv


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", DT.PRIM_CASES, ids=DT.ids(DT.PRIM_CASES))
def test_box_dist_loss(hip, c, bf):
    import torch
    from mxdetection_amd.core import loss as L
    b, g, x = DT.prim_data(c)
    ref = DT.prim_ref(c)
    n, R = c["n"], c["R"]
    real, ld = 4 * (R + 1), 4 * (R + 1) + c["pad"]
    dt = torch.bfloat16 if bf else torch.float32
    xin = torch.full((n, ld), 7.0, dtype=dt, device="cuda")
    xin[:, :real] = _t(x, dt)                                         # the tables' logits are bf16-exact
    grad = Guarded((n, ld), dt)
    lb, ld_, q, gv = L.box_dist_loss(_t(b), _t(g), xin[:, :real], R, c["s"], c["kind"], c["rw"], c["dw"], c["gs"],
                                     grad_logits=grad.view[:, :real])
    torch.cuda.synchronize()
    assert grad.outside_intact() and bool((grad.view[:, real:] == SENT).all()) and not bool((grad.view[:, :real] == SENT).any())
    assert _close("loss_box", _np(lb), ref["box"], DT.ATOL_BOX)        # measured on the weighted terms: no factor
    assert _close("loss_dfl", _np(ld_), ref["dfl"], DT.ATOL_DFL)
    assert _close("quality", _np(q), ref["q"], DT.ATOL_Q)
    assert _close("grad", _np(grad.view[:, :real]), ref["grad"], DT.ATOL_GRAD, ref["unit"], bf)
    if n >= len(DT.NAMED):
        assert float(q[DT.NAMED.index("disjoint")]) == 0.0
    lb2, ld2, q2, g2 = L.box_dist_loss(_t(b), _t(g), xin[:, :real], R, c["s"], c["kind"], c["rw"], c["dw"], c["gs"], want_quality=False)
    torch.cuda.synchronize()
    assert q2 is None and torch.equal(lb2, lb) and torch.equal(ld2, ld_) and torch.equal(g2, grad.view[:, :real])


def test_box_dist_loss_of_nothing(hip):
    import torch
    from mxdetection_amd.core import loss as L
    e = torch.empty((0, 4), device="cuda")
    lb, ld, q, g = L.box_dist_loss(e, e, torch.empty((0, 68), dtype=torch.bfloat16, device="cuda"), 16, 8.0)
    torch.cuda.synchronize()
    assert lb.shape == ld.shape == q.shape == (0,) and g.shape == (0, 68)


# ---------------------------------------------------------------------------------------------------------------------
def _run_level(c, d, entry="dfl", gt=None, shift=0):
    """shift: the class and box tensors start `shift` elements into their buffers (unaligned views: the scalar form)."""
    import torch
    from mxdetection_amd.core import loss as L
    N, H, W, A, Cc, R = c["shape"]
    ldc, ldr = DT.level_ld(c)
    bf = torch.bfloat16
    real = 4 * (R + 1) * A

    def shifted(a, ld):
        flat = torch.zeros((a.size + shift + 8,), dtype=bf, device="cuda")
        flat[shift:shift + a.size] = _t(a, bf).reshape(-1)
        return flat[shift:shift + a.size].view(N, H, W, ld)
    cls, reg = shifted(d["cls"], ldc), shifted(d["reg"], ldr)
    gc, gr = Guarded((N, H, W, ldc), bf, offset=shift), Guarded((N, H, W, ldr), bf, offset=shift)
    nparts = L.retina_loss_num_partials(N, H, W, A)
    ncomp = 3 if entry == "dfl" else 2
    part, out = Guarded((ncomp * nparts,), torch.float32), Guarded((ncomp,), torch.float32)
    nfg = torch.tensor([d["num_fg"]], dtype=torch.int32, device="cuda")
    lab = _t(d["cls_labels"])
    gt = _t(d["gt"]) if gt is None else gt
    args = (cls, reg, A, Cc, lab, _t(d["anchors"]), _t(d["matched"]), gt, c["off"])
    if entry == "dfl":
        L.retina_loss_level_dfl(*args, c["cls_loss"], c["alpha"], c["gamma"], c["kind"], R, c["s"], c["rw"], c["dw"], nfg,
                                float(c["ls"]), gc.view, gr.view, part.view)
    elif entry == "quality":
        L.retina_loss_level_quality(*args, c["cls_loss"], c["alpha"], c["gamma"], c["kind"], (1.0,) * 4, c["rw"], nfg, float(c["ls"]),
                                    gc.view, gr.view, part.view)
    else:
        L.retina_loss_level_iou(*args, c["alpha"], c["gamma"], c["kind"], (1.0,) * 4, c["rw"], nfg, float(c["ls"]), gc.view, gr.view,
                                part.view)
    L.loss_finalize(part.view, nparts, ncomp, out.view)
    torch.cuda.synchronize()
    for t in (gc, gr, part, out):
        assert t.outside_intact()
    assert not bool((part.view == SENT).any()) and not bool((gc.view[..., :A * Cc] == SENT).any())
    assert bool((gc.view[..., A * Cc:] == SENT).all())
    if entry == "dfl":
        assert bool((gr.view[..., real:] == SENT).all()) and not bool((gr.view[..., :real] == SENT).any())
    return gc.view[..., :A * Cc].clone(), gr.view[..., :real].clone(), part.view.clone(), out.view.clone()


def _check_level(c, d, got, ref):
    N, H, W, A, Cc, R = c["shape"]
    gc, gr, part, out = got
    real = 4 * (R + 1) * A
    n_lvl = H * W * A
    inv = ref["unit"] / c["ls"]
    nfg = ref["nfg"]
    ok = [_close("grad_reg", _np(gr), ref["grad_reg"][..., :real], DT.ATOL_GRAD, ref["unit"], True),
          _sum_ok("box loss", out[1], ref["loss"][1], DT.ATOL_BOX, inv, nfg),
          _sum_ok("dfl loss", out[2], ref["loss"][2], DT.ATOL_DFL, inv, nfg)]
    # the class half: the bounds of the quality / focal tables
    import test_quality_loss_cases_cpu as QT
    cerr = np.abs(_np(gc) - ref["grad_cls"][..., :A * Cc]) / ref["unit"]
    cbound = QT.ATOL_CLS_GRAD + DT.BF16_STEP * np.abs(ref["grad_cls"][..., :A * Cc]) / ref["unit"]
    print("grad_cls: max |got-ref|/unit = %.3e, max excess %.3e" % (cerr.max(), (cerr - cbound).max()))
    ok.append(bool(np.all(cerr <= cbound)))
    ok.append(_sum_ok("class loss", out[0], ref["loss"][0], QT.ATOL_CLS_LOSS, inv, ref["n_valid"]))
    lv = d["cls_labels"][:, c["off"]:c["off"] + n_lvl]
    import torch
    ign = torch.from_numpy(lv < 0).cuda()
    ok.append(not bool(gc.reshape(N, n_lvl, Cc)[ign].any()))
    _, _, n_i, a_i = D.level_positives(A, d["cls_labels"], d["matched"], DT.LEVEL_G, c["off"], n_lvl)
    idle = np.ones((N, n_lvl), bool)
    idle[n_i, a_i] = False                                           # anchors that do not regress: zeros, not left-overs
    ok.append(not bool(gr.reshape(N, n_lvl, 4 * (R + 1))[torch.from_numpy(idle).cuda()].any()))
    return ok


@pytest.mark.parametrize("c", DT.LEVEL_CASES, ids=DT.ids(DT.LEVEL_CASES))
def test_retina_loss_level_dfl(hip, c):
    import torch
    d, ref = DT.level_data(c), DT.level_ref(c)
    got = _run_level(c, d)
    again = _run_level(c, d)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    assert all(_check_level(c, d, got, ref))
    if c["name"] == "bg":
        assert not got[1].any() and float(got[3][1]) == 0.0 and float(got[3][2]) == 0.0 and float(got[3][0]) > 0.0
        assert ref["unit"] == float(c["ls"])                         # normaliser max(1, 0)


@pytest.mark.parametrize("name,ck", [("coco", "focal"), ("c3", "focal"), ("tail", "focal")])
def test_focal_class_half_is_the_iou_entry(hip, name, ck):
    """cls_kind focal: grad_cls and the class partials are mxdet_retina_loss_level_iou's bits (same labels, same walk).
    The plain entry reads reg as deltas; its box half is not compared."""
    import torch
    c = next(x for x in DT.LEVEL_CASES if x["name"] == name and x["cls_loss"] == ck)
    d = DT.level_data(c)
    gc, _, part, out = _run_level(c, d)
    igc, _, ipart, iout = _run_level(c, d, "iou")
    assert np.array_equal(_bits(gc), _bits(igc)) and torch.equal(part[0::3], ipart[0::2]) and torch.equal(out[0], iout[0])


@pytest.mark.parametrize("name", ["coco", "c3"])
@pytest.mark.parametrize("ck", ["qfl", "vfl"])
def test_quality_class_half_is_the_quality_walk(hip, name, ck):
    """Equal logits, labels and QUALITY give the _quality entry's bits. The two entries decode different boxes, so the
    quality is made equal the only way both allow: no anchor regresses (every match out of range), q == 0 everywhere."""
    import torch
    c = next(x for x in DT.LEVEL_CASES if x["name"] == name and x["cls_loss"] == ck)
    d = dict(DT.level_data(c))
    d["matched"] = np.full_like(d["matched"], DT.LEVEL_G)
    gc, gr, part, out = _run_level(c, d)
    qgc, _, qpart, qout = _run_level(c, d, "quality")
    assert not gr.any() and float(out[1]) == 0.0 and float(out[2]) == 0.0
    assert np.array_equal(_bits(gc), _bits(qgc)) and torch.equal(part[0::3], qpart[0::2]) and torch.equal(out[0], qout[0])


@pytest.mark.parametrize("name", ["coco", "c3"])
@pytest.mark.parametrize("ck", ["qfl", "vfl"])
def test_class_half_with_nonzero_quality_is_the_unfused_pair(hip, name, ck):
    """The qs[] hand-off with q > 0: the level's grad_cls equals, bit for bit, mxdet_quality_focal_loss fed the quality that
    mxdet_box_dist_loss returns for the level's regressing anchors (the same quad code, the same class element, the same
    g * inv * loss_scale; the level holds every foreground anchor, so both normalise by the same count)."""
    import torch
    from mxdetection_amd.core import loss as L
    c = next(x for x in DT.LEVEL_CASES if x["name"] == name and x["cls_loss"] == ck)
    d = DT.level_data(c)
    N, H, W, A, Cc, R = c["shape"]
    n_lvl = H * W * A
    assert c["off"] == 0 and d["A_total"] == n_lvl and d["num_fg"] == int((d["cls_labels"] > 0).sum())
    gc, _, _, _ = _run_level(c, d)
    b, g, x = DT.level_rows(c)
    lab, m, n_i, a_i = D.level_positives(A, d["cls_labels"], d["matched"], DT.LEVEL_G, 0, n_lvl)
    _, _, q, _ = L.box_dist_loss(_t(b), _t(g), _t(x, torch.bfloat16), R, c["s"], c["kind"], c["rw"], c["dw"])
    quality = torch.zeros((N, n_lvl), device="cuda")
    quality[torch.from_numpy(n_i).cuda(), torch.from_numpy(a_i).cuda()] = q
    assert bool((q > 0).any())                                       # the point of the test: a quality that is not 0
    logits = _t(d["cls"][..., :A * Cc].reshape(N * n_lvl, Cc), torch.bfloat16).contiguous()
    _, pg = L.quality_focal_loss(logits, _t(np.ascontiguousarray(lab.reshape(-1))), quality.reshape(-1), ck, c["alpha"], c["gamma"],
                                 float(c["ls"]))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(gc.reshape(N * n_lvl, Cc)), _bits(pg))
    pos = torch.from_numpy(n_i * n_lvl + a_i).cuda()
    assert bool(pg[pos].any())


@pytest.mark.parametrize("name", ["coco", "tail"])
def test_unaligned_views_take_the_scalar_form_and_agree(hip, name):
    """Tensors that start 2 elements into their buffers (4-byte aligned): the scalar split. Results against float64 as
    usual, and the box half bit-identical to the vector form (the same quad code)."""
    import torch
    c = next(x for x in DT.LEVEL_CASES if x["name"] == name and x["cls_loss"] == "qfl")
    d, ref = DT.level_data(c), DT.level_ref(c)
    assert DT.level_route(c, off_reg=4, off_cls=4)[1] is False
    got = _run_level(c, d, shift=2)
    assert all(_check_level(c, d, got, ref))
    vec = _run_level(c, d)
    assert np.array_equal(_bits(got[1]), _bits(vec[1])) and torch.equal(got[2][1::3], vec[2][1::3]) and torch.equal(got[2][2::3], vec[2][2::3])


def test_graph_replay_follows_new_ground_truth(hip):
    import torch
    from mxdetection_amd.core import loss as L
    c = next(x for x in DT.LEVEL_CASES if x["id"].startswith("coco-vec-qfl-giou"))
    d = DT.level_data(c)
    N, H, W, A, Cc, R = c["shape"]
    gt_b = d["gt"].copy()
    gt_b[..., :4] += np.array([3.0, -2.0, 5.0, 4.0], np.float32)
    want = [_run_level(c, d, gt=_t(g)) for g in (d["gt"], gt_b)]
    assert not torch.equal(want[0][0], want[1][0]) and not torch.equal(want[0][1], want[1][1])
    ldc, ldr = DT.level_ld(c)
    bf = torch.bfloat16
    cls, reg, lab, anchors, matched = _t(d["cls"], bf), _t(d["reg"], bf), _t(d["cls_labels"]), _t(d["anchors"]), _t(d["matched"])
    gt = _t(d["gt"])
    gc, gr = torch.zeros((N, H, W, ldc), dtype=bf, device="cuda"), torch.zeros((N, H, W, ldr), dtype=bf, device="cuda")
    nparts = L.retina_loss_num_partials(N, H, W, A)
    part, out = torch.zeros((3 * nparts,), device="cuda"), torch.zeros((3,), device="cuda")
    nfg = torch.tensor([d["num_fg"]], dtype=torch.int32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap):
        graph.capture_begin(capture_error_mode="thread_local")
        L.retina_loss_level_dfl(cls, reg, A, Cc, lab, anchors, matched, gt, c["off"], c["cls_loss"], c["alpha"], c["gamma"], c["kind"], R,
                                c["s"], c["rw"], c["dw"], nfg, float(c["ls"]), gc, gr, part)
        L.loss_finalize(part, nparts, 3, out)
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(cap)
    real = 4 * (R + 1) * A
    for g, w in ((d["gt"], want[0]), (gt_b, want[1]), (d["gt"], want[0])):
        gt.copy_(torch.from_numpy(g))
        gc.fill_(3.0)
        gr[..., :real].fill_(3.0)
        part.fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gc[..., :A * Cc], w[0]) and torch.equal(gr[..., :real], w[1]) and torch.equal(part, w[2]) and torch.equal(out, w[3])


# ---------------------------------------------------------------------------------------------------------------------
DET_SHAPES, DET_STRIDES, DET_A, DET_C, DET_R = ((16, 20), (8, 10), (4, 5)), (8, 16, 32), 1, 5, 16


def _det_case(oracle, exact, seed=31, N=2):
    """cls [l][N,H,W,64], dist [l][N,H*W,A,4,R+1] (bf16-exact), base, info. exact: one-hot and two-equal-bin sides (E a
    multiple of 0.5); else general logits."""
    import _soft_nms_ref as S
    rng = np.random.default_rng(seed)
    cls, _, _, info = S.retina_case(oracle, rng, N, DET_A, DET_C, DET_SHAPES, DET_STRIDES, ld=64, nobj=8)
    base = [oracle.base_anchors(s, ratios=(1.0,), scales=(8.0,)) for s in DET_STRIDES]
    nb, dist = DET_R + 1, []
    for (H, W) in DET_SHAPES:
        if exact:
            x = np.full((N, H * W, DET_A, 4, nb), -200.0, np.float32)
            first = rng.integers(1, 6, (N, H * W, DET_A, 4))          # from bin 1: the other bins' e^-87 round away in Z and S
            second = np.where(rng.random(first.shape) < 0.5, first, first + 1)      # the same bin, or its neighbour: E = k or k + 0.5
            np.put_along_axis(x, first[..., None], 0.0, axis=-1)
            np.put_along_axis(x, second[..., None], 0.0, axis=-1)
        else:
            at = rng.uniform(0.5, 5.0, (N, H * W, DET_A, 4, 1))
            x = oracle.round_bf16((-1.5 * np.abs(np.arange(nb) - at) + 0.4 * rng.standard_normal((N, H * W, DET_A, 4, nb))).astype(np.float32))
        dist.append(x.astype(np.float32))
    return cls, dist, base, info


def _det_run(cls, dist, base, info, method, nms_thresh, pre_n=60, max_det=30, ld_reg=128):
    import torch
    from mxdetection_amd.core.evaluation import RetinaDetect
    N = cls[0].shape[0]
    tc = [_t(c).to(torch.bfloat16) for c in cls]
    tr = []
    for (H, W), x in zip(DET_SHAPES, dist):
        r = torch.full((N, H, W, ld_reg), 9.0, dtype=torch.bfloat16, device="cuda")
        r[..., :DET_A * 4 * (DET_R + 1)] = _t(x.reshape(N, H, W, -1)).to(torch.bfloat16)
        tr.append(r)
    det = RetinaDetect(DET_C, list(DET_STRIDES), [_t(b) for b in base], pre_nms_top_n=pre_n, score_thresh=0.05, nms_thresh=nms_thresh,
                       max_per_image=max_det, nms_method=method, soft_sigma=0.5, reg_max=DET_R)
    dets, num = det(tc, tr, _t(info))
    torch.cuda.synchronize()
    return dets.cpu().numpy(), num.cpu().numpy()


@pytest.mark.parametrize("method", ["hard", "linear", "gaussian"])
def test_retina_detect_dfl_bit_exact_where_the_decode_is(hip, oracle, method):
    cls, dist, base, info = _det_case(oracle, exact=True)
    N = cls[0].shape[0]
    E = D.expect_fp32(np.concatenate([x.reshape(-1, DET_R + 1) for x in dist]))[0]
    assert np.all(E * 2 == np.round(E * 2)) and len(np.unique(E)) >= 8                       # exact halves, several of them
    cls_o = [c[..., :DET_A * DET_C].reshape(N, -1) for c in cls]
    Hs, Ws = [s[0] for s in DET_SHAPES], [s[1] for s in DET_SHAPES]
    want, wnum, boxes, num = D.detect_ref(oracle, cls_o, dist, base, Hs, Ws, DET_STRIDES, info, DET_C, DET_R, 60, 0.05, 0.5, 30, method, 0.5)
    assert wnum.min() >= 10
    hard = D.detect_ref(oracle, cls_o, dist, base, Hs, Ws, DET_STRIDES, info, DET_C, DET_R, 60, 0.05, 2.0, 30, "hard")
    assert not np.array_equal(hard[0], want)                                                  # suppression happens in this case
    got, gnum = _det_run(cls, dist, base, info, method, 0.5)
    assert np.array_equal(gnum, wnum)
    assert np.array_equal(got[..., 5], want[..., 5])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for n in range(N):                                                                        # clipped as mxdet_decode_clip clips
        k = int(gnum[n])
        assert got[n, :k, 0].min() >= 0 and got[n, :k, 2].max() <= info[n, 1] - 1 and got[n, :k, 3].max() <= info[n, 0] - 1
    assert any((got[n, :int(gnum[n]), :4] == 0).any() or (got[n, :int(gnum[n]), 2] == info[n, 1] - 1).any() for n in range(N))


def test_retina_detect_dfl_general_logits(hip, oracle):
    """Nothing suppressed (no IoU exceeds 1): order and classes exact, boxes within the decode bound of the float64 decode."""
    cls, dist, base, info = _det_case(oracle, exact=False, seed=37)
    N = cls[0].shape[0]
    cls_o = [c[..., :DET_A * DET_C].reshape(N, -1) for c in cls]
    Hs, Ws = [s[0] for s in DET_SHAPES], [s[1] for s in DET_SHAPES]
    want, wnum, _, _ = D.detect_ref(oracle, cls_o, dist, base, Hs, Ws, DET_STRIDES, info, DET_C, DET_R, 60, 0.05, 1.0, 30, "hard", decode="f64")
    got, gnum = _det_run(cls, dist, base, info, "hard", 1.0)
    assert np.array_equal(gnum, wnum) and wnum.min() >= 20
    assert np.array_equal(got[..., 4:].view(np.uint32), want[..., 4:].view(np.uint32))       # scores, classes, order
    err = np.abs(got[..., :4].astype(np.float64) - want[..., :4])
    print("decoded boxes: max |got - float64| = %.3e px (bound %.3e)" % (err.max(), DT.ATOL_DECODE))
    assert err.max() <= DT.ATOL_DECODE
