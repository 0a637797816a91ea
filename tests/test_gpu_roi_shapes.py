"""RoIAlign (csrc/roi_align.hip: forward, scatter backward, gather backward in its segment and table forms), mask_target and
mask_paste (csrc/mask.hip) through ops/roi_align.py and core/mask.py, at the shapes and on the lines where their branches
leave the simplest arm. Inputs, and the CPU proof that each case reaches its branch: tests/test_roi_cases_cpu.py.
Reference: tests/_roi_ref.py (float64, written from the definitions; it agrees with the C oracle, checked on the CPU).

Tolerances, the ones the project asserts for these kernels already, here against float64:
  bf16 outputs (forward, gather maps)   |got - ref| <= 2^-7 |ref| + 2^-7 rms(ref), no element exempt
  scatter form (fp32 atomics)           rtol 1e-5, atol 1e-5 of the gradient map's scale
  gather with accumulate                rtol 2^-7, atol 2e-5 max|grad| + 2^-8 max|sum|
  mask_target / mask_paste              equal, outside the 1e-5 band around the threshold that the case tables bound
Every case prints achieved error / bound.
"""
import ctypes as C

import numpy as np
import pytest

import test_roi_cases_cpu as T
from test_gpu_keypoint import _guarded, _guards_intact

pytestmark = pytest.mark.gpu


def _dev(c):
    import torch
    return dict(rois=torch.from_numpy(c["rois"]).cuda(), levels=torch.from_numpy(c["levels"]).cuda(), gout=c["gout"].cuda(),
                feats=[f.cuda() for f in c["feats"]])


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16).cpu()


def _run_gather(c, d, maps, accumulate=False, table=False, **kw):
    import torch
    from mxdetection_amd import _lib
    from mxdetection_amd.ops.roi_align import roi_align_backward_gather
    lib = _lib.load()
    if table:
        lib.mxdet_debug_set_tuning(_lib.TUNING_KEYS["ROI_TABLE"], 1)
    try:
        roi_align_backward_gather(maps, c["scales"], d["rois"], d["levels"], d["gout"], c["sr"], c["lvl_min"],
                                  accumulate=accumulate, **kw)
        torch.cuda.synchronize()
    finally:
        if table:
            lib.mxdet_debug_set_tuning(_lib.TUNING_KEYS["ROI_TABLE"], -1)
    return maps


def _filled(c, value):
    import torch
    return [torch.full((c["N"], H, W, c["C"]), value, dtype=torch.bfloat16, device="cuda") for H, W in c["maps"]]


def _bf16_bound(want):
    want = np.asarray(want, np.float64)
    return T.BF16_REL * np.abs(want) + T.BF16_REL * np.sqrt((want ** 2).mean())


def _check_gather_overwrite(c, got, want, tag):
    for l, (g, w) in enumerate(zip(got, want)):
        g, w = g.float().cpu().numpy(), w.numpy()
        T.close_bf16(g, w, "%s level %d" % (tag, l))
        assert not g[w == 0].any(), "%s level %d: an element no roi reaches must be written as zero" % (tag, l)
    if c["exact"]:
        # dyadic weights and a gradient of 1: every fp32 sum is exact, so the map is the rounded reference, bit for bit
        import torch
        for g, w in zip(got, want):
            assert torch.equal(g[..., 0].cpu(), w[..., 0].to(torch.bfloat16)), tag + ": constant channel is not exact"


@pytest.mark.parametrize("name", T.GATHER_NAMES)
def test_gather_backward_both_forms(hip, name):
    """Sentinel-filled maps fully overwritten and within the bound, in the default route and in the forced table form; the
    two forms agree; two runs and prepare + prepared give the same bits; accumulate adds within its bound and leaves the
    pixels the reference does not touch bit for bit."""
    import torch
    from mxdetection_amd.ops.roi_align import roi_align_backward_gather_prepare, roi_align_backward_gather_workspace
    c = T.gather_case(name)
    R = c["rois"].shape[0]
    want = T.ref_backward("gather", name)
    route = T.plan(c["maps"], R, c["PW"], c["sr"])["route"]
    d = _dev(c)
    first = _run_gather(c, d, _filled(c, 7.0))
    _check_gather_overwrite(c, first, want, "%s %s form" % (name, route))
    again = _run_gather(c, d, _filled(c, float("nan")))
    for a, b in zip(first, again):
        assert torch.equal(_bits(a), _bits(b)), name + ": two runs differ"
    ws = roi_align_backward_gather_workspace(first, c["scales"], R, c["lvl_min"])
    roi_align_backward_gather_prepare(first, c["scales"], d["rois"], d["levels"], (c["PH"], c["PW"]), c["sr"], c["lvl_min"], ws)
    pre = _run_gather(c, d, _filled(c, 3.0), workspace=ws, prepared=True)
    for a, b in zip(first, pre):
        assert torch.equal(_bits(a), _bits(b)), name + ": prepare + prepared differs from the one-call form"
    if route == "segment":
        tab = _run_gather(c, d, _filled(c, 7.0), table=True)
        _check_gather_overwrite(c, tab, want, name + " table form (forced)")
        for l, (a, t, w) in enumerate(zip(first, tab, want)):
            diff = np.abs(a.float().cpu().numpy().astype(np.float64) - t.float().cpu().numpy())
            bound = _bf16_bound(w.numpy())
            print("%s level %d: segment vs table, max difference / bound = %.3f"
                  % (name, l, float((diff / np.where(bound > 0, bound, 1.0)).max())))
            assert np.all(diff <= bound), name + ": the two forms disagree"
    # accumulate
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(m.shape, generator=g).to(torch.bfloat16) for m in first]
    for table in ([False, True] if route == "segment" and name.startswith("round") else [False]):
        acc = _run_gather(c, d, [b.cuda() for b in base], accumulate=True, table=table)
        for l, (a, b0, w) in enumerate(zip(acc, base, want)):
            w = w.numpy()
            total = b0.double().numpy() + w
            bound = 2.0 ** -7 * np.abs(total) + 2e-5 * np.abs(w).max() + 2.0 ** -8 * np.abs(total).max()
            err = np.abs(a.float().cpu().numpy() - total)
            print("%s level %d accumulate%s: max error / bound = %.3f" % (name, l, " (table)" if table else "",
                                                                           float((err / bound).max())))
            assert np.all(err <= bound)
            untouched = torch.from_numpy((w == 0).all(axis=-1))
            assert torch.equal(_bits(a)[untouched], _bits(b0)[untouched]), name + ": an untouched pixel changed"


def test_gather_backward_without_rois(hip):
    """R = 0 is the limit of the definition: OK, zero maps (overwrite) or untouched maps (accumulate); rois, levels and
    grad_out may be null, and the workspace size asked for R = 0 is the one the entry demands."""
    import torch
    from mxdetection_amd._lib import check, ptr, stream_ptr
    from mxdetection_amd.ops import roi_align as RA
    c = T.gather_case("r0")
    lib = hip.load()
    maps = _filled(c, 7.0)
    desc = RA._pyr(maps, c["scales"], c["lvl_min"])
    need0 = lib.mxdet_roi_align_bwd_gather_workspace_bytes(C.byref(desc), c["N"], 0)
    assert need0 > 0 and need0 == lib.mxdet_roi_align_bwd_gather_workspace_bytes(C.byref(desc), c["N"], 1)
    assert lib.mxdet_roi_align_bwd_gather_workspace_bytes(C.byref(desc), c["N"], -1) == 0
    ws = torch.empty((need0,), dtype=torch.uint8, device="cuda")
    for fn in (lib.mxdet_roi_align_bwd_gather, lib.mxdet_roi_align_bwd_gather_prepared):
        for accumulate in (0, 1):
            maps = _filled(c, 7.0)
            desc = RA._pyr(maps, c["scales"], c["lvl_min"])
            check(fn(C.byref(desc), c["N"], c["C"], None, None, 0, 7, 7, 2, None, accumulate, ptr(ws), ws.numel(), stream_ptr()),
                  "roi_align_bwd_gather R=0")
            torch.cuda.synchronize()
            for m in maps:
                assert bool((m == 7.0).all()) if accumulate else not bool(m.any())
    check(lib.mxdet_roi_align_bwd_gather_prepare(C.byref(desc), c["N"], None, None, 0, 7, 7, 2, ptr(ws), ws.numel(), stream_ptr()),
          "roi_align_bwd_gather_prepare R=0")
    # an empty grad_out still says how many bins there are: 16 columns are the table form's, with or without rois
    d = _dev(c)
    wide = torch.empty((0, 2, 16, c["C"]), dtype=torch.bfloat16, device="cuda")
    out = _filled(c, 7.0)
    RA.roi_align_backward_gather(out, c["scales"], d["rois"], d["levels"], wide, 2, c["lvl_min"])
    torch.cuda.synchronize()
    assert not any(bool(m.any()) for m in out)


@pytest.mark.parametrize("name", T.FORWARD_NAMES)
def test_forward(hip, name):
    import torch
    from mxdetection_amd.ops.roi_align import roi_align_forward
    c = T.forward_case(name)
    want = T.ref_forward("forward", name).numpy()
    d = _dev(c)
    R = c["rois"].shape[0]
    whole, out = _guarded((R, c["PH"], c["PW"], c["C"]), torch.bfloat16, 776.0)
    roi_align_forward(d["feats"], c["scales"], d["rois"], d["levels"], (c["PH"], c["PW"]), c["sr"], c["lvl_min"], out=out)
    torch.cuda.synchronize()
    assert _guards_intact(whole, 776.0)
    got = out.float().cpu().numpy()
    T.close_bf16(got, want, "forward " + name)
    inside = np.array([T.fully_inside(g) for g in T.geoms(c)])
    assert np.all(got[inside][..., 0] == 1.0), "the constant channel of a fully-inside roi must be exactly 1"
    if c["exact"]:
        assert np.array_equal(got[..., 0], T.bf16(want[..., 0]))


@pytest.mark.parametrize("name", T.SCATTER_NAMES)
def test_scatter_backward_accumulates(hip, name):
    import torch
    from mxdetection_amd.ops.roi_align import roi_align_backward
    c = T.scatter_case(name)
    want = T.ref_backward("scatter", name)
    base = T.scatter_base(c)
    d = _dev(c)
    acc = [b.clone().cuda() for b in base]
    roi_align_backward(acc, c["scales"], d["rois"], d["levels"], d["gout"], c["sr"], c["lvl_min"])
    torch.cuda.synchronize()
    for l, (a, b0, w) in enumerate(zip(acc, base, want)):
        T.close_scatter(a.cpu().numpy(), b0.double().numpy() + w.numpy(), float(w.abs().max()), "scatter %s level %d" % (name, l))


def _mask_target_check(c):
    import torch
    from mxdetection_amd.core.mask import mask_target
    R, S = c["rois"].shape[0], c["S"]
    tw, tg = _guarded((R, S, S), torch.uint8, 9)
    cw, cls = _guarded((R,), torch.int32, -77)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    mask_target(dev(c["rois"]), dev(c["matched"]), dev(c["labels"]), dev(c["masks"]), S, out=(tg, cls))
    torch.cuda.synchronize()
    assert _guards_intact(tw, 9) and _guards_intact(cw, -77)
    got = tg.cpu().numpy()
    assert got.max() <= 1 and np.array_equal(cls.cpu().numpy(), c["cls"])
    wrong = (got != c["target"]) & c["compare"]
    print("mask_target S=%d G=%d: %d of %d pixels compared, %d differ" % (S, c["G"], int(c["compare"].sum()), got.size,
                                                                         int(wrong.sum())))
    assert not wrong.any(), np.argwhere(wrong)[:8]


@pytest.mark.parametrize("G", T.MT_G)
@pytest.mark.parametrize("S", T.MT_SIZES)
def test_mask_target(hip, S, G):
    _mask_target_check(T.mask_target_case(S, G))


def test_mask_target_on_the_tie(hip):
    c = T.mask_target_dyadic()
    assert c["compare"].all()
    _mask_target_check(c)


@pytest.mark.parametrize("S,Cpad,frame,thresh", T.MP_CASES, ids=T.MP_IDS)
def test_mask_paste(hip, S, Cpad, frame, thresh):
    import torch
    from mxdetection_amd.core.mask import mask_paste
    c = T.mask_paste_case(S, Cpad, frame, thresh)
    H, W = frame
    R = c["dets"].shape[0]
    whole, out = _guarded((R, H, W), torch.uint8, 9)
    mask_paste(torch.from_numpy(c["logits"]).cuda().to(torch.bfloat16), torch.from_numpy(c["dets"]).cuda(), H, W, thresh, out=out)
    torch.cuda.synchronize()
    assert _guards_intact(whole, 9)
    got = out.cpu().numpy()
    wrong = (got != c["mask"]) & c["compare"]
    print("mask_paste S=%d Cpad=%d %dx%d thresh=%g: %d of %d pixels compared, %d differ"
          % (S, Cpad, H, W, thresh, int(c["compare"].sum()), got.size, int(wrong.sum())))
    assert got.max() <= 1 and not wrong.any(), np.argwhere(wrong)[:8]
