"""The data-pipeline kernels of csrc/preprocess.hip on the case tables of tests/test_preprocess_cases_cpu.py: every case
through mxdet_image_preprocess / mxdet_polygon_masks into prefilled, guarded outputs, asserted against the C oracle's
bits exactly, against the fp64 resample within the derived bound B, against the exact polygon masks outside the ambiguous
set, and against the same identities the CPU module proves for the oracle. The bounds, the references and the reasons for
each case are in that module's docstring; nothing here is derived from what the kernels return."""
import ctypes as C

import numpy as np
import pytest
import torch

import _preprocess_ref as ref
import test_preprocess_cases_cpu as K
from mxdetection_amd._lib import ImageDescT, MxdetError, check, ptr, stream_ptr
from mxdetection_amd.process_data import transform as T

pytestmark = pytest.mark.gpu

GUARD = 64                   # elements on either side of a guarded output (64 B / 128 B: the view stays 16-byte aligned)
NAN_BITS = 0x7FC1            # a bf16 NaN: no kernel output, so an element still holding it was never written
IMG_SENTINEL, MASK_SENTINEL, MASK_PREFILL = 0x5A5A, 0xA5, 0xFF
ZERO3, ONE3 = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def _guarded(shape, dtype, prefill, sentinel):
    """(view, intact): a contiguous `shape` view full of `prefill` inside a larger allocation of sentinels."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
    view = whole[GUARD:GUARD + n].view(shape)
    view.fill_(prefill)

    def intact():
        return bool((whole[:GUARD] == sentinel).all()) and bool((whole[GUARD + n:] == sentinel).all())
    return view, intact


def _image_out(N, Hp, Wp):
    return _guarded((max(N, 1), 3, Hp, Wp), torch.int16, NAN_BITS, IMG_SENTINEL)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _f3(v):
    return (C.c_float * 3)(*v)


def _call(hip, case, frames, mean, std, swap, out, Wp=None):
    """mxdet_image_preprocess on explicit destination sizes and inverse scales; `frames` are device views."""
    N = len(frames)
    descs = (ImageDescT * max(N, 1))()
    for d, f, t in zip(descs, case["frames"], frames):
        assert t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == (f["sh"], f["sw"], 3)
        d.src, d.src_h, d.src_w, d.dst_h, d.dst_w, d.flip, d.inv_scale = t.data_ptr(), f["sh"], f["sw"], f["dh"], f["dw"], \
            int(f["flip"]), f["inv"]
    out_ptr = out if isinstance(out, C.c_void_p) else ptr(out)
    check(hip.load().mxdet_image_preprocess(C.cast(descs, C.c_void_p), N, case["Hp"], case["Wp"] if Wp is None else Wp,
                                            C.cast(_f3(mean), C.c_void_p), C.cast(_f3(std), C.c_void_p), int(swap), out_ptr,
                                            stream_ptr()), "image_preprocess")


def _upload(name, case=None, srcs=None):
    """The case's source buffer on the device (from its host buffer, or re-laid from `srcs`), and its frame views."""
    case = K.RESIZE_CASES[name] if case is None else case
    buf, starts = K.host_buffer(name)
    if srcs is not None:
        for f, s, im in zip(case["frames"], starts, srcs):
            buf[s:s + im.size] = im.reshape(-1)
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 16 == 0              # so that the leads are those the CPU module computed from the layout
    return K.views(dev, case, starts)


def _run(hip, case, frames, mean, std, swap):
    out, intact = _image_out(len(frames), case["Hp"], case["Wp"])
    _call(hip, case, frames, mean, std, swap, out)
    torch.cuda.synchronize()
    assert intact(), "a sentinel around the image batch was overwritten"
    return _u16(out)


@pytest.mark.parametrize("name", list(K.RESIZE_CASES))
def test_resize_case(hip, oracle, name):
    case = K.RESIZE_CASES[name]
    buf, starts = K.host_buffer(name)
    srcs = K.views(buf, case, starts)
    frames = _upload(name)
    bits = _run(hip, case, frames, ZERO3, ONE3, False)
    vs = K.grey_levels(case, bits)               # every element written: integral grey levels inside, +0 bits around
    K.check_bound(name, case, srcs, vs, who="kernel")
    K.check_identities(name, case, srcs, vs)
    assert np.array_equal(bits, K.oracle_run(oracle, case, srcs, ZERO3, ONE3, False))
    assert np.array_equal(bits, _run(hip, case, frames, ZERO3, ONE3, False)), "two runs differ"
    for mean, std in K.NORM_SETS:
        got = _run(hip, case, frames, mean, std, False)
        assert np.array_equal(got, K.expected_bits(case, vs, mean, std)), (name, std)
        assert np.array_equal(got, K.oracle_run(oracle, case, srcs, mean, std, False))


@pytest.mark.parametrize("name", K.MIRROR_CASES)
def test_flip_is_the_mirrored_source(hip, name):
    case = K.RESIZE_CASES[name]
    buf, starts = K.host_buffer(name)
    srcs = K.views(buf, case, starts)
    mc, ms = K.mirrored(case, srcs)
    a = _run(hip, case, _upload(name), K.PROD_MEAN, K.ALT_STD, False)
    assert np.array_equal(a, _run(hip, mc, _upload(name, mc, ms), K.PROD_MEAN, K.ALT_STD, False))


@pytest.mark.parametrize("name", K.SWAP_CASES)
def test_swap_is_the_reversed_channel_order(hip, name):
    case = K.RESIZE_CASES[name]
    buf, starts = K.host_buffer(name)
    srcs = K.views(buf, case, starts)

    def run(case, srcs, mean, std, swap):
        return _run(hip, case, _upload(name, case, srcs), mean, std, swap)
    a = run(case, srcs, K.PROD_MEAN, K.ALT_STD, True)
    for other in K.swap_equivalents(run, case, srcs):
        assert np.array_equal(a, other)
    sw = K.grey_levels(case, run(case, srcs, ZERO3, ONE3, True))
    K.check_bound(name + "/swap", case, srcs, sw, swap=True, who="kernel")


def test_narrow_frame_batched_with_a_wide_one(hip):
    """A batch takes its route from its widest frame: the 40-wide frame goes through the direct form next to a 20479-wide
    one and through the row-staged form alone, and must not change by a bit."""
    both, alone = K.RESIZE_CASES["wide_and_narrow"], K.RESIZE_CASES["narrow_alone"]
    assert K.route(both) == "direct" and K.route(alone) == "staged"
    a = _run(hip, both, _upload("wide_and_narrow"), K.PROD_MEAN, K.ALT_STD, True)
    b = _run(hip, alone, _upload("narrow_alone"), K.PROD_MEAN, K.ALT_STD, True)
    assert np.array_equal(a[1], b[0]) and a[1].any()


@pytest.mark.parametrize("name", ["lds_staged_edge", "wide_20478", "mixed_scales", "wch257_up", "n64_tiny"])
def test_staged_and_direct_forms_agree(hip, name):
    """Both forms on the same inputs: at the LDS limit (the row-staged form's largest allocation), on the widest frame,
    and on the cases with every lead and tail."""
    case = K.RESIZE_CASES[name]
    frames = _upload(name)
    a = _run(hip, case, frames, K.PROD_MEAN, K.ALT_STD, True)
    hip.load().mxdet_debug_preprocess_direct(1)
    try:
        b = _run(hip, case, frames, K.PROD_MEAN, K.ALT_STD, True)
    finally:
        hip.load().mxdet_debug_preprocess_direct(0)
    assert np.array_equal(a, b)


def test_refused_preprocess_calls_leave_the_output_untouched(hip):
    def untouched(out, intact):
        torch.cuda.synchronize()
        return intact() and bool((out == NAN_BITS).all())
    tiny = dict(Hp=4, Wp=8, frames=K.N65_FRAMES)
    buf, starts = K.host_buffer("n65", frames=K.N65_FRAMES)
    frames = K.views(torch.from_numpy(buf).cuda(), tiny, starts)
    out, intact = _image_out(K.MAX_BATCH + 1, 4, 8)
    # the descriptor table holds MAX_BATCH entries: one more is refused before anything is read
    with pytest.raises(MxdetError, match=r"outside 0\.\."):
        _call(hip, tiny, frames, ZERO3, ONE3, False, out)
    assert untouched(out, intact)
    # N = 0 is accepted and writes nothing
    _call(hip, dict(tiny, frames=[]), [], ZERO3, ONE3, False, out)
    assert untouched(out, intact)
    one = dict(tiny, frames=tiny["frames"][:1])
    with pytest.raises(MxdetError, match="multiple of 8"):
        _call(hip, one, frames[:1], ZERO3, ONE3, False, out, Wp=12)
    assert untouched(out, intact)
    with pytest.raises(MxdetError, match="16-byte aligned"):
        _call(hip, one, frames[:1], ZERO3, ONE3, False, C.c_void_p(out.data_ptr() + 2))
    assert untouched(out, intact)
    # and the same output is written in full by the call that is accepted
    _call(hip, dict(tiny, frames=tiny["frames"][:K.MAX_BATCH]), frames[:K.MAX_BATCH], ZERO3, ONE3, False, out)
    torch.cuda.synchronize()
    assert intact() and not bool((out[:K.MAX_BATCH] == NAN_BITS).any()) and bool((out[K.MAX_BATCH] == NAN_BITS).all())


# ---- polygons -----------------------------------------------------------------------------------------------------------

def _mask_out(G, H, W):
    return _guarded((1, G, H, W), torch.uint8, MASK_PREFILL, MASK_SENTINEL)


def _masks(hip, packed, G, H, W):
    out, intact = _mask_out(G, H, W)
    T.polygon_masks(*[torch.from_numpy(a).cuda() for a in packed], 1, G, H, W, out=out)
    torch.cuda.synchronize()
    assert intact(), "a sentinel around the masks was overwritten"
    got = out.cpu().numpy()[0]
    assert got.max() <= 1, "a mask byte is neither 0 nor 1 (never written, or not a byte per pixel)"
    return got


@pytest.mark.parametrize("name", list(K.POLY_CASES))
def test_polygon_case(hip, oracle, name):
    c = K.POLY_CASES[name]
    G, H, W = len(c["insts"]), c["H"], c["W"]
    packed = K.polygon_reference(name)[0]
    got = _masks(hip, packed, G, H, W)
    K.check_polygon(name, got, who="kernel")
    assert np.array_equal(got, oracle.polygon_masks(*packed, G, H, W))
    assert np.array_equal(got, _masks(hip, packed, G, H, W)), "two runs differ"


def test_refused_polygon_calls_leave_the_output_untouched(hip):
    packed = [torch.from_numpy(a).cuda() for a in T.pack_polygons([[[K._rect(0, 0, 3, 3)]]], 1, 1)]
    out, intact = _guarded((1, 1, 2, 6), torch.uint8, MASK_PREFILL, MASK_SENTINEL)
    with pytest.raises(MxdetError, match="multiple of 4"):
        T.polygon_masks(*packed, 1, 1, 2, 6, out=out)
    torch.cuda.synchronize()
    assert intact() and bool((out == MASK_PREFILL).all())
    G = 65536                                           # N * G past the grid's z limit
    first = torch.ones(G + 1, dtype=torch.int32, device="cuda")
    first[0] = 0
    out, intact = _guarded((1, G, 1, 4), torch.uint8, MASK_PREFILL, MASK_SENTINEL)
    with pytest.raises(MxdetError, match="exceeds the grid"):
        T.polygon_masks(packed[0], packed[1], first, 1, G, 1, 4, out=out)
    torch.cuda.synchronize()
    assert intact() and bool((out == MASK_PREFILL).all())


# ---- one convention for image, box, polygon and keypoint -----------------------------------------------------------------

@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("scale", K.CONV_SCALES)
def test_image_box_polygon_keypoint_agree(hip, scale, flip):
    case, im, box, poly, kp = K.convention_case(scale, flip)
    bits = _run(hip, case, [torch.from_numpy(im).cuda()], ZERO3, ONE3, False)
    v = K.grey_levels(case, bits)[0][..., 0]
    packed = T.pack_polygons([[[poly]]], 1, 1)
    mask = _masks(hip, packed, 1, case["Hp"], case["Wp"])[0]
    assert np.array_equal(mask, ref.polygon_mask_exact(*packed, 1, case["Hp"], case["Wp"])[0][0])
    K.check_convention(scale, flip, case, box, kp, v, mask)
