"""Case tables for the data-pipeline kernels of csrc/preprocess.hip (image_preprocess_rows_kernel, image_preprocess_kernel,
polygon_masks_kernel): the inputs of tests/test_gpu_preprocess_edges.py and, proven here without a GPU, (a) that each
named case reaches the branch it is named after, computed from its shapes, (b) that the project's C oracle -- the bits
the kernels must reproduce -- stays within a derived bound of the references of tests/_preprocess_ref.py, which share no
arithmetic with it, and (c) the identities and conventions that pin the half-pixel centre, the flip and the channel swap.

B -- the resize bound, in grey levels
-------------------------------------
Per axis the kernel rounds the source coordinate to fp32, splits it into an index and a fraction f, and rounds 2048 (1-f)
and 2048 f to integers a0, a1 (b0, b1 vertically): a = 2048 alpha + e with |e| <= 1/2 + 2^-14 =: EC (the 2^-14 covers the
fp32 rounding of 1 - f). Let h0, h1 be the exact horizontal blends of the two rows with the weights alpha (taken at the
fp32 coordinate), E = beta0 h0 + beta1 h1, p <= 255 the grey levels.
  t  = p0 a0 + p1 a1             = 2048 h + dt,        |dt| <= 255 * 2 EC
  u  = t >> 4                    = 128 h + dt/16 - phi, 0 <= phi <= 15/16;   u <= 255 * 2049 / 16
  S  = (b0 u0 >> 16) + (b1 u1 >> 16) = (b0 u0 + b1 u1) / 65536 - psi,  0 <= psi < 2
  b0 u0 + b1 u1 = 2048 * 128 * E + 2048 (beta0 (dt0/16 - phi0) + beta1 (dt1/16 - phi1)) + (g0 u0 + g1 u1),  |g| <= EC
so, with beta0 + beta1 = 1,
  S - 4 E in [ -(255*2*EC/16 + 15/16)/32 - 2*EC*(255*2049/16)/65536 - 2 ,  (255*2*EC/16)/32 + 2*EC*(255*2049/16)/65536 ]
          =  [ -3.0257 , +0.9964 ]
  v = (S + 2) >> 2 = (S + 2)/4 - rho, 0 <= rho <= 3/4   =>   v - E in [ -1.0065 , +0.7491 ].
B0 = 1.0065 grey levels (the floors only ever pull down, which is why the low side is the larger; a symmetric count of
the same terms gives the "little under 1.3" one gets by adding magnitudes). The remaining term is the fp32 coordinate:
bilinear interpolation is 255-Lipschitz per axis in the (clamped) coordinate, and the coordinate is rounded to fp32 once,
so E moves by at most 255 (ulp32(src_w)/2 + ulp32(src_h)/2): 0.016 for a 2048-wide source, 0.25 for a 20479-wide one.
  B = B0 + 255 * (ulp32(src_w) + ulp32(src_h)) / 2.
B < 2 in every case, so the integer v is within one grey level of round(exact) or equal to it.

2x upsampling (inv_scale = 1/2): the coefficients are 512 / 1536 exactly and t, u are exact, but the two `>> 16` still
floor A/4 and B/4 separately (A + B = 16 * exact), so v = floor(exact + 1/2) exactly when the source levels are multiples
of 4 (A, B multiples of 4) and v in {floor(exact + 1/2) - 1, floor(exact + 1/2)} otherwise -- OpenCV's own behaviour, e.g.
the 2x2 source [[0, 1], [1, 2]] has exact = 1 at its centre sample and blends to 0. Both statements are asserted.

delta -- the polygon kernel's fp32 error in the crossing, in pixels
-------------------------------------------------------------------
xi = a.x + ((py - a.y) * (b.x - a.x)) / (b.y - a.y), each operation rounded once to fp32 (u = 2^-24; py = y + 1/2 and the
vertices are exact). With Q the exact quotient, |Q| <= |b.x - a.x| because py lies between a.y and b.y:
  three subtractions, one product, one quotient:  |q - Q| <= ((1+u)^4 / (1-u) - 1) |Q| <= 5.0001 u |b.x - a.x|
  the final addition:                             |xi_fp32 - (a.x + q)| <= u |a.x + q|,   |xi| <= max(|a.x|, |b.x|)
  delta = 2^-24 * (6 * max_edges |b.x - a.x| + max_vertices |x|)      (6 absorbs the second-order terms)
A case whose straddling edges are all vertical has b.x - a.x = 0, q = 0 and xi = a.x exactly: delta = 0 and no pixel is
ambiguous, even one whose centre lies on the edge (margin 0: the strict `<` decides, identically in every arithmetic).
A pixel is ambiguous when delta > 0 and margin <= delta.
"""
import zlib

import numpy as np
import pytest

import _preprocess_ref as ref
from mxdetection_amd.process_data import transform as T

# ---- resize: bound ------------------------------------------------------------------------------------------------------

EC = 0.5 + 2.0 ** -14
_U_MAX = 255.0 * 2049.0 / 16.0
S_LOW = -((255.0 * 2 * EC / 16 + 15.0 / 16) / 32 + 2 * EC * _U_MAX / 65536 + 2.0)
S_HIGH = (255.0 * 2 * EC / 16) / 32 + 2 * EC * _U_MAX / 65536
V_LOW, V_HIGH = S_LOW / 4 + 0.5 - 0.75, S_HIGH / 4 + 0.5
B0 = max(-V_LOW, V_HIGH)


def bound(sh, sw):
    """B of the module docstring for a source of sh x sw pixels."""
    return B0 + 255.0 * float(np.spacing(np.float32(sw)) + np.spacing(np.float32(sh))) / 2


PROD_MEAN, PROD_STD = T.PIXEL_MEANS, T.PIXEL_STDS
ALT_STD = (58.4, 57.1, 57.4)
MAX_BATCH = 64                      # MXDET_PREPROCESS_MAX_BATCH
LDS_LIMIT = 60 * 1024
W_STAGED, W_DIRECT = 10239, 10240   # the widest source the row-staged form takes, and the first it does not

# ---- resize: cases ------------------------------------------------------------------------------------------------------


def F(sh, sw, dh, dw, inv, flip=False, off=0):
    return dict(sh=sh, sw=sw, dh=dh, dw=dw, inv=float(inv), flip=bool(flip), off=off)


def _tiny_batch(n):
    shapes = ((1, 1), (2, 3), (3, 2), (1, 5), (3, 3), (2, 1), (3, 6))
    fr = []
    for k in range(n):
        sh, sw = shapes[k % len(shapes)]
        inv = (1.0, 0.75, 1.5)[k % 3]
        fr.append(F(sh, sw, max(1, min(4, int(round(sh / inv)))), max(1, min(8, int(round(sw / inv)))), inv, k % 2 == 1, k % 4))
    return fr


RESIZE_CASES = {
    # name: Hp, Wp, frames; `fill` = what the frames hold (noise unless named)
    "wch1_identity": dict(Hp=8, Wp=8, frames=[F(5, 7, 5, 7, 1.0, False, 1)]),
    "wch1_identity_flip": dict(Hp=8, Wp=8, frames=[F(5, 7, 5, 7, 1.0, True, 3)]),
    "wch256_up": dict(Hp=16, Wp=2048, frames=[F(7, 1021, 14, 2041, 1021.0 / 2041.0, True, 2)]),
    "wch257_up": dict(Hp=12, Wp=2056, frames=[F(5, 1030, 10, 2056, 1030.0 / 2056.0, False, 3)]),
    "wch320_down": dict(Hp=10, Wp=2560, frames=[F(9, 3000, 8, 2559, 3000.0 / 2559.0, True, 0)]),
    "lds_staged_edge": dict(Hp=2, Wp=2560, frames=[F(3, W_STAGED, 1, 2559, W_STAGED / 2559.0, False, 1)]),
    "lds_direct_edge": dict(Hp=2, Wp=2560, frames=[F(3, W_DIRECT, 1, 2559, W_DIRECT / 2559.0, True, 2)]),
    "wide_20478": dict(Hp=2, Wp=2560, frames=[F(3, 20478, 1, 2559, 20478.0 / 2559.0, False, 0)]),
    "wide_20479": dict(Hp=2, Wp=2560, frames=[F(3, 20479, 1, 2559, 20479.0 / 2559.0, True, 3)]),
    "wide_and_narrow": dict(Hp=12, Wp=2560, frames=[F(3, 20479, 1, 2559, 20479.0 / 2559.0, False, 1),
                                                     F(5, 40, 10, 80, 0.5, True, 2)]),
    "narrow_alone": dict(Hp=12, Wp=2560, same_as=("wide_and_narrow", 1), frames=[F(5, 40, 10, 80, 0.5, True, 2)]),
    "mixed_scales": dict(Hp=16, Wp=64, frames=[F(9, 13, 14, 21, 0.625, False, 0), F(11, 18, 5, 8, 2.3, True, 1),
                                                F(7, 23, 11, 37, 0.625, True, 2), F(15, 40, 15, 40, 1.0, False, 3),
                                                F(13, 57, 4, 17, 3.3, False, 1), F(3, 5, 16, 27, 0.19, True, 3)]),
    "up2x_mult4": dict(Hp=16, Wp=32, fill="mult4", frames=[F(7, 13, 14, 26, 0.5, False, 1), F(5, 9, 10, 18, 0.5, True, 2)]),
    "up2x_noise": dict(Hp=16, Wp=32, frames=[F(7, 13, 14, 26, 0.5, False, 3), F(5, 9, 10, 18, 0.5, True, 0)]),
    "up2x_floor_pair": dict(Hp=8, Wp=8, fill="floor_pair", frames=[F(2, 2, 4, 4, 0.5, False, 0)]),
    "one_pixel": dict(Hp=8, Wp=16, frames=[F(1, 1, 7, 13, 1.0 / 13.0, False, 1), F(1, 1, 3, 9, 2.0, True, 2)]),
    "n64_tiny": dict(Hp=4, Wp=8, frames=_tiny_batch(MAX_BATCH)),
}
N65_FRAMES = _tiny_batch(MAX_BATCH + 1)        # one more than the batch table holds: the call must be refused

IDENTITY_CASES = ("wch1_identity", "wch1_identity_flip")
MIRROR_CASES = ("mixed_scales", "wch257_up", "wch320_down", "lds_staged_edge")      # flip == no flip of the mirrored source
SWAP_CASES = ("mixed_scales", "wch256_up", "lds_direct_edge")                     # swap_rb == reversed channels, mean, std
NORM_SETS = ((PROD_MEAN, PROD_STD), (PROD_MEAN, ALT_STD))


def layout(case):
    """Byte position of each frame inside the case's one source buffer: 16-byte slots, then the frame's own offset."""
    starts, pos = [], 0
    for f in case["frames"]:
        starts.append(pos + f["off"])
        pos = (pos + f["off"] + f["sh"] * f["sw"] * 3 + 15) // 16 * 16
    return starts, pos + 16


def host_buffer(name, frames=None, fill=None):
    """(buf, starts): a 16-byte aligned uint8 buffer holding the case's frames at layout()'s positions."""
    case = RESIZE_CASES[name] if frames is None else dict(frames=frames, fill=fill)
    starts, total = layout(case)
    raw = np.zeros(total + 16, np.uint8)
    a = (-raw.ctypes.data) % 16
    buf = raw[a:a + total]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    buf[:] = rng.integers(0, 256, total, dtype=np.uint8)          # bytes between the frames are noise too
    for f, s in zip(case["frames"], starts):
        n = f["sh"] * f["sw"] * 3
        if case.get("fill") == "mult4":
            buf[s:s + n] &= 0xFC
        elif case.get("fill") == "floor_pair":
            buf[s:s + n] = np.repeat(np.array([0, 1, 1, 2], np.uint8), 3)
    if case.get("same_as"):                                       # the one frame of this case is a frame of another case
        other, k = case["same_as"]
        obuf, ostarts = host_buffer(other)
        n = case["frames"][0]["sh"] * case["frames"][0]["sw"] * 3
        buf[starts[0]:starts[0] + n] = obuf[ostarts[k]:ostarts[k] + n]
    return buf, starts


def views(buf, case, starts):
    """The frames as contiguous [sh, sw, 3] views into `buf` (numpy array or torch tensor)."""
    out = []
    for f, s in zip(case["frames"], starts):
        v = buf[s:s + f["sh"] * f["sw"] * 3]
        out.append(v.reshape(f["sh"], f["sw"], 3) if isinstance(v, np.ndarray) else v.view(f["sh"], f["sw"], 3))
    return out


def mirrored(case, srcs):
    """The same batch stated the other way round: every source mirrored left-right, every flip flag toggled."""
    c = dict(case, frames=[dict(f, flip=not f["flip"]) for f in case["frames"]])
    return c, [np.ascontiguousarray(s[:, ::-1]) for s in srcs]


def swap_equivalents(run, case, srcs):
    """Two other statements of run(case, srcs, PROD_MEAN, ALT_STD, swap=True): plane c holds source channel 2 - c
    normalised with mean[c] -- the channel-reversed source without the swap, and the plain source normalised with the
    reversed mean / std, its planes then read in reverse order."""
    yield run(case, [np.ascontiguousarray(s[..., ::-1]) for s in srcs], PROD_MEAN, ALT_STD, False)
    yield run(case, srcs, PROD_MEAN[::-1], ALT_STD[::-1], False)[:, ::-1]


# ---- resize: which branch a case reaches, from its shapes ----------------------------------------------------------------

def lds_bytes(case):
    return 2 * ((3 * max(f["sw"] for f in case["frames"]) + 6) & ~3)


def route(case):
    return "staged" if lds_bytes(case) <= LDS_LIMIT else "direct"


def leads(case):
    """For each frame, the set of (lead of row 0, lead of row 1) pairs its output rows stage, in a 4-byte aligned buffer."""
    starts, _ = layout(case)
    out = []
    for f, s in zip(case["frames"], starts):
        y0, y1, _ = ref._axis(f["dh"], f["inv"], f["sh"])
        rb = 3 * f["sw"]
        out.append({((s + int(a) * rb) & 3, (s + int(b) * rb) & 3) for a, b in zip(y0, y1)})
    return out


def test_cases_reach_their_branches():
    R = RESIZE_CASES
    assert [R[k]["Wp"] >> 3 for k in ("wch1_identity", "wch256_up", "wch257_up", "wch320_down")] == [1, 256, 257, 320]
    assert {R[k]["frames"][0]["dw"] % 8 for k in ("wch256_up", "wch257_up", "wch320_down")} == {1, 0, 7}
    for name, c in R.items():
        for f in c["frames"]:
            assert 0 < f["dh"] <= c["Hp"] <= 16 and 0 < f["dw"] <= c["Wp"] and c["Wp"] % 8 == 0, name
            assert f["sh"] * f["sw"] * 3 <= 3 * 20479 * 3
        assert len(c["frames"]) <= MAX_BATCH
    for k in ("wch1_identity", "wch256_up", "wch257_up", "wch320_down", "mixed_scales"):
        assert any(f["dh"] < R[k]["Hp"] for f in R[k]["frames"]), k + ": no row below the frame to zero"
        assert route(R[k]) == "staged"
    # the second trip of the `xc += 256` loop and of the row-zeroing loop needs wch > 256 in the staged form
    for k in ("wch257_up", "wch320_down", "lds_staged_edge", "narrow_alone"):
        assert route(R[k]) == "staged" and R[k]["Wp"] >> 3 > 256, k
    # both sides of the LDS limit, at the limit
    assert lds_bytes(R["lds_staged_edge"]) == LDS_LIMIT and route(R["lds_staged_edge"]) == "staged"
    assert lds_bytes(R["lds_direct_edge"]) == LDS_LIMIT + 8 and route(R["lds_direct_edge"]) == "direct"
    # the widest frames (184 KiB) are far past it: both take the direct form, and so does the narrow frame batched with one
    assert route(R["wide_20478"]) == route(R["wide_20479"]) == route(R["wide_and_narrow"]) == "direct"
    assert route(R["narrow_alone"]) == "staged"
    assert R["wide_and_narrow"]["frames"][1] == R["narrow_alone"]["frames"][0]
    # source widths of every residue mod 4, odd heights, pointers of every residue, and every lead value on either row --
    # among them rows whose two leads differ (a kernel using lead[0] for both would read shifted bytes)
    staged = [c for c in R.values() if route(c) == "staged"]
    fr = [f for c in staged for f in c["frames"]]
    assert {f["sw"] % 4 for f in fr} == {0, 1, 2, 3} and {f["off"] for f in fr} == {0, 1, 2, 3}
    assert any(f["sh"] % 2 == 1 and f["sh"] > 1 for f in fr)
    pairs = set().union(*[p for c in staged for p in leads(c)])
    assert {a for a, _ in pairs} == {0, 1, 2, 3} and {b for _, b in pairs} == {0, 1, 2, 3}
    assert {(a - b) & 3 for a, b in pairs} == {0, 1, 2, 3}
    # dword tail: staged rows whose lead + 3 * src_w is not a multiple of 4
    assert {(a + 3 * f["sw"]) & 3 for c in staged for f, p in zip(c["frames"], leads(c)) for a, _ in p} == {0, 1, 2, 3}
    assert len(R["n64_tiny"]["frames"]) == MAX_BATCH and len(N65_FRAMES) == MAX_BATCH + 1
    # mixed batch: upscaling, downscaling and both flips
    m = R["mixed_scales"]["frames"]
    assert any(f["inv"] < 1 for f in m) and any(f["inv"] > 1 for f in m) and {f["flip"] for f in m} == {False, True}
    assert 1.0 < B0 < 1.01 and max(bound(f["sh"], f["sw"]) for c in R.values() for f in c["frames"]) < 1.3


# ---- resize: runners and checks shared with the GPU module --------------------------------------------------------------

def oracle_run(oracle, case, srcs, mean, std, swap):
    """The C oracle on explicit destination sizes and inverse scales: bf16 bits [N, 3, Hp, Wp]."""
    import ctypes as C
    N, Hp, Wp = len(case["frames"]), case["Hp"], case["Wp"]
    out = np.zeros((N, 3, Hp, Wp), np.uint16)
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    for n, (f, im) in enumerate(zip(case["frames"], srcs)):
        im = np.ascontiguousarray(im, np.uint8)
        oracle.lib().oracle_image_preprocess(oracle._vp(im), C.c_int(f["sh"]), C.c_int(f["sw"]), C.c_int(f["dh"]),
                                             C.c_int(f["dw"]), C.c_int(int(f["flip"])), C.c_double(f["inv"]), C.c_int(Hp),
                                             C.c_int(Wp), oracle._vp(m), oracle._vp(s), C.c_int(int(swap)),
                                             oracle._vp(out[n]), None)
    return out


def grey_levels(case, bits):
    """The integer v of every frame, [dh, dw, 3], read back from a mean-0 / std-1 run; checks that the padding is +0."""
    vs = []
    for n, f in enumerate(case["frames"]):
        val = ref.bf16_bits_to_f32(bits[n])
        v = val[:, :f["dh"], :f["dw"]]
        assert np.array_equal(v, np.floor(v)) and v.min() >= 0 and v.max() <= 255
        pad = bits[n].copy()
        pad[:, :f["dh"], :f["dw"]] = 0
        assert not pad.any(), "padding is not +0"
        vs.append(v.transpose(1, 2, 0).astype(np.int64))
    return vs


def check_bound(name, case, srcs, vs, swap=False, who="oracle"):
    """Every v within B of the fp64 resample; returns the largest (v - exact) deviations (low, high) of the case."""
    lo = hi = 0.0
    for f, src, v in zip(case["frames"], srcs, vs):
        e = ref.resize_exact(src, f["dh"], f["dw"], f["inv"], f["flip"])
        d = v - (e[..., ::-1] if swap else e)
        lo, hi = min(lo, float(d.min())), max(hi, float(d.max()))
        b = bound(f["sh"], f["sw"])
        assert np.all(np.abs(d) <= b), "%s: v - exact in [%.4f, %.4f], bound %.4f" % (name, d.min(), d.max(), b)
        assert d.min() >= V_LOW - (b - B0) and d.max() <= V_HIGH + (b - B0)
    print("%s %s: v - exact in [%.4f, %+.4f], B = %.4f" % (who, name, lo, hi, max(bound(f["sh"], f["sw"]) for f in case["frames"])))
    return lo, hi


def expected_bits(case, vs, mean, std):
    """The whole output tensor that follows from the grey levels: normalise_bits inside each frame, +0 around it."""
    out = np.zeros((len(vs), 3, case["Hp"], case["Wp"]), np.uint16)
    for n, (f, v) in enumerate(zip(case["frames"], vs)):
        for c in range(3):
            out[n, c, :f["dh"], :f["dw"]] = ref.normalise_bits(v[..., c], mean[c], std[c])
    return out


def check_identities(name, case, srcs, vs):
    """The cases with an exact answer."""
    if name in IDENTITY_CASES:
        for f, s, v in zip(case["frames"], srcs, vs):
            assert np.array_equal(v, s[:, ::-1] if f["flip"] else s), name
    if name.startswith("up2x"):
        low = 0
        for f, s, v in zip(case["frames"], srcs, vs):
            want = np.floor(ref.resize_exact(s, f["dh"], f["dw"], f["inv"], f["flip"]) + 0.5).astype(np.int64)
            if name == "up2x_mult4":
                assert np.array_equal(v, want), name
            assert np.all((want - v >= 0) & (want - v <= 1)), name
            low += int((want - v).sum())
        if name == "up2x_floor_pair":
            assert vs[0][:, :, 0].tolist() == [[0, 0, 1, 1], [0, 0, 1, 1], [1, 1, 1, 2], [1, 1, 2, 2]]
        return low
    if name == "one_pixel":
        for s, v in zip(srcs, vs):
            assert np.array_equal(v, np.broadcast_to(s[0, 0], v.shape)), name
    return 0


@pytest.fixture(scope="module")
def resize_runs(oracle):
    """Each case's frames and the oracle's mean-0 / std-1 grey levels, computed once."""
    out = {}
    for name, case in RESIZE_CASES.items():
        buf, starts = host_buffer(name)
        srcs = views(buf, case, starts)
        bits = oracle_run(oracle, case, srcs, (0, 0, 0), (1, 1, 1), False)
        out[name] = (case, srcs, grey_levels(case, bits))
    return out


@pytest.mark.parametrize("name", list(RESIZE_CASES))
def test_oracle_resize_within_bound_and_identities(resize_runs, name):
    case, srcs, vs = resize_runs[name]
    check_bound(name, case, srcs, vs)
    low = check_identities(name, case, srcs, vs)
    if name == "up2x_noise":
        print("up2x_noise: %d of %d values one below floor(exact + 1/2)" % (low, sum(v.size for v in vs)))
        assert low > 0


@pytest.mark.parametrize("name", list(RESIZE_CASES))
def test_oracle_normalisation_bits(oracle, resize_runs, name):
    case, srcs, vs = resize_runs[name]
    for mean, std in NORM_SETS:
        assert np.array_equal(oracle_run(oracle, case, srcs, mean, std, False), expected_bits(case, vs, mean, std)), (name, std)


@pytest.mark.parametrize("name", MIRROR_CASES)
def test_oracle_flip_is_the_mirrored_source(oracle, resize_runs, name):
    case, srcs, vs = resize_runs[name]
    mc, ms = mirrored(case, srcs)
    got = grey_levels(mc, oracle_run(oracle, mc, ms, (0, 0, 0), (1, 1, 1), False))
    assert all(np.array_equal(a, b) for a, b in zip(got, vs))


@pytest.mark.parametrize("name", SWAP_CASES)
def test_oracle_swap_is_the_reversed_channel_order(oracle, resize_runs, name):
    case, srcs, vs = resize_runs[name]
    sw = grey_levels(case, oracle_run(oracle, case, srcs, (0, 0, 0), (1, 1, 1), True))
    assert all(np.array_equal(a, b[..., ::-1]) for a, b in zip(sw, vs))
    check_bound(name + "/swap", case, srcs, sw, swap=True)
    for other in swap_equivalents(lambda *a: oracle_run(oracle, *a), case, srcs):
        assert np.array_equal(oracle_run(oracle, case, srcs, PROD_MEAN, ALT_STD, True), other)


def test_oracle_narrow_frame_alone_equals_batched(resize_runs):
    assert np.array_equal(resize_runs["wide_and_narrow"][2][1], resize_runs["narrow_alone"][2][0])


def test_references_known_answers():
    """The references against values worked by hand, so that they are not only compared with the code they judge."""
    row = np.zeros((1, 2, 3), np.uint8)
    row[0, 1] = 255
    e = ref.resize_exact(row, 2, 4, 0.5, False)
    assert e[0, :, 0].tolist() == [0.0, 63.75, 191.25, 255.0] and np.array_equal(e[0], e[1])
    assert ref.resize_exact(row, 2, 4, 0.5, True)[0, :, 0].tolist() == [255.0, 191.25, 63.75, 0.0]
    g = np.arange(12, dtype=np.uint8).reshape(2, 2, 3) * 10
    assert ref.resize_exact(g, 1, 1, 2.0, False)[0, 0].tolist() == [45.0, 55.0, 65.0]          # the centre of a 2x2
    # bf16: 1 + 2^-8 is a tie -> even (1.0); 1 + 3 * 2^-8 is a tie -> even (1 + 2^-6); (200 - 100) / 3 = 33.33.. -> 33.25
    assert ref.f32_to_bf16_bits(np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -2.5])).tolist() == [0x3F80, 0x3F82, 0xC020]
    assert ref.bf16_bits_to_f32(ref.normalise_bits(np.array([200]), 100.0, 3.0)).tolist() == [33.25]
    sq = np.float32([[1, 1], [5, 1], [5, 4], [1, 4]])
    m, mg = ref.polygon_mask_exact(sq, [0, 4], [0, 1, 1], 2, 6, 8)
    want = np.zeros((6, 8), np.uint8)
    want[1:4, 1:5] = 1
    assert np.array_equal(m[0], want) and not m[1].any() and np.isinf(mg[1]).all() and np.isinf(mg[0, 0]).all()
    assert mg[0, 2].tolist() == [0.5, 0.5, 1.5, 1.5, 0.5, 0.5, 1.5, 2.5]
    tri = np.float32([[0, 0], [4, 0], [0, 4]])                      # hypotenuse x + y = 4: centres with x + y + 1 < 4
    m, mg = ref.polygon_mask_exact(tri, [0, 3], [0, 1], 1, 4, 4)
    assert m[0].tolist() == [[1, 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]] and mg[0, 1, 2] == 0.0


# ---- polygons -----------------------------------------------------------------------------------------------------------

POLY_WS = (4, 1020, 1024, 1028, 1344, 2052)
MAX_AMBIGUOUS = 1e-4


def _rect(x1, y1, x2, y2):
    return np.float32([[x1, y1], [x2, y1], [x2, y2], [x1, y2]])


def _star(cx, cy, r, n=5, rng=None):
    """A {n/2} star polygon: consecutive vertices two steps apart on the circle, so the middle is wound twice (a hole)."""
    k = np.arange(n)
    a = 2 * np.pi * ((2 * k) % n) / n + 0.3
    p = np.stack([cx + r * np.cos(a), cy + 0.45 * r * np.sin(a)], 1)
    return (p + (rng.uniform(-0.2, 0.2, p.shape) if rng is not None else 0)).astype(np.float32)


def _aligned_instances(H, W):
    """Axis-aligned rectangles on the half-pixel grid; every straddling edge is vertical, so the crossing is exact."""
    r = W - 1.5
    return [
        [],                                                             # an empty instance first
        [_rect(0.5, 0.5, W - 1.5, 2.5)],                                # vertices on pixel centres
        [_rect(1, 1, W - 1, H - 2)],                                    # on pixel edges
        [_rect(0, 1.5, min(W, 1026), 3.5)],                             # on y + 0.5 rows, across column 1024 where W reaches it
        [_rect(-9, -9, -1, H + 9)], [_rect(W + 1, 0, W + 9, H)], [_rect(0, -9, W, -0.5)], [_rect(0, H + 0.5, W, H + 9)],
        [],                                                             # ... in the middle
        [_rect(-3, 2, 2.5, 5)], [_rect(r, 1, W + 7, 4)], [_rect(1, -4, 3, 1.5)], [_rect(1, H - 2.5, 3, H + 4)],   # clipped
        [_rect(0, 0, 3, 3), _rect(2, 2, min(W, 1030), 5)],              # two overlapping polygons: OR, not XOR
        [np.zeros((0, 2), np.float32), _rect(1, 1, 3, 3)[:1], _rect(1, 1, 3, 3)[:2]],      # 0, 1 and 2 vertices
        [_rect(1, 1, 3, 3)[:2], _rect(0.5, 4.5, W - 0.5, 6.5)],         # a degenerate polygon beside a real one
        [],                                                             # ... and last
    ]


def _general_instances(H, W, rng):
    """Slanted edges: a polygon across column 1024 (or the right border), stars, clipped and outside shapes, and one
    polygon stated three ways (as is, rotated, reversed)."""
    xm = min(W - 2.0, 1024.0)
    span = np.float32([[xm - 19.3, 0.2], [xm + 1.4, 1.1], [W + 3.7, H - 0.7], [xm + 0.6, H + 1.3], [xm - 25.1, H - 2.2]])
    base = np.float32(rng.uniform([-2, -2], [W + 2, H + 2], (7, 2)))
    return [
        [span],
        [_star(W / 2.0, H / 2.0, W / 2.5, 5, rng)],                     # self-intersecting: even-odd hole in the middle
        [_star(W - 3.0, H / 2.0, 9.0, 7, rng)],                         # clipped at the right border
        [],
        [_star(-40.0, H / 2.0, 9.0, 5, rng)], [_star(W + 40.0, -30.0, 9.0, 5, rng)],        # wholly outside
        [np.float32([[-5.5, -3.2], [W * 0.73, -1.1], [W * 0.41, H + 6.3]])],                  # clipped above, below and left
        [np.float32([[0.3, 0.4], [W - 1.2, 0.9], [W - 2.9, H - 1.6], [1.7, H - 0.3]]),
         np.float32([[W * 0.3, 1.2], [W * 0.9, 2.8], [W * 0.5, H - 0.1]])],                 # two overlapping polygons
        [base], [np.roll(base, 3, axis=0)], [base[::-1].copy()],        # the same polygon, rotated, reversed
    ]


ROTATED = (8, 9, 10)        # instances of _general_instances: base, rotated (same bits), reversed (same off the ambiguous set)


def _random_instances(H, W, rng):
    out = []
    for g in range(6):
        if g == 2:
            out.append([])
            continue
        inst = []
        for _ in range(int(rng.integers(1, 4))):
            inst.append(rng.uniform([-8, -8], [W + 8, H + 8], (int(rng.integers(3, 12)), 2)).astype(np.float32))
        out.append(inst)
    return out


# seeds under which the reference alone finds at most MAX_AMBIGUOUS of a case's pixels ambiguous (asserted below)
POLY_SEEDS = {"general_w4": 11, "general_w1020": 12, "general_w1024": 13, "general_w1028": 14, "general_w1344": 15,
              "general_w2052": 16, "random_40x64": 17}


def polygon_cases():
    cases = {}
    for W in POLY_WS:
        cases["aligned_w%d" % W] = dict(H=8, W=W, aligned=True, insts=_aligned_instances(8, W))
        name = "general_w%d" % W
        cases[name] = dict(H=7, W=W, aligned=False, insts=_general_instances(7, W, np.random.default_rng(POLY_SEEDS[name])))
    cases["random_40x64"] = dict(H=40, W=64, aligned=False,
                                 insts=_random_instances(40, 64, np.random.default_rng(POLY_SEEDS["random_40x64"])))
    return cases


POLY_CASES = polygon_cases()


def delta(insts):
    """delta of the module docstring for a case's polygons (0 when every straddling edge is vertical)."""
    dx = ax = 0.0
    for inst in insts:
        for p in inst:
            if p.shape[0] < 3:
                continue
            q = np.roll(p, 1, axis=0).astype(np.float64)
            slanted = (q[:, 1] != p[:, 1]) & (q[:, 0] != p[:, 0])
            if slanted.any():
                dx = max(dx, float(np.abs(q[:, 0] - p[:, 0])[slanted].max()))
                ax = max(ax, float(np.abs(p[:, 0].astype(np.float64)).max()))
    return 2.0 ** -24 * (6 * dx + ax)


_POLY_MEMO = {}


def polygon_reference(name):
    """(packed polygons, exact mask, ambiguous pixels) of a case, computed once per process."""
    if name not in _POLY_MEMO:
        c = POLY_CASES[name]
        G = len(c["insts"])
        packed = T.pack_polygons([c["insts"]], 1, G)
        mask, margin = ref.polygon_mask_exact(*packed, G, c["H"], c["W"])
        d = delta(c["insts"])
        _POLY_MEMO[name] = (packed, mask, (margin <= d) & (d > 0), d)
    return _POLY_MEMO[name]


def check_polygon(name, got, who="oracle"):
    """`got` [G, H, W] against the exact mask outside the ambiguous set; returns the ambiguous-pixel count."""
    c = POLY_CASES[name]
    _, mask, amb, d = polygon_reference(name)
    assert got.shape == mask.shape and set(np.unique(got).tolist()) <= {0, 1}
    bad = (got != mask) & ~amb
    print("%s %s: delta = %.3g px, %d of %d pixels ambiguous, %d of them differ" %
          (who, name, d, int(amb.sum()), amb.size, int(((got != mask) & amb).sum())))
    assert not bad.any(), "%s: %d pixels differ from the exact mask, first at %s" % (name, int(bad.sum()), np.argwhere(bad)[0])
    if name.startswith("general"):
        assert np.array_equal(got[ROTATED[0]], got[ROTATED[1]]), name + ": a rotated vertex list changed the mask"
        rev = (got[ROTATED[0]] != got[ROTATED[2]]) & ~(amb[ROTATED[0]] | amb[ROTATED[2]])
        assert not rev.any(), name + ": a reversed vertex list changed the mask"
    return int(amb.sum())


def test_polygon_cases_reach_their_branches():
    assert {c["W"] for c in POLY_CASES.values()} == set(POLY_WS) | {64}
    for name, c in POLY_CASES.items():
        assert c["W"] % 4 == 0 and (c["H"] <= 8 or name == "random_40x64")
        packed, mask, amb, d = polygon_reference(name)
        assert amb.sum() <= MAX_AMBIGUOUS * amb.size, "%s: %d ambiguous pixels" % (name, int(amb.sum()))
        if c["aligned"]:
            assert d == 0.0 and not amb.any()
        if c["W"] > 1024:
            # blockIdx.x > 0: set pixels, and a polygon's span, on both sides of column 1024
            assert mask[:, :, 1024:].any() and any((m[:, :1024].any() and m[:, 1024:].any()) for m in mask), name
            assert (mask[:, :, 1024:] != mask[:, :, :c["W"] - 1024]).any(), name     # not a copy of block 0's columns
    a = POLY_CASES["aligned_w1028"]["insts"]
    _, mask, _, _ = polygon_reference("aligned_w1028")
    empty = [g for g, inst in enumerate(a) if not inst]
    assert empty[0] == 0 and empty[-1] == len(a) - 1 and len(empty) == 3
    assert not mask[empty].any() and not mask[4:8].any() and not mask[14].any() and mask[15].any()
    assert all(mask[g].any() for g in (1, 2, 3, 9, 10, 11, 12, 13))
    assert mask[13].sum() == 9 + 3 * 1026 - 1                               # OR of the two rectangles, not XOR
    # vertices on pixel centres: the centre on the left edge is inside, the one on the right edge outside (strict `<`),
    # the row on the top edge inside, the one on the bottom edge outside (half-open in y)
    assert mask[1, 0, :3].tolist() == [1, 1, 1] and mask[1, 0, 1025:].tolist() == [1, 0, 0]
    assert mask[1, :, 5].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    _, mask, _, _ = polygon_reference("general_w1344")
    assert mask[1].any() and not mask[1, 3, 660:684].any()                 # the star's middle is a hole
    assert not mask[3:6].any() and mask[2].any() and mask[6].any() and mask[7].any()


@pytest.mark.parametrize("name", list(POLY_CASES))
def test_oracle_polygon_masks_equal_exact(oracle, name):
    c = POLY_CASES[name]
    packed = polygon_reference(name)[0]
    check_polygon(name, oracle.polygon_masks(*packed, len(c["insts"]), c["H"], c["W"]))


# ---- one convention for image, box, polygon and keypoint -----------------------------------------------------------------

CONV_H, CONV_W = 20, 30
CONV_RECT = (6, 4, 13, 11)          # x1, y1, x2, y2 inclusive; chosen so that no scaled edge falls on a pixel centre
CONV_SCALES = (1.0, 0.5, 1.6)


def convention_case(scale, flip):
    """A black frame with one bright rectangle and its annotations, taken through the host transforms."""
    x1, y1, x2, y2 = CONV_RECT
    im = np.zeros((CONV_H, CONV_W, 3), np.uint8)
    im[y1:y2 + 1, x1:x2 + 1] = 255
    box = T.transform_boxes(np.float32([[x1, y1, x2, y2]]), scale, flip, CONV_W)[0]
    poly = T.transform_polygons([[x1, y1, x2 + 1, y1, x2 + 1, y2 + 1, x1, y2 + 1]], scale, flip, CONV_W)[0]
    kp = T.transform_keypoints(np.float32([[[x1, y1, 2]]]), scale, flip, CONV_W, flip_pairs=())[0, 0]
    dh, dw = T.resized_shape(CONV_H, CONV_W, scale)
    case = dict(Hp=(dh + 7) // 8 * 8, Wp=(dw + 7) // 8 * 8, frames=[F(CONV_H, CONV_W, dh, dw, 1.0 / scale, flip, 0)])
    return case, im, box, poly, kp


def check_convention(scale, flip, case, box, kp, v, mask):
    """v [dh, dw] grey levels of one channel, mask [Hp, Wp]: image, polygon, box and keypoint describe one region."""
    f = case["frames"][0]
    bright = np.zeros((case["Hp"], case["Wp"]), bool)
    bright[:f["dh"], :f["dw"]] = v > 127.5
    ys, xs = np.nonzero(bright)
    tol = 1.0 + scale
    ext = np.array([xs.min(), ys.min(), xs.max(), ys.max()], np.float64)
    assert np.all(np.abs(ext - box[:4]) <= tol), (scale, flip, ext.tolist(), box.tolist())
    yy, xx = np.nonzero(bright != (mask != 0))
    near = (np.minimum(np.abs(xx - box[0]), np.abs(xx - box[2])) <= 1) | (np.minimum(np.abs(yy - box[1]), np.abs(yy - box[3])) <= 1)
    assert near.all(), (scale, flip, "mask and image differ away from the box border")
    # the rectangle's scaled edges avoid pixel centres, so the two must in fact be the same set of pixels
    assert np.array_equal(bright, mask != 0), (scale, flip)
    # the keypoint on the rectangle's top-left pixel is the box corner it started on (the other x corner when flipped)
    assert kp[2] == 2 and kp[1] == box[1] and kp[0] == (box[2] if flip else box[0]), (scale, flip, kp.tolist(), box.tolist())
    assert np.min(np.hypot(xs - kp[0], ys - kp[1])) <= 1.0


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("scale", CONV_SCALES)
def test_oracle_image_box_polygon_keypoint_agree(oracle, scale, flip):
    case, im, box, poly, kp = convention_case(scale, flip)
    v = grey_levels(case, oracle_run(oracle, case, [im], (0, 0, 0), (1, 1, 1), False))[0][..., 0]
    pv, ps, pf = T.pack_polygons([[[poly]]], 1, 1)
    mask = oracle.polygon_masks(pv, ps, pf, 1, case["Hp"], case["Wp"])[0]
    exact, margin = ref.polygon_mask_exact(pv, ps, pf, 1, case["Hp"], case["Wp"])
    assert np.array_equal(mask, exact[0]) and margin.min() > 0.05
    check_convention(scale, flip, case, box, kp, v, mask)
