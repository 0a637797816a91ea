"""Case tables for csrc/roi_align.hip (forward, scatter backward, gather backward in its segment and table forms) and for
mask_target / mask_paste of csrc/mask.hip: the input generators of tests/test_gpu_roi_shapes.py and, checked here without
a GPU, the property each case exists for (a generator that silently misses its branch makes its GPU test worthless), the
clearance of every randomised sample from the lines where the operator is discontinuous, the share of thresholded pixels
the comparison has to leave out, the adjoint identity of the reference, and the agreement of tests/_roi_ref.py with the
project's C oracle -- two independent statements of each operation that agree before any kernel runs.

`plan` restates, as index arithmetic only, how the host lays out the segment form of the gather backward:
  segs = ceil(W / 8), chunks = ceil(segs / 4), segs_per_wg = ceil(segs / chunks)   workgroups along a row, waves per workgroup
  rows_per_wg = 1 if R > 1024 or H < 64 else 2                                     rows of a tile
  PW <= 14 and R > 0 -> segment form, else table form; PW <= 7 and sr == 2 pick the template instance.
"""
import functools

import numpy as np
import pytest
import torch

import _roi_ref as ref

CLEAR = 2.0 ** -10         # px: the constant of tests/test_deform_shapes_cpu.py (DP_CLEAR), for the same reason: the kernel's
                           # fp32 and the reference's fp64 must not disagree about which samples count
SEG_W, SEG_WAVES, CHUNK = 8, 4, 1024
ROWS_SWITCH = 64           # maps with at least this many rows get two-row tiles
MAX_SAMPLES = 32           # kRoiMaxSamples
BAND = 1e-5                # thresholded outputs: pixels whose fp64 value lies this close to the threshold are not compared
MAX_EXCLUDED = 0.005       # ... and they may be at most this share of a case's compared pixels
BF16_REL = 2.0 ** -7       # bf16 outputs: |got - ref| <= 2^-7 |ref| + 2^-7 rms(ref)

STD_MAPS = ((32, 40), (16, 20), (8, 10), (4, 5))
FIVE_MAPS = STD_MAPS + ((2, 3),)
EIGHT_MAPS = ((40, 36), (20, 18), (10, 9), (5, 5), (3, 3), (2, 2), (1, 2), (1, 1))


def bf16(x):
    return torch.as_tensor(np.asarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def bf16_bits(x):
    """uint16 bit patterns of a bf16-exact float array (what the C oracle takes)."""
    x = np.ascontiguousarray(x, np.float32)
    assert np.array_equal(bf16(x), x)
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def close_bf16(got, want, what):
    """The project's bound for a bf16 output against fp64, no element exempt; returns achieved error / bound."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = BF16_REL * np.abs(want) + BF16_REL * np.sqrt((want ** 2).mean()) if want.size else np.zeros_like(want)
    err = np.abs(got - want)
    ratio = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max()) if (bound > 0).any() else 0.0
    print("%s: max error / bound = %.3f" % (what, ratio))
    assert np.all(err <= bound), "%s: %d elements outside the bound, worst %.3g x" % (what, int((err > bound).sum()), ratio)
    return ratio


def close_scatter(got, want, scale, what):
    """The scatter form's bound: rtol 1e-5, atol 1e-5 of the gradient map's scale."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = 1e-5 * np.abs(want) + 1e-5 * scale
    err = np.abs(got - want)
    ratio = float((err / np.where(bound > 0, bound, 1.0)).max()) if want.size else 0.0
    print("%s: max error / bound = %.3f" % (what, ratio))
    assert np.all(err <= bound), "%s: worst %.3g x the bound" % (what, ratio)
    return ratio


# ---- the planner restatement ----------------------------------------------------------------------------------------

def plan(maps, R, PW, sr):
    lv = []
    for H, W in maps:
        segs = -(-W // SEG_W)
        chunks = -(-segs // SEG_WAVES)
        spw = -(-segs // chunks)
        rows = 1 if (R > CHUNK or H < ROWS_SWITCH) else 2
        lv.append(dict(segs=segs, chunks=chunks, segs_per_wg=spw, rows_per_wg=rows, bands=-(-H // rows)))
    return dict(levels=lv, route="segment" if (PW <= 14 and R > 0) else "table", rounds=-(-R // CHUNK),
                instance=(7 if PW <= 7 else 14, 2 if sr == 2 else 0))


# ---- RoIAlign cases ---------------------------------------------------------------------------------------------------

def _scales(maps, stride0=4):
    return [1.0 / (stride0 << l) for l in range(len(maps))]


def _geom(c, r, rois=None, levels=None):
    return ref.roi_geometry(c["maps"], c["scales"], c["rois"] if rois is None else rois, c["levels"] if levels is None else levels,
                            c["PH"], c["PW"], c["sr"], c["lvl_min"], c["N"], r)


def geoms(c):
    return [_geom(c, r) for r in range(c["rois"].shape[0])]


def clearance(g, sr):
    """Smallest distance of a sample of this roi from the lines -1 and L (and, adaptive grid, of a bin size from an integer)."""
    d = np.inf
    for (v, _, _, _, _), L in ((g["ys"], g["H"]), (g["xs"], g["W"])):
        d = min(d, np.abs(v + 1.0).min(), np.abs(v - L).min())
    if sr == 0:
        for b in (g["bin_h"], g["bin_w"]):
            d = min(d, abs(b - round(b)))
    return d


def random_rois(rng, maps, scales, N, R, PH, PW, sr, lvl_min, shapes=None):
    """R rois all over (and a little past) the image, log-uniform sizes, a random level each (so that every level sees rois
    of every size: off-map, sub-pixel, clipped), every one redrawn until its samples keep CLEAR from the lines. shapes:
    optional list of (w, h) factors cycled over the rois (tall and wide ones for the adaptive grid)."""
    img_h, img_w = maps[0][0] / scales[0], maps[0][1] / scales[0]
    rois, levels = np.zeros((R, 5), np.float32), np.zeros((R,), np.int32)
    c = dict(maps=maps, scales=scales, PH=PH, PW=PW, sr=sr, lvl_min=lvl_min, N=N)
    for r in range(R):
        for _ in range(100):
            w, h = np.exp(rng.uniform(np.log(2.0), np.log(1.2 * max(img_h, img_w)), 2))
            if shapes is not None:
                w, h = w * shapes[r % len(shapes)][0], h * shapes[r % len(shapes)][1]
            x1, y1 = rng.uniform(-0.15 * img_w, img_w), rng.uniform(-0.15 * img_h, img_h)
            rois[r] = (rng.integers(0, N), x1, y1, x1 + w, y1 + h)
            levels[r] = lvl_min + rng.integers(0, len(maps))
            if clearance(_geom(c, r, rois, levels), sr) >= CLEAR:
                break
        else:
            raise AssertionError("roi %d: no draw keeps its samples off the lines" % r)
    return rois, levels


def make_case(name, maps, N, C, PH, PW, sr, rois, levels, lvl_min=2, scales=None, seed=0, exact=False):
    """bf16-exact N(0,1) features and output gradients; channel 0 of both is the constant 1."""
    g = torch.Generator().manual_seed(1000 + seed)
    feats = [torch.randn((N, H, W, C), generator=g).to(torch.bfloat16) for H, W in maps]
    R = rois.shape[0]
    gout = torch.randn((R, PH, PW, C), generator=g).to(torch.bfloat16)
    for f in feats:
        f[..., 0] = 1.0
    gout[..., 0] = 1.0
    return dict(name=name, maps=tuple(maps), scales=_scales(maps) if scales is None else scales, N=N, C=C, PH=PH, PW=PW, sr=sr,
                lvl_min=lvl_min, rois=np.ascontiguousarray(rois, np.float32).reshape(-1, 5),
                levels=np.ascontiguousarray(levels, np.int32), feats=feats, gout=gout, exact=exact)


def _std(name, seed, R=24, maps=STD_MAPS, N=2, C=8, PH=7, PW=7, sr=2, extra=None, shapes=None, lvl_min=2):
    rng = np.random.default_rng(seed)
    sc = _scales(maps)
    rois, levels = random_rois(rng, maps, sc, N, R, PH, PW, sr, lvl_min, shapes)
    if extra is not None:
        er, el = extra
        rois, levels = np.concatenate([np.asarray(er, np.float32), rois]), np.concatenate([np.asarray(el, np.int32), levels])
    return make_case(name, maps, N, C, PH, PW, sr, rois, levels, lvl_min, sc, seed)


def _one_level(name, seed, H, W, R, C, PH, PW, sr=2, N=1, extra=None, lvl_min=2):
    return _std(name, seed, R, ((H, W),), N, C, PH, PW, sr, extra, lvl_min=lvl_min)


# w33: level-0 pixel coordinates times 4 (scale 1/4). 2 x 2 bins of one pixel, 2 samples each: x samples at x1 + .25, .75,
# 1.25, 1.75 -> (22.75 .. 24.25): a sample between pixels 23 | 24, the seam of the two workgroups; (30.75 .. 32.25): a
# sample between 31 | 32, the seam into the one-pixel last segment
W33_EXTRA = ([[0, 90, 2, 98, 10], [0, 122, 4, 130, 12]], [2, 2])

# rois smaller than a pixel of the coarsest standard level (scale 1/32) that start on a pixel line: width and height clamp
# to one pixel, so the samples of all PH (PW) bins lie strictly inside one pixel row (column)
TINY_EXTRA = ([[0, 64, 32, 70, 40], [1, 32, 64, 33, 65]], [5, 5])

GRIDS = [(1, 1, 1), (7, 7, 2), (14, 14, 2), (7, 14, 2), (14, 7, 2), (8, 8, 4), (7, 7, 4), (6, 10, 3), (2, 2, 5), (16, 3, 2),
         (3, 16, 2), (2, 16, 2)]
CHANNELS = [4, 252, 256, 260, 516]
ROUNDS = [1024, 1025, 2049]
ROWS = [63, 64, 65]


def _empty_case(C=8):
    """Three levels, N = 2: every roi is of image 0 and of level 2 or 4 (image 1 and level 3 get nothing); roi 0 lies
    outside its map on both axes, roi 1 on the y axis only."""
    maps, rng = STD_MAPS[:3], np.random.default_rng(41)
    sc = _scales(maps)
    rois, levels = random_rois(rng, maps, sc, 1, 14, 7, 7, 2, 2)
    levels[:] = np.where(levels == 3, 2, levels)
    levels[:2] = (2, 4)
    rois[0] = (0, 400, 300, 460, 340)
    rois[1] = (0, 20, 300, 90, 340)
    c = dict(maps=maps, scales=sc, PH=7, PW=7, sr=2, lvl_min=2, N=2)
    assert all(clearance(_geom(c, r, rois, levels), 2) >= CLEAR for r in range(14))
    return make_case("empty", maps, 2, C, 7, 7, 2, rois, levels, 2, sc, 41)


def _clamped_case(C=8, sr=2):
    """Image indices -1 and N (= 2), levels lvl_min - 1 and lvl_min + num_levels on the first eight rois."""
    c = _std("clamped", 42, R=16, C=C, sr=sr)
    c["rois"][0:8, 0] = (-1, 2, -1, 2, 0, 1, -1, 2)
    c["levels"][0:8] = (1, 1, 6, 6, 1, 6, 3, 4)
    assert all(clearance(g, sr) >= CLEAR for g in geoms(c))
    return c


# on the line: one 8 x 8 level at scale 1/2, 2 x 2 bins. Per axis a roi is one of (start, length) on the level; with two
# samples per bin the samples sit at start + length * (1, 3, 5, 7) / 8 -- all dyadic, exact in fp32:
LINE_L = 8
LINE_AXIS = [(-2.0, 8.0),    # -1 (counts, pixel 0), 1, 3, 5 (interior integers)
             (1.0, 8.0),     # 2, 4, 6, 8 = L (counts, pixel L-1)
             (-1.0, 8.0),    # 0, 2, 4, 6
             (0.0, 8.0),     # 1, 3, 5, 7 = L-1
             (-1.5, 2.0),    # -1.25 (dropped), -0.75, -0.25, 0.25
             (6.5, 2.0),     # 6.75, 7.25, 7.75, 8.25 = L + 0.25 (dropped)
             (-1.5, 4.0)]    # bin exactly 2.0: the adaptive grid is 2; -1, 0, 1, 2


def _line_case(C=8, sr=2):
    rois = [[(i + j) % 2, 2 * xs, 2 * ys, 2 * (xs + xl), 2 * (ys + yl)]
            for i, (ys, yl) in enumerate(LINE_AXIS) for j, (xs, xl) in enumerate(LINE_AXIS)]
    rois = np.asarray(rois, np.float32)
    return make_case("on_the_line", ((LINE_L, LINE_L),), 2, C, 2, 2, sr, rois, np.full(len(rois), 1, np.int32), 1, [0.5], 43,
                     exact=True)


@functools.lru_cache(maxsize=None)
def gather_case(name):
    """The gather-backward table; names as in GATHER_NAMES."""
    kind, _, arg = name.partition(":")
    if kind == "narrow":
        return _one_level(name, 1, 3, 5, 3, 4, 2, 2)
    if kind == "w33":
        return _one_level(name, 2, 4, 33, 12, 8, 2, 2, extra=W33_EXTRA)
    if kind == "rows":
        return _one_level(name, 3 + int(arg), int(arg), 9, 48, 8, 7, 7)
    if kind == "round":
        return _one_level(name, 100 + int(arg), 64, 9, int(arg), 4, 2, 2)
    if kind == "channels":
        return _one_level(name, 200 + int(arg), 5, 10, 6, int(arg), 7, 7)
    if kind == "grids":
        PH, PW, sr = (int(v) for v in arg.split("x"))
        return _std(name, 300 + 100 * PH + 10 * PW + sr, PH=PH, PW=PW, sr=sr, extra=TINY_EXTRA)
    if kind == "empty":
        return _empty_case()
    if kind == "clamped":
        return _clamped_case()
    if kind == "thin_levels":
        return _std(name, 44, R=64, maps=EIGHT_MAPS, N=3)
    if kind == "on_the_line":
        return _line_case()
    if kind == "r0":
        return _std(name, 45, R=0)
    raise KeyError(name)


GATHER_NAMES = (["narrow", "w33"] + ["rows:%d" % h for h in ROWS] + ["round:%d" % r for r in ROUNDS]
                + ["channels:%d" % c for c in CHANNELS] + ["grids:%dx%dx%d" % g for g in GRIDS]
                + ["empty", "clamped", "thin_levels", "on_the_line", "r0"])

FWD_GRIDS = [(PH, PW, sr) for (PH, PW) in ((1, 1), (7, 7), (14, 14), (5, 9)) for sr in (0, 1, 2, 3)]
TALL_WIDE = [(1.0, 1.0), (0.2, 3.0), (3.0, 0.2)]


@functools.lru_cache(maxsize=None)
def forward_case(name):
    """The forward table (C a multiple of 8): the geometry tables above where they apply, channel-group counts 1, 3, 8, 33,
    bin grids x sampling ratios on the five-level pyramid (tall and wide rois: gh != gw under the adaptive grid)."""
    kind, _, arg = name.partition(":")
    if kind == "narrow":
        return _one_level(name, 1, 3, 5, 3, 8, 2, 2)
    if kind == "channels":
        return _std(name, 500 + int(arg), C=int(arg))
    if kind == "grids":
        PH, PW, sr = (int(v) for v in arg.split("x"))
        return _std(name, 600 + 100 * PH + 10 * PW + sr, maps=FIVE_MAPS, PH=PH, PW=PW, sr=sr, shapes=TALL_WIDE)
    if kind == "on_the_line_adaptive":
        return _line_case(sr=0)
    if kind in ("w33", "rows", "empty", "clamped", "thin_levels", "on_the_line"):
        return gather_case(name)
    raise KeyError(name)


FORWARD_NAMES = (["narrow", "w33", "rows:65", "empty", "clamped", "thin_levels", "on_the_line", "on_the_line_adaptive"]
                 + ["channels:%d" % c for c in (8, 24, 64, 264)] + ["grids:%dx%dx%d" % g for g in FWD_GRIDS])


@functools.lru_cache(maxsize=None)
def scatter_case(name):
    """The scatter-backward table: narrow, w33, a subset of the grids with the adaptive one, clamped, on the line."""
    kind, _, arg = name.partition(":")
    if kind == "grids":
        PH, PW, sr = (int(v) for v in arg.split("x"))
        # (1 x 1 adaptive: a roi clamped to one pixel has a bin size of exactly 1, an integer -- no sub-pixel rois there)
        return _std(name, 700 + 100 * PH + 10 * PW + sr, PH=PH, PW=PW, sr=sr, shapes=TALL_WIDE,
                    extra=None if (PH, PW, sr) == (1, 1, 0) else TINY_EXTRA)
    if kind == "clamped_adaptive":
        return _clamped_case(sr=0)
    if kind == "on_the_line_adaptive":
        return _line_case(sr=0)
    return gather_case(name)


SCATTER_NAMES = ["narrow", "w33", "grids:7x7x2", "grids:14x14x0", "grids:5x9x0", "grids:6x10x3", "grids:1x1x0", "clamped",
                 "clamped_adaptive", "on_the_line", "on_the_line_adaptive"]


def scatter_base(c):
    """The random fp32 contents the scatter form adds to."""
    g = torch.Generator().manual_seed(77)
    return [torch.randn((c["N"], H, W, c["C"]), generator=g) for H, W in c["maps"]]


@functools.lru_cache(maxsize=None)
def ref_forward(table, name):
    c = {"gather": gather_case, "forward": forward_case, "scatter": scatter_case}[table](name)
    return ref.roi_align_ref([f.double() for f in c["feats"]], c["scales"], c["rois"], c["levels"], c["PH"], c["PW"], c["sr"],
                             c["lvl_min"], c["N"])


@functools.lru_cache(maxsize=None)
def ref_backward(table, name):
    c = {"gather": gather_case, "forward": forward_case, "scatter": scatter_case}[table](name)
    return ref.roi_align_ref_backward(c["maps"], c["scales"], c["rois"], c["levels"], c["gout"].double(), c["sr"], c["lvl_min"],
                                      c["N"])


def footprint(g):
    """(level, image, rows, columns) of the pixels the counted samples of a roi touch (empty sets: the roi adds nothing)."""
    ys, xs = g["ys"], g["xs"]
    rows = set(ys[2][ys[1]].tolist()) | set(ys[3][ys[1]].tolist())
    cols = set(xs[2][xs[1]].tolist()) | set(xs[3][xs[1]].tolist())
    if not rows or not cols:
        rows, cols = set(), set()
    return g["l"], g["n"], rows, cols


def fully_inside(g):
    return bool(g["ys"][1].all() and g["xs"][1].all())


def bins_on_row(g, P, gsz, axis="ys"):
    """{pixel line: set of bins with a counted sample that touches it} along one axis."""
    _, counts, lo, hi, _ = g[axis]
    out = {}
    for s in np.nonzero(counts)[0]:
        for y in (int(lo[s]), int(hi[s])):
            out.setdefault(y, set()).add(int(s) // gsz)
    return out


# ---- the properties ---------------------------------------------------------------------------------------------------

def _all_cases():
    return ([("gather", n) for n in GATHER_NAMES] + [("forward", n) for n in FORWARD_NAMES]
            + [("scatter", n) for n in SCATTER_NAMES])


def _case(table, name):
    return {"gather": gather_case, "forward": forward_case, "scatter": scatter_case}[table](name)


@pytest.mark.parametrize("table,name", _all_cases())
def test_inputs_are_bf16_exact_small_and_clear_of_the_lines(table, name):
    c = _case(table, name)
    for f in c["feats"] + [c["gout"]]:
        assert bool((f[..., 0] == 1.0).all())
    assert all(H <= 70 and W <= 40 for H, W in c["maps"]) and c["C"] <= 520 and len(c["maps"]) <= 8
    assert c["C"] % (8 if table == "forward" else 4) == 0
    if table == "gather":
        assert c["sr"] > 0 and c["PH"] * c["sr"] <= MAX_SAMPLES and c["PW"] * c["sr"] <= MAX_SAMPLES
    if not c["exact"]:
        worst = min([clearance(g, c["sr"]) for g in geoms(c)] + [np.inf])
        assert worst >= CLEAR, worst


def test_narrow_is_one_partial_segment_of_one_live_wave():
    c = gather_case("narrow")
    p = plan(c["maps"], c["rois"].shape[0], c["PW"], c["sr"])
    lv = p["levels"][0]
    assert c["maps"] == ((3, 5),) and c["N"] == 1 and c["C"] == 4 and c["rois"].shape[0] == 3
    assert (lv["segs"], lv["chunks"], lv["segs_per_wg"], lv["rows_per_wg"]) == (1, 1, 1, 1) and c["maps"][0][1] < SEG_W
    assert p["route"] == "segment" and p["instance"] == (7, 2)
    assert any(footprint(g)[2] for g in geoms(c))


def test_w33_has_the_seam_samples_and_a_dead_wave():
    c = gather_case("w33")
    W = c["maps"][0][1]
    lv = plan(c["maps"], c["rois"].shape[0], c["PW"], c["sr"])["levels"][0]
    assert (lv["segs"], lv["chunks"], lv["segs_per_wg"]) == (5, 2, 3)
    X0 = 1 * lv["segs_per_wg"] * SEG_W                      # the second workgroup's first pixel
    assert X0 == 24 and X0 + 1 * SEG_W < W <= X0 + 2 * SEG_W  # its second wave is live, its third (x0 = 40) is not
    assert W - (X0 + SEG_W) == 1                               # ... and owns the one-pixel last segment
    pairs = set()
    for g in geoms(c):
        _, counts, lo, hi, frac = g["xs"]
        if g["ys"][1].any():
            pairs |= {(int(a), int(b)) for a, b, ok, f in zip(lo, hi, counts, frac) if ok and 0 < f < 1}
    assert (X0 - 1, X0) in pairs and (31, 32) in pairs


@pytest.mark.parametrize("H", ROWS)
def test_rows_cases_switch_the_tile_height_and_straddle_the_band_seams(H):
    c = gather_case("rows:%d" % H)
    lv = plan(c["maps"], c["rois"].shape[0], c["PW"], c["sr"])["levels"][0]
    assert lv["rows_per_wg"] == {63: 1, 64: 2, 65: 2}[H] and lv["bands"] == {63: 63, 64: 32, 65: 33}[H]
    seams, last = set(), False
    for g in geoms(c):
        _, counts, lo, hi, frac = g["ys"]
        if not g["xs"][1].any():
            continue
        seams |= {int(a) for a, b, ok, f in zip(lo, hi, counts, frac) if ok and 0 < f < 1 and a % 2 == 1 and b == a + 1}
        last |= bool(((hi == H - 1) & counts).any())
    assert len(seams) >= 8 and last                           # samples between an odd row and the next: a two-row tile's seam
    if H == 65:
        assert lv["bands"] * 2 - H == 1                       # the last band is one row


@pytest.mark.parametrize("R", ROUNDS)
def test_round_cases_cross_the_list_round_and_carry_sums(R):
    c = gather_case("round:%d" % R)
    p = plan(c["maps"], R, c["PW"], c["sr"])
    assert c["maps"] == ((64, 9),) and c["C"] == 4 and (c["PH"], c["PW"]) == (2, 2) and c["rois"].shape[0] == R
    assert p["rounds"] == {1024: 1, 1025: 2, 2049: 3}[R] and p["levels"][0]["rows_per_wg"] == (2 if R == 1024 else 1)
    gs = geoms(c)
    for first in range(CHUNK, R, CHUNK):                      # roi 1024 (and 2048): the only roi of a round's tail, or its head
        _, _, rows, cols = footprint(gs[first])
        assert rows and cols
        earlier = False
        for g in gs[:first]:
            _, _, r2, c2 = footprint(g)
            earlier |= bool(rows & r2) and bool(cols & c2)
        assert earlier                                        # ... lands on a pixel whose sum earlier rounds started


@pytest.mark.parametrize("C", CHANNELS)
def test_channel_cases_leave_the_intended_lanes_dead(C):
    c = gather_case("channels:%d" % C)
    assert c["maps"] == ((5, 10),) and c["rois"].shape[0] == 6 and c["C"] == C
    chunks, last_live = -(-C // 256), (C - 256 * (-(-C // 256) - 1)) // 4
    assert (chunks, last_live) == {4: (1, 1), 252: (1, 63), 256: (1, 64), 260: (2, 1), 516: (3, 1)}[C]


@pytest.mark.parametrize("PH,PW,sr", GRIDS)
def test_grid_cases_take_their_route_and_fill_the_load_groups(PH, PW, sr):
    c = gather_case("grids:%dx%dx%d" % (PH, PW, sr))
    p = plan(c["maps"], c["rois"].shape[0], PW, sr)
    assert p["route"] == ("table" if PW > 14 else "segment")
    assert p["instance"] == (7 if PW <= 7 else 14, 2 if sr == 2 else 0)
    assert ((PH * sr == MAX_SAMPLES or PW * sr == MAX_SAMPLES)
            == ((PH, PW, sr) in [(8, 8, 4), (16, 3, 2), (3, 16, 2), (2, 16, 2)]))
    assert len({g["l"] for g in geoms(c)}) == 4
    # the sub-pixel rois: all PH bins on one pixel row, all PW bins on one pixel column
    for r in (0, 1):
        g = _geom(c, r)
        assert fully_inside(g)
        rows, cols = bins_on_row(g, PH, sr, "ys"), bins_on_row(g, PW, sr, "xs")
        assert max(len(v) for v in rows.values()) == PH and max(len(v) for v in cols.values()) == PW
    if (PH, PW) in ((7, 7), (14, 14)) and sr == 2:
        trips = -(-PH // 3)                                   # the three-bin load group over PH row bins
        assert trips == {7: 3, 14: 5}[PH] and PH % 3 != 0     # ... ends in a partial trip


def test_grid_table_covers_what_the_issue_lists():
    assert {(sr * sr) for _, _, sr in GRIDS} >= {1, 4, 9, 16, 25}      # power-of-two counts (1, 4, 16) and others (9, 25)
    assert any(PH == 16 for PH, _, _ in GRIDS) and sum(PW > 14 for _, PW, _ in GRIDS) == 2
    assert any(PH != PW and PW <= 14 for PH, PW, _ in GRIDS)
    assert {(PH, PW) for PH, PW, _ in FWD_GRIDS} == {(1, 1), (7, 7), (14, 14), (5, 9)} and {s for _, _, s in FWD_GRIDS} == {0, 1, 2, 3}
    assert any(sr == 0 for n in SCATTER_NAMES if n.startswith("grids") for sr in [int(n.split("x")[-1])])


def test_empty_case_leaves_an_image_and_a_level_without_rois():
    c = gather_case("empty")
    gs = geoms(c)
    assert len(c["maps"]) == 3 and c["N"] == 2
    assert {g["n"] for g in gs} == {0} and {g["l"] for g in gs} == {0, 2}
    assert not gs[0]["ys"][1].any() and not gs[0]["xs"][1].any()          # outside on both axes: the record with no level
    assert not gs[1]["ys"][1].any() and gs[1]["xs"][1].all()              # outside on one axis only
    assert sum(bool(footprint(g)[2]) for g in gs) >= 8
    back = ref_backward("gather", "empty")
    assert not back[1].any() and not back[0][1].any() and back[0][0].any() and back[2][0].any()


@pytest.mark.parametrize("table,name", [("gather", "clamped"), ("scatter", "clamped_adaptive")])
def test_clamped_case_has_indices_out_of_range_on_both_sides(table, name):
    c = _case(table, name)
    nl = len(c["maps"])
    assert {-1.0, float(c["N"])} <= set(c["rois"][:, 0].tolist())
    assert {c["lvl_min"] - 1, c["lvl_min"] + nl} <= set(c["levels"].tolist())
    for r, g in enumerate(geoms(c)):
        assert g["n"] == min(max(int(c["rois"][r, 0]), 0), c["N"] - 1)
        assert g["l"] == min(max(int(c["levels"][r]) - c["lvl_min"], 0), nl - 1)


def test_thin_levels_reach_the_one_pixel_maps():
    c = gather_case("thin_levels")
    assert len(c["maps"]) == 8 and c["maps"][-2:] == ((1, 2), (1, 1)) and c["N"] == 3
    hit = {(g["l"], g["n"]) for g in geoms(c) if footprint(g)[2]}
    assert {l for l, _ in hit} == set(range(8)) and {n for _, n in hit} == {0, 1, 2}
    assert forward_case("grids:7x7x2")["maps"] == FIVE_MAPS


@pytest.mark.parametrize("sr", [2, 0])
def test_on_the_line_samples_sit_exactly_where_the_table_says(sr):
    c = _line_case(sr=sr)
    L = LINE_L
    seen = {}
    for g in geoms(c):
        for v, counts, lo, hi, frac in (g["ys"], g["xs"]):
            assert np.array_equal(v * 8, np.round(v * 8))                    # dyadic: fp32 holds them exactly
            for a, ok, p_lo, p_hi, f in zip(v, counts, lo, hi, frac):
                seen[float(a)] = (bool(ok), int(p_lo), int(p_hi), float(f))
    assert seen[-1.0] == (True, 0, 1, 0.0)                                    # exactly -1 counts and lands on pixel 0
    if sr == 2:
        assert seen[float(L)] == (True, L - 1, L - 1, 0.0)                    # exactly L counts and lands on pixel L-1
        assert seen[0.0][:2] == (True, 0) and seen[0.0][3] == 0.0
        assert seen[L - 1.0] == (True, L - 1, L - 1, 0.0)
        assert seen[3.0] == (True, 3, 4, 0.0)                                 # an interior integer
        assert seen[-1.25][0] is False and seen[L + 0.25][0] is False         # the first dyadic step outside: dropped
    else:
        g = _geom(c, len(LINE_AXIS) * 6 + 6)                                  # (start -1.5, length 4) on both axes
        assert g["bin_h"] == 2.0 and g["bin_w"] == 2.0 and (g["gh"], g["gw"]) == (2, 2)
        assert g["ys"][0].tolist() == [-1.0, 0.0, 1.0, 2.0] and g["ys"][1].all()
        assert {(g2["gh"], g2["gw"]) for g2 in geoms(c)} >= {(1, 1), (2, 2), (4, 4), (1, 4)}


def test_r0_case_takes_the_table_route():
    c = gather_case("r0")
    assert c["rois"].shape == (0, 5) and c["gout"].shape[0] == 0
    assert plan(c["maps"], 0, c["PW"], c["sr"])["route"] == "table"
    assert ref_forward("gather", "r0").shape == (0, 7, 7, 8) and not any(m.any() for m in ref_backward("gather", "r0"))


def test_adaptive_forward_cases_have_unequal_grids():
    for PH, PW in ((1, 1), (7, 7), (14, 14), (5, 9)):
        gs = geoms(forward_case("grids:%dx%dx0" % (PH, PW)))
        assert any(g["gh"] > g["gw"] for g in gs) and any(g["gw"] > g["gh"] for g in gs)
        assert max(max(g["gh"], g["gw"]) for g in gs) >= (3 if PH <= 7 else 2)      # (a 32 x 40 map holds 14 bins of <= 3 px)


# ---- the reference: adjoint identity, the constant channel ----------------------------------------------------------------

@pytest.mark.parametrize("table,name", _all_cases())
def test_reference_backward_is_the_adjoint_of_its_forward(table, name):
    c = _case(table, name)
    x = [f.double().requires_grad_(True) for f in c["feats"]]
    g = c["gout"].double()
    out = ref.roi_align_ref(x, c["scales"], c["rois"], c["levels"], c["PH"], c["PW"], c["sr"], c["lvl_min"], c["N"])
    auto = torch.autograd.grad(out, x, g, allow_unused=True) if out.requires_grad else [None] * len(x)     # (R = 0: no graph)
    back = ref_backward(table, name)
    lhs = float((out.detach() * g).sum())
    rhs = float(sum((a.detach() * b).sum() for a, b in zip(x, back)))
    scale = float(sum((a.detach().abs() * b.abs()).sum() for a, b in zip(x, back))) + 1.0
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)
    for a, b in zip(auto, back):
        a = torch.zeros_like(b) if a is None else a
        assert float((a - b).abs().max()) <= 1e-12 * (1.0 + float(b.abs().max()))


@pytest.mark.parametrize("table,name", [("gather", "rows:64"), ("gather", "on_the_line"), ("forward", "grids:7x7x0"),
                                        ("gather", "grids:8x8x4")])
def test_constant_channel_of_the_reference(table, name):
    """Forward of a fully-inside roi is 1 on the constant channel; the backward of a gradient of 1 sums to PH PW per such
    roi, and to the counted share of its samples otherwise."""
    c = _case(table, name)
    out, back, gs = ref_forward(table, name), ref_backward(table, name), geoms(c)
    inside = np.array([fully_inside(g) for g in gs])
    assert inside.any() and not inside.all()
    assert float((out[torch.from_numpy(inside)][..., 0] - 1.0).abs().max()) <= 1e-13
    want = sum(g["ys"][1].sum() * g["xs"][1].sum() / float(g["gh"] * g["gw"]) for g in gs)
    got = float(sum(m[..., 0].sum() for m in back))
    assert abs(got - want) <= 1e-10 * want and want >= c["PH"] * c["PW"] * inside.sum()


# ---- the reference against the C oracle ---------------------------------------------------------------------------------

ORACLE_FWD = FORWARD_NAMES
ORACLE_BWD = [n for n in GATHER_NAMES if n != "r0"]         # (no rois: nothing to compare)


def _bits_of(ts):
    return [bf16_bits(t.float().numpy()) for t in ts]


@pytest.mark.parametrize("name", ORACLE_FWD)
def test_reference_forward_agrees_with_the_oracle(oracle, name):
    c = forward_case(name)
    got = oracle.bf16_bits_to_f32(oracle.roi_align(_bits_of(c["feats"]), c["scales"], c["rois"], c["levels"], c["PH"], c["PW"],
                                                   c["sr"], c["lvl_min"]))
    close_bf16(got, ref_forward("forward", name).numpy(), "oracle forward " + name)


@pytest.mark.parametrize("table,name", [("gather", n) for n in ORACLE_BWD] + [("scatter", n) for n in SCATTER_NAMES])
def test_reference_backward_agrees_with_the_oracle(oracle, table, name):
    c = _case(table, name)
    got = oracle.roi_align(_bits_of(c["feats"]), c["scales"], c["rois"], c["levels"], c["PH"], c["PW"], c["sr"], c["lvl_min"],
                           grad_out_bits=bf16_bits(c["gout"].float().numpy()))
    for l, (g, w) in enumerate(zip(got, ref_backward(table, name))):
        close_scatter(g, w.numpy(), float(w.abs().max()), "oracle backward %s level %d" % (name, l))


# ---- mask targets -----------------------------------------------------------------------------------------------------

MT_H, MT_W, MT_N = 17, 23, 3
MT_SIZES = [1, 7, 14, 28]
MT_G = [1, 3]


def mt_masks(G):
    """[N,G,H,W] u8, the four kinds in turn: checkerboard, single pixel, full, ellipse."""
    m = np.zeros((MT_N, G, MT_H, MT_W), np.uint8)
    yy, xx = np.mgrid[0:MT_H, 0:MT_W]
    for n in range(MT_N):
        for g in range(G):
            k = (n * G + g) % 4 if G > 1 else (n + 3) % 4
            if k == 0:
                m[n, g] = (yy + xx) % 2
            elif k == 1:
                m[n, g, 5 + n, 9 + g] = 1
            elif k == 2:
                m[n, g] = 1
            else:
                m[n, g] = ((xx - 11.0) / 8.5) ** 2 + ((yy - 8.0) / 6.5) ** 2 <= 1.0
    return m


def _mt_draw(S, G, seed):
    rng = np.random.default_rng(seed)
    H, W = MT_H, MT_W
    boxes = []
    for n in range(MT_N):
        u = lambda a, b: float(rng.uniform(a, b))                      # noqa: E731
        boxes += [(n, u(2, 8), u(2, 6), u(12, 20), u(9, 14)),          # inside
                  (n, u(-9, -2), u(2, 6), u(6, 12), u(9, 14)),         # clipped left
                  (n, u(12, 16), u(2, 6), u(W + 2, W + 9), u(9, 14)),  # clipped right
                  (n, u(2, 8), u(-9, -2), u(12, 20), u(6, 10)),        # clipped top
                  (n, u(2, 8), u(8, 11), u(12, 20), u(H + 2, H + 9)),  # clipped bottom
                  (n, u(W + 3, W + 6), u(2, 6), u(W + 9, W + 15), u(9, 14)),   # fully outside
                  (n, u(-30, -20), u(-30, -20), u(-12, -5), u(-12, -5)),        # fully outside, top left
                  (n, u(9, 10), u(5, 6), 0.0, 0.0),                    # narrower than one pixel (x2, y2 set below)
                  (n, u(14, 18), u(10, 13), u(4, 8), u(3, 6)),         # inverted: width and height clamp to one pixel
                  (n, u(-3, 0), u(-3, 0), u(W, W + 3), u(H, H + 3))]   # the whole mask and a little more
    rois = np.asarray(boxes, np.float32)
    thin = np.arange(7, len(rois), 10)
    rois[thin, 3], rois[thin, 4] = rois[thin, 1] + 0.4, rois[thin, 2] + 0.3
    R = len(rois)
    matched = rng.integers(0, G, R).astype(np.int32)
    labels = rng.integers(1, 81, R).astype(np.int32)
    extra = rois[[0, 10, 20, 1, 11, 21]].copy()                         # rois that must come out as cls -1, target 0
    rois = np.concatenate([rois, extra])
    matched = np.concatenate([matched, np.array([-1, G, 0, 0, -1, G], np.int32)])
    labels = np.concatenate([labels, np.array([5, 5, 0, -1, -1, 0], np.int32)])
    return dict(rois=rois, matched=matched, labels=labels, masks=mt_masks(G), S=S, G=G)


def excluded_share(val, thresh, compared=None):
    near = np.abs(val - thresh) < BAND
    n = val.size if compared is None else int(compared.sum())
    return float(near.sum()) / max(n, 1), near


@functools.lru_cache(maxsize=None)
def mask_target_case(S, G):
    """Seeds are redrawn until at most MAX_EXCLUDED of the pixels sit in the band around 0.5."""
    for seed in range(900 + 10 * S + G, 900 + 10 * S + G + 4000, 97):
        c = _mt_draw(S, G, seed)
        tg, cls, val = ref.mask_target_ref(c["rois"], c["matched"], c["labels"], c["masks"], S)
        share, near = excluded_share(val, 0.5)
        if share <= MAX_EXCLUDED:
            c.update(target=tg, cls=cls, value=val, compare=~near, seed=seed)
            return c
    raise AssertionError("no seed keeps the excluded share under %g" % MAX_EXCLUDED)


@functools.lru_cache(maxsize=None)
def mask_target_dyadic():
    """S = 2, rois one pixel wide and high on a mask with a vertical edge (image 0: columns < 6 set) and a horizontal one
    (image 1: rows < 6 set): the samples sit at start + 0.25 and start + 0.75, so the interpolated value across the edge
    is exactly 1, 0.75, 0.5, 0.25 or 0 -- the >= 0.5 tie is hit exactly, and nothing is excluded."""
    masks = np.zeros((2, 1, MT_H, MT_W), np.uint8)
    masks[0, 0, :, :6] = 1
    masks[1, 0, :6, :] = 1
    rois = []
    for start in (4.0, 4.25, 4.5, 4.75, 5.0, 5.25):
        rois.append((0, start, 3.0, start + 1.0, 4.0))
        rois.append((1, 3.0, start, 4.0, start + 1.0))
        rois.append((0, start, 4.25, start + 0.5, 4.5))                  # narrower than a pixel: clamps to one
    rois = np.asarray(rois, np.float32)
    R = len(rois)
    c = dict(rois=rois, matched=np.zeros(R, np.int32), labels=np.full(R, 3, np.int32), masks=masks, S=2, G=1)
    tg, cls, val = ref.mask_target_ref(rois, c["matched"], c["labels"], masks, 2)
    c.update(target=tg, cls=cls, value=val, compare=np.ones_like(tg, bool))
    return c


@pytest.mark.parametrize("G", MT_G)
@pytest.mark.parametrize("S", MT_SIZES)
def test_mask_target_cases_cover_their_kinds_and_exclude_little(oracle, S, G):
    c = mask_target_case(S, G)
    assert c["masks"].shape == (MT_N, G, MT_H, MT_W) and set(c["rois"][:, 0].tolist()) == {0.0, 1.0, 2.0}
    share, near = excluded_share(c["value"], 0.5)
    assert share <= MAX_EXCLUDED and np.array_equal(~near, c["compare"])
    assert {-1, G} <= set(c["matched"].tolist()) and {-1, 0} <= set(c["labels"].tolist())
    bad = ~((c["labels"] > 0) & (c["matched"] >= 0) & (c["matched"] < G))
    assert bad.sum() == 6 and np.all(c["cls"][bad] == -1) and not c["target"][bad].any()
    assert np.array_equal(c["cls"][~bad], c["labels"][~bad])
    kinds = c["value"][:30].reshape(3, 10, S, S)
    assert not kinds[:, 5:7].any()                                      # fully outside: every sample dropped
    assert c["target"].any()
    r = c["rois"]
    assert np.all(r[7:30:10, 3] - r[7:30:10, 1] < 1) and np.all(r[8:30:10, 3] < r[8:30:10, 1])
    if S > 1:
        assert 0 < c["target"][~bad].mean() < 1
    # the C oracle states the same operation
    tg, cls = oracle.mask_target(c["rois"], c["matched"], c["labels"], c["masks"], S)
    assert np.array_equal(cls, c["cls"]) and np.array_equal(tg[c["compare"]], c["target"][c["compare"]])


def test_mask_target_dyadic_set_pins_the_tie(oracle):
    c = mask_target_dyadic()
    v = c["value"]
    assert np.array_equal(v * 16, np.round(v * 16)) and {0.25, 0.5, 0.75, 0.0, 1.0} <= set(np.unique(v).tolist())
    assert c["compare"].all() and np.all(c["target"][v == 0.5] == 1) and (v == 0.5).sum() >= 8
    assert np.all(c["target"][v == 0.25] == 0) and np.all(c["target"][v == 0.75] == 1)
    tg, cls = oracle.mask_target(c["rois"], c["matched"], c["labels"], c["masks"], 2)
    assert np.array_equal(tg, c["target"]) and np.array_equal(cls, c["cls"])


# ---- mask paste -----------------------------------------------------------------------------------------------------------

MP_FRAMES = [(6, 1028), (40, 64)]
MP_CASES = [(S, Cpad, frame, th) for S in (14, 28) for Cpad in (8, 88) for frame in MP_FRAMES for th in (0.5, 0.3)]
MP_IDS = ["S%d-C%d-%dx%d-t%g" % (S, Cpad, frame[0], frame[1], th) for S, Cpad, frame, th in MP_CASES]


def _mp_draw(S, Cpad, frame, seed):
    H, W = frame
    rng = np.random.default_rng(seed)
    j = lambda: float(rng.uniform(-0.45, 0.45))                          # noqa: E731  (corners stay clear of the .5 ties)
    xm, ym = W // 2, H // 2
    boxes = [(xm - 9 + j(), 1 + j(), xm + 12 + j(), H - 2 + j()),        # inside, fractional corners
             (-20 + j(), -8 + j(), 14 + j(), ym + j()),                  # clipped by the frame top-left
             (W - 12 + j(), ym + j(), W + 40 + j(), H + 30 + j()),       # clipped bottom-right
             (xm + j(), 1 + j(), xm + j(), H - 1 + j()),                 # one pixel wide
             (2.5, 1.5, 7.5, 4.5),                                       # half-way corners: 2, 2, 8, 4 (half-up: 3, 2, 8, 5)
             (30.5, 0.5, 41.5, 3.5),                                     # ... 30, 0, 42, 4
             (xm + 10.0, 4.0, xm - 10.0, 2.0),                           # inverted: nothing
             (0.0, 0.0, 0.0, 0.0),                                       # padding row (class -1)
             (0.0, 0.0, W - 1.0, H - 1.0),                               # the whole frame
             (5 + j(), 2 + j(), 7 + j(), 4 + j()),                       # 3 x 3 pixels: down-scaling by more than 4
             (-60.0 + j(), 1 + j(), -5.0 + j(), 4 + j()),                # fully outside: left
             (W + 5.0 + j(), 1 + j(), W + 60.0 + j(), 4 + j()),          # ... right
             (3 + j(), -40.0 + j(), 20 + j(), -3.0 + j()),               # ... above
             (3 + j(), H + 3.0 + j(), 20 + j(), H + 40.0 + j()),         # ... below
             (4 + j(), 1 + j(), 30 + j(), 5 + j()),                      # class = Cpad
             (4 + j(), 1 + j(), 30 + j(), 5 + j()),                      # class = Cpad + 1: nothing
             (-200.0 + j(), -150.0 + j(), 300.0 + j(), 250.0 + j())]     # 500 x 400: up-scaling by more than 10
    if W > 1024:
        boxes.append((1000.3, 1 + j(), 1027.0, 4 + j()))                 # straddles the x-block seam 1023 | 1024
    R = len(boxes)
    cls = np.array([1 + (3 * k) % Cpad for k in range(R)], np.float32)
    cls[7], cls[14], cls[15] = -1, Cpad, Cpad + 1
    dets = np.zeros((R, 6), np.float32)
    dets[:, :4], dets[:, 4], dets[:, 5] = np.asarray(boxes, np.float32), rng.uniform(0.1, 1, R), cls
    logits = bf16(rng.standard_normal((R, S, S, Cpad)) * 3.0)
    if W > 1024:                                                         # set and clear pixels on both sides of the seam
        logits[17, :, :, int(cls[17]) - 1] = np.where(np.arange(S) % 2, 3.0, -3.0)[None, :]
    return dict(logits=logits, dets=dets, H=H, W=W, S=S, Cpad=Cpad)


@functools.lru_cache(maxsize=None)
def mask_paste_case(S, Cpad, frame, thresh):
    for seed in range(1300 + S + Cpad, 1300 + S + Cpad + 4000, 89):
        c = _mp_draw(S, Cpad, frame, seed)
        m, val = ref.mask_paste_ref(c["logits"], c["dets"], c["H"], c["W"], thresh)
        share, near = excluded_share(val, float(np.float32(thresh)), val > 0)    # of the pixels inside a pasted box
        if share <= MAX_EXCLUDED:
            c.update(mask=m, value=val, compare=~near, thresh=thresh, seed=seed)
            return c
    raise AssertionError("no seed keeps the excluded share under %g" % MAX_EXCLUDED)


@pytest.mark.parametrize("S,Cpad,frame,thresh", MP_CASES, ids=MP_IDS)
def test_mask_paste_cases_cover_their_kinds_and_exclude_little(oracle, S, Cpad, frame, thresh):
    c = mask_paste_case(S, Cpad, frame, thresh)
    H, W = frame
    m, val, d = c["mask"], c["value"], c["dets"]
    share, near = excluded_share(val, float(np.float32(thresh)), val > 0)
    assert share <= MAX_EXCLUDED and W % 4 == 0
    for r in (6, 7, 10, 11, 12, 13, 15):
        assert not val[r].any()                                          # inverted, padding, outside on each side, class > Cpad
    for r in (0, 1, 2, 3, 4, 5, 8, 9, 14, 16):
        assert val[r].any() and m[r].any()
    assert d[14, 5] == Cpad and d[15, 5] == Cpad + 1
    assert (d[16, 2] - d[16, 0]) / S > 10 and S / 3.0 > 4 and np.count_nonzero(val[9].any(0)) == 3
    assert np.nonzero(val[4].any(0))[0].tolist() == list(range(2, 9)) and np.nonzero(val[4].any(1))[0].tolist() == [2, 3, 4]
    assert np.nonzero(val[5].any(0))[0].tolist() == list(range(30, 43)) and np.nonzero(val[5].any(1))[0].tolist() == [0, 1, 2, 3, 4]
    if W > 1024:
        cols = np.nonzero(val[17].any(0))[0]
        assert cols.min() == 1000 and cols.max() == 1027 and W - 1024 == 4   # the second x-block has one live lane
        assert m[17][:, 1024:].any() and m[17][:, :1024].any()
    want = oracle.mask_paste(c["logits"], d, H, W, thresh)
    assert np.array_equal(want[c["compare"]], m[c["compare"]])
