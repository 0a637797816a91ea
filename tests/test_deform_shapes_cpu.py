"""Shape-dependent branches of csrc/deform_conv.hip and csrc/deform_roi_pool.hip: the input generators of
tests/test_gpu_deform_conv_shapes.py and tests/test_gpu_deform_roi_pool_shapes.py, and, checked here without a GPU, the
property each generated case exists for (a generator that silently misses its branch makes its GPU test worthless).

Two numpy restatements of how the kernels bucket work (index arithmetic only):
  dcn_list_counts   entries per col2im list = in-map corners of the valid samples per (g, n, y, x);
  dpool_round_hits  per 8-pixel row segment of the feature adjoint, the roi rounds (r // 1024) whose sample box reaches it.
"""
import numpy as np
import pytest
import torch

from test_deform_roi_pool_cpu import _geometry, _samples
from test_gpu_deform_conv import _bf16, _offsets

SCAN_BLOCK = 2048          # lists per scan workgroup (kScanThreads * kScanPerThread)
SCAN_THREADS = 256         # block sums per pass of deform_scan_blocks_kernel
DP_CHUNK = 1024            # rois per list round of dpool_gather_kernel (kSegChunk)
DP_SEG = 8                 # pixels per wave (kSegW)
DP_CLEAR = 2.0 ** -10      # px: every generated dpool sample keeps this distance from the lines below
AWAY = -100.0              # an offset that puts a sample outside every map used here (|AWAY| < 128, bf16-exact)


# ---- deformable convolution ---------------------------------------------------------------------------------------------

def dcn_case(N, H, W, C, stride=1, pad=1, G=1, mod=True, seed=0):
    Ho, Wo = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    Coff = ((27 if mod else 18) * G // 8 + 1) * 8      # a multiple of 8 with padding channels behind the real ones
    return dict(N=N, H=H, W=W, C=C, stride=stride, pad=pad, G=G, mod=mod, seed=seed, Ho=Ho, Wo=Wo, Coff=Coff)


def dcn_nl(c):
    return c["G"] * c["N"] * c["H"] * c["W"]


def dcn_nb(c):
    return -(-dcn_nl(c) // SCAN_BLOCK)


def dcn_seg_width(c):
    """L of col2im_coord: the largest power of two <= 8 dividing C / (8 G)."""
    cgg, L = c["C"] // (8 * c["G"]), 8
    while cgg % L:
        L >>= 1
    return L


def dcn_random_offsets(c):
    rng = np.random.default_rng(c["seed"])
    return _offsets(rng, c["N"], c["Ho"], c["Wo"], c["Coff"], c["G"], c["mod"], c["H"], c["W"])


def dcn_positions(c, off):
    """(py, px) [N,Ho,Wo,G,9] of every sample, float32 as the kernel computes them (exact for bf16 offsets)."""
    base_y = (np.arange(c["Ho"]) * c["stride"] - c["pad"]).astype(np.float32)[None, :, None, None, None]
    base_x = (np.arange(c["Wo"]) * c["stride"] - c["pad"]).astype(np.float32)[None, None, :, None, None]
    k = np.arange(9)
    o = off[..., :18 * c["G"]].reshape(c["N"], c["Ho"], c["Wo"], c["G"], 9, 2).astype(np.float32)
    py = base_y + (k // 3).astype(np.float32) + o[..., 0]
    px = base_x + (k % 3).astype(np.float32) + o[..., 1]
    return py, px


def dcn_list_counts(c, off):
    """[G,N,H,W] entries per list: every corner inside the map of every sample inside (-1, H) x (-1, W)."""
    H, W = c["H"], c["W"]
    py, px = dcn_positions(c, off)
    valid = (py > -1) & (py < H) & (px > -1) & (px < W)
    y0, x0 = np.floor(py).astype(np.int64), np.floor(px).astype(np.int64)
    n = np.broadcast_to(np.arange(c["N"])[:, None, None, None, None], py.shape)
    g = np.broadcast_to(np.arange(c["G"])[None, None, None, :, None], py.shape)
    cnt = np.zeros((c["G"], c["N"], H, W), np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            y, x = y0 + dy, x0 + dx
            m = valid & (y >= 0) & (y < H) & (x >= 0) & (x < W)
            np.add.at(cnt, (g[m], n[m], y[m], x[m]), 1)
    return cnt


# A.1 scan sizes: one block + a few lists, tens of blocks, and more blocks than one pass of the block-sum scan holds
SCAN_CASES = {
    "two_blocks": (dcn_case(1, 46, 45, 16, seed=101), (2, 2)),
    "tens_of_blocks": (dcn_case(2, 120, 150, 16, G=2, seed=102), (20, 64)),
    "carry_loop": (dcn_case(1, 728, 728, 8, seed=103), (SCAN_THREADS + 1, 4 * SCAN_THREADS)),
}

# A.2 long lists: per group, (number of (pixel, tap) samples aimed at one position, target y, target x); the four pixels
# around (ty + 0.5, tx + 0.5) of image 1 collect lists of exactly that length, nothing else reaches them
LONG_SHAPE = dict(N=2, H=24, W=40)
LONG_CASES = {
    "len63": (dcn_case(C=32, G=1, seed=201, **LONG_SHAPE), [(63, 5, 7)]),
    "len64": (dcn_case(C=32, G=1, seed=202, **LONG_SHAPE), [(64, 17, 30)]),
    "len65": (dcn_case(C=32, G=1, seed=203, **LONG_SHAPE), [(65, 11, 3)]),
    "len300": (dcn_case(C=32, G=1, seed=204, **LONG_SHAPE), [(300, 20, 21)]),
    "two_groups": (dcn_case(C=32, G=2, seed=205, **LONG_SHAPE), [(65, 3, 33), (400, 15, 12)]),
    "len65_v1": (dcn_case(C=32, G=1, mod=False, seed=206, **LONG_SHAPE), [(65, 9, 20)]),
    "len300_v1": (dcn_case(C=32, G=1, mod=False, seed=207, **LONG_SHAPE), [(300, 6, 30)]),
}
LONG_CAP = 1024            # the fallback sort is quadratic: keep every list at or under this


def dcn_long_list_offsets(c, targets):
    """Random offsets, except that (1) the first `count` (pixel, tap) pairs of a 6-wide block of output pixels of image 1
    all sample (ty + 0.5, tx + 0.5) and (2) every other sample that would touch one of the four pixels around that
    position is sent off the map. Offsets stay bf16-exact: integers and halves below 128."""
    off = dcn_random_offsets(c).copy()
    assert c["stride"] == 1 and c["pad"] == 1 and len(targets) == c["G"]
    py, px = dcn_positions(c, off)
    for g, (count, ty, tx) in enumerate(targets):
        y0, x0 = np.floor(py[..., g, :]), np.floor(px[..., g, :])
        near = (np.abs(y0 - ty) <= 1) & (np.abs(x0 - tx) <= 1)
        near[0] = False                                     # the target is in image 1; image 0 keeps its random lists
        n, ho, wo, k = np.nonzero(near)
        off[n, ho, wo, g * 18 + 2 * k] = AWAY
        off[n, ho, wo, g * 18 + 2 * k + 1] = AWAY
        for i in range(count):
            pix, k = divmod(i, 9)
            ho, wo = 2 + pix // 6, 4 + pix % 6
            off[1, ho, wo, g * 18 + 2 * k] = ty + 0.5 - (ho - 1 + k // 3)
            off[1, ho, wo, g * 18 + 2 * k + 1] = tx + 0.5 - (wo - 1 + k % 3)
    assert np.array_equal(off, _bf16(off)) and np.abs(off[..., :18 * c["G"]]).max() < 128
    return off


def dcn_order_sensitive_dcol(c, targets):
    """A column gradient whose fp32 list sums depend on the order of the terms, visibly after the rounding to bf16: small
    terms +-2^e (e in -3..3) everywhere, and in every channel of the targeted list a quarter of the entries +2^24 and
    another quarter -2^24 at random places. The large terms cancel exactly; which small terms are absorbed while the
    running sum is large depends on where they stand."""
    rng = np.random.default_rng(c["seed"] + 11)
    shape = (c["N"], c["Ho"], c["Wo"], 9 * c["C"])
    dcol = (np.sign(rng.standard_normal(shape)) * 2.0 ** rng.integers(-3, 4, shape)).astype(np.float32)
    Cg = c["C"] // c["G"]
    for g, (count, ty, tx) in enumerate(targets):
        for ch in range(g * Cg, (g + 1) * Cg):
            where = rng.permutation(count)[:2 * (count // 4)]
            for j, i in enumerate(where):
                pix, k = divmod(int(i), 9)
                dcol[1, 2 + pix // 6, 4 + pix % 6, k * c["C"] + ch] = 2.0 ** 24 if j % 2 else -2.0 ** 24
    return dcol


def dcn_key_order_sum(c, targets, dcol, order=None):
    """What col2im promises for the four pixels around each target of dcn_long_list_offsets (v1): the fp32 sum of
    weight * dcol row over the list in ascending key = (output pixel, tap) order, rounded once to bf16. Every weight is
    0.5 * 0.5. Returns [G][Cg] float32 (the four pixels get the same entries). order: a permutation to sum in instead."""
    assert not c["mod"]
    Cg = c["C"] // c["G"]
    sums = []
    for g, (count, ty, tx) in enumerate(targets):
        acc = np.zeros(Cg, np.float32)
        for i in (range(count) if order is None else order[g]):
            pix, k = divmod(i, 9)
            d = dcol[1, 2 + pix // 6, 4 + pix % 6, k * c["C"] + g * Cg:k * c["C"] + (g + 1) * Cg]
            acc = acc + np.float32(0.25) * d.astype(np.float32)
        sums.append(_bf16(acc))
    return sums


# A.3 segment widths of col2im_coord: C / (8 G) in {1, 2, 3, 6} -> L = 1, 2, 1, 2; 189 output pixels
SEG_CASES = {
    "cgg1": (dcn_case(3, 7, 9, 8, G=1, seed=301), 1, 1),
    "cgg2": (dcn_case(3, 7, 9, 32, G=2, seed=302), 2, 2),
    "cgg3": (dcn_case(3, 7, 9, 24, G=1, seed=303), 3, 1),
    "cgg6": (dcn_case(3, 7, 9, 96, G=2, seed=304), 6, 2),
}

# A.4 geometry: pad 0 / 2, stride 3, maps 1 or 2 pixels high or wide (every sample has corners off the map)
GEOM_CASES = {
    "pad0": dcn_case(2, 9, 11, 16, pad=0, seed=401),
    "pad2_v1_g2": dcn_case(2, 9, 11, 16, pad=2, G=2, mod=False, seed=402),
    "stride3": dcn_case(2, 13, 17, 16, stride=3, seed=403),
    "stride3_pad0": dcn_case(2, 10, 14, 16, stride=3, pad=0, seed=404),
    "stride3_pad2": dcn_case(2, 8, 11, 16, stride=3, pad=2, mod=False, seed=405),
    "h1": dcn_case(2, 1, 12, 16, seed=406),
    "w1": dcn_case(2, 12, 1, 16, G=2, seed=407),
    "h2_pad2": dcn_case(2, 2, 9, 16, pad=2, seed=408),
    "w2": dcn_case(2, 7, 2, 16, mod=False, seed=409),
    "h1_w1": dcn_case(64, 1, 1, 8, seed=410),
}

# A.5 exact edges on a 6 x 6 map (stride 1, pad 1): output row ho puts all its taps at the y position below, output column
# wo at the x position of the same table (L = H = W = 6). "0": outside the open window (-1, L), the column entry is zero.
#   index   position        col
#   0       -1 + 2^-7       2^-7 of pixel 0 (the other corner is off the map)
#   1       -1              0
#   2       L               0
#   3       L - 1           pixel L-1 itself (the other corner is off the map, weight 0)
#   4       random          bilinear
#   5       L - 2^-7        2^-7 of pixel L-1
EDGE_L = 6
EDGE_POS = [-1 + 2.0 ** -7, -1.0, float(EDGE_L), EDGE_L - 1.0, None, EDGE_L - 2.0 ** -7]
EDGE_ZERO = [False, True, True, False, False, False]


def dcn_edge_case(mod, G=1):
    return dcn_case(2, EDGE_L, EDGE_L, 16 * G, G=G, mod=mod, seed=501 + int(mod))


def dcn_edge_offsets(c):
    off = dcn_random_offsets(c).copy()
    rng = np.random.default_rng(c["seed"] + 1000)
    off[..., :18 * c["G"]] = _bf16(rng.uniform(-1.5, 0.9, off[..., :18 * c["G"]].shape))     # index 4: inside, fractional
    for i, pos in enumerate(EDGE_POS):
        if pos is None:
            continue
        for g in range(c["G"]):
            for k in range(9):
                off[:, i, :, g * 18 + 2 * k] = pos - (i - 1 + k // 3)
                off[:, :, i, g * 18 + 2 * k + 1] = pos - (i - 1 + k % 3)
    return off


def dcn_integer_offsets(c):
    """Random offsets with every (dy, dx) an integer in [-3, 3]: samples sit on pixels or outside the map."""
    off = dcn_random_offsets(c).copy()
    rng = np.random.default_rng(c["seed"] + 2000)
    off[..., :18 * c["G"]] = rng.integers(-3, 4, off[..., :18 * c["G"]].shape)
    return off


INT_CASES = {
    "s1": dcn_case(2, 9, 13, 32, G=2, mod=False, seed=511),
    "s2_pad2": dcn_case(2, 10, 7, 16, stride=2, pad=2, mod=False, seed=512),
}

# A.6 the DCN layers of ResNet-50 at 800 x 1344: conv2 of C3's stride-2 first block (200 x 336 in, 100 x 168 out), C4, C5
BENCH_LAYERS = {"c3_stride2": (200, 336, 128, 2), "c4": (50, 84, 256, 1), "c5": (25, 42, 512, 1)}


def dcn_bench_case(layer, G):
    H, W, C, s = BENCH_LAYERS[layer]
    return dcn_case(1, H, W, C, stride=s, G=G, mod=True, seed=601 + G)


@pytest.mark.parametrize("name", sorted(SCAN_CASES))
def test_scan_cases_reach_their_block_counts(name):
    c, (lo, hi) = SCAN_CASES[name]
    assert lo <= dcn_nb(c) <= hi, (dcn_nl(c), dcn_nb(c))
    if name == "carry_loop":
        # the block sums of the second pass of the carry loop are not all zero: the last lists hold entries
        cnt = dcn_list_counts(c, dcn_random_offsets(c)).reshape(-1)
        assert cnt[SCAN_THREADS * SCAN_BLOCK:].sum() > 0 and cnt[:SCAN_THREADS * SCAN_BLOCK].sum() > 0


@pytest.mark.parametrize("name", sorted(LONG_CASES))
def test_long_list_cases_have_exactly_the_intended_lengths(name):
    c, targets = LONG_CASES[name]
    cnt = dcn_list_counts(c, dcn_long_list_offsets(c, targets))
    for g, (count, ty, tx) in enumerate(targets):
        assert np.all(cnt[g, 1, ty:ty + 2, tx:tx + 2] == count), cnt[g, 1, ty:ty + 2, tx:tx + 2]
        rest = cnt[g].copy()
        rest[1, ty:ty + 2, tx:tx + 2] = 0
        assert rest.max() < min(count, 64)                 # the target lists are the longest of their group
        assert rest.max() > 9                              # and the background is ordinary
    assert cnt.max() == max(t[0] for t in targets) and cnt.max() <= LONG_CAP


@pytest.mark.parametrize("name", ["len65_v1", "len300_v1"])
def test_key_order_sum_depends_on_the_order(name):
    """The crafted column gradient tells a list summed in key order from the same list summed in any other order."""
    c, targets = LONG_CASES[name]
    dcol = dcn_order_sensitive_dcol(c, targets)
    assert np.array_equal(dcol, _bf16(dcol))
    want = dcn_key_order_sum(c, targets, dcol)[0]
    rng = np.random.default_rng(1)
    n = targets[0][0]
    for order in (list(range(n))[::-1], list(rng.permutation(n)), list(range(64, n)) + list(range(64))):
        other = dcn_key_order_sum(c, targets, dcol, [order])[0]
        assert (other != want).mean() > 0.25


def test_long_list_lengths_cover_both_sides_of_the_wave_sort():
    lens = sorted(t[0] for _, ts in LONG_CASES.values() for t in ts)
    assert 63 in lens and 64 in lens and 65 in lens and any(200 <= n <= LONG_CAP for n in lens)
    c, targets = LONG_CASES["two_groups"]
    assert c["G"] == 2 and targets[0][1:] != targets[1][1:]


@pytest.mark.parametrize("name", sorted(SEG_CASES))
def test_segment_cases_have_their_width_and_a_partial_last_wave(name):
    c, cgg, L = SEG_CASES[name]
    assert c["C"] // (8 * c["G"]) == cgg and dcn_seg_width(c) == L
    P = c["N"] * c["Ho"] * c["Wo"]
    assert (P * 9 * c["G"] * L) % 64 != 0 and P * 9 * c["G"] * L > 256
    assert c["Coff"] > 27 * c["G"]                          # there are padding channels to find zeroed


def test_segment_cases_cover_the_strided_loop():
    assert sorted((cgg, L) for _, cgg, L in SEG_CASES.values()) == [(1, 1), (2, 2), (3, 1), (6, 2)]


@pytest.mark.parametrize("name", sorted(GEOM_CASES))
def test_geometry_cases_are_accepted_shapes_with_live_samples(name):
    c = GEOM_CASES[name]
    assert c["Ho"] > 0 and c["Wo"] > 0
    py, px = dcn_positions(c, dcn_random_offsets(c))
    valid = (py > -1) & (py < c["H"]) & (px > -1) & (px < c["W"])
    assert valid.any() and not valid.all()
    if min(c["H"], c["W"]) <= 2:
        # every valid sample in a 1-pixel-thin map, and most in a 2-pixel one, has a corner off the map
        thin_y, thin_x = c["H"] <= 2, c["W"] <= 2
        y0, x0 = np.floor(py), np.floor(px)
        offmap = (thin_y & ((y0 < 0) | (y0 + 1 >= c["H"]))) | (thin_x & ((x0 < 0) | (x0 + 1 >= c["W"])))
        assert offmap[valid].mean() > 0.5
    assert sorted({(v["pad"], v["stride"]) for v in GEOM_CASES.values()}) == [(0, 1), (0, 3), (1, 1), (1, 3), (2, 1), (2, 3)]


@pytest.mark.parametrize("mod", [False, True])
def test_edge_offsets_are_bf16_exact_and_land_where_the_table_says(mod):
    c = dcn_edge_case(mod)
    off = dcn_edge_offsets(c)
    assert np.array_equal(off, _bf16(off))
    py, px = dcn_positions(c, off)
    for i, pos in enumerate(EDGE_POS):
        if pos is not None:
            assert np.all(py[:, i] == np.float32(pos)) and np.all(px[:, :, i] == np.float32(pos))
            assert EDGE_ZERO[i] == (not (-1 < pos < EDGE_L))
    assert np.all((py[:, 4] > -1) & (py[:, 4] < EDGE_L) & (py[:, 4] != np.floor(py[:, 4])))


@pytest.mark.parametrize("name", sorted(INT_CASES))
def test_integer_offsets_put_every_sample_on_a_pixel_or_outside(name):
    c = INT_CASES[name]
    py, px = dcn_positions(c, dcn_integer_offsets(c))
    assert np.all(py == np.floor(py)) and np.all(px == np.floor(px)) and not c["mod"]
    inside = (py >= 0) & (py < c["H"]) & (px >= 0) & (px < c["W"])
    assert 0.2 < inside.mean() < 0.95
    # the last row / column (other corner off the map) and the row / column just outside are all present
    assert (py == c["H"] - 1).any() and (py == c["H"]).any() and (py == -1).any() and (px == c["W"]).any()


@pytest.mark.parametrize("layer", sorted(BENCH_LAYERS))
def test_bench_layers_are_the_resnet50_shapes(layer):
    c = dcn_bench_case(layer, 4)
    want = {"c3_stride2": (100, 168, 128), "c4": (50, 84, 256), "c5": (25, 42, 512)}[layer]
    assert (c["Ho"], c["Wo"], c["C"]) == want and dcn_seg_width(c) in (4, 8)
    assert dcn_nb(dcn_bench_case(layer, 1)) >= 1


# ---- deformable RoI pooling ---------------------------------------------------------------------------------------------

def dpool_case(R, C, maps=((32, 40), (16, 20), (8, 10), (4, 5)), stride0=4, lvl_min=2, N=2, pooled=(7, 7), S=4,
               trans_std=0.1, ts_pad=0, ms_pad=0, identical=None, shift_bins=2.0, seed=0):
    """CPU tensors of one call: bf16 maps[l] [N,H,W,C] at strides stride0 * 2^l, rois [R,5] f32 all over (and a little
    past) the image so that they overlap heavily, levels by size, trans of up to +-shift_bins bins (some bins pushed off
    the map), mask logits in [-3, 3], dout. identical = (first, count): that block of rois is one box."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    PH, PW = pooled
    NB = PH * PW
    nl = len(maps)
    img_h, img_w = maps[0][0] * stride0, maps[0][1] * stride0
    feats = [torch.randn((N, h, w, C), generator=g).to(torch.bfloat16) for h, w in maps]
    scales = [1.0 / (stride0 << l) for l in range(nl)]
    sz = np.exp(rng.uniform(np.log(4), np.log(1.2 * max(img_h, img_w)), (R, 2)))
    x1 = rng.uniform(-8, max(img_w - 4, 1), R)
    y1 = rng.uniform(-8, max(img_h - 4, 1), R)
    rois = np.stack([rng.integers(0, N, R), x1, y1, x1 + sz[:, 0], y1 + sz[:, 1]], 1).astype(np.float32)
    if R >= 4:
        rois[:2, 3:] = rois[:2, 1:3]                       # zero-size rois (the 0.1 clamp on the coarse levels)
    if identical is not None:
        first, count = identical
        rois[first:first + count] = np.array([1, 0.3 * img_w, 0.2 * img_h, 0.8 * img_w, 0.7 * img_h], np.float32)
    area = np.maximum(rois[:, 3] - rois[:, 1], 1) * np.maximum(rois[:, 4] - rois[:, 2], 1)
    lv = np.floor(np.log2(np.sqrt(area) / (4.0 * stride0)) + 1e-6).astype(np.int64)
    levels = (np.clip(lv, 0, nl - 1) + lvl_min).astype(np.int32)
    if R >= 4:
        levels[:2] = lvl_min + nl - 1
    amp = shift_bins / (max(PH, PW) * trans_std)
    trans = torch.zeros((R, 2 * NB + ts_pad))
    trans[:, :2 * NB] = (torch.rand((R, 2 * NB), generator=g) * 2 - 1) * amp
    if R >= 4:
        trans[2:4, :NB] = 40.0 / trans_std                 # bins far off the map (count 0)
    trans = _dpool_clear_of_grid_lines(trans.to(torch.bfloat16).float(), rois, levels, scales, pooled, S, trans_std,
                                       lvl_min, [m[1] for m in maps], [m[0] for m in maps], amp, rng)
    mask = torch.zeros((R, NB + ms_pad))
    mask[:, :NB] = (torch.rand((R, NB), generator=g) * 2 - 1) * 3
    dout = torch.randn((R, PH, PW, C), generator=g).to(torch.bfloat16)
    return dict(feats=feats, scales=scales, rois=torch.from_numpy(rois), levels=torch.from_numpy(levels),
                trans=trans.to(torch.bfloat16), mask=mask.to(torch.bfloat16), dout=dout, lvl_min=lvl_min, pooled=pooled,
                S=S, trans_std=trans_std, NB=NB)


def _dpool_clear_of_grid_lines(trans, rois, levels, scales, pooled, S, trans_std, lvl_min, Ws, Hs, amp, rng):
    """Redraw the trans of every bin that has a sample within DP_CLEAR of an integer coordinate or of a window edge
    (-0.5, L - 0.5). On those lines the operator is discontinuous (the count of a bin at the window edge; d_trans, a
    one-sided derivative, at an integer), and the kernels evaluate sample positions in fp32 as MXNet does while the
    reference uses fp64: with coordinates and shifts below 2^8 px and a handful of roundings of 2^-24 relative each, the
    two can disagree by up to about 2^-13 px, so a sample nearer than that to a line can fall on either side of it. With
    thousands of rois some always do; DP_CLEAR = 2^-10 px keeps the comparison away from them with a margin of 8."""
    PH, PW = pooled
    NB = PH * PW
    t = trans.numpy().astype(np.float64)
    i = np.arange(S)

    def bad_bins(r):
        l = int(levels[r]) - lvl_min
        rsw, rsh, roi_w, roi_h, sub_w, sub_h = _geometry(rois[r], scales[l], pooled, S)
        b = np.arange(NB)
        w = (b % PW) * (roi_w / PW) + rsw + t[r, :NB] * trans_std * roi_w
        h = (b // PW) * (roi_h / PH) + rsh + t[r, NB:2 * NB] * trans_std * roi_h
        out = np.zeros(NB, bool)
        for v, L in ((w[:, None] + i * sub_w, Ws[l]), (h[:, None] + i * sub_h, Hs[l])):
            d = np.minimum(np.abs(v - np.round(v)), np.minimum(np.abs(v + 0.5), np.abs(v - (L - 0.5))))
            out |= (d < DP_CLEAR).any(1)
        return np.nonzero(out)[0]

    for r in range(t.shape[0]):
        for _ in range(64):
            b = bad_bins(r)
            if b.size == 0:
                break
            for col in (b, NB + b):
                t[r, col] = _bf16(rng.uniform(-amp, amp, b.size))
        else:
            raise AssertionError("roi %d: could not move its samples off the grid lines" % r)
    return torch.from_numpy(t).float()


def dpool_round_hits(case):
    """{(level, image, row, 8-pixel segment): set of roi rounds r // 1024 whose valid samples' corner box reaches it}."""
    f64 = [f.double() for f in case["feats"]]
    rois, levels, trans = case["rois"].double(), [int(v) for v in case["levels"]], case["trans"].double()
    hits = {}
    for r in range(rois.shape[0]):
        s = _samples(f64, case["scales"], rois, levels, r, trans, case["pooled"], case["S"], case["trans_std"],
                     case["lvl_min"])
        v = s["valid"]
        if not v.any():
            continue
        ylo, yhi = int(s["y0"][v].min()), int(s["y1"][v].max())
        xlo, xhi = int(s["x0"][v].min()), int(s["x1"][v].max())
        for y in range(ylo, yhi + 1):
            for seg in range(xlo // DP_SEG, xhi // DP_SEG + 1):
                hits.setdefault((s["l"], s["n"], y, seg), set()).add(r // DP_CHUNK)
    return hits


# B.1 roi rounds: (R, block of identical boxes)
ROUND_CASES = {1023: None, 1025: (1000, 25), 2500: (2040, 16)}


def dpool_round_case(R):
    return dpool_case(R, 64, identical=ROUND_CASES[R], seed=700 + R)


# B.3 bin grids; B.4 narrow maps (one level, lvl_min = that level)
POOLED = [(1, 1), (3, 5), (8, 8)]
SAMPLES = [1, 2, 16]
TRANS_STD = [0.05, 0.5]
NARROW_W = [1, 7, 9, 33]


def dpool_grid_case(pooled, S, trans_std, padded):
    NB = pooled[0] * pooled[1]
    pad = (128 - 2 * NB, 64 - NB) if padded else (0, 0)
    if padded and pad[1] == 0:
        pad = (16, 8)
    return dpool_case(24, 16, pooled=pooled, S=S, trans_std=trans_std, ts_pad=pad[0], ms_pad=pad[1],
                      seed=800 + 10 * NB + S)


def dpool_narrow_case(W):
    return dpool_case(32, 16, maps=((11, W),), stride0=8, lvl_min=3, seed=900 + W)


@pytest.mark.parametrize("R", sorted(ROUND_CASES))
def test_roi_round_cases_mix_rounds_inside_row_segments(R):
    case = dpool_round_case(R)
    hits = dpool_round_hits(case)
    rounds = -(-R // DP_CHUNK)
    full = [k for k, v in hits.items() if len(v) == rounds]
    assert rounds == {1023: 1, 1025: 2, 2500: 3}[R]
    assert len(full) >= 8, (len(full), len(hits))                 # row segments that see rois of every round
    if R == 2500:                                                 # most of them do, on every level
        assert len(full) > len(hits) // 2 and {k[0] for k in full} == {0, 1, 2, 3}
    ident = ROUND_CASES[R]
    if ident is not None:
        first, count = ident
        assert first < DP_CHUNK * (first // DP_CHUNK + 1) < first + count      # the block straddles a round boundary
        assert torch.all(case["rois"][first:first + count] == case["rois"][first])
    assert len(set(case["levels"].tolist())) == 4


def test_grid_cases_cover_both_strides():
    for pooled in POOLED:
        NB = pooled[0] * pooled[1]
        a, b = dpool_grid_case(pooled, 2, 0.5, False), dpool_grid_case(pooled, 2, 0.5, True)
        assert a["trans"].shape[1] == 2 * NB and a["mask"].shape[1] == NB
        assert b["trans"].shape[1] > 2 * NB and b["mask"].shape[1] > NB
        assert torch.equal(a["trans"], b["trans"][:, :2 * NB]) and torch.equal(a["mask"], b["mask"][:, :NB])
        assert not b["trans"][:, 2 * NB:].any()


@pytest.mark.parametrize("W", NARROW_W)
def test_narrow_cases_are_single_level_and_hit_every_segment(W):
    case = dpool_narrow_case(W)
    assert len(case["feats"]) == 1 and case["feats"][0].shape[2] == W and set(case["levels"].tolist()) == {3}
    segs = {k[3] for k in dpool_round_hits(case)}
    assert segs == set(range(-(-W // DP_SEG)))
    assert W < 32 or W % 32 != 0
