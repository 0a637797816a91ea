"""The kernels of csrc/dense_misc.hip in the modes and at the sizes the models use and tests/test_gpu_dense.py does not reach:
the stem's wave-uniform interior path, accumulating and overwriting resampling adjoints, in-place elementwise calls, the
accumulating fp32 -> bf16 fold, layout changes over several tiles, the optimizer's tails.

Inputs are exact wherever the operation allows it, so there is no tolerance to argue about: small integers are bf16-exact,
integer products and sums below 2^24 are exact in fp32 in any order. The reference is then an fp64 computation followed by one
round-to-nearest-even to bf16, and the comparison is bit for bit (on the 16-bit patterns: -0.0 is not +0.0, NaN is not lost).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _same_bits(got, want, what):
    import torch
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), "%s: %s %s, want %s %s" % (
        what, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    view = {torch.bfloat16: torch.int16, torch.float32: torch.int32}[got.dtype]
    a, b = got.contiguous().view(view).cpu(), want.contiguous().view(view).cpu()
    if not torch.equal(a, b):
        idx = (a != b).nonzero()
        first = tuple(int(i) for i in idx[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r" % (
            what, idx.shape[0], a.numel(), first, float(got.cpu()[first]), float(want.cpu()[first])))


def _ints(g, shape, lo, hi, dtype=None):
    import torch
    t = torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)
    return t if dtype is None else t.to(dtype)


def _bf16(t):
    """fp64 / fp32 CPU tensor -> bf16 on the device, one round-to-nearest-even."""
    import torch
    return t.to(torch.float32).to(torch.bfloat16).cuda()


# ---- stem -------------------------------------------------------------------------------------------------------------------
STEM_SIZES = [(1, 19, 520), (2, 9, 131), (1, 6, 510), (1, 33, 64), (1, 1, 1), (1, 2, 3)]
SP_PC, SP_COLS, SP_ROWS = 63, 128, 5       # stem_pool_kernel: pooled columns per workgroup; stem columns / rows under a tile


def _interior_tiles(H, W):
    """The (ht, wt) workgroups of the fused stem + pool kernel that take its `interior` path, from the kernel's formulas:
    a workgroup owns pooled rows 2 ht, 2 ht + 1 and pooled columns 63 wt .. 63 wt + 62, i.e. stem rows cr0 .. cr0 + 4 and
    stem columns cc0 .. cc0 + 127 with cr0 = 4 ht - 1, cc0 = 126 wt - 1; interior = all of them inside the stem map."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    tiles = [(ht, wt) for ht in range((Hp + 1) // 2) for wt in range((Wp + SP_PC - 1) // SP_PC)]
    inside = [(ht, wt) for ht, wt in tiles
              if 4 * ht - 1 >= 0 and 4 * ht - 1 + SP_ROWS <= Ho and 2 * SP_PC * wt - 1 >= 0 and 2 * SP_PC * wt - 1 + SP_COLS <= Wo]
    return tiles, inside


def test_stem_sizes_cover_the_interior_path():
    """(19, 520): 3 x 3 workgroups, exactly the middle one is interior -- the path almost every workgroup of a real image
    takes; the other sizes have none (they cover the borders). A retiling of the kernel that loses this has to update the
    sizes here."""
    tiles, inside = _interior_tiles(19, 520)
    assert len(tiles) == 9 and inside == [(1, 1)]
    for _, h, w in STEM_SIZES[1:]:
        assert _interior_tiles(h, w)[1] == []
    assert (((520 - 1) // 2 + 1) + 127) // 128 == 3 and ((520 - 1) // 2 + 1) - 2 * 128 == 4    # unfused: a third, 4-pixel W tile


def _stem_reference(img, w, bias):
    """img [N,3,H,W], w [64,7,7,3], bias [64] or None: integer-valued fp64 -> (stem, pooled) as bf16, rounded once."""
    import torch
    import torch.nn.functional as F
    y = F.conv2d(img.double(), w.double().permute(0, 3, 1, 2), None if bias is None else bias.double(), stride=2, padding=3)
    y = torch.relu(y)
    assert float(y.max()) < 2 ** 24
    yb = y.to(torch.float32).to(torch.bfloat16)
    pooled = F.max_pool2d(yb.float(), 3, 2, 1).to(torch.bfloat16)
    return yb.permute(0, 2, 3, 1).contiguous().cuda(), pooled.permute(0, 2, 3, 1).contiguous().cuda()


@pytest.mark.parametrize("size", STEM_SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_stem_exact_integers(hip, size):
    """Image integers in [-4, 4], filter integers in [-2, 2], bias integers in [-8, 8]: |sum| <= 4 * 2 * 147 + 8 = 1184, every
    partial sum exact in fp32 in any order. The unfused stem, the fused stem + pool and maxpool(unfused) equal the reference
    bit for bit, with fp32 and bf16 images, with and without a bias."""
    import torch
    from mxdetection_amd.ops import dense
    Nn, H, W = size
    g = torch.Generator().manual_seed(H * 1000 + W)
    img = _ints(g, (Nn, 3, H, W), -4, 4)
    w = _ints(g, (64, 7, 7, 3), -2, 2)
    bias = _ints(g, (64,), -8, 8)
    # random sums stay below 256, where every integer is a bf16: a block of the image at +4 under three constant filters
    # gives sums up to 1176 + bias in its interior and a ramp of integers, ties among them, along its edges
    img[:, :, H // 4:, W // 3:2 * W // 3] = 4.0
    w[0], w[1], w[2] = 2.0, -2.0, 1.0
    wd = w.to(torch.bfloat16).cuda()
    for b in (bias, None):
        want, want_pool = _stem_reference(img, w, b)
        if H * W >= 64:                                 # values past the bf16-exact integers: the rounding is exercised
            assert float(want.float().max()) > 256
        bd = None if b is None else b.cuda()
        tag = "%s, bias %s" % (size, b is not None)
        for dt in (torch.float32, torch.bfloat16):
            image = img.to(dt).cuda()
            y = dense.stem_conv7x7(image, wd, bd, out=torch.full(tuple(want.shape), NAN, dtype=torch.bfloat16, device="cuda"))
            _same_bits(y, want, "stem %s, %s image" % (tag, dt))
            fused = dense.stem_conv7x7_pool(image, wd, bd,
                                            out=torch.full(tuple(want_pool.shape), NAN, dtype=torch.bfloat16, device="cuda"))
            _same_bits(fused, want_pool, "fused stem + pool %s, %s image" % (tag, dt))
            _same_bits(dense.maxpool3x3s2(y), want_pool, "maxpool(stem) %s" % tag)


@pytest.mark.parametrize("size", [(1, 19, 520), (2, 9, 131)], ids=lambda s: "%dx%dx%d" % s)
def test_stem_one_hot_filters_name_the_tap(hip, size):
    """Three launches; in launch j output channel co holds a single 1 at tap co + 64 j of the 147 (kh, kw, c): the output
    channel is the image plane c shifted by (kh - 3, kw - 3), sampled at stride 2, zero padded, ReLU'd."""
    import torch
    import torch.nn.functional as F
    from mxdetection_amd.ops import dense
    Nn, H, W = size
    g = torch.Generator().manual_seed(77)
    img = _ints(g, (Nn, 3, H, W), -4, 4)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    padded = F.pad(img, (3, 4, 3, 4))
    image = img.cuda()
    for j in range(3):
        w = torch.zeros((64, 147))
        want = torch.zeros((Nn, Ho, Wo, 64))
        for co in range(64):
            tap = co + 64 * j
            if tap >= 147:
                continue
            w[co, tap] = 1.0
            kh, kw, c = tap // 21, (tap % 21) // 3, tap % 3
            want[..., co] = torch.relu(padded[:, c, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2])
        wd = w.view(64, 7, 7, 3).to(torch.bfloat16).cuda()
        want = want.to(torch.bfloat16)
        want_pool = F.max_pool2d(want.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(torch.bfloat16)
        y = dense.stem_conv7x7(image, wd, None).cpu()
        fused = dense.stem_conv7x7_pool(image, wd, None).cpu()
        for co in range(64):
            tap = co + 64 * j
            name = "tap %d (kh %d, kw %d, c %d)" % (tap, tap // 21, (tap % 21) // 3, tap % 3) if tap < 147 else "empty filter %d" % co
            assert torch.equal(y[..., co], want[..., co]), "stem: " + name
            assert torch.equal(fused[..., co], want_pool[..., co]), "fused stem + pool: " + name


# ---- pooling and resampling -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (3, 5), (8, 6), (9, 7)], ids=lambda s: "%dx%d" % s)
def test_maxpool_both_signs(hip, hw, C):
    import torch
    import torch.nn.functional as F
    from mxdetection_amd.ops import dense
    g = torch.Generator().manual_seed(hw[0] * 10 + hw[1] + C)
    for lo, hi in ((-9, 9), (-9, -1)):                      # mixed signs; every window all negative
        x = _ints(g, (2,) + hw + (C,), lo, hi)
        want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()
        out = torch.full(tuple(want.shape), NAN, dtype=torch.bfloat16, device="cuda")
        _same_bits(dense.maxpool3x3s2(_bf16(x), out), want, "maxpool %s C %d values [%d, %d]" % (hw, C, lo, hi))


@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (9, 7), (8, 6)], ids=lambda s: "%dx%d" % s)
def test_subsample2_and_its_adjoint(hip, hw, C):
    import torch
    from mxdetection_amd.ops import dense
    g = torch.Generator().manual_seed(hw[0] * 10 + hw[1] + C)
    H, W = hw
    x = _ints(g, (2, H, W, C), -100, 100)
    sub = dense.subsample2(_bf16(x), torch.full((2, (H + 1) // 2, (W + 1) // 2, C), NAN, dtype=torch.bfloat16, device="cuda"))
    _same_bits(sub, _bf16(x[:, ::2, ::2]), "subsample2")
    dy = _ints(g, tuple(sub.shape), -100, 100)
    # overwriting form into NaN: dy on the even grid, zeros (not what was there) everywhere else
    dx = torch.full((2, H, W, C), NAN, dtype=torch.bfloat16, device="cuda")
    assert dense.subsample2_backward(_bf16(dy), dx, accumulate=False) is dx
    want = torch.zeros((2, H, W, C))
    want[:, ::2, ::2] = dy
    _same_bits(dx, _bf16(want), "subsample2_backward, overwriting")
    # accumulating form onto integers: exact
    old = _ints(g, (2, H, W, C), -100, 100)
    dx = _bf16(old)
    dense.subsample2_backward(_bf16(dy), dx, accumulate=True)
    _same_bits(dx, _bf16(want.double() + old.double()), "subsample2_backward, accumulating")


@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("hw", [(13, 10), (7, 5), (4, 3), (1, 1), (2, 2)], ids=lambda s: "%dx%d" % s)
def test_upsample2_backward_both_modes(hip, hw, C):
    """Exact integer sum of the up-to-four fine cells (+ the old content), rounded once. |sum| <= 5 * 60 = 300: sums past 256
    are rounded, and some land on ties."""
    import torch
    import torch.nn.functional as F
    from mxdetection_amd.ops import dense
    g = torch.Generator().manual_seed(hw[0] * 10 + hw[1] + C)
    Hf, Wf = hw
    Hc, Wc = (Hf + 1) // 2, (Wf + 1) // 2
    fine = _ints(g, (2, Hf, Wf, C), -60, 60)
    s = F.pad(fine.double(), (0, 0, 0, 2 * Wc - Wf, 0, 2 * Hc - Hf)).reshape(2, Hc, 2, Wc, 2, C).sum(dim=(2, 4))
    coarse = torch.full((2, Hc, Wc, C), NAN, dtype=torch.bfloat16, device="cuda")
    assert dense.upsample2_backward(_bf16(fine), coarse, accumulate=False) is coarse
    _same_bits(coarse, _bf16(s), "upsample2_backward, overwriting")
    old = _ints(g, (2, Hc, Wc, C), -60, 60)
    coarse = _bf16(old)
    dense.upsample2_backward(_bf16(fine), coarse, accumulate=True)
    _same_bits(coarse, _bf16(s + old.double()), "upsample2_backward, accumulating")


# ---- elementwise ------------------------------------------------------------------------------------------------------------
SHAPES_1D = [(8,), (2, 9, 7, 72)]          # one vector; 9072 elements: four full blocks of 256 x 8 and a partial fifth


@pytest.mark.parametrize("shape", SHAPES_1D, ids=["n8", "n9072"])
def test_add_and_relu_in_and_out_of_place(hip, shape):
    import torch
    from mxdetection_amd.ops import dense
    assert shape == (8,) or int(np.prod(shape)) % (256 * 8) != 0
    g = torch.Generator().manual_seed(len(shape))
    a, b = _ints(g, shape, -150, 150), _ints(g, shape, -150, 150)          # sums up to 300: some are rounded
    want = _bf16(a.double() + b.double())
    ad, bd = _bf16(a), _bf16(b)
    _same_bits(dense.add_bf16(ad, bd), want, "add_bf16")
    _same_bits(dense.add_bf16(ad, bd, torch.full(shape, NAN, dtype=torch.bfloat16, device="cuda")), want, "add_bf16 into out")
    _same_bits(ad, _bf16(a), "add_bf16 changed its input")
    acc = ad.clone()
    assert dense.add_bf16(acc, bd, acc) is acc                             # Bottleneck.backward / RetinaFPN.backward: in place
    _same_bits(acc, want, "add_bf16 in place")
    # ReLU backward: y with +0.0, -0.0, the smallest positive subnormal and normal bf16 and their negatives
    y = _bf16(b)
    special = np.array([0x0000, 0x8000, 0x0001, 0x0080, 0x8001, 0x8080, 0x7F7F, 0xFF7F], dtype=np.uint16).view(np.int16)
    y.view(-1)[:8] = torch.from_numpy(special).view(torch.bfloat16).cuda()
    passes = torch.tensor([False, False, True, True, False, False, True, False]).cuda()
    dy = ad.clone()
    dy.view(-1)[:8] = torch.arange(1, 9).to(torch.bfloat16).cuda()
    want = torch.where(y.float() > 0, dy, torch.zeros_like(dy))
    assert torch.equal(want.view(-1)[:8] != 0, passes)
    _same_bits(dense.relu_backward(dy, y), want, "relu_backward")
    g_in = dy.clone()
    assert dense.relu_backward(g_in, y, g_in) is g_in
    _same_bits(g_in, want, "relu_backward in place")
    # ReLU forward (RetinaFPN: out of place into a cached buffer); -0.0 and negatives become +0.0
    out = torch.full(shape, NAN, dtype=torch.bfloat16, device="cuda")
    assert dense.relu_forward(y, out) is out
    _same_bits(out, torch.where(y.float() > 0, y, torch.zeros_like(y)), "relu_forward")
    z = y.clone()
    dense.relu_forward(z, z)
    _same_bits(z, out, "relu_forward in place")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2055])
def test_f32_fold_to_bf16(hip, n, accumulate):
    """f32_to_bf16 and f32_accum_to_bf16 (the RoI extractor's fold): integer values, so the fp32 add is exact; sums on bf16
    ties of both parities (257 -> 256, 259 -> 260 and their negatives); 8 elements past the end stay untouched."""
    import torch
    from mxdetection_amd.ops import dense
    g = torch.Generator().manual_seed(n)
    ties = torch.tensor([257.0, 259.0, -257.0, -259.0, 513.0 + 1.0, 518.0, 1026.0, 1030.0])     # 514/518: ties at step 4
    old = _ints(g, (n,), -64, 64) if accumulate else torch.zeros((n,))
    total = _ints(g, (n,), -700, 700)
    total[:min(n, 8)] = ties[:min(n, 8)]
    if n > 8:
        total[-1] = 259.0                                            # a tie in the scalar tail too
    x = (total - old).cuda()                                         # x + old = total exactly
    want = _bf16(x.cpu().double() + old.double())
    assert not torch.equal(want.float().cpu(), total)                # something is rounded
    full = torch.full((n + 8,), -3.0, dtype=torch.bfloat16, device="cuda")
    full[:n] = _bf16(old) if accumulate else NAN
    y = full[:n]
    dense.f32_accum_to_bf16(x, y, accumulate)
    _same_bits(y, want, "f32_accum_to_bf16")
    assert (full[n:] == -3.0).all(), "wrote past the end"
    if not accumulate:
        out = torch.full((n,), NAN, dtype=torch.bfloat16, device="cuda")
        _same_bits(dense.f32_to_bf16(x, out), want, "f32_to_bf16")
        _same_bits(dense.f32_to_bf16(x), x.to(torch.bfloat16), "f32_to_bf16 vs torch")


@pytest.mark.parametrize("shape", [(2, 40, 3, 70), (1, 32, 1, 32), (1, 33, 2, 31), (2, 3, 5, 64)], ids=lambda s: "x".join(map(str, s)))
def test_layout_changes_over_several_tiles(hip, shape):
    """(N, C, H, W): several 32 x 32 tiles along both axes with partial last tiles; f32 and bf16 input; the two are inverses."""
    import torch
    from mxdetection_amd.ops import dense
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g)
    xb = x.to(torch.bfloat16)
    want = xb.permute(0, 2, 3, 1).contiguous().cuda()
    _same_bits(dense.nchw_to_nhwc(x.cuda()), want, "nchw_to_nhwc, f32 input")
    nhwc = dense.nchw_to_nhwc(xb.cuda())
    _same_bits(nhwc, want, "nchw_to_nhwc, bf16 input")
    back = dense.nhwc_to_nchw(nhwc)
    _same_bits(back, xb.float().cuda(), "nhwc_to_nchw")
    _same_bits(dense.nchw_to_nhwc(back), nhwc, "round trip")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_sgd_momentum_tails(hip, n):
    """The vector body and the scalar tail, with and without the bf16 copy (the binding passes None as a null pointer, which
    the kernel accepts), with lr as a float and as a device scalar: fp64 update within rtol = atol = 1e-6 (the bound of
    test_sgd_momentum), wb == bf16(w) and the forms among each other bit for bit."""
    import torch
    from mxdetection_amd.ops import dense
    g = torch.Generator().manual_seed(n)
    w0, g0, m0 = (torch.randn((n,), generator=g) for _ in range(3))
    lr, mom, wd, rescale = 0.02, 0.9, 1e-4, 0.5
    m_ref = mom * m0.double() + (g0.double() * rescale + wd * w0.double())
    w_ref = w0.double() - float(np.float32(lr)) * m_ref
    runs = {}
    for with_wb in (True, False):
        for dev_lr in (False, True):
            w, gr, m = w0.clone().cuda(), g0.clone().cuda(), m0.clone().cuda()
            full = torch.full((n + 8,), -3.0, dtype=torch.bfloat16, device="cuda")
            wb = full[:n] if with_wb else None
            dense.sgd_momentum_update(w, gr, m, wb, torch.tensor([lr], dtype=torch.float32).cuda() if dev_lr else lr, mom, wd,
                                      rescale)
            torch.cuda.synchronize()
            assert torch.allclose(m.cpu().double(), m_ref, rtol=1e-6, atol=1e-6)
            assert torch.allclose(w.cpu().double(), w_ref, rtol=1e-6, atol=1e-6)
            _same_bits(gr, g0.cuda(), "the gradient changed")
            if with_wb:
                _same_bits(wb, w.to(torch.bfloat16), "bf16 copy")
                assert (full[n:] == -3.0).all(), "wrote past the end"
            runs[(with_wb, dev_lr)] = (w, m)
    for key, (w, m) in runs.items():
        _same_bits(w, runs[(True, False)][0], "w of %s" % (key,))
        _same_bits(m, runs[(True, False)][1], "m of %s" % (key,))
