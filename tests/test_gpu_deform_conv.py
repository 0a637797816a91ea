"""Deformable convolution (DCN v1 / v2, include/mxdet.h mxdet_deform_*): the bilinear gather, its two adjoints and the
1x1 contraction on the column tensor, against an fp64 torch-CPU restatement of the semantics with autograd.

Tolerance: _close of tests/test_gpu_dense.py (bf16 storage, fp32 accumulation in another order):
|got - ref| <= 2^-7 * |ref| + 2^-7 * rms(ref) elementwise.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _close(got, ref, what="", tol=2.0 ** -7):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rms = np.sqrt(np.mean(ref ** 2)) + 1e-30
    err = np.abs(got - ref)
    bound = tol * np.abs(ref) + tol * rms
    bad = err > bound
    assert not bad.any(), "%s: %d/%d outside tolerance, max err %.4g (rms %.4g)" % (what, bad.sum(), bad.size, err.max(), rms)


def deform_conv_ref(x, off, w, stride, pad, groups, modulated):
    """fp64 torch-CPU deformable convolution (MXNet deformable_im2col semantics, include/mxdet.h). x [N,H,W,C],
    off [N,Ho,Wo,Coff], w [Cout,3,3,C] (torch tensors; gradients flow to all three through autograd, the floor of the
    sample position held fixed). Returns (y [N,Ho,Wo,Cout], col [N,Ho,Wo,9C])."""
    import torch
    N, H, W, Cc = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    G, Cg = groups, Cc // groups
    dt = x.dtype
    ho = torch.arange(Ho, dtype=dt).view(1, Ho, 1)
    wo = torch.arange(Wo, dtype=dt).view(1, 1, Wo)
    nidx = torch.arange(N).view(N, 1, 1)
    taps = []
    for k in range(9):
        i, j = divmod(k, 3)
        parts = []
        for g in range(G):
            py = ho * stride - pad + i + off[..., g * 18 + 2 * k]
            px = wo * stride - pad + j + off[..., g * 18 + 2 * k + 1]
            valid = ((py > -1) & (py < H) & (px > -1) & (px < W)).to(dt)
            y0, x0 = torch.floor(py).detach(), torch.floor(px).detach()
            ly, lx = py - y0, px - x0
            hy, hx = 1 - ly, 1 - lx
            xg = x[..., g * Cg:(g + 1) * Cg]

            def corner(yy, xx):
                inb = ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).to(dt)
                v = xg[nidx, yy.clamp(0, H - 1).long(), xx.clamp(0, W - 1).long()]
                return v * inb[..., None]

            s = ((hy * hx)[..., None] * corner(y0, x0) + (hy * lx)[..., None] * corner(y0, x0 + 1) +
                 (ly * hx)[..., None] * corner(y0 + 1, x0) + (ly * lx)[..., None] * corner(y0 + 1, x0 + 1))
            s = s * valid[..., None]
            if modulated:
                s = s * torch.sigmoid(off[..., 18 * G + 9 * g + k])[..., None]
            parts.append(s)
        taps.append(torch.cat(parts, 3))
    col = torch.stack(taps, 3).reshape(N, Ho, Wo, 9 * Cc)
    y = col @ w.reshape(Cout, 9 * Cc).t()
    return y, col


def _bf16(a):
    import torch
    return torch.as_tensor(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def _offsets(rng, N, Ho, Wo, Coff, G, modulated, H, W):
    """bf16 offsets in [-4, 4], some exact integers, some that push samples > 1 px outside every border."""
    off = np.zeros((N, Ho, Wo, Coff), np.float32)
    nreal = 18 * G
    off[..., :nreal] = rng.uniform(-4, 4, (N, Ho, Wo, nreal))
    ints = rng.random((N, Ho, Wo, nreal)) < 0.1
    off[..., :nreal][ints] = rng.integers(-3, 4, ints.sum())
    far = rng.random((N, Ho, Wo, nreal)) < 0.05
    span = np.where(np.arange(nreal) % 2 == 0, H + 2.5, W + 2.5)[None, None, None, :]
    off[..., :nreal] = np.where(far, np.sign(rng.standard_normal(far.shape)) * span, off[..., :nreal])
    if modulated:
        off[..., nreal:nreal + 9 * G] = rng.standard_normal((N, Ho, Wo, 9 * G)) * 2
    off[..., (27 if modulated else 18) * G:] = rng.standard_normal((N, Ho, Wo, Coff - (27 if modulated else 18) * G)) * 9
    return _bf16(off)


def _gpu_layer(x, off, w, dy, stride, pad, G, modulated, ws=None):
    """Forward + backward of one deformable convolution through the library (column form). Returns the outputs."""
    import torch
    from mxdetection_amd.ops import dense
    from mxdetection_amd.ops import deform_conv as dc
    Cout = w.shape[0]
    N, H, W, Cc = x.shape
    w1 = w.view(Cout, 1, 1, 9 * Cc)
    wt = dense.filter_transpose(w1)
    col = dc.im2col(x, off, stride, pad, G, modulated)
    y = dense.conv2d_forward(col, w1, None, None, 1, 0)
    dcol = dense.conv2d_dgrad(dy, wt, col.shape, 1, 1, 1, 0)
    doff = dc.col2im_coord(x, off, dcol, stride, pad, G, modulated)
    dx = dc.col2im(off, dcol, x.shape, stride, pad, G, modulated, workspace=ws)
    dw = dense.conv2d_wgrad(col, dy, 1, 1, 1, 0)
    return y, col, dcol, doff, dx, dw


CASES = [
    # N, H, W, C, stride, G, modulated
    (2, 11, 14, 64, 1, 1, False),
    (2, 13, 10, 128, 2, 4, True),
    (2, 9, 12, 256, 1, 4, False),
    (2, 15, 8, 64, 2, 1, True),
    (2, 7, 12, 128, 1, 1, True),
    (2, 12, 9, 256, 2, 1, False),
]


@pytest.mark.parametrize("case", CASES)
def test_deform_conv_matches_reference(hip, case):
    import torch
    N, H, W, Cc, s, G, mod = case
    pad, Cout = 1, 64
    Ho, Wo = (H + 2 * pad - 3) // s + 1, (W + 2 * pad - 3) // s + 1
    Coff = ((27 if mod else 18) * G // 8 + 1) * 8         # multiple of 8 with padding channels behind the real ones
    rng = np.random.default_rng(abs(hash(case)) % 2 ** 31)
    x = _bf16(rng.standard_normal((N, H, W, Cc)))
    w = _bf16(rng.standard_normal((Cout, 3, 3, Cc)) * (2.0 / (9 * Cc)) ** 0.5)
    off = _offsets(rng, N, Ho, Wo, Coff, G, mod, H, W)
    dy = _bf16(rng.standard_normal((N, Ho, Wo, Cout)))
    bf = lambda a: torch.from_numpy(a).cuda().to(torch.bfloat16)   # noqa: E731
    y, col, dcol, doff, dx, dw = _gpu_layer(bf(x), bf(off), bf(w), bf(dy), s, pad, G, mod)
    torch.cuda.synchronize()
    wr = torch.from_numpy(w).double().requires_grad_()
    yr, colr = deform_conv_ref(torch.from_numpy(x).double(), torch.from_numpy(off).double(), wr, s, pad, G, mod)
    dyr = torch.from_numpy(dy).double()
    (yr * dyr).sum().backward()
    _close(col.float().cpu().numpy(), colr.detach().numpy(), "col")
    _close(y.float().cpu().numpy(), yr.detach().numpy(), "y")
    _close(dw.cpu().numpy().reshape(Cout, 3, 3, Cc), wr.grad.numpy(), "dW")
    _close(dcol.float().cpu().numpy(), (dyr @ wr.detach().reshape(Cout, 9 * Cc)).numpy(), "dcol")
    # the adjoints of the gather against autograd of the reference, fed the column gradient the library produced (its
    # bf16 rounding alone moves a cancelling offset-gradient sum by more than the tolerance)
    xr, offr = (torch.from_numpy(a).double().requires_grad_() for a in (x, off))
    _, colr = deform_conv_ref(xr, offr, wr.detach(), s, pad, G, mod)
    (colr * dcol.float().cpu().double()).sum().backward()
    _close(dx.float().cpu().numpy(), xr.grad.numpy(), "dx")
    nreal = (27 if mod else 18) * G
    got_off = doff.float().cpu().numpy()
    _close(got_off[..., :18 * G], offr.grad.numpy()[..., :18 * G], "d offsets")
    if mod:
        _close(got_off[..., 18 * G:nreal], offr.grad.numpy()[..., 18 * G:nreal], "d mask logits")
    assert not got_off[..., nreal:].any(), "padding channels of doff must be zero"


def test_zero_offsets_match_plain_conv(hip):
    """v1 with zero offsets is a plain 3x3 convolution: forward, data and weight gradient agree with mxdet_conv2d_*."""
    import torch
    from mxdetection_amd.ops import dense
    rng = np.random.default_rng(11)
    for (N, H, W, Cc, s) in ((2, 13, 17, 64, 1), (2, 14, 11, 128, 2)):
        Cout = 128
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        bf = lambda a: torch.from_numpy(_bf16(a)).cuda().to(torch.bfloat16)   # noqa: E731
        x = bf(rng.standard_normal((N, H, W, Cc)))
        w = bf(rng.standard_normal((Cout, 3, 3, Cc)) * 0.05)
        dy = bf(rng.standard_normal((N, Ho, Wo, Cout)))
        off = torch.zeros((N, Ho, Wo, 24), dtype=torch.bfloat16, device="cuda")
        y, col, dcol, doff, dx, dw = _gpu_layer(x, off, w, dy, s, 1, 1, False)
        y3 = dense.conv2d_forward(x, w, None, None, s, 1)
        dx3 = dense.conv2d_dgrad(dy, dense.filter_transpose(w), x.shape, 3, 3, s, 1)
        dw3 = dense.conv2d_wgrad(x, dy, 3, 3, s, 1)
        torch.cuda.synchronize()
        _close(y.float().cpu().numpy(), y3.float().cpu().numpy(), "fwd")
        # two bf16 results against each other, and the column form rounds dcol before its 9 taps are summed: 2^-6
        _close(dx.float().cpu().numpy(), dx3.float().cpu().numpy(), "dgrad", tol=2.0 ** -6)
        _close(dw.cpu().numpy().reshape(dw3.shape), dw3.cpu().numpy(), "wgrad")


def test_backward_is_bit_reproducible(hip):
    """dx and doff are bit-identical across launches, one of them into a dirty output buffer."""
    import torch
    from mxdetection_amd.ops import deform_conv as dc
    rng = np.random.default_rng(5)
    N, H, W, Cc, G = 2, 23, 31, 128, 2
    Ho, Wo = H, W
    bf = lambda a: torch.from_numpy(_bf16(a)).cuda().to(torch.bfloat16)   # noqa: E731
    x = bf(rng.standard_normal((N, H, W, Cc)))
    off = bf(_offsets(rng, N, Ho, Wo, 64, G, True, H, W))
    dcol = bf(rng.standard_normal((N, Ho, Wo, 9 * Cc)))
    outs = []
    for dirty in (False, True):
        dx = torch.full((N, H, W, Cc), float("nan") if dirty else 0.0, dtype=torch.bfloat16, device="cuda")
        doff = torch.full((N, Ho, Wo, 64), 7.0 if dirty else 0.0, dtype=torch.bfloat16, device="cuda")
        dc.col2im(off, dcol, x.shape, 1, 1, G, True, out=dx)
        dc.col2im_coord(x, off, dcol, 1, 1, G, True, out=doff)
        outs.append((dx.view(torch.int16).cpu(), doff.view(torch.int16).cpu()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]), "dx differs between launches"
    assert torch.equal(outs[0][1], outs[1][1]), "doff differs between launches"
    # accumulate adds the same gradient once more (one bf16 rounding of old + sum)
    dx2 = dc.col2im(off, dcol, x.shape, 1, 1, G, True)
    base = dx2.clone()
    dc.col2im(off, dcol, x.shape, 1, 1, G, True, out=dx2, accumulate=True)
    _close(dx2.float().cpu().numpy(), 2 * base.float().cpu().numpy(), "accumulate")


def test_graph_replay_equals_eager(hip):
    """One layer's forward + backward captured in a hipGraph and replayed equals eager, bit for bit."""
    import torch
    from mxdetection_amd.ops import deform_conv as dc
    rng = np.random.default_rng(9)
    N, H, W, Cc, Cout, s = 2, 19, 26, 128, 64, 2
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    bf = lambda a: torch.from_numpy(_bf16(a)).cuda().to(torch.bfloat16)   # noqa: E731
    x = bf(rng.standard_normal((N, H, W, Cc)))
    w = bf(rng.standard_normal((Cout, 3, 3, Cc)) * 0.05)
    off = bf(_offsets(rng, N, Ho, Wo, 64, 1, True, H, W))
    dy = bf(rng.standard_normal((N, Ho, Wo, Cout)))
    ws = torch.empty((dc.col2im_workspace_bytes(x.shape, s, 1, 1, True, 64),), dtype=torch.uint8, device="cuda")
    eager = [t.clone() for t in _gpu_layer(x, off, w, dy, s, 1, 1, True, ws)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _gpu_layer(x, off, w, dy, s, 1, 1, True, ws)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = _gpu_layer(x, off, w, dy, s, 1, 1, True, ws)
    for t in outs:
        t.zero_()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(("y", "col", "dcol", "doff", "dx", "dw"), eager, outs):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                           b.view(torch.int16) if b.dtype == torch.bfloat16 else b), name
