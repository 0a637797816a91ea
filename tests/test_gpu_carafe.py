"""The CARAFE entries on the GPU through the C-ABI against tests/_carafe_ref.py (fp64) on bf16-rounded inputs.

Grid: N = 2; (H, W) in {(1, 1) -- all halo, a map smaller than the window --, (2, 3), (5, 4), (7, 9), (13, 21), (8, 8), (9, 7)}: the
kernels' source tile is 8 x 8, so each axis sees tile - 1, tile and tile + 1, and (13, 21) is 2 x 3 workgroups; all four
crops (2H | 2H - 1) x (2W | 2W - 1); C in {8 (one channel thread), 72 (no multiple of the forward's 64-channel slice nor of
the dM kernel's 4 lanes x 8), 256 (the model's)}; Cm exact (4 k^2) and padded to a multiple of 64; k in {3, 5}.

Tolerances (the rule of tests/test_gpu_attention.py).
  forward   the weights sum to 1, so |Y| <= max_t |X_t,c| and the output's bf16 rounding is at most 2^-9 of that; allowed
            2^-8 max_t |X_t,c| per output element (a factor 2 for the fp32 summation order and the hardware exp).
  dX, dM    E = max |emulated - exact| of the CPU reference (the one bf16 rounding of each output, of prefill + dX when the
            entry accumulates; no kernel result enters it); the GPU result must lie within 2 E + 2^-9 max |exact|.
Every case prints E and the achieved error (DESIGN.md 5t holds the table).
"""
import ctypes
import functools

import pytest

import _carafe_ref as ref

pytestmark = pytest.mark.gpu

N = 2
SHAPES = ((1, 1), (2, 3), (5, 4), (7, 9), (13, 21), (8, 8), (9, 7))
CS = (8, 72, 256)
KS = (3, 5)
CROPS = ((0, 0), (0, 1), (1, 0), (1, 1))
SENTINEL = 7.0
GUARD = 64           # bf16 elements on either side of a guarded view (a multiple of 8: the view stays 16-byte aligned)


def _padded(k):
    return (4 * k * k + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def _reference(H, W, C, k, crop):
    """Inputs and the exact / emulated results of one case: computed once, never modified."""
    out_hw = (2 * H - crop[0], 2 * W - crop[1])
    x, m, d_out, pre = ref.random_case(N, H, W, C, k, out_hw, seed=((H * 31 + W) * 7 + C) * 11 + k + 1000 * (2 * crop[0] + crop[1]))
    y = ref.forward(x, m, k, out_hw)
    dx, dm = ref.backward(x, m, d_out, k)
    edx, edm = ref.emulate_backward(dx, dm)
    eacc, _ = ref.emulate_backward(dx, dm, pre)
    E = dict(dX=float((edx - dx).abs().max()), dM=float((edm - dm).abs().max()), dXacc=float((eacc - (pre + dx)).abs().max()))
    return dict(x=x, m=m, d_out=d_out, pre=pre, y=y, dx=dx, dm=dm, E=E, out_hw=out_hw)


def _guarded(shape, fill):
    """A contiguous bf16 view of `shape` inside a larger allocation full of sentinels; (view, whole, check)."""
    import torch
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.bfloat16, device="cuda")
    view = whole[GUARD:GUARD + n].view(shape)
    view.fill_(fill)

    def intact():
        return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())
    return view, intact


def _logits(m, k, Cm, pad_value):
    """The [N, H, W, Cm] logit tensor of the entries: the real channels of `m`, `pad_value` in the padding."""
    import torch
    out = torch.full(tuple(m.shape[:3]) + (Cm,), pad_value, dtype=torch.bfloat16, device="cuda")
    out[..., :4 * k * k] = m.to(torch.bfloat16).cuda()
    return out


def _run(x, m, d_out, k, Cm, out_hw, pad_value=1e4, prefill=None):
    """Forward and backward through the plan on guarded outputs; returns cpu float64 (Y, dX, dM) and the guards' state."""
    import torch
    from mxdetection_amd.ops.carafe import CarafePlan
    plan = CarafePlan(tuple(x.shape), Cm, k, out_hw)
    xg = x.to(torch.bfloat16).cuda()
    mg = _logits(m, k, Cm, pad_value)
    gg = d_out.to(torch.bfloat16).cuda()
    y, y_ok = _guarded(plan.y_shape, float("nan"))
    dx, dx_ok = _guarded(plan.x_shape, float("nan"))
    dm, dm_ok = _guarded(plan.m_shape, float("nan"))
    if prefill is not None:
        dx.copy_(prefill.to(torch.bfloat16).cuda())
    plan.forward(xg, mg, y)
    plan.backward(xg, mg, gg, dx, dm, accumulate=prefill is not None)
    torch.cuda.synchronize()
    return y.double().cpu(), dx.double().cpu(), dm.double().cpu(), (y_ok(), dx_ok(), dm_ok())


def _tap_max(x, k, out_hw):
    """max_t |X[src(t), c]| per output element (zero outside the map)."""
    import torch.nn.functional as F
    a = F.max_pool2d(x.abs().permute(0, 3, 1, 2), k, stride=1, padding=k // 2).permute(0, 2, 3, 1)
    return ref.nearest_up(a, out_hw)


def _check(tag, r, k, Cm, got, accumulate):
    import torch
    y, dx, dm, guards = got
    assert guards == (True, True, True), "%s: a sentinel around Y / dX / dM was overwritten %s" % (tag, guards)
    real = 4 * k * k
    tol_y = 2.0 ** -8 * _tap_max(r["x"], k, r["out_hw"])
    err_y = (y - r["y"]).abs()
    assert bool(torch.isfinite(y).all()) and bool((err_y <= tol_y).all()), "%s: Y off by %.3e" % (tag, float((err_y - tol_y).max()))
    want_dx = r["pre"] + r["dx"] if accumulate else r["dx"]
    E = r["E"]["dXacc" if accumulate else "dX"]
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dm).all()), "%s: NaN prefill survived" % tag
    rows = [("dX+" if accumulate else "dX", dx, want_dx, E), ("dM", dm[..., :real], r["dm"], r["E"]["dM"])]
    print("%s Y: max err %.3e (smallest margin %.3e)" % (tag, float(err_y.max()), float((tol_y - err_y).min())))
    for name, g, exact, e in rows:
        tol = 2.0 * e + 2.0 ** -9 * float(exact.abs().max())
        err = float((g - exact).abs().max())
        print("%s %s: E %.3e  tolerance %.3e  achieved %.3e" % (tag, name, e, tol, err))
        assert err <= tol, "%s: %s off by %.3e > %.3e" % (tag, name, err, tol)
    assert not dm[..., real:].any(), "%s: dM's padding channels are not exactly zero" % tag
    H, W = r["x"].shape[1:3]
    sub = dm[..., :real].reshape(N, H, W, k * k, 4)
    if r["out_hw"][0] == 2 * H - 1:
        assert not sub[:, H - 1, :, :, 2:].any(), "%s: dM of the cropped row is not exactly zero" % tag
    if r["out_hw"][1] == 2 * W - 1:
        assert not sub[:, :, W - 1, :, 1::2].any(), "%s: dM of the cropped column is not exactly zero" % tag


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("hw", SHAPES)
def test_parity_with_fp64(hip, hw, C, k):
    import torch
    H, W = hw
    for crop in CROPS:
        r = _reference(H, W, C, k, crop)
        outs = {}
        for Cm in (4 * k * k, _padded(k)):
            tag = "%dx%d crop %s C=%d k=%d Cm=%d" % (H, W, crop, C, k, Cm)
            outs[Cm] = _run(r["x"], r["m"], r["d_out"], k, Cm, r["out_hw"])
            _check(tag, r, k, Cm, outs[Cm], accumulate=False)
        a, b = outs[4 * k * k], outs[_padded(k)]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "1e4 in the padding channels of M changed Y or dX"
        tag = "%dx%d crop %s C=%d k=%d accumulate" % (H, W, crop, C, k)
        _check(tag, r, k, _padded(k), _run(r["x"], r["m"], r["d_out"], k, _padded(k), r["out_hw"], prefill=r["pre"]), accumulate=True)


@pytest.mark.parametrize("k", KS)
def test_adversarial_logits(hip, k):
    """All logits at +100 (exp overflows fp32 unless the maximum is subtracted): the zero-padded box mean. One-hot centre:
    nearest upsampling bit for bit. One-hot corner tap: that shift of X, zeros where it leaves the map."""
    import torch
    H, W, C = 7, 9, 72
    rr = k // 2
    for crop in ((0, 0), (1, 1)):
        out_hw = (2 * H - crop[0], 2 * W - crop[1])
        x, _, d_out, _ = ref.random_case(N, H, W, C, k, out_hw, seed=50 + k)
        hot = torch.full((N, H, W, 4 * k * k), 100.0, dtype=ref.F64)
        y, dx, dm, guards = _run(x, hot, d_out, k, _padded(k), out_hw)
        want = ref.forward(x, hot, k, out_hw)
        assert guards == (True, True, True) and bool(torch.isfinite(y).all()) and bool(torch.isfinite(dm).all())
        assert bool(((y - want).abs() <= 2.0 ** -8 * _tap_max(x, k, out_hw)).all())
        wdx, wdm = ref.backward(x, hot, d_out, k)
        for name, g, exact in (("dX", dx, wdx), ("dM", dm[..., :4 * k * k], wdm)):
            e = float((ref.round_bf16(exact) - exact).abs().max())
            assert float((g - exact).abs().max()) <= 2.0 * e + 2.0 ** -9 * float(exact.abs().max()), name
        y, _, _, _ = _run(x, ref.one_hot_logits(N, H, W, k, (k * k) // 2), d_out, k, _padded(k), out_hw)
        assert torch.equal(y, ref.nearest_up(x, out_hw)), "one-hot centre is not nearest upsampling bit for bit"
        for tap in (0, k - 1, k * k - k, k * k - 1):
            y, _, _, _ = _run(x, ref.one_hot_logits(N, H, W, k, tap), d_out, k, 4 * k * k, out_hw)
            want = ref.nearest_up(ref.shift(x, tap // k - rr, tap % k - rr), out_hw)
            assert torch.equal(y, want), "one-hot tap %d" % tap
            assert not y[:, :2 * rr].any() if tap < k else not y[:, 2 * (H - rr):].any()      # the rows that read outside the map


@pytest.mark.parametrize("k", KS)
def test_adjoint_identity(hip, k):
    """<Y(X), G> = <X, dX(G)> for fixed weights, within what the two results' own tolerances allow."""
    H, W, C = 13, 21, 72
    for crop in CROPS:
        r = _reference(H, W, C, k, crop)
        y, dx, _, _ = _run(r["x"], r["m"], r["d_out"], k, _padded(k), r["out_hw"])
        lhs, rhs = float((y * r["d_out"]).sum()), float((r["x"] * dx).sum())
        exact = float((r["y"] * r["d_out"]).sum())
        assert abs(exact - float((r["x"] * r["dx"]).sum())) <= 1e-9 * max(1.0, abs(exact))      # the identity itself, in fp64
        tol_dx = 2.0 * r["E"]["dX"] + 2.0 ** -9 * float(r["dx"].abs().max())
        tol = float((r["d_out"].abs() * 2.0 ** -8 * _tap_max(r["x"], k, r["out_hw"])).sum()) + float(r["x"].abs().sum()) * tol_dx
        print("k=%d crop %s: <Y,G> %.6f  <X,dX> %.6f  difference %.3e  allowed %.3e" % (k, crop, lhs, rhs, abs(lhs - rhs), tol))
        assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize("k", KS)
def test_repeatable(hip, k):
    """Forward and backward twice: every output bit for bit."""
    import torch
    r = _reference(13, 21, 256, k, (1, 0))
    a = _run(r["x"], r["m"], r["d_out"], k, _padded(k), r["out_hw"], prefill=r["pre"])
    b = _run(r["x"], r["m"], r["d_out"], k, _padded(k), r["out_hw"], prefill=r["pre"])
    for u, v, name in zip(a[:3], b[:3], ("Y", "dX", "dM")):
        assert torch.equal(u, v), name


def test_refusals_leave_the_outputs_alone(hip):
    """Every host check returns its error and message before any launch."""
    import torch
    from mxdetection_amd import _lib
    lib = _lib.load()
    H, W, C, k, Cm = 4, 5, 16, 5, 128
    x = torch.zeros((N, H, W, C), dtype=torch.bfloat16, device="cuda")
    m = torch.zeros((N, H, W, Cm), dtype=torch.bfloat16, device="cuda")
    y = torch.full((N, 2 * H, 2 * W, C), 3.0, dtype=torch.bfloat16, device="cuda")
    dx, dm = torch.full_like(x, 3.0), torch.full_like(m, 3.0)
    p = _lib.ptr

    def both(rc_want, text, **bad):
        d = _lib.CarafeDescT()
        d.N, d.H, d.W, d.C, d.Cm, d.k, d.Hf, d.Wf = N, H, W, C, Cm, k, 2 * H, 2 * W
        for name, v in bad.items():
            setattr(d, name, v)
        for rc in (lib.mxdet_carafe_fwd(ctypes.byref(d), p(x), p(m), p(y), _lib.stream_ptr()),
                   lib.mxdet_carafe_bwd(ctypes.byref(d), p(x), p(m), p(y), p(dx), p(dm), 0, _lib.stream_ptr())):
            assert rc == rc_want and text in lib.mxdet_last_error(), (bad, rc, lib.mxdet_last_error())

    both(-2, b"multiple of 8", C=12)
    both(-2, b"3 or 5", k=4)
    both(-2, b"3 or 5", k=7)
    both(-2, b"4 k^2", Cm=96)
    both(-2, b"Hf", Hf=2 * H + 1)
    both(-2, b"Hf", Hf=2 * H - 2)
    both(-2, b"Wf", Wf=2 * W - 2)
    both(-2, b"Wf", Wf=W)
    d = _lib.CarafeDescT()
    d.N, d.H, d.W, d.C, d.Cm, d.k, d.Hf, d.Wf = N, H, W, C, Cm, k, 2 * H, 2 * W
    for args in ((None, p(m), p(y)), (p(x), None, p(y)), (p(x), p(m), None)):
        assert lib.mxdet_carafe_fwd(ctypes.byref(d), *args, _lib.stream_ptr()) == -1 and b"null" in lib.mxdet_last_error()
    for i in range(5):
        args = [p(x), p(m), p(y), p(dx), p(dm)]
        args[i] = None
        assert lib.mxdet_carafe_bwd(ctypes.byref(d), *args, 0, _lib.stream_ptr()) == -1 and b"null" in lib.mxdet_last_error()
    assert lib.mxdet_carafe_fwd(None, p(x), p(m), p(y), _lib.stream_ptr()) == -1 and b"null" in lib.mxdet_last_error()
    torch.cuda.synchronize()
    assert bool((y == 3.0).all()) and bool((dx == 3.0).all()) and bool((dm == 3.0).all())
