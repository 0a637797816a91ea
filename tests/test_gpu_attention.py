"""The attention entries on the GPU through the C-ABI against tests/_nonlocal_ref.py (fp64) on bf16-rounded inputs.

Shapes: L in {1, 63, 64, 65, 130, 200} -- a single partial tile, an exact tile, tile + 1, two tiles + tail, more than three
tiles (and 1 / 2 / 3 / 5 / 7 workgroups of 32 rows) -- x d in {64, 128}, N = 2 (batch stride), the packed layout with
row_stride = 3d and 3d + 8 (a sentinel in the padding columns of d_qkv must survive), scale in {1, 1/sqrt(d)}.

Tolerances.
  forward   p <= 1 rounded to bf16 contributes at most 2^-9 max_j |V_jc| to column c, the output rounding another
            2^-9 |O| <= the same: 2^-8 max_j |V_jc|. Allowed: 2^-7 max_j |V_jc| (a factor 2 for fp32 accumulation order
            and the hardware exp).
  LSE       1e-3 absolute (the worst-case fp32 dot-product error at d = 128, |s| <= 32 is about 2.5e-4).
  backward  per tensor, E = max |emulated - exact| of the CPU reference (the roundings of p, dS and the outputs to bf16; no
            kernel result enters it); the GPU result must lie within 2 E + 2^-9 max |exact| of the exact reference.
Every case prints E and the achieved error (DESIGN.md 5s holds the table).
"""
import functools
import math

import pytest

import _nonlocal_ref as ref

pytestmark = pytest.mark.gpu

N = 2
LS = (1, 63, 64, 65, 130, 200)
DS = (64, 128)


@functools.lru_cache(maxsize=None)
def _reference(kind, L, d, pad, scale):
    """(packed, d_out, exact (O, LSE, dQ, dK, dV), E (dQ, dK, dV)): computed once per case, never modified."""
    if kind == "random":
        packed, d_out = ref.random_packed(N, L, d, pad, seed=1000 * L + d + pad)
    else:
        packed, d_out = ref.adversarial_packed(N, L, d, kind, seed=7 * L + d)
    q, k, v = ref.split_packed(packed, d, 0, d, 2 * d)
    o, lse = ref.attention_forward(q, k, v, scale)
    exact = ref.attention_backward(q, k, v, d_out, scale, o, lse)
    emulated = ref.attention_backward(q, k, v, d_out, scale, emulate=True)
    E = tuple(float((a - b).abs().max()) for a, b in zip(emulated, exact))
    return packed, d_out, (o, lse) + tuple(exact), E


def _run(packed, d_out, d, scale, sentinel=None):
    """Forward and backward through the plan; returns cpu float64 (O, LSE, d_qkv)."""
    import torch
    from mxdetection_amd.ops.attention import AttentionPlan
    L, rs = packed.shape[1], packed.shape[2]
    plan = AttentionPlan(N, L, d, rs, 0, d, 2 * d, scale, "cuda")
    qkv = packed.to(torch.bfloat16).cuda()
    g = d_out.to(torch.bfloat16).cuda()
    out = torch.empty((N, L, d), dtype=torch.bfloat16, device="cuda")
    d_qkv = torch.full((N, L, rs), 0.0 if sentinel is None else sentinel, dtype=torch.bfloat16, device="cuda")
    plan.forward(qkv, out)
    plan.backward(qkv, out, g, d_qkv)
    torch.cuda.synchronize()
    return out.double().cpu(), plan.lse.double().cpu(), d_qkv.double().cpu()


def _compare(tag, packed, d_out, want, E, d, scale, pad):
    import torch
    v = packed[..., 2 * d:3 * d]
    o, lse, d_qkv = _run(packed, d_out, d, scale, sentinel=-7.0)
    # forward: per image and column, 2^-7 max_j |V_jc|
    tol_o = 2.0 ** -7 * v.abs().max(dim=1, keepdim=True).values
    err_o = (o - want[0]).abs()
    print("%s O: max err %.3e (smallest margin %.3e)" % (tag, float(err_o.max()), float((tol_o - err_o).min())))
    assert bool((err_o <= tol_o).all()), "%s: O off by %.3e" % (tag, float((err_o - tol_o).max()))
    err_l = float((lse - want[1]).abs().max())
    print("%s LSE: max err %.3e" % (tag, err_l))
    assert err_l <= 1e-3, "%s: LSE off by %.3e" % (tag, err_l)
    for i, name in enumerate(("dQ", "dK", "dV")):
        got, exact = d_qkv[..., i * d:(i + 1) * d], want[2 + i]
        tol = 2.0 * E[i] + 2.0 ** -9 * float(exact.abs().max())
        err = float((got - exact).abs().max())
        print("%s %s: E %.3e  tolerance %.3e  achieved %.3e" % (tag, name, E[i], tol, err))
        assert err <= tol, "%s: %s off by %.3e > %.3e" % (tag, name, err, tol)
    if pad:
        assert bool((d_qkv[..., 3 * d:] == -7.0).all()), "%s: padding columns of d_qkv were written" % tag
    assert bool(torch.isfinite(d_qkv).all())


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("L", LS)
def test_parity_with_fp64(hip, L, d):
    for pad in (0, 8):
        for scale in (1.0, 1.0 / math.sqrt(d)):
            packed, d_out, want, E = _reference("random", L, d, pad, scale)
            _compare("L=%d d=%d rs=3d+%d scale=%.4f" % (L, d, pad, scale), packed, d_out, want, E, d, scale, pad)


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("where", ["last", "first"])
def test_online_rescale(hip, where, d):
    """The row maximum in the last key tile (every earlier tile is rescaled) / in the first one with the later logits 60
    below; scale 1 and |s| <= 32."""
    L = 200
    packed, d_out, want, E = _reference(where, L, d, 0, 1.0)
    q, k, _ = ref.split_packed(packed, d, 0, d, 2 * d)
    s = q @ k.transpose(1, 2)
    assert float(s.abs().max()) <= 32.0
    if where == "last":
        assert bool((s.argmax(dim=2) >= 192).all())                       # the last tile: keys 192 .. 199
        tile_max = [s[..., a:a + 64].max(dim=2).values for a in (0, 64, 128)]
        assert bool((tile_max[0] < tile_max[1]).all()) and bool((tile_max[1] < tile_max[2]).all())
    else:
        assert bool((s.argmax(dim=2) < 8).all())
        assert float((s[..., :8].min(dim=2).values - s[..., 8:].max(dim=2).values).min()) >= 55.0
    _compare("%s d=%d" % (where, d), packed, d_out, want, E, d, 1.0, 0)


@pytest.mark.parametrize("d", DS)
def test_repeatable(hip, d):
    """Forward and backward twice: every output bit for bit."""
    import torch
    packed, d_out, _, _ = _reference("random", 200, d, 8, 1.0)
    a = _run(packed, d_out, d, 1.0)
    b = _run(packed, d_out, d, 1.0)
    for x, y, name in zip(a, b, ("O", "LSE", "d_qkv")):
        assert torch.equal(x, y), name


def test_refusals_leave_the_outputs_alone(hip):
    """d = 256 (mmdetection's reduction = 1) is refused on the host: nothing is launched."""
    import torch
    from mxdetection_amd import _lib
    from mxdetection_amd.ops.attention import AttentionPlan
    with pytest.raises(_lib.MxdetError, match="d = 256"):
        AttentionPlan(N, 64, 256, 768, 0, 256, 512, 1.0, "cuda")
    plan = AttentionPlan(N, 64, 64, 192, 0, 64, 128, 1.0, "cuda")
    qkv = torch.zeros((N, 64, 192), dtype=torch.bfloat16, device="cuda")
    out = torch.full((N, 64, 64), 3.0, dtype=torch.bfloat16, device="cuda")
    plan.desc.q_off = 136
    with pytest.raises(_lib.MxdetError, match="row_stride"):
        plan.forward(qkv, out)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
