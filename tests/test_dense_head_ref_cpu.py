"""The fp64 reference of the dense heads (tests/_dense_head_ref.py) against torch.autograd, on a machine without a GPU: with the
ReLU masks of the reference's own forward, both hand-written backwards equal the autograd gradients of the plain fp64
composition (written here once more) to 1e-12 relative, on a tiny pyramid with padded output layers; the emulated variants
differ from the exact ones (else E of the GPU tests would be zero), by bf16-sized amounts only, and what they store holds bf16
values. Also RetinaHead's refusal of a head without tower layers."""
import pytest
import torch
import torch.nn.functional as F

import _dense_head_ref as ref
from _backbone_ref import round_bf16

F64 = torch.float64
RTOL = 1e-12
N, C = 2, 4
SIZES = [(5, 4), (3, 2), (1, 1)]
# a stored map carries one bf16 rounding (relative 2^-9) per stored map on its path, at most 6 here (four tower layers, the
# output layer's gradient, the in-place sum); errors of one layer reach the next scaled by about the layer's gain. 2^-6 of the
# map's largest magnitude is eight such roundings landing on one element with gain 1: "bf16-sized", and far below any wiring error
EMU_REL = 2.0 ** -6


def _rand(g, shape, scale=1.0):
    return round_bf16(torch.randn(shape, generator=g, dtype=F64) * scale)


def _same(got, want, what):
    err = float((got - want).abs().max())
    top = float(want.abs().max())
    assert top > 0, what + ": the autograd gradient is zero, the case checks nothing"
    assert err <= RTOL * top, "%s: off by %.3e (max %.3e)" % (what, err, top)


def _bf16_sized(emu, exact, what, stored=True):
    err = float((emu - exact).abs().max())
    top = float(exact.abs().max())
    assert 0 < err <= EMU_REL * top, "%s: emulated differs from exact by %.3e (max |exact| %.3e)" % (what, err, top)
    if stored:
        assert torch.equal(emu, round_bf16(emu)), what + ": a stored map that holds no bf16 values"


def _c(x, w, b):
    """Plain NHWC convolution, stride 1, pad k // 2, for the autograd side."""
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, padding=w.shape[1] // 2).permute(0, 2, 3, 1)


def _layer(g, p, name, cout, k, cin, real=None):
    w = _rand(g, (cout, k, k, cin), (2.0 / (k * k * cin)) ** 0.5)
    b = torch.randn((cout,), generator=g, dtype=F64) * 0.1
    if real is not None:        # alignment padding: zero filter rows, zero biases
        w[real:] = 0
        b[real:] = 0
    p[name + ".weight"], p[name + ".bias"] = w, b


def _leaves(p):
    return {k: v.clone().requires_grad_(True) for k, v in p.items()}


def _padded_grad(g, shape, real):
    t = _rand(g, shape)
    t[..., real:] = 0
    return t


@pytest.mark.parametrize("num_convs", [1, 4])
def test_retina_head_backward_is_autograd(num_convs):
    g = torch.Generator().manual_seed(11 + num_convs)
    ld_cls, real_cls, ld_reg, real_reg = 8, 6, 6, 4
    p = {}
    _layer(g, p, "retina.cls_out", ld_cls, 3, C, real_cls)
    _layer(g, p, "retina.box_out", ld_reg, 3, C, real_reg)
    for i in range(num_convs):
        _layer(g, p, "retina.cls%d" % i, C, 3, C)
        _layer(g, p, "retina.box%d" % i, C, 3, C)
    P = [_rand(g, (N, h, w, C)) for h, w in SIZES]
    fwd = ref.retina_head_forward(P, p, num_convs)
    assert all(len(a) == num_convs + 1 for a in fwd["cact"] + fwd["bact"])
    assert all(not t[..., real_cls:].any() for t in fwd["co"]) and all(not t[..., real_reg:].any() for t in fwd["bo"])
    gco = [_padded_grad(g, tuple(t.shape), real_cls) for t in fwd["co"]]
    gbo = [_padded_grad(g, tuple(t.shape), real_reg) for t in fwd["bo"]]
    masks = ref.retina_head_masks(fwd)
    got = ref.retina_head_backward(P, fwd, p, gco, gbo, masks)
    # autograd of the plain composition: one set of leaves shared by all levels
    pl, Pl = _leaves(p), [x.clone().requires_grad_(True) for x in P]
    loss = 0.0
    for l, x in enumerate(Pl):
        for tower, want, dy in (("cls", fwd["co"][l], gco[l]), ("box", fwd["bo"][l], gbo[l])):
            a = x
            for i in range(num_convs):
                a = torch.relu(_c(a, pl["retina.%s%d.weight" % (tower, i)], pl["retina.%s%d.bias" % (tower, i)]))
            y = _c(a, pl["retina.%s_out.weight" % tower], pl["retina.%s_out.bias" % tower])
            assert torch.equal(y.detach(), want)
            loss = loss + (y * dy).sum()
    names = sorted(p)
    assert len(names) == 2 * (2 * num_convs + 2) and sorted(got["grads"]) == names
    grads = torch.autograd.grad(loss, Pl + [pl[k] for k in names])
    for l in range(len(P)):
        _same(got["dP"][l], grads[l], "dP[%d]" % l)
    for k, gw in zip(names, grads[len(P):]):
        _same(got["grads"][k], gw, k)
    assert not got["grads"]["retina.cls_out.weight"][real_cls:].any() and not got["grads"]["retina.box_out.bias"][real_reg:].any()
    # the emulated variant rounds what the device stores, and nothing else
    emu = ref.retina_head_forward(P, p, num_convs, emulate=True)
    eb = ref.retina_head_backward(P, emu, p, gco, gbo, masks, emulate=True)
    for l in range(len(P)):
        _bf16_sized(emu["co"][l], fwd["co"][l], "co[%d]" % l)
        _bf16_sized(emu["bo"][l], fwd["bo"][l], "bo[%d]" % l)
        _bf16_sized(emu["cact"][l][num_convs], fwd["cact"][l][num_convs], "class tower, level %d" % l)
        _bf16_sized(eb["dP"][l], got["dP"][l], "dP[%d]" % l)
    for k in names:
        if k.endswith("_out.bias"):       # sums of the given gradients: nothing on their path is stored
            assert torch.equal(eb["grads"][k], got["grads"][k])
        else:
            _bf16_sized(eb["grads"][k], got["grads"][k], k, stored=False)
    assert any(not torch.equal(eb["grads"][k], round_bf16(eb["grads"][k])) for k in names), "weight gradients were rounded"


@pytest.mark.parametrize("has_grad", [[False] * 3, [True] * 3, [True, False, True]], ids=["none", "all", "mixed"])
def test_rpn_head_backward_is_autograd(has_grad):
    g = torch.Generator().manual_seed(17)
    A, cpad = 1, 8
    p = {}
    _layer(g, p, "rpn.out", cpad, 1, C, 5 * A)
    _layer(g, p, "rpn.conv", C, 3, C)
    P = [_rand(g, (N, h, w, C)) for h, w in SIZES]
    fwd = ref.rpn_head_forward(P, p)
    assert all(not h[..., 5 * A:].any() for h in fwd["h"])
    gh = [_padded_grad(g, tuple(h.shape), 5 * A) for h in fwd["h"]]
    pre = [_rand(g, tuple(x.shape)) for x in P]
    masks = [(t > 0).to(F64) for t in fwd["t"]]
    got = ref.rpn_head_backward(P, fwd, p, gh, masks, pre, has_grad)
    pl, Pl = _leaves(p), [x.clone().requires_grad_(True) for x in P]
    loss = 0.0
    for l, x in enumerate(Pl):
        t = torch.relu(_c(x, pl["rpn.conv.weight"], pl["rpn.conv.bias"]))
        h = _c(t, pl["rpn.out.weight"], pl["rpn.out.bias"])
        assert torch.equal(t.detach(), fwd["t"][l]) and torch.equal(h.detach(), fwd["h"][l])
        loss = loss + (h * gh[l]).sum() + ((x * pre[l]).sum() if has_grad[l] else 0.0)   # the prefill: a second consumer of P
    names = sorted(p)
    assert sorted(got["grads"]) == names
    grads = torch.autograd.grad(loss, Pl + [pl[k] for k in names])
    for l in range(len(P)):
        _same(got["dP"][l], grads[l], "dP[%d]" % l)
    for k, gw in zip(names, grads[len(P):]):
        _same(got["grads"][k], gw, k)
    assert not got["grads"]["rpn.out.weight"][5 * A:].any() and not got["grads"]["rpn.out.bias"][5 * A:].any()
    emu = ref.rpn_head_forward(P, p, emulate=True)
    eb = ref.rpn_head_backward(P, emu, p, gh, masks, pre, has_grad, emulate=True)
    for l in range(len(P)):
        _bf16_sized(emu["t"][l], fwd["t"][l], "t[%d]" % l)
        _bf16_sized(emu["h"][l], fwd["h"][l], "h[%d]" % l)
        _bf16_sized(eb["dt"][l], got["dt"][l], "dt[%d]" % l)
        _bf16_sized(eb["dP"][l], got["dP"][l], "dP[%d]" % l)
    assert torch.equal(eb["grads"]["rpn.out.bias"], got["grads"]["rpn.out.bias"])
    for k in ("rpn.out.weight", "rpn.conv.weight", "rpn.conv.bias"):
        _bf16_sized(eb["grads"][k], got["grads"][k], k, stored=False)


@pytest.mark.parametrize("num_convs", [0, -1, True, 2.0])
def test_retina_head_refuses_a_head_without_tower_layers(num_convs):
    """With num_convs = 0 backward() would mask cls_out's data gradient by P > 0 and never write dP: the constructor raises
    before it registers anything."""
    from mxdetection_amd.models.rpn_heads.retina_head import RetinaHead
    from mxdetection_amd.models.utils.layers import ParamArena
    arena = ParamArena("cpu")
    with pytest.raises(ValueError, match="num_convs"):
        RetinaHead(64, [8, 16], arena, None, "cpu", torch.Generator().manual_seed(0), num_convs=num_convs)
    assert arena.entries == []
