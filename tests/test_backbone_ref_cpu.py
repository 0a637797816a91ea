"""The fp64 reference of the backbone blocks and FPN necks (tests/_backbone_ref.py) against torch.autograd, on a machine
without a GPU: with the ReLU masks of the reference's own forward, every hand-written backward equals the autograd gradients of
the plain fp64 composition (written here once more, without the reference's helpers for the structure) to 1e-12 relative, at
tiny channel counts; the emulated variants differ from the exact ones (else E of the GPU tests would be zero)."""
import pytest
import torch
import torch.nn.functional as F

import _backbone_ref as ref

F64 = torch.float64
RTOL = 1e-12


def _rand(g, shape, scale=1.0):
    return ref.round_bf16(torch.randn(shape, generator=g, dtype=F64) * scale)


def _same(got, want, what):
    err = float((got - want).abs().max())
    top = float(want.abs().max())
    assert top > 0, what + ": the autograd gradient is zero, the case checks nothing"
    assert err <= RTOL * top, "%s: off by %.3e (max %.3e)" % (what, err, top)


def _c(x, w, b, stride=1, pad=None):
    """Plain NHWC convolution for the autograd side."""
    pad = w.shape[1] // 2 if pad is None else pad
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, stride=stride, padding=pad).permute(0, 2, 3, 1)


def _block_params(g, cin, planes, stride, down):
    p = {}
    for name, ci, co, k in (("conv1", cin, planes, 1), ("conv2", planes, planes, 3), ("conv3", planes, 4 * planes, 1)) + \
            ((("down", cin, 4 * planes, 1),) if down else ()):
        p[name + ".weight"] = _rand(g, (co, k, k, ci), (2.0 / (k * k * ci)) ** 0.5)
        p[name + ".bias"] = torch.randn((co,), generator=g, dtype=F64) * 0.1
    return p


def _block_autograd(x, p, stride):
    a1 = torch.relu(_c(x, p["conv1.weight"], p["conv1.bias"]))
    a2 = torch.relu(_c(a1, p["conv2.weight"], p["conv2.bias"], stride))
    sc = _c(x, p["down.weight"], p["down.bias"], stride, 0) if "down.weight" in p else x
    return torch.relu(_c(a2, p["conv3.weight"], p["conv3.bias"]) + sc)


def _leaves(p):
    return {k: v.clone().requires_grad_(True) for k, v in p.items()}


@pytest.mark.parametrize("cin,planes,stride,down,hw,prefill", [
    (16, 4, 1, False, (5, 4), False), (16, 4, 1, False, (5, 4), True),
    (8, 4, 2, True, (5, 4), True), (8, 4, 2, True, (6, 4), False), (8, 2, 1, True, (3, 3), True)])
def test_bottleneck_backward_is_autograd(cin, planes, stride, down, hw, prefill):
    g = torch.Generator().manual_seed(1)
    p = _block_params(g, cin, planes, stride, down)
    z = torch.randn((2,) + hw + (cin,), generator=g, dtype=F64)
    x = torch.relu(z)
    fwd = ref.bottleneck_forward(x, p, stride)
    dy = _rand(g, tuple(fwd["y"].shape))
    pre = _rand(g, tuple(x.shape)) if prefill else None
    ds = dy * (fwd["y"] > 0)
    got = ref.bottleneck_backward(x, fwd, p, stride, ds, ref.block_masks(x, fwd), prefill=pre)
    # autograd: the input is ReLU(z), so d/dz carries the (x > 0) mask; the lateral gradient is a second consumer of x
    zl, pl = z.clone().requires_grad_(True), _leaves(p)
    xl = torch.relu(zl)
    y = _block_autograd(xl, pl, stride)
    assert torch.equal(y.detach(), fwd["y"])
    loss = (y * dy).sum() + ((xl * pre).sum() if prefill else 0.0)
    names = sorted(k for k in p if k.endswith(".weight"))
    grads = torch.autograd.grad(loss, [zl] + [pl[k] for k in names])
    _same(got["dx"], grads[0], "dx")
    for k, gw in zip(names, grads[1:]):
        _same(got["grads"][k], gw, k)
    assert sorted(got["grads"]) == names
    # need_dx = False: the same weight gradients, no dx
    nodx = ref.bottleneck_backward(x, fwd, p, stride, ds, ref.block_masks(x, fwd), need_dx=False)
    assert nodx["dx"] is None and all(torch.equal(nodx["grads"][k], got["grads"][k]) for k in names)
    # the emulated variant rounds
    emu = ref.bottleneck_forward(x, p, stride, emulate=True)
    assert float((emu["y"] - fwd["y"]).abs().max()) > 0
    eb = ref.bottleneck_backward(x, emu, p, stride, ds, ref.block_masks(x, fwd), prefill=pre, emulate=True)
    assert float((eb["dx"] - got["dx"]).abs().max()) > 0
    assert torch.equal(eb["dx"], ref.round_bf16(eb["dx"]))
    assert float((eb["grads"]["conv1.weight"] - got["grads"]["conv1.weight"]).abs().max()) > 0


def test_stage_walk_backward_is_autograd():
    """Three stages of 2, 3 and 2 blocks (the first without a data gradient into its frozen input), lateral gradients at
    every stage output."""
    g = torch.Generator().manual_seed(2)
    stages, cin = [], 8
    for planes, n in ((2, 2), (4, 3), (8, 2)):
        blocks = []
        for b in range(n):
            blocks.append((_block_params(g, cin if b == 0 else 4 * planes, planes, 2 if b == 0 else 1, b == 0), 2 if b == 0 else 1))
        stages.append(blocks)
        cin = 4 * planes
    c2 = torch.relu(torch.randn((1, 9, 7, 8), generator=g, dtype=F64))
    fwds = ref.resnet_forward(c2, stages)
    outs = [f[-1]["y"] for f in fwds]
    lat = [_rand(g, tuple(o.shape)) for o in outs]
    dC = lat[:-1] + [lat[-1] * (outs[-1] > 0)]
    masks = [[ref.block_masks(f["x"], f) for f in fs] for fs in fwds]
    got_dC, got = ref.resnet_backward(stages, fwds, dC, masks)
    # autograd of the plain composition
    leaves = [[_leaves(p) for p, _ in blocks] for blocks in stages]
    x, loss = c2, 0.0
    for blocks, ls, d in zip(stages, leaves, lat):
        for (p, stride), pl in zip(blocks, ls):
            x = _block_autograd(x, pl, stride)
        loss = loss + (x * d).sum()
    flat = [(j, b, k) for j, ls in enumerate(leaves) for b, pl in enumerate(ls) for k in sorted(pl) if k.endswith(".weight")]
    grads = torch.autograd.grad(loss, [leaves[j][b][k] for j, b, k in flat])
    for (j, b, k), gw in zip(flat, grads):
        _same(got[j][b][k], gw, "stage %d block %d %s" % (j, b, k))
    assert torch.equal(got_dC[-1], dC[-1])
    # dC[j] for j < last ends as the total gradient at that stage's output, masked: compare with autograd through a ReLU'd leaf
    for j in range(len(stages) - 1):
        zl = outs[j].clone().requires_grad_(True)      # outs[j] >= 0; the mask is applied by hand below
        x, loss = zl, (zl * lat[j]).sum()
        for jj in range(j + 1, len(stages)):
            for p, stride in stages[jj]:
                x = _block_autograd(x, p, stride)
            loss = loss + (x * lat[jj]).sum()
        gz, = torch.autograd.grad(loss, zl)
        _same(got_dC[j], gz * (outs[j] > 0), "dC[%d]" % j)
    emu = ref.resnet_forward(c2, stages, emulate=True)
    e_dC, e = ref.resnet_backward(stages, emu, dC, masks, emulate=True)
    assert float((e_dC[0] - got_dC[0]).abs().max()) > 0
    assert float((e[0][0]["conv1.weight"] - got[0][0]["conv1.weight"]).abs().max()) > 0


def _neck_params(g, chans, C, base, names=()):
    p = {}
    for i, ci in enumerate(chans):
        for name, cin, k in (("fpn.lat%d" % (i + base), ci, 1), ("fpn.out%d" % (i + base), C, 3)):
            p[name + ".weight"] = _rand(g, (C, k, k, cin), (1.0 / (k * k * cin)) ** 0.5)
            p[name + ".bias"] = torch.randn((C,), generator=g, dtype=F64) * 0.1
    for name, cin in names:
        p[name + ".weight"] = _rand(g, (C, 3, 3, cin), (1.0 / (9 * cin)) ** 0.5)
        p[name + ".bias"] = torch.randn((C,), generator=g, dtype=F64) * 0.1
    return p


def _neck_autograd(feats, pl, base):
    L = len(feats)
    inner = [None] * L
    for i in reversed(range(L)):
        t = _c(feats[i], pl["fpn.lat%d.weight" % (i + base)], pl["fpn.lat%d.bias" % (i + base)])
        if i + 1 < L:
            h, w = feats[i].shape[1:3]
            t = t + inner[i + 1].repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :h, :w]
        inner[i] = t
    return [_c(inner[i], pl["fpn.out%d.weight" % (i + base)], pl["fpn.out%d.bias" % (i + base)]) for i in range(L)]


SIZES = [(7, 5), (4, 3), (2, 2)]


@pytest.mark.parametrize("extra_p6", [True, False])
def test_fpn_backward_is_autograd(extra_p6):
    g = torch.Generator().manual_seed(3)
    chans, C = [4, 6, 8], 4
    p = _neck_params(g, chans, C, 2)
    zs = [torch.randn((2, h, w, c), generator=g, dtype=F64) for (h, w), c in zip(SIZES, chans)]
    feats = zs[:-1] + [torch.relu(zs[-1])]
    fwd = ref.fpn_forward(feats, p, extra_p6)
    assert len(fwd["P"]) == 3 + extra_p6
    dP = [_rand(g, tuple(t.shape)) for t in fwd["P"]]
    got = ref.fpn_backward(feats, fwd, p, dP, (feats[-1] > 0).to(F64), [True] * 3, extra_p6)
    pl = _leaves(p)
    leaves = [z.clone().requires_grad_(True) for z in zs]
    P = _neck_autograd(leaves[:-1] + [torch.relu(leaves[-1])], pl, 2)
    if extra_p6:
        P.append(P[-1][:, ::2, ::2])
    for a, b in zip(P, fwd["P"]):
        assert torch.equal(a.detach(), b)
    names = sorted(p)
    grads = torch.autograd.grad(sum((a * d).sum() for a, d in zip(P, dP)), leaves + [pl[k] for k in names])
    for i in range(3):
        _same(got["dC"][i], grads[i], "dC[%d]" % i)
    for k, gw in zip(names, grads[3:]):
        _same(got["grads"][k], gw, k)
    assert sorted(got["grads"]) == names
    part = ref.fpn_backward(feats, fwd, p, dP, (feats[-1] > 0).to(F64), [False, True, True], extra_p6)
    assert part["dC"][0] is None and torch.equal(part["dC"][1], got["dC"][1])
    emu = ref.fpn_forward(feats, p, extra_p6, emulate=True)
    eb = ref.fpn_backward(feats, emu, p, dP, (feats[-1] > 0).to(F64), [True] * 3, extra_p6, emulate=True)
    assert float((emu["P"][0] - fwd["P"][0]).abs().max()) > 0 and float((eb["dC"][0] - got["dC"][0]).abs().max()) > 0
    if extra_p6:
        assert torch.equal(emu["P"][3], emu["P"][2][:, ::2, ::2])
        assert float((eb["dP_top"] - got["dP_top"]).abs().max()) > 0       # the in-place sum is rounded once more


@pytest.mark.parametrize("sizes", [SIZES, [(8, 6), (4, 3), (2, 2)]])
def test_retina_fpn_backward_is_autograd(sizes):
    g = torch.Generator().manual_seed(4)
    chans, C = [4, 6, 8], 4
    p = _neck_params(g, chans, C, 3, (("fpn.p6", chans[-1]), ("fpn.p7", C)))
    p["fpn.p6.bias"] = p["fpn.p6.bias"] + 0.3          # P6 is 1 x 1: keep both signs likely among its channels
    zs = [torch.randn((2, h, w, c), generator=g, dtype=F64) for (h, w), c in zip(sizes, chans)]
    feats = zs[:-1] + [torch.relu(zs[-1])]
    fwd = ref.retina_forward(feats, p)
    p6 = fwd["P"][3]
    assert (p6 > 0).any() and (p6 < 0).any()
    dP = [_rand(g, tuple(t.shape)) for t in fwd["P"]]
    got = ref.retina_backward(feats, fwd, p, dP, (p6 > 0).to(F64), (feats[-1] > 0).to(F64))
    pl = _leaves(p)
    leaves = [z.clone().requires_grad_(True) for z in zs]
    fl = leaves[:-1] + [torch.relu(leaves[-1])]
    P = _neck_autograd(fl, pl, 3)
    P.append(_c(fl[-1], pl["fpn.p6.weight"], pl["fpn.p6.bias"], 2))
    P.append(_c(torch.relu(P[3]), pl["fpn.p7.weight"], pl["fpn.p7.bias"], 2))
    for a, b in zip(P, fwd["P"]):
        assert torch.equal(a.detach(), b)
    names = sorted(p)
    grads = torch.autograd.grad(sum((a * d).sum() for a, d in zip(P, dP)), leaves + [pl[k] for k in names])
    for i in range(3):
        _same(got["dC"][i], grads[i], "dC[%d]" % i)
    for k, gw in zip(names, grads[3:]):
        _same(got["grads"][k], gw, k)
    assert sorted(got["grads"]) == names
    emu = ref.retina_forward(feats, p, emulate=True)
    eb = ref.retina_backward(feats, emu, p, dP, (p6 > 0).to(F64), (feats[-1] > 0).to(F64), emulate=True)
    assert float((emu["P"][4] - fwd["P"][4]).abs().max()) > 0 and float((eb["dC"][2] - got["dC"][2]).abs().max()) > 0
    assert float((eb["dP6"] - got["dP6"]).abs().max()) > 0
    assert torch.equal(eb["dP6"], ref.round_bf16(eb["dP6"]))


def test_resampling_adjoints():
    g = torch.Generator().manual_seed(5)
    for hf, wf in ((13, 10), (7, 5), (4, 3), (1, 1), (2, 2)):
        hc, wc = (hf + 1) // 2, (wf + 1) // 2
        c = torch.randn((2, hc, wc, 3), generator=g, dtype=F64).requires_grad_(True)
        d = torch.randn((2, hf, wf, 3), generator=g, dtype=F64)
        want, = torch.autograd.grad((ref.nearest_up(c, (hf, wf)) * d).sum(), c)
        _same(ref.upsample2_backward(d, (hc, wc)), want, "upsample2_backward %dx%d" % (hf, wf))
        x = torch.randn((2, hf, wf, 3), generator=g, dtype=F64).requires_grad_(True)
        dy = torch.randn((2, hc, wc, 3), generator=g, dtype=F64)
        want, = torch.autograd.grad((x[:, ::2, ::2] * dy).sum(), x)
        _same(ref.subsample2_backward(dy, x.shape), want, "subsample2_backward %dx%d" % (hf, wf))


def test_check_rows_reports_a_violation():
    exact = torch.tensor([1.0, -2.0, 4.0], dtype=F64)
    emu = ref.round_bf16(exact * (1 + 2.0 ** -9))
    ok, _ = ref.check_rows([("same", exact.clone(), exact, emu)])
    assert ok == []
    bad, worst = ref.check_rows([("off", exact + 0.5, exact, emu), ("nan", exact * float("nan"), exact, emu)])
    assert [b[0] for b in bad] == ["off", "nan"] and worst > 1
