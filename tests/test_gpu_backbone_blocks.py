"""The Python that wires the convolution kernels into bottlenecks, stages and the C3..C5 backward walk
(models/backbones/resnet.py) against the fp64 restatement of tests/_backbone_ref.py.

Parts are built on their own (ParamArena, Workspace, finalize, materialize, refresh, plan) at the model's real channel widths,
so the convolution routes are the model's, on maps of a few pixels. Every layer's folded-BN shift (`frozen_bias`, all zeros by
default) is drawn from N(0, 0.1) so a dropped or doubled bias shows; every buffer a module must fully write is pre-filled with
NaN, the gradient arena included.

Rule (that of the kernel tests and tests/test_gpu_carafe_model.py): |got - exact| <= 2 E + 2^-9 max |exact|,
E = max |emulated - exact| from the CPU reference alone. The forward maps are compared with the exact forward; the backward is
teacher-forced: the reference receives the ReLU masks of the DEVICE's stored activations (a1 > 0, a2 > 0, x > 0 -- what the
model itself uses) and is the exact linear adjoint under them (tests/_backbone_ref.py explains why).

The negative controls change Python wiring only, never a kernel: the numbers are wrong, nothing else, and the rule must say so.
"""
import pytest

import _backbone_ref as ref

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _cpu(t):
    return t.double().cpu()


def _fill_biases(layers, g):
    import torch
    for l in layers:
        l.frozen_bias.copy_((torch.randn((l.cout,), generator=g) * 0.1).to(l.frozen_bias.device))


def _finish(arena, layers, g):
    """After registration: allocate, load the initial filters, random folded-BN shifts, bf16 + transposed copies."""
    arena.finalize()
    for l in layers:
        l.materialize()
    _fill_biases(layers, g)
    arena.refresh_bf16()
    for l in layers:
        l.refresh_transposed()


def _block_params(b):
    p = {}
    for key, l in (("conv1", b.conv1), ("conv2", b.conv2), ("conv3", b.conv3), ("down", b.down)):
        if l is not None:
            p[key + ".weight"] = _cpu(l.w_bf16)
            p[key + ".bias"] = _cpu(l.bias_f32)
    return p


def _block_grads(b):
    return {key + ".weight": _cpu(l.arena.view(l.wi, "g"))
            for key, l in (("conv1", b.conv1), ("conv2", b.conv2), ("conv3", b.conv3), ("down", b.down)) if l is not None}


def _nan_block_bufs(b, x_shape, value=NAN):
    """Create (or refill) every buffer the block writes in forward and backward with `value`."""
    s1 = b.conv1.out_shape(x_shape)
    s2 = b.conv2.out_shape(s1)
    so = b.conv3.out_shape(s2)
    for key, s in (("a1", s1), ("a2", s2), (b.y_key, so), ("d_a1", s1), ("d_a2", s2), ("dx", tuple(x_shape))) + \
            ((("sc", so),) if b.down is not None else ()):
        b._buf(key, s).fill_(value)


def _device_masks(b):
    return {"a1": _cpu(b.a1 > 0), "a2": _cpu(b.a2 > 0), "x": _cpu(b.x > 0)}


CASES = {
    # cin, planes, stride, projection, H, W, need_dx, dx_has_grad
    "A": (512, 128, 1, False, 9, 7, True, False),
    "B-odd": (512, 256, 2, True, 9, 7, True, True),
    "B-even": (512, 256, 2, True, 8, 6, True, True),
    "C": (256, 128, 2, True, 9, 7, False, False),
    "D": (2048, 512, 1, False, 3, 4, True, False),
    "E": (512, 128, 1, False, 9, 7, True, True),
}
N = 2


def _run_block(case, seed=5, dx_has_grad=None, lateral_scale=1.0, wrap=None):
    """Build the block of `case`, run forward + backward on the device and both references.
    dx_has_grad: override of the flag passed to Bottleneck.backward (the dx buffer is prepared as the case says).
    wrap: callable(block) applied before the run (negative controls). Returns (rows, device outputs for bit comparisons)."""
    import torch
    from mxdetection_amd.models.backbones.resnet import Bottleneck
    from mxdetection_amd.models.utils.layers import ParamArena, Workspace
    cin, planes, stride, down, H, W, need_dx, has_grad = CASES[case]
    g = torch.Generator().manual_seed(seed)
    arena, ws = ParamArena("cuda"), Workspace("cuda")
    b = Bottleneck("blk", cin, planes, stride, down, True, need_dx, arena, ws, "cuda", g)
    _finish(arena, b.layers(), g)
    x_shape = (N, H, W, cin)
    b.plan(x_shape)
    _nan_block_bufs(b, x_shape)
    arena.g.fill_(NAN)
    if wrap is not None:
        wrap(b)
    x = torch.relu(torch.randn(x_shape, generator=g)).to(torch.bfloat16).cuda()        # a block input is never negative
    y = b.forward(x)
    ds = (torch.randn(tuple(y.shape), generator=g) * 0.5).to(torch.bfloat16).cuda() * (y > 0)
    pre = None
    if not need_dx:
        dx_buf = None
    elif has_grad:
        pre = (torch.randn(x_shape, generator=g) * lateral_scale).to(torch.bfloat16).cuda()   # the "lateral gradient"
        dx_buf = pre.clone()
    else:
        dx_buf = torch.full(x_shape, NAN, dtype=torch.bfloat16, device="cuda")
    dx = b.backward(ds, dx_buf, has_grad if dx_has_grad is None else dx_has_grad)
    ws.join()
    torch.cuda.synchronize()
    if not need_dx:
        assert dx is None
    else:
        assert dx is dx_buf
    dev = dict(a1=b.a1.clone(), a2=b.a2.clone(), y=y.clone(), dx=None if dx is None else dx.clone(),
               d_a1=b.bufs[("d_a1", tuple(b.a1.shape), torch.bfloat16)].clone(),
               d_a2=b.bufs[("d_a2", tuple(b.a2.shape), torch.bfloat16)].clone())
    dev.update({"g." + k: v for k, v in _block_grads(b).items()})
    # ---- references
    p, xr, dsr = _block_params(b), _cpu(x), _cpu(ds)
    masks = _device_masks(b)
    prer = None if pre is None else _cpu(pre)
    want = {}
    for e in (False, True):
        f = ref.bottleneck_forward(xr, p, stride, emulate=e)
        want[e] = (f, ref.bottleneck_backward(xr, f, p, stride, dsr, masks, prefill=prer, need_dx=need_dx, emulate=e))
    rows = [(k, _cpu(dev[k]), want[False][0][k], want[True][0][k]) for k in ("a1", "a2", "y")]
    rows += [(k, _cpu(dev[k]), want[False][1][k], want[True][1][k]) for k in ("d_a2", "d_a1")]
    if need_dx:
        rows.append(("dx", _cpu(dx), want[False][1]["dx"], want[True][1]["dx"]))
    for k in sorted(want[False][1]["grads"]):
        rows.append((k + " gradient", dev["g." + k], want[False][1]["grads"][k], want[True][1]["grads"][k]))
    assert len(rows) == 5 + need_dx + 3 + down
    return rows, dev


@pytest.mark.parametrize("case", sorted(CASES))
def test_bottleneck_against_fp64(hip, case):
    rows, dev = _run_block(case)
    bad, _ = ref.check_rows(rows, "case %s " % case)
    assert not bad, bad


@pytest.mark.parametrize("case", ["A", "B-odd", "B-even"])
def test_bottleneck_bitmasks_change_no_bit(hip, monkeypatch, case):
    """1-bit ReLU masks stand in for the activations in the data gradients: every output and gradient is bit-identical to
    the run that reads the activations."""
    import torch
    from mxdetection_amd.models.backbones import resnet
    assert resnet.BITMASKS, "the default is the bitmask path"
    _, with_bits = _run_block(case)
    monkeypatch.setattr(resnet, "BITMASKS", False)
    _, without = _run_block(case)
    assert sorted(with_bits) == sorted(without)
    for k in with_bits:
        assert torch.equal(with_bits[k], without[k]), "case %s: %s differs without the 1-bit masks" % (case, k)


# ---- frozen C2 stage and the stage walk, on one ResNet-50 ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def resnet50(hip):
    import torch
    from mxdetection_amd.models.backbones.resnet import ResNet
    from mxdetection_amd.models.utils.layers import ParamArena, Workspace
    g = torch.Generator().manual_seed(9)
    arena, ws = ParamArena("cuda"), Workspace("cuda")
    net = ResNet(50, arena, ws, "cuda", g)
    _finish(arena, net.layers(), g)
    return net, arena, ws


def test_frozen_c2_stage_chained_and_unchained(hip, resnet50, monkeypatch):
    """The three frozen C2 blocks through _stage_forward in the three settings of the chained launch: conv2 -> conv3 with the
    next block's conv1 riding along, conv2 -> conv3 only, three launches. The block outputs are bit-identical across the
    settings and follow the rule against the fp64 forward. The cached buffers hold another sentinel before each run: a run
    that inherited the previous run's result would show it."""
    import torch
    from mxdetection_amd.models.backbones import resnet
    net = resnet50[0]
    stage = net.stages[0]
    assert len(stage) == 3 and not any(b.trainable for b in stage)
    g = torch.Generator().manual_seed(21)
    x = torch.relu(torch.randn((2, 11, 9, 64), generator=g)).to(torch.bfloat16).cuda()
    runs = {}
    for (chain, chain3), sentinel in (((True, True), NAN), ((True, False), -7.0), ((False, False), 1.0e30)):
        monkeypatch.setattr(resnet, "CHAIN_FROZEN", chain)
        monkeypatch.setattr(resnet, "CHAIN3_FROZEN", chain3)
        assert stage[0].chainable() == chain
        s = tuple(x.shape)
        for b in stage:
            _nan_block_bufs(b, s, sentinel)
            s = b.conv3.out_shape(b.conv2.out_shape(b.conv1.out_shape(s)))
        out = net._stage_forward(stage, x, None)
        torch.cuda.synchronize()
        assert out is stage[-1].y
        assert [b.a2 is None for b in stage] == [chain] * 3              # the chained launch never writes a2
        runs[(chain, chain3)] = dict(y=[b.y.clone() for b in stage], a1=[b.a1.clone() for b in stage],
                                     a2=[None if b.a2 is None else b.a2.clone() for b in stage])
    base = runs[(False, False)]
    for key, r in runs.items():
        for i in range(3):
            assert torch.equal(r["y"][i], base["y"][i]), "setting %s: y of block %d differs from the three launches" % (key, i)
            assert torch.equal(r["a1"][i], base["a1"][i]), "setting %s: a1 of block %d differs" % (key, i)
    blocks = [(_block_params(b), 1) for b in stage]
    want = {e: ref.stage_forward(_cpu(x), blocks, emulate=e) for e in (False, True)}
    rows = []
    for i in range(3):
        for k in ("a1", "a2", "y"):
            rows.append(("layer1.%d %s" % (i, k), _cpu(base[k][i]), want[False][i][k], want[True][i][k]))
    bad, _ = ref.check_rows(rows, "frozen C2 ")
    assert not bad, bad


def _walk(resnet50, seed=31, scale=1.0):
    """forward(None) from a C2 override and backward(dC) on the ResNet-50; returns the rows of the rule."""
    import torch
    net, arena, ws = resnet50
    g = torch.Generator().manual_seed(seed)
    c2 = torch.relu(torch.randn((1, 12, 10, 256), generator=g)).to(torch.bfloat16).cuda()
    s = tuple(c2.shape)
    for st in net.stages[1:]:
        for b in st:
            _nan_block_bufs(b, s)
            s = b.plan(s)
    arena.g.fill_(NAN)
    net.front_override = c2
    try:
        outs = net.forward(None)
    finally:
        net.front_override = None
    assert outs[0] is c2 and [tuple(o.shape) for o in outs[1:]] == [(1, 6, 5, 512), (1, 3, 3, 1024), (1, 2, 2, 2048)]
    dC = [torch.full(tuple(c2.shape), NAN, dtype=torch.bfloat16, device="cuda")]
    dC += [(torch.randn(tuple(o.shape), generator=g) * scale).to(torch.bfloat16).cuda() for o in outs[1:]]
    dC[3] = dC[3] * (outs[3] > 0)
    dC_in = [t.clone() for t in dC]
    net.backward(dC)
    ws.join()
    torch.cuda.synchronize()
    assert torch.isnan(dC[0]).all(), "dC[0] belongs to the frozen C2: the backbone must not touch it"
    assert torch.equal(dC[3], dC_in[3])
    # no frozen layer has a gradient: they are not in the arena at all, and every arena entry is a filter of layer2..layer4
    frozen = [l for b in net.stages[0] for l in b.layers()]
    assert all(not l.trainable and not hasattr(l, "wi") for l in frozen)
    trainable = [l for st in net.stages[1:] for b in st for l in b.layers()]
    assert sorted(e[0] for e in arena.entries) == sorted(l.name + ".weight" for l in trainable)
    # ---- references, teacher-forced by the device's masks
    stages = [[(_block_params(b), b.conv2.stride) for b in st] for st in net.stages[1:]]
    masks = [[_device_masks(b) for b in st] for st in net.stages[1:]]
    dCr = [_cpu(t) for t in dC_in[1:]]
    want = {}
    for e in (False, True):
        f = ref.resnet_forward(_cpu(c2), stages, emulate=e)
        want[e] = (f, ref.resnet_backward(stages, f, dCr, masks, emulate=e))
    rows = [("C%d" % (j + 3), _cpu(outs[j + 1]), want[False][0][j][-1]["y"], want[True][0][j][-1]["y"]) for j in range(3)]
    for j in range(2):
        rows.append(("dC[%d]" % (j + 1), _cpu(dC[j + 1]), want[False][1][0][j], want[True][1][0][j]))
    for j, st in enumerate(net.stages[1:]):
        for bi, b in enumerate(st):
            got = _block_grads(b)
            for k in sorted(got):
                rows.append(("%s gradient" % getattr(b, k.split(".")[0]).name, got[k], want[False][1][1][j][bi][k],
                             want[True][1][1][j][bi][k]))
    assert len(rows) == 3 + 2 + 3 * 13 + 3
    return rows


def test_stage_walk_against_fp64(hip, resnet50):
    """C3..C5 forward from a C2 override and ResNet.backward through layer4 -> layer2: C3, C4, C5, the final contents of
    dC[1] and dC[2] (the lateral gradient plus the stage's own, masked) and the weight gradient of every layer."""
    bad, _ = ref.check_rows(_walk(resnet50), "walk ")
    assert not bad, bad


# ---- negative controls: wrong Python wiring, same kernels --------------------------------------------------------------------
def test_control_lost_lateral_gradient_is_detected(hip):
    """Case B told dx_has_grad=False although dx_buf holds a lateral gradient: the projection shortcut overwrites it."""
    good, _ = ref.check_rows(_run_block("B-odd")[0], "control 1, right flag ")
    assert not good
    bad, _ = ref.check_rows(_run_block("B-odd", dx_has_grad=False)[0], "control 1, wrong flag ")
    assert [b[0] for b in bad] == ["dx"], bad


def test_control_dropped_relu_mask_is_detected(hip):
    """Case A with conv1's data gradient called without its ReLU mask: dx is no longer masked by x > 0."""
    def drop_mask(b):
        inner = b.conv1.backward_data

        def backward_data(dy, x_shape, residual=None, relu_mask=None, accumulate=False, out=None, relu_bits=None):
            return inner(dy, x_shape, residual=residual, accumulate=accumulate, out=out)
        b.conv1.backward_data = backward_data
    bad, _ = ref.check_rows(_run_block("A", wrap=drop_mask)[0], "control 2 ")
    assert [b[0] for b in bad] == ["dx"], bad
