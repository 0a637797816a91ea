"""The plain FPN (nearest top-down, optional P6 subsample) and the RetinaNet FPN (P6 / P7 convolutions) of models/necks/fpn.py
on their own, forward and backward against the fp64 restatement of tests/_backbone_ref.py, on the odd pyramid of
tests/test_gpu_carafe_model.py: real channel widths, maps of a few pixels, random trainable biases, NaN in every buffer the
neck must fully write (the gradient arena included).

Rule: |got - exact| <= 2 E + 2^-9 max |exact|, E = max |emulated - exact| from the CPU reference alone (every stored map and
stored gradient map rounded to bf16, an in-place sum once more). The ReLU masks of the backward are the device's own
(C5 > 0, P6 > 0): the reference is the exact linear adjoint under them. Every Cout is a multiple of 64: no padding rows."""
import pytest

import _backbone_ref as ref

pytestmark = pytest.mark.gpu
NAN = float("nan")
N = 2


def _cpu(t):
    return t.double().cpu()


def _build(make, c_shapes, seed):
    """make(arena, ws, gen) -> neck; finalize, materialize, random biases, bf16 + transposed copies, plan, NaN gradients."""
    import torch
    from mxdetection_amd.models.utils.layers import ParamArena, Workspace
    arena, ws = ParamArena("cuda"), Workspace("cuda")
    neck = make(arena, ws, torch.Generator().manual_seed(seed))
    arena.finalize()
    g = torch.Generator().manual_seed(seed + 1)
    for l in neck.layers():
        l.materialize()
        arena.view(l.bi, "w").copy_((torch.randn((l.cout,), generator=g) * 0.1).cuda())
    arena.refresh_bf16()
    for l in neck.layers():
        l.refresh_transposed()
    neck.plan(c_shapes)
    arena.g.fill_(NAN)
    return neck, arena, ws, g


def _params(neck, arena):
    p = {}
    for l in neck.layers():
        p[l.name + ".weight"] = _cpu(arena.view(l.wi, "wb"))
        p[l.name + ".bias"] = _cpu(arena.view(l.bi, "w"))
    return p


def _grad_rows(neck, arena, want):
    rows = []
    for l in neck.layers():
        for key, idx in ((l.name + ".weight", l.wi), (l.name + ".bias", l.bi)):
            rows.append((key + " gradient", _cpu(arena.view(idx, "g")), want[False]["grads"][key], want[True]["grads"][key]))
    assert sorted(want[False]["grads"]) == sorted(k for l in neck.layers() for k in (l.name + ".weight", l.name + ".bias"))
    return rows


CHANS = [256, 512, 1024, 2048]
SIZES = [(13, 10), (7, 5), (4, 3), (2, 2)]


def _run_fpn(extra_p6, c_needs_grad, seed=3):
    import torch
    from mxdetection_amd.models.necks import FPN
    c_shapes = [(N, h, w, c) for (h, w), c in zip(SIZES, CHANS)]
    neck, arena, ws, g = _build(lambda a, w, gen: FPN(CHANS, 256, a, w, "cuda", gen, extra_p6=extra_p6, upsample="nearest"),
                                c_shapes, seed)
    p_sizes = SIZES + ([(1, 1)] if extra_p6 else [])
    for i, s in enumerate(c_shapes):                       # the buffers forward / backward must fully write
        for key in ("inner%d" % i, "P%d" % i, "dinner%d" % i):
            neck._buf(key, s[:3] + (256,)).fill_(NAN)
    if extra_p6:
        neck._buf("P6", (N, 1, 1, 256)).fill_(NAN)
    feats = [torch.randn(s, generator=g).to(torch.bfloat16).cuda() for s in c_shapes]
    dP = [(torch.randn((N, h, w, 256), generator=g) * 0.5).to(torch.bfloat16).cuda() for h, w in p_sizes]
    dP_in = [_cpu(t) for t in dP]
    dC = [torch.full(s, NAN, dtype=torch.bfloat16, device="cuda") for s in c_shapes]
    P = neck.forward(feats)
    neck.backward(dP, dC, c_needs_grad)
    ws.join()
    torch.cuda.synchronize()
    assert len(P) == 4 + extra_p6
    if extra_p6:
        assert torch.equal(P[4], P[3][:, ::2, ::2]) and tuple(P[4].shape) == (N, 1, 1, 256)
    for i in range(4):
        assert c_needs_grad[i] or torch.isnan(dC[i]).all(), "dC[%d] is not wanted and must stay untouched" % i
        if i < 3 or not extra_p6:
            assert torch.equal(_cpu(dP[i]), dP_in[i]), "dP[%d] changed" % i
    f64 = [_cpu(f) for f in feats]
    p = _params(neck, arena)
    mask = (f64[-1] > 0).double()
    want = {}
    for e in (False, True):
        f = ref.fpn_forward(f64, p, extra_p6, emulate=e)
        want[e] = ref.fpn_backward(f64, f, p, dP_in, mask, c_needs_grad, extra_p6, emulate=e)
        want[e].update(f)
    rows = []
    for i in range(4):
        rows.append(("inner%d" % i, _cpu(neck.inner[i]), want[False]["inner"][i], want[True]["inner"][i]))
        rows.append(("P%d" % (i + 2), _cpu(P[i]), want[False]["P"][i], want[True]["P"][i]))
        if c_needs_grad[i]:
            rows.append(("dC%d" % i, _cpu(dC[i]), want[False]["dC"][i], want[True]["dC"][i]))
    if extra_p6:
        rows.append(("dP5 + P6 gradient", _cpu(dP[3]), want[False]["dP_top"], want[True]["dP_top"]))
    return rows + _grad_rows(neck, arena, want)


@pytest.mark.parametrize("c_needs_grad", [[True] * 4, [False, True, True, True]], ids=["all", "c2-frozen"])
@pytest.mark.parametrize("extra_p6", [True, False], ids=["p6", "no-p6"])
def test_fpn_forward_and_backward_against_fp64(hip, extra_p6, c_needs_grad):
    rows = _run_fpn(extra_p6, c_needs_grad)
    assert len(rows) == 8 + sum(c_needs_grad) + extra_p6 + 16
    bad, _ = ref.check_rows(rows, "FPN ")
    assert not bad, bad


def test_control_overwriting_top_down_adjoint_is_detected(hip, monkeypatch):
    """dense.upsample2_backward forced to accumulate=False (Python wiring only): each coarser d(inner) loses its own output
    convolution's gradient, and the rule must report it."""
    from mxdetection_amd.ops import dense
    inner = dense.upsample2_backward
    monkeypatch.setattr(dense, "upsample2_backward", lambda dfine, dcoarse, accumulate=False: inner(dfine, dcoarse, False))
    bad, _ = ref.check_rows(_run_fpn(True, [True] * 4), "control 3 ")
    names = [b[0] for b in bad]
    assert "dC1" in names and "dC3" in names and "fpn.lat3.weight gradient" in names, names
    assert "dC0" not in names and not any(n.startswith("fpn.out") or n.startswith("inner") or n.startswith("P") for n in names)


@pytest.mark.parametrize("sizes", [[(7, 5), (4, 3), (2, 2)], [(8, 6), (4, 3), (2, 2)]], ids=["7x5", "8x6"])
def test_retina_fpn_forward_and_backward_against_fp64(hip, sizes):
    import torch
    from mxdetection_amd.models.necks.fpn import RetinaFPN
    chans = [512, 1024, 2048]
    c_shapes = [(N, h, w, c) for (h, w), c in zip(sizes, chans)]
    neck, arena, ws, g = _build(lambda a, w, gen: RetinaFPN(chans, 256, a, w, "cuda", gen), c_shapes, 5)
    for i, s in enumerate(c_shapes):
        for key in ("inner%d" % i, "P%d" % i, "dinner%d" % i):
            neck._buf(key, s[:3] + (256,)).fill_(NAN)
    for key in ("P6", "P6r", "P7", "dP6r"):
        neck._buf(key, (N, 1, 1, 256)).fill_(NAN)
    feats = [torch.randn(s, generator=g).to(torch.bfloat16).cuda() for s in c_shapes]
    dP = [(torch.randn((N, h, w, 256), generator=g) * 0.5).to(torch.bfloat16).cuda() for h, w in sizes + [(1, 1), (1, 1)]]
    dP_in = [t.clone() for t in dP]
    dC = [torch.full(s, NAN, dtype=torch.bfloat16, device="cuda") for s in c_shapes]
    P = neck.forward(feats)
    neck.backward(dP, dC)
    ws.join()
    torch.cuda.synchronize()
    assert [tuple(t.shape) for t in P] == [(N, h, w, 256) for h, w in sizes + [(1, 1), (1, 1)]]
    p6 = P[3]
    assert (p6 > 0).any() and (p6 < 0).any(), "P6 of one sign: the P7 mask would check nothing"
    assert torch.equal(neck.p6_relu, torch.relu(p6))
    for i in (0, 1, 2, 4):
        assert torch.equal(dP[i], dP_in[i]), "dP[%d] changed" % i
    # the in-place sum: dP[L] = bf16(dP[L] + the stored masked P7 data gradient), bit for bit
    t = neck.bufs[("dP6r", (N, 1, 1, 256), torch.bfloat16)]
    assert not t[p6 <= 0].any()
    assert torch.equal(dP[3], (dP_in[3].float() + t.float()).to(torch.bfloat16))
    f64 = [_cpu(f) for f in feats]
    p = _params(neck, arena)
    want = {}
    for e in (False, True):
        f = ref.retina_forward(f64, p, emulate=e)
        want[e] = ref.retina_backward(f64, f, p, [_cpu(d) for d in dP_in], _cpu(p6 > 0), (f64[-1] > 0).double(), emulate=e)
        want[e].update(f)
    rows = []
    for i in range(3):
        rows.append(("inner%d" % i, _cpu(neck.inner[i]), want[False]["inner"][i], want[True]["inner"][i]))
        rows.append(("dC%d" % i, _cpu(dC[i]), want[False]["dC"][i], want[True]["dC"][i]))
    for i in range(5):
        rows.append(("P%d" % (i + 3), _cpu(P[i]), want[False]["P"][i], want[True]["P"][i]))
    rows.append(("dP6 + masked P7 gradient", _cpu(dP[3]), want[False]["dP6"], want[True]["dP6"]))
    rows += _grad_rows(neck, arena, want)
    assert len(rows) == 6 + 5 + 1 + 16
    bad, _ = ref.check_rows(rows, "RetinaFPN %dx%d " % sizes[0])
    assert not bad, bad
