"""RetinaHead (models/rpn_heads/retina_head.py) on its own, forward and backward against the fp64 restatement of
tests/_dense_head_ref.py: a standalone head on its own arena and workspace, N = 2, the odd pyramid of the neck tests plus a
1 x 1 level, random trainable biases (zero on the padded channels, the focal prior on retina.cls_out), NaN in every buffer and in
the gradient arena that the head must fully write. The upstream gradients are injected (head.gco / head.gbo: random bf16 maps,
zero in the padded channels, as every loss kernel leaves them), so the head chain is tested apart from the losses.

Rule: |got - exact| <= 2 E + 2^-9 max |exact|, E = max |emulated - exact| from the CPU reference alone (_backbone_ref.check_rows).
The ReLU masks of the backward are the device's own stored activations. Every layout runs with the weight gradients summed by
accumulate flags (ws.grouping = False) and by the grouped plan (ws.grouping = True, ws.flush(), ws.join()), three times on the
same head without clearing the arena: fresh inputs twice, then one level whose gco / gbo are all zero.

Largest achieved / bound over all rows, layouts, runs and both summation paths, measured on an MI355X: 0.449 (the reg_max = 16
layout; 0.428 .. 0.436 for the others, the same figures with accumulate flags and with the grouped plan).
The two controls (Python wiring only) show that the rule reports an overwritten weight-gradient sum (532 x the bound) and an
overwritten dP (94 x the bound)."""
import pytest

import _backbone_ref as bref
import _dense_head_ref as ref

pytestmark = pytest.mark.gpu
NAN = float("nan")
N = 2
SIZES = [(13, 10), (7, 5), (4, 3), (2, 2), (1, 1)]
STRIDES = [8, 16, 32, 64, 128]
# channels, num_classes, head arguments, (ld_cls, real), (ld_reg, real), num_convs
LAYOUTS = {
    "c64-3cls": (64, 3, {}, (64, 27), (64, 36), 4),
    "c64-80cls": (64, 80, {}, (768, 720), (64, 36), 4),
    "c64-gfl": (64, 3, dict(ratios=(1.0,), octave_scales=(1.0,), reg_max=16, reg_loss="giou"), (64, 3), (128, 68), 4),
    "c64-1conv": (64, 3, {}, (64, 27), (64, 36), 1),
    "c256-80cls": (256, 80, {}, (768, 720), (64, 36), 4),
}


def _cpu(t):
    return t.double().cpu()


def _build(layout, seed=3):
    """finalize, materialize, random biases on the real channels, post_materialize, bf16 + transposed copies, plan; NaN in the
    gradient arena and in every buffer forward / backward must fully write."""
    import torch
    from mxdetection_amd.models.rpn_heads.retina_head import RetinaHead
    from mxdetection_amd.models.utils.layers import ParamArena, Workspace
    C, ncls, kw, (ld_cls, real_cls), (ld_reg, real_reg), n = LAYOUTS[layout]
    arena, ws = ParamArena("cuda"), Workspace("cuda")
    head = RetinaHead(C, STRIDES, arena, ws, "cuda", torch.Generator().manual_seed(seed), num_classes=ncls, num_convs=n, **kw)
    assert (head.ld_cls, head.cls_out.cout_real, head.ld_reg, head.box_out.cout_real) == (ld_cls, real_cls, ld_reg, real_reg)
    assert len(head.layers()) == 2 * n + 2 and len({l.name for l in head.layers()}) == 2 * n + 2
    arena.finalize()
    g = torch.Generator().manual_seed(seed + 1)
    for l in head.layers():
        l.materialize()
        b = torch.zeros((l.cout,))
        b[:l.cout_real] = torch.randn((l.cout_real,), generator=g) * 0.1
        arena.view(l.bi, "w").copy_(b.cuda())
    head.post_materialize()
    arena.refresh_bf16()
    for l in head.layers():
        l.refresh_transposed()
    shapes = [(N, h, w, C) for h, w in SIZES]
    head.plan(shapes, 4)
    ws.get()
    arena.g.fill_(NAN)
    for l, s in enumerate(shapes):
        for i in range(n):
            for key in ("c%d_%d", "b%d_%d", "dc%d_%d", "db%d_%d"):
                head._buf(key % (l, i + (key[0] == "d")), s).fill_(NAN)
        head._buf("co%d" % l, s[:3] + (ld_cls,)).fill_(NAN)
        head._buf("bo%d" % l, s[:3] + (ld_reg,)).fill_(NAN)
    dev = dict(P=[torch.empty(s, dtype=torch.bfloat16, device="cuda") for s in shapes],
               gco=[torch.empty(s[:3] + (ld_cls,), dtype=torch.bfloat16, device="cuda") for s in shapes],
               gbo=[torch.empty(s[:3] + (ld_reg,), dtype=torch.bfloat16, device="cuda") for s in shapes],
               dP=[torch.empty(s, dtype=torch.bfloat16, device="cuda") for s in shapes])
    return head, arena, ws, dev, g


def _params(head, arena):
    p = {}
    for l in head.layers():
        p[l.name + ".weight"] = _cpu(arena.view(l.wi, "wb"))
        p[l.name + ".bias"] = _cpu(arena.view(l.bi, "w"))
    return p


def _inputs(head, g, zero_level=None):
    """P, gco, gbo of one run: bf16 values; the padded channels of gco / gbo zero, one level all zero if asked."""
    import torch
    P = [torch.randn((N, h, w, head.C), generator=g).to(torch.bfloat16) for h, w in SIZES]
    grads = []
    for ld, real in ((head.ld_cls, head.cls_out.cout_real), (head.ld_reg, head.box_out.cout_real)):
        ts = []
        for l, (h, w) in enumerate(SIZES):
            t = torch.randn((N, h, w, ld), generator=g) * 0.5
            t[..., real:] = 0
            if l == zero_level:
                t.zero_()
            ts.append(t.to(torch.bfloat16))
        grads.append(ts)
    return P, grads[0], grads[1]


def _run(head, arena, ws, dev, inputs, grouping):
    """One forward and backward on the device; returns the rows of the rule. The arena is left as the previous run left it."""
    import torch
    n, L = len(head.cls_convs), len(SIZES)
    for key, src in zip(("P", "gco", "gbo"), inputs):
        for d, s in zip(dev[key], src):
            d.copy_(s.cuda())
    for d in dev["dP"]:
        d.fill_(NAN)
    ws.grouping = grouping
    co, bo = head.forward(dev["P"])
    head.gco, head.gbo = dev["gco"], dev["gbo"]
    head.backward(dev["dP"])
    if grouping:
        ws.flush()
    ws.join()
    torch.cuda.synchronize()
    assert not ws.pending
    P64, gco64, gbo64 = ([t.double() for t in src] for src in inputs)
    for key, want in zip(("P", "gco", "gbo"), (P64, gco64, gbo64)):
        for l in range(L):
            assert torch.equal(_cpu(dev[key][l]), want[l]), "%s[%d] changed" % (key, l)
    for name, t, real in (("co", co, head.cls_out.cout_real), ("bo", bo, head.box_out.cout_real)):
        for l in range(L):
            assert not t[l][..., real:].any(), "%s[%d]: padded output channels are not exactly zero" % (name, l)
    for l in range(L):
        assert not torch.isnan(dev["dP"][l]).any(), "NaN left in dP[%d]" % l
    for idx, (name, _, _, _) in enumerate(arena.entries):
        assert torch.isfinite(arena.view(idx, "g")).all(), "NaN left in the gradient of " + name
    for lay in (head.cls_out, head.box_out):
        assert not arena.view(lay.wi, "g")[lay.cout_real:].any(), lay.name + ": weight gradient beyond cout_real"
        assert not arena.view(lay.bi, "g")[lay.cout_real:].any(), lay.name + ": bias gradient beyond cout_real"
    p = _params(head, arena)
    masks = {k: [[None] + [_cpu(a > 0) for a in acts[1:]] for acts in src]
             for k, src in (("cls", head.cact), ("box", head.bact))}
    want = {}
    for e in (False, True):
        f = ref.retina_head_forward(P64, p, n, emulate=e)
        want[e] = ref.retina_head_backward(P64, f, p, gco64, gbo64, masks, emulate=e)
        want[e].update(f)
    rows = []
    for l in range(L):
        for i in range(1, n + 1):
            rows.append(("cls tower %d level %d" % (i - 1, l), _cpu(head.cact[l][i]), want[False]["cact"][l][i], want[True]["cact"][l][i]))
            rows.append(("box tower %d level %d" % (i - 1, l), _cpu(head.bact[l][i]), want[False]["bact"][l][i], want[True]["bact"][l][i]))
        rows.append(("co%d" % l, _cpu(co[l]), want[False]["co"][l], want[True]["co"][l]))
        rows.append(("bo%d" % l, _cpu(bo[l]), want[False]["bo"][l], want[True]["bo"][l]))
        rows.append(("dP%d" % l, _cpu(dev["dP"][l]), want[False]["dP"][l], want[True]["dP"][l]))
    for lay in head.layers():
        for key, idx in ((lay.name + ".weight", lay.wi), (lay.name + ".bias", lay.bi)):
            rows.append((key + " gradient", _cpu(arena.view(idx, "g")), want[False]["grads"][key], want[True]["grads"][key]))
    assert sorted(want[False]["grads"]) == sorted(p)
    assert len(rows) == L * (2 * n + 3) + 2 * (2 * n + 2)
    return rows


@pytest.mark.parametrize("grouping", [False, True], ids=["accumulate", "grouped"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_retina_head_forward_and_backward_against_fp64(hip, layout, grouping):
    import torch
    head, arena, ws, dev, g = _build(layout)
    real = head.cls_out.cout_real
    bias = arena.view(head.cls_out.bi, "w")
    assert torch.equal(bias[:real], torch.full((real,), head.prior_bias, dtype=torch.float32, device="cuda"))
    assert not bias[real:].any() and not arena.view(head.box_out.bi, "w")[head.box_out.cout_real:].any()
    worst = 0.0
    for tag, zero_level in (("first", None), ("second", None), ("level 2 zero", 2)):
        rows = _run(head, arena, ws, dev, _inputs(head, g, zero_level), grouping)
        bad, w = bref.check_rows(rows, "RetinaHead %s %s, %s run: " % (layout, "grouped" if grouping else "accumulate", tag))
        assert not bad, bad
        worst = max(worst, w)
        if zero_level is not None:      # nothing flows from that level: its dP is exactly zero
            assert not dev["dP"][zero_level].any()
    print("RetinaHead %s %s: worst achieved / bound over the runs %.3f" % (layout, "grouped" if grouping else "accumulate", worst))


def _control_rows(monkeypatch, patch):
    head, arena, ws, dev, g = _build("c64-3cls")
    patch()
    return _run(head, arena, ws, dev, _inputs(head, g), False)


def test_control_overwriting_weight_gradient_sum_is_detected(hip, monkeypatch):
    """ConvLayer.backward_weight forced to accumulate=False (Python wiring only): every shared filter keeps the last level's
    gradient alone. The rule must report the filters' gradients and nothing on the data path."""
    from mxdetection_amd.models.utils.layers import ConvLayer
    inner = ConvLayer.backward_weight
    rows = _control_rows(monkeypatch, lambda: monkeypatch.setattr(
        ConvLayer, "backward_weight", lambda self, x, dy, accumulate=False: inner(self, x, dy, False)))
    bad, _ = bref.check_rows(rows, "control weight-gradient sum: ")
    names = [b[0] for b in bad]
    for tower in ("cls", "box"):
        for k in ["%s%d" % (tower, i) for i in range(4)] + [tower + "_out"]:
            assert "retina.%s.weight gradient" % k in names, (k, names)
    assert all(n.endswith(" gradient") for n in names), names


def test_control_overwriting_box_tower_data_gradient_is_detected(hip, monkeypatch):
    """The box tower's last dgrad_call forced to accumulate=False (Python wiring only; no other call of the head accumulates):
    dP loses the class tower's gradient on every level. The rule must report every dP[l] and no parameter gradient."""
    from mxdetection_amd.models.utils.layers import ConvLayer
    inner = ConvLayer.dgrad_call
    seen = []

    def call(self, dy, x_shape, residual=None, relu_mask=None, accumulate=False, out=None, relu_bits=None):
        seen.append((self.name, accumulate))
        return inner(self, dy, x_shape, residual, relu_mask, False, out, relu_bits)

    rows = _control_rows(monkeypatch, lambda: monkeypatch.setattr(ConvLayer, "dgrad_call", call))
    assert sorted(set(s for s in seen if s[1])) == [("retina.box0", True)]
    bad, _ = bref.check_rows(rows, "control box-tower data gradient: ")
    assert sorted(b[0] for b in bad) == ["dP%d" % l for l in range(len(SIZES))], bad
