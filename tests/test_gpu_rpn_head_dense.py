"""The dense path of RPNHead (models/rpn_heads/rpn_head.py; RPN_SPARSE = 0) on its own, forward and backward against the fp64
restatement of tests/_dense_head_ref.py. It is the truth of the sparse-backward tests (tests/test_gpu_rpn_sparse.py), so it gets
a reference of its own: a standalone head on its own arena and workspace, N = 2, C in {64, 256}, the odd five-level pyramid of
the neck tests plus a 1 x 1 level, and a one-level pyramid whose grouped call lists are empty; random trainable biases (zero on
the padded channels of rpn.out), NaN in every buffer and in the gradient arena the head must fully write, the upstream gradient
head.gh injected (random bf16, zero beyond 5 A channels).

Rule: |got - exact| <= 2 E + 2^-9 max |exact|, E = max |emulated - exact| from the CPU reference alone (_backbone_ref.check_rows);
the ReLU masks of the backward are those of the device's own stored t. Cases: dP_has_grad all false (dP prefilled with NaN and
fully overwritten), all true (prefill + gradient, one stored rounding) and mixed; weight gradients summed by accumulate flags and
by the grouped plan; the 1-bit and the bf16 form of the ReLU mask, which must give identical bits in dt and dP.

Largest achieved / bound over all rows and cases, measured on an MI355X: 0.397 (C = 256, five levels; 0.376 .. 0.392 for the
other pyramids and widths, the same figures for both mask forms and both summation paths)."""
import pytest

import _backbone_ref as bref
import _dense_head_ref as ref

pytestmark = pytest.mark.gpu
NAN = float("nan")
N = 2
PYRAMIDS = {"five": [(13, 10), (7, 5), (4, 3), (2, 2), (1, 1)], "one": [(7, 5)]}
HAS_GRAD = {"none": [False] * 5, "all": [True] * 5, "mixed": [True, False, True, False, True]}


def _cpu(t):
    return t.double().cpu()


def _run(monkeypatch, C, sizes, has_grad, grouping, relu_bits, seed=5):
    """A fresh head, one forward and backward; returns (rows of the rule, dt and dP as the device left them)."""
    import torch
    from mxdetection_amd.models.rpn_heads import rpn_head as RH
    from mxdetection_amd.models.utils.layers import ParamArena, Workspace
    monkeypatch.setattr(RH, "RPN_SPARSE", 0)
    monkeypatch.setattr(RH, "RELU_BITS", relu_bits)
    L = len(sizes)
    arena, ws = ParamArena("cuda"), Workspace("cuda")
    head = RH.RPNHead(C, [4, 8, 16, 32, 64][:L], arena, ws, "cuda", torch.Generator().manual_seed(seed))
    arena.finalize()
    g = torch.Generator().manual_seed(seed + 1)
    real = 5 * head.A
    assert head.out.cout_real == real and head.out.cout == RH.HEAD_CPAD
    for l in head.layers():
        l.materialize()
        b = torch.zeros((l.cout,))
        b[:l.cout_real] = torch.randn((l.cout_real,), generator=g) * 0.1
        arena.view(l.bi, "w").copy_(b.cuda())
    arena.refresh_bf16()
    for l in head.layers():
        l.refresh_transposed()
    shapes = [(N, h, w, C) for h, w in sizes]
    head.plan(shapes, 4)
    assert head.sparse is None and head.dt_map is None
    ws.get()
    arena.g.fill_(NAN)
    for l, s in enumerate(shapes):
        head._buf("t%d" % l, s).fill_(NAN)
        head._buf("dt%d" % l, s).fill_(NAN)
        head._buf("h%d" % l, s[:3] + (RH.HEAD_CPAD,)).fill_(NAN)
    P = [torch.randn(s, generator=g).to(torch.bfloat16).cuda() for s in shapes]
    gh = []
    for s in shapes:
        t = torch.randn(s[:3] + (RH.HEAD_CPAD,), generator=g) * 0.5
        t[..., real:] = 0
        gh.append(t.to(torch.bfloat16).cuda())
    # the prefill at the size of the gradient that is added to it, so that neither hides the other: gh 0.5 x rpn.out's filter
    # (std 0.01, 15 real channels) x rpn.conv's (std 0.01, 9 C taps, half of them masked) = 3e-3 .. 7e-3 here
    pre = [(torch.randn(s, generator=g) * 2.0 ** -8).to(torch.bfloat16) for s in shapes]
    dP = [pre[l].cuda() if has_grad[l] else torch.full(shapes[l], NAN, dtype=torch.bfloat16, device="cuda") for l in range(L)]
    P_in, gh_in = [t.clone() for t in P], [t.clone() for t in gh]
    ws.grouping = grouping
    h = head.forward(P)
    assert (head.tbits[0] is not None) == relu_bits
    head.gh = gh
    head.backward(dP, has_grad[:L])           # flush=True: the head issues the recorded weight gradients itself
    ws.join()
    torch.cuda.synchronize()
    assert not ws.pending
    for l in range(L):
        assert torch.equal(P[l], P_in[l]) and torch.equal(gh[l], gh_in[l]), "P / gh of level %d changed" % l
        assert not h[l][..., real:].any(), "h[%d]: padded output channels are not exactly zero" % l
        assert not torch.isnan(dP[l]).any(), "NaN left in dP[%d]" % l
    for idx, (name, _, _, _) in enumerate(arena.entries):
        assert torch.isfinite(arena.view(idx, "g")).all(), "NaN left in the gradient of " + name
    assert not arena.view(head.out.wi, "g")[real:].any() and not arena.view(head.out.bi, "g")[real:].any()
    p = {}
    for l in head.layers():
        p[l.name + ".weight"] = _cpu(arena.view(l.wi, "wb"))
        p[l.name + ".bias"] = _cpu(arena.view(l.bi, "w"))
    P64, gh64, pre64 = [_cpu(t) for t in P], [_cpu(t) for t in gh], [t.double() for t in pre]
    masks = [_cpu(t > 0) for t in head.t]
    dt = [head._buf("dt%d" % l, shapes[l]) for l in range(L)]
    want = {}
    for e in (False, True):
        f = ref.rpn_head_forward(P64, p, emulate=e)
        want[e] = ref.rpn_head_backward(P64, f, p, gh64, masks, pre64, has_grad[:L], emulate=e)
        want[e].update(f)
    rows = []
    for l in range(L):
        rows.append(("t%d" % l, _cpu(head.t[l]), want[False]["t"][l], want[True]["t"][l]))
        rows.append(("h%d" % l, _cpu(h[l]), want[False]["h"][l], want[True]["h"][l]))
        rows.append(("dt%d" % l, _cpu(dt[l]), want[False]["dt"][l], want[True]["dt"][l]))
        rows.append(("dP%d" % l, _cpu(dP[l]), want[False]["dP"][l], want[True]["dP"][l]))
    for lay in head.layers():
        for key, idx in ((lay.name + ".weight", lay.wi), (lay.name + ".bias", lay.bi)):
            rows.append((key + " gradient", _cpu(arena.view(idx, "g")), want[False]["grads"][key], want[True]["grads"][key]))
    assert len(rows) == 4 * L + 4
    return rows, [t.clone() for t in dt] + [t.clone() for t in dP]


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("grouping", [False, True], ids=["accumulate", "grouped"])
@pytest.mark.parametrize("has_grad", list(HAS_GRAD))
@pytest.mark.parametrize("pyramid", list(PYRAMIDS))
@pytest.mark.parametrize("C", [64, 256])
def test_rpn_head_dense_forward_and_backward_against_fp64(hip, monkeypatch, C, pyramid, has_grad, grouping):
    import torch
    tag = "RPNHead dense C%d %s %s %s" % (C, pyramid, has_grad, "grouped" if grouping else "accumulate")
    maps = {}
    for relu_bits in (True, False):
        rows, maps[relu_bits] = _run(monkeypatch, C, PYRAMIDS[pyramid], HAS_GRAD[has_grad], grouping, relu_bits)
        bad, _ = bref.check_rows(rows, "%s, %s mask: " % (tag, "1-bit" if relu_bits else "bf16"))
        assert not bad, bad
    for a, b in zip(maps[True], maps[False]):       # same seed, same inputs: the two mask forms give the same bits
        assert torch.equal(_bits(a), _bits(b)), "dt / dP differ between the 1-bit and the bf16 ReLU mask"
