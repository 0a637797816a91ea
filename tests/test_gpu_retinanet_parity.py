"""One RetinaNet training step (models/retinanet.py: backbone -> RetinaFPN -> RetinaHead -> losses and back, dP and dC handed
from head to neck to backbone) against fp64, on RetinaNet(depth=50), N = 2, a 64 x 96 image -- the smallest for which P7 still
exists (P3 8 x 12 ... P6 1 x 2, P7 1 x 1) -- and a few synthetic ground-truth boxes.

1. The parts are driven by hand in the order of forward_backward, and dP / dC are copied at each boundary. Each part is compared
   with its fp64 restatement, teacher-forced with the DEVICE's maps at its boundary so that error does not add up across parts:
   the head (tests/_dense_head_ref.py) from the device's P and its gco / gbo, the neck (_backbone_ref.retina_*) from the device's
   C3..C5 and the dP the head left, the trainable stages (_backbone_ref.resnet_*) from the device's C2 and the dC the neck left;
   every ReLU mask is that of the device's stored activation. Rule for every parameter gradient and every handed-over map:
   |got - exact| <= 2 E + 2^-9 max |exact|, E = max |emulated - exact| from the CPU reference alone (_backbone_ref.check_rows).
2. forward_backward itself, on the same inputs and a gradient arena full of NaN, must leave the losses and the whole arena as the
   hand-driven sequence did, bit for bit (the step has no fp32-atomic path), and no NaN in any registered entry.
3. A second model of the same seed with enable_grouped_wgrad(): same losses, and its arena under the rule against the same
   references (the summation order differs, so no bits are compared).

Largest achieved / bound, measured on an MI355X: 0.539 (the weight gradient of layer2.3.conv1), hand-driven and grouped alike;
the largest handed-over map is C5 at 0.460."""
import numpy as np
import pytest

import _backbone_ref as bref
import _dense_head_ref as href
from conftest import synth_gt

pytestmark = pytest.mark.gpu
NAN = float("nan")
N, H, W, G_MAX, SEED = 2, 64, 96, 8, 7


def _cpu(t):
    return t.double().cpu()


def _inputs():
    import torch
    gt = synth_gt(np.random.default_rng(41), N, G_MAX, H, W, 3, 6)
    img = torch.randn((N, 3, H, W), generator=torch.Generator().manual_seed(9)).cuda()
    info = torch.tensor([[H, W, 1.0]] * N).cuda()
    return img, torch.from_numpy(gt).cuda(), info


def _model(grouped):
    from mxdetection_amd.models import RetinaNet
    m = RetinaNet("cuda", depth=50, seed=SEED)
    if grouped:
        m.enable_grouped_wgrad()
    return m


def _layer_params(layers, arena):
    p = {}
    for l in layers:
        p[l.name + ".weight"] = _cpu(arena.view(l.wi, "wb"))
        p[l.name + ".bias"] = _cpu(arena.view(l.bi, "w"))
    return p


BLOCK_LAYERS = ("conv1", "conv2", "conv3", "down")


def _block_params(b):
    p = {}
    for key in BLOCK_LAYERS:
        l = getattr(b, key)
        if l is not None:
            p[key + ".weight"] = _cpu(l.w_bf16)
            p[key + ".bias"] = _cpu(l.bias_f32)
    return p


def _arena_bits(arena):
    import torch
    return arena.g.view(torch.int32).clone()


@pytest.fixture(scope="module")
def hand(hip):
    """The hand-driven step on the eager model, the copies taken at the boundaries, and both references of every part."""
    import torch
    m = _model(False)
    img, gt, info = _inputs()
    m.plan(N, H, W, G_MAX)
    m.arena.g.fill_(NAN)
    for t in m.dP + m.dC[1:]:
        t.fill_(NAN)
    C = m.backbone.forward(img)
    P = m.neck.forward(C[1:])
    co, bo = m.head.forward(P)
    loss = m.head.loss_and_grad(gt, info).clone()
    m.head.backward(m.dP)
    dP_head = [_cpu(t) for t in m.dP]
    m.neck.backward(m.dP, m.dC[1:])
    dP6 = _cpu(m.dP[3])
    dC_neck = [_cpu(t) for t in m.dC[1:]]
    m._backbone_backward(0)
    m.ws.flush()
    m.ws.join()
    torch.cuda.synchronize()
    assert [tuple(t.shape[1:3]) for t in P] == [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
    nfg = int(m.head.num_fg)
    print("RetinaNet parity: losses %s, %d foreground anchors" % (loss.tolist(), nfg))
    assert nfg > 0 and any(bool(t.any()) for t in m.head.gbo), "no foreground anchor: the box tower would carry no gradient"
    assert torch.isfinite(loss).all() and float(loss[0]) > 0 and float(loss[1]) > 0
    head, neck, stages_dev = m.head, m.neck, m.backbone.stages[1:]
    rows, want_g = [], {False: {}, True: {}}

    # ---- head: from the device's P and gco / gbo
    n = len(head.cls_convs)
    P64 = [_cpu(t) for t in P]
    p = _layer_params(head.layers(), m.arena)
    masks = {k: [[None] + [_cpu(a > 0) for a in acts[1:]] for acts in src] for k, src in (("cls", head.cact), ("box", head.bact))}
    gco, gbo = [_cpu(t) for t in head.gco], [_cpu(t) for t in head.gbo]
    want = {}
    for e in (False, True):
        f = href.retina_head_forward(P64, p, n, emulate=e)
        want[e] = href.retina_head_backward(P64, f, p, gco, gbo, masks, emulate=e)
        want[e].update(f)
        want_g[e].update(want[e]["grads"])
    for l in range(5):
        rows.append(("head co%d" % l, _cpu(co[l]), want[False]["co"][l], want[True]["co"][l]))
        rows.append(("head bo%d" % l, _cpu(bo[l]), want[False]["bo"][l], want[True]["bo"][l]))
        rows.append(("head dP%d" % l, dP_head[l], want[False]["dP"][l], want[True]["dP"][l]))

    # ---- neck: from the device's C3..C5 and the dP the head left
    feats = [_cpu(t) for t in C[1:]]
    p = _layer_params(neck.layers(), m.arena)
    want = {}
    for e in (False, True):
        f = bref.retina_forward(feats, p, emulate=e)
        want[e] = bref.retina_backward(feats, f, p, dP_head, _cpu(neck.p6_raw > 0), (feats[-1] > 0).double(), emulate=e)
        want[e].update(f)
        want_g[e].update(want[e]["grads"])
    for i in range(5):
        rows.append(("neck P%d" % (i + 3), P64[i], want[False]["P"][i], want[True]["P"][i]))
    for i in range(3):
        rows.append(("neck dC%d" % (i + 3), dC_neck[i], want[False]["dC"][i], want[True]["dC"][i]))
    rows.append(("neck dP6 + masked P7 gradient", dP6, want[False]["dP6"], want[True]["dP6"]))

    # ---- trainable stages: from the device's C2 and the dC the neck left
    stages = [[(_block_params(b), b.conv2.stride) for b in st] for st in stages_dev]
    bmasks = [[{"a1": _cpu(b.a1 > 0), "a2": _cpu(b.a2 > 0), "x": _cpu(b.x > 0)} for b in st] for st in stages_dev]
    want = {}
    for e in (False, True):
        f = bref.resnet_forward(_cpu(C[0]), stages, emulate=e)
        want[e] = (f, bref.resnet_backward(stages, f, dC_neck, bmasks, emulate=e))
        for j, st in enumerate(stages_dev):
            for bi, b in enumerate(st):
                for k, t in want[e][1][1][j][bi].items():
                    want_g[e][getattr(b, k.split(".")[0]).name + ".weight"] = t
    for j in range(3):
        rows.append(("backbone C%d" % (j + 3), feats[j], want[False][0][j][-1]["y"], want[True][0][j][-1]["y"]))
    for j in range(2):
        rows.append(("backbone dC%d, final" % (j + 3), _cpu(m.dC[j + 1]), want[False][1][0][j], want[True][1][0][j]))
    assert torch.equal(_cpu(m.dC[3]), dC_neck[2]), "dC5 belongs to the neck: the backbone must not change it"

    names = [e[0] for e in m.arena.entries]
    assert sorted(want_g[False]) == sorted(names) and len(set(names)) == len(names), "a parameter without a reference gradient"
    return dict(model=m, rows=rows, want_g=want_g, names=names, loss=loss, bits=_arena_bits(m.arena))


def _grad_rows(arena, names, want_g):
    return [(name + " gradient", _cpu(arena.view(idx, "g")), want_g[False][name], want_g[True][name])
            for idx, name in enumerate(names)]


def _no_nan(arena):
    import torch
    for idx, (name, _, _, _) in enumerate(arena.entries):
        assert torch.isfinite(arena.view(idx, "g")).all(), "NaN left in the gradient of " + name


def test_hand_driven_parts_against_fp64(hand):
    _no_nan(hand["model"].arena)
    rows = hand["rows"] + _grad_rows(hand["model"].arena, hand["names"], hand["want_g"])
    assert len(rows) == 15 + 9 + 5 + len(hand["names"]) and len(hand["names"]) == 20 + 16 + 13 * 3 + 3
    bad, _ = bref.check_rows(rows, "RetinaNet step, by hand: ")
    assert not bad, bad


def test_forward_backward_leaves_the_hand_driven_bits(hand):
    import torch
    m = hand["model"]
    img, gt, info = _inputs()
    m.arena.g.fill_(NAN)
    for t in m.dP + m.dC[1:]:
        t.fill_(NAN)
    (loss,) = m.forward_backward(img, gt, info)
    m.ws.join()
    torch.cuda.synchronize()
    assert torch.equal(loss.view(torch.int32), hand["loss"].view(torch.int32)), (loss.tolist(), hand["loss"].tolist())
    _no_nan(m.arena)
    bits = _arena_bits(m.arena)
    for idx, (name, _, off, numel) in enumerate(m.arena.entries):
        assert torch.equal(bits[off:off + numel], hand["bits"][off:off + numel]), name + ": gradient differs from the hand-driven step"
    assert torch.equal(bits, hand["bits"])       # the alignment gaps between the entries too: nothing writes them


def test_grouped_weight_gradients_against_fp64(hand):
    import torch
    m = _model(True)
    assert m.ws.grouping
    img, gt, info = _inputs()
    m.plan(N, H, W, G_MAX)
    m.arena.g.fill_(NAN)
    (loss,) = m.forward_backward(img, gt, info)
    m.ws.join()
    torch.cuda.synchronize()
    assert not m.ws.pending
    assert [e[0] for e in m.arena.entries] == hand["names"]
    assert torch.equal(m.arena.wb, hand["model"].arena.wb), "same seed, other parameters"
    assert torch.equal(loss.view(torch.int32), hand["loss"].view(torch.int32))
    _no_nan(m.arena)
    bad, _ = bref.check_rows(_grad_rows(m.arena, hand["names"], hand["want_g"]), "RetinaNet step, grouped: ")
    assert not bad, bad
