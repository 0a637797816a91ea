"""Ordered sparse weight gradients of the RPN head (csrc/rpn_sparse.hip, WGRAD_ORDERED) against the dense grouped
weight-gradient kernels in the same process: all four gradients must carry the dense BITS (int32 compare), at the default
tunings, with the splits forced deep (several slabs per level) and with the three-tap tile switched off (all one-tap).

The pyramid is test_gpu_rpn_sparse.py's (N = 2, C = 256, 24x40 ... 2x3, Smax = 128): levels 0-2 take the three-tap tile
(virtual pixels), 3x5 and 2x3 the one-tap tile. The "boundary" labels are built from the schedule itself: two adjacent
cells on either side of a split-K slab boundary of each layer, and two cells in one 32-pixel half-step."""
import numpy as np
import pytest

from test_gpu_rpn_sparse import A, BATCH, C, CASES, COFF, CT, LEVELS, N, _bits, _head_grads, _inputs, _model

pytestmark = pytest.mark.gpu

L = len(LEVELS)
TUNINGS = {"default": {}, "deep": {"T3_MINSTEPS": 2, "WG_MINSTEPS": 2, "WG_MAXSTEPS": 2}, "onetap": {"T3_ENABLE": 0},
           "onetap_deep": {"T3_ENABLE": 0, "WG_MINSTEPS": 2, "WG_MAXSTEPS": 3}}
RUNS = [(c, t) for c in ("main", "full", "empty", "boundary") for t in ("default", "deep")] + \
       [("main", "onetap"), ("full", "onetap_deep"), ("boundary", "onetap_deep")]


def _pixel(sched_item, p):
    """(n, h, w) of reduction pixel p of an item, or None for a pad pixel of the virtual row."""
    H, W = sched_item.H, sched_item.W
    Wv = W + 1 if sched_item.kind else W
    n, r = divmod(p, H * Wv)
    h, w = divmod(r, Wv)
    return (n, h, w) if w < W and n < N else None


def _labels_boundary(sched):
    """For both layers: the two cells around the first slab boundary of level 0 and of level 1 that has real cells on
    both sides; two neighbours in one half-step; a few cells on the one-tap levels."""
    cells, pairs = [(0, 0, 10, 10), (0, 0, 10, 11), (1, 3, 1, 1), (1, 3, 1, 2), (0, 4, 0, 0), (1, 4, 1, 2)], []
    for q in range(2):
        for l in (0, 1):
            it = sched[q * L + l]
            span = it.halves_per_slab * 32
            total = N * it.H * (it.W + 1 if it.kind else it.W)
            for b in range(span, total, span):
                lo, hi = _pixel(it, b - 1), _pixel(it, b)
                if lo is not None and hi is not None:
                    cells += [(lo[0], l) + lo[1:], (hi[0], l) + hi[1:]]
                    pairs.append((q, l, b))
                    break
    lab = -np.ones((N, CT, A), np.int32)
    for k, (n, l, h, w) in enumerate(cells):
        lab[n, int(COFF[l]) + h * LEVELS[l][1] + w, k % A] = k & 1
    return lab, pairs


@pytest.fixture(scope="module", params=RUNS, ids=lambda r: "%s-%s" % r)
def run(request, hip):
    import torch
    from mxdetection_amd import _lib
    from mxdetection_amd.models.rpn_heads import rpn_head as RH
    from mxdetection_amd.models.utils.layers import ParamArena, Workspace
    case, tuning = request.param
    assert RH.RPN_SPARSE == 1 and RH.RPN_ORDERED == 1
    lib = _lib.load()
    for k, v in TUNINGS[tuning].items():
        lib.mxdet_debug_set_tuning(_lib.TUNING_KEYS[k], v)
    try:
        dev = "cuda"
        gen = torch.Generator().manual_seed(3)
        arena, ws = ParamArena(dev), Workspace(dev)
        ws.grouping = True
        head = RH.RPNHead(C, [4, 8, 16, 32, 64], arena, ws, dev, gen, batch_size=BATCH)
        arena.finalize()
        for l in head.layers():
            l.materialize()
        arena.refresh_bf16()
        for l in head.layers():
            l.refresh_transposed()
        shapes = [(N, h, w, C) for h, w in LEVELS]
        head.plan(shapes, 8)
        sp = head.sparse
        P = [torch.randn(s, generator=gen).to(torch.bfloat16).to(dev) for s in shapes]
        head.forward(P)
        targets = (0.5 * torch.randn((N, CT * A, 4), generator=gen)).to(dev)
        gt = torch.zeros((N, 8, 5), device=dev)

        def set_labels(lab):
            labels = torch.from_numpy(lab.reshape(N, CT * A)).to(dev)
            head._assigned = (labels, targets)
            sp.build_list(labels)
            head.loss_and_grad(gt, None, 0, 0, assigned=True)

        set_labels(CASES["empty"]())                         # allocates gh: the schedule does not depend on the labels
        g = [arena.view(i, "g") for i in (head.out.wi, head.out.bi, head.conv.wi, head.conv.bi)]
        sp.plan_ordered([(head.t[l], head.gh[l], 1, 1, 1, 0, g[0], g[1], False) for l in range(L)] +
                        [(head.P[l], head.dt_map[l], 3, 3, 1, 1, g[2], g[3], False) for l in range(L)])
        sched = [sp.ordered[i] for i in range(2 * L)]
        pairs = None
        if case == "boundary":
            lab, pairs = _labels_boundary(sched)
        else:
            lab = CASES[case]()
        set_labels(lab)
        dP0 = [torch.randn(s, generator=gen).to(torch.bfloat16).to(dev) for s in shapes]
        out = {"case": case, "tuning": tuning, "sched": sched, "pairs": pairs, "S": int(sp.state[0].item())}
        head.sparse = None                                   # the reference: the dense grouped kernels
        dP = [x.clone() for x in dP0]
        head.backward(dP, [False] * L)
        ws.join()
        assert len(ws.plans) == 1                            # one grouped launch over the ten items
        out["dense"] = (dP, _head_grads(head))
        head.sparse = sp
        for rep in ("ordered", "again"):
            dP = [x.clone() for x in dP0]
            for x in g:
                x.fill_(float("nan"))                        # the ordered path overwrites every element
            head.backward(dP, [False] * L)
            ws.join()
            assert not ws.pending and len(ws.plans) == 1     # nothing recorded, nothing planned
            out[rep] = (dP, _head_grads(head))
        torch.cuda.synchronize()
        return out
    finally:
        for k in TUNINGS[tuning]:
            lib.mxdet_debug_set_tuning(_lib.TUNING_KEYS[k], -1)


def test_schedule_describes_the_case(run):
    sched, tuning = run["sched"], run["tuning"]
    assert [(it.H, it.W) for it in sched] == LEVELS + LEVELS
    assert [it.kind for it in sched[:L]] == [0] * L           # rpn.out is 1x1: one-tap
    assert [it.kind for it in sched[L:]] == ([0] * L if tuning.startswith("onetap") else [1, 1, 1, 0, 0])
    for q in range(2):
        items = sched[q * L:(q + 1) * L]
        slabs = [b.slab0 - a.slab0 for a, b in zip(items, items[1:])] + [items[-1].fold_ksplit - items[-1].slab0]
        assert items[0].slab0 == 0 and all(s >= 1 for s in slabs)
        if tuning.endswith("deep"):
            assert all(s >= 2 for s in slabs[:3]), slabs      # every level that has more than one step has several slabs
    assert run["S"] == {"main": 39, "empty": 0, "full": N * BATCH}.get(run["case"], run["S"])
    if run["pairs"] is not None:
        # boundary case: a pair around a slab boundary for both layers wherever level 0 / 1 has more than one slab
        want = sum(1 for q in range(2) for l in (0, 1)
                   if (sched[q * L + l + 1].slab0 - sched[q * L + l].slab0) > 1)
        assert len(run["pairs"]) == want and (not tuning.endswith("deep") or want == 4), (run["pairs"], want)


def test_weight_gradients_carry_the_dense_grouped_bits(run):
    import torch
    for name, x, y in zip(("out.weight", "out.bias", "conv.weight", "conv.bias"), run["dense"][1], run["ordered"][1]):
        same = torch.equal(x.view(torch.int32), y.view(torch.int32))
        print("%s-%s %-12s S %3d  max|dense| %.3e  max|diff| %.3e" % (run["case"], run["tuning"], name, run["S"],
                                                                      x.abs().max().item(), (x - y).abs().max().item()))
        assert same, (run["case"], run["tuning"], name)
    if run["case"] == "empty":
        assert all(not x.view(torch.int32).any() for x in run["ordered"][1])      # exact (+0) zeros
    else:
        assert all(x.abs().max().item() > 0 for x in run["ordered"][1])


def test_data_gradients_are_unchanged(run):
    import torch
    for l in range(L):
        assert torch.equal(_bits(run["dense"][0][l]), _bits(run["ordered"][0][l])), l


def test_two_runs_agree_bit_for_bit(run):
    import torch
    for x, y in zip(run["ordered"][1], run["again"][1]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_model_step_ordered_on_against_off(hip, monkeypatch):
    """2 x 256 x 320, grouped weight gradients: the whole gradient arena, bit for bit."""
    import torch
    from mxdetection_amd.models.rpn_heads import rpn_head as RH
    batch = _inputs(256, 320, 5)
    arenas = {}
    for ordered in (0, 1):
        monkeypatch.setattr(RH, "RPN_ORDERED", ordered)
        m = _model(1, monkeypatch)
        m.enable_grouped_wgrad()
        losses = torch.cat(m.forward_backward(*batch, step=3, image_offset=0)).clone()
        m.ws.join()
        torch.cuda.synchronize()
        assert (m.rpn_head.sparse.ordered is not None) == bool(ordered)
        assert bool(m.ws_rpn.plans) == (not ordered)          # ordered: nothing went through the RPN workspace
        arenas[ordered] = (m.arena.g.clone(), losses)
    assert 0 < int(m.rpn_head.sparse.state[0].item()) <= 2 * 256
    assert torch.equal(arenas[0][1], arenas[1][1])
    assert torch.equal(arenas[0][0].view(torch.int32), arenas[1][0].view(torch.int32))
