"""Sparse RPN-head backward (csrc/rpn_sparse.hip) against the dense kernels it replaces, on a small pyramid with
hand-built anchor labels, and at model level (sparse on against off, eager and replayed).

Data gradients (compact dt rows, every element of dP) must carry the dense kernels' BITS. In the default mode
(MXDET_TUNE_RPN_SPARSE=1) the weight gradients come from the dense kernels on a scattered dt map and must carry the dense
bits too. In mode 2 they are sums over the slots and differ from the dense ones in fp32 association only; both are measured against an fp64 sum over the same bf16 operands,
err = max|x - ref| / max|ref|, and the sparse error may be at most max(2 * err_dense, 2^-24 * ceil(S / 32)): the sparse sum
has fewer terms than the dense one (factor 2 for the different association), and never less than one fp32 rounding per
32-slot MFMA step."""
import math

import numpy as np
import pytest

from conftest import synth_gt

pytestmark = pytest.mark.gpu

N, C, A, BATCH = 2, 256, 3, 64                         # Smax = N * BATCH = 128 slots
LEVELS = [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)]
COFF = np.concatenate([[0], np.cumsum([h * w for h, w in LEVELS])]).astype(np.int64)
CT = int(COFF[-1])


def _cell(n, l, h, w):
    return n * CT + int(COFF[l]) + h * LEVELS[l][1] + w


def _labels_main():
    """39 active cells: every case of the table in DESIGN.md section 5 (sparse RPN-head backward)."""
    lab = -np.ones((N, CT, A), np.int32)
    cells = []
    cells += [(0, 0, 0, 0), (0, 0, 0, 39), (0, 0, 23, 0), (0, 0, 23, 39)]            # corners (23,39: last cell of image 0)
    cells += [(0, 0, 0, 17), (0, 0, 23, 5), (0, 0, 11, 0), (0, 0, 7, 39)]             # edges
    cells += [(0, 0, 10, 10), (0, 0, 10, 11)]                                         # horizontal neighbours
    cells += [(0, 0, 14, 20), (0, 0, 15, 20)]                                         # vertical
    cells += [(0, 0, 18, 30), (0, 0, 19, 31), (0, 0, 3, 30), (0, 0, 4, 29)]           # both diagonals
    cells += [(0, 0, h, w) for h in (8, 9, 10) for w in (25, 26, 27)]                 # a full 3x3 block
    cells += [(0, 0, 20, 12)]                                                         # its ReLU bits are cleared below
    cells += [(1, 0, 0, 0)]                                                           # first cell of image 1
    cells += [(1, 1, 0, 0), (1, 1, 11, 19), (1, 1, 5, 7), (1, 1, 5, 8)]
    cells += [(0, 2, 2, 3), (1, 2, 5, 9), (0, 3, 1, 2), (1, 3, 0, 0)]
    cells += [(0, 4, 0, 0), (0, 4, 1, 2), (1, 4, 0, 1)]                               # the 2 x 3 level
    for k, (n, l, h, w) in enumerate(cells):
        lab[n, int(COFF[l]) + h * LEVELS[l][1] + w, k % A] = k & 1
    lab[0, 5 * 40 + 5, 0] = 1                                                         # two anchors in one cell
    lab[0, 5 * 40 + 5, 2] = 0
    return lab


def _labels_full():
    rng = np.random.default_rng(11)
    lab = -np.ones((N * CT, A), np.int32)
    ids = rng.choice(N * CT, N * BATCH, replace=False)
    lab[ids, rng.integers(0, A, ids.size)] = rng.integers(0, 2, ids.size)
    return lab.reshape(N, CT, A)


CASES = {"main": _labels_main, "empty": lambda: -np.ones((N, CT, A), np.int32), "full": _labels_full}


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16)


def _rows(ids):
    """(level, row of the level's [N*H*W, *] tensors) of global cell ids."""
    n, gc = ids // CT, ids % CT
    l = np.searchsorted(COFF, gc, side="right") - 1
    return l, n * np.array([h * w for h, w in LEVELS])[l] + gc - COFF[l]


def _wgrad_ref64(P, t, gh, dt):
    """fp64 sums over the bf16 operands: (dw_out, db_out, dw_conv, db_conv)."""
    import torch
    ghf = torch.cat([g.reshape(-1, g.shape[-1]).double() for g in gh])
    tf = torch.cat([x.reshape(-1, x.shape[-1]).double() for x in t])
    dw_conv = torch.zeros((C, 3, 3, C), dtype=torch.float64, device=ghf.device)
    db_conv = torch.zeros((C,), dtype=torch.float64, device=ghf.device)
    for p, d in zip(P, dt):
        n, h, w, _ = p.shape
        pp = torch.nn.functional.pad(p.double(), (0, 0, 1, 1, 1, 1))
        df = d.reshape(-1, C).double()
        db_conv += df.sum(0)
        for kh in range(3):
            for kw in range(3):
                dw_conv[:, kh, kw, :] += df.t() @ pp[:, kh:kh + h, kw:kw + w, :].reshape(-1, C)
    return (ghf.t() @ tf).view(-1, 1, 1, C), ghf.sum(0), dw_conv, db_conv


def _err(x, ref):
    d = ref.abs().max().item()
    e = (x.double() - ref).abs().max().item()
    return e / d if d > 0 else (0.0 if e == 0 else math.inf)


def _check_wgrad(sparse, dense, ref, S):
    floor = 2.0 ** -24 * math.ceil(S / 32)
    for name, xs, xd, r in zip(("out.weight", "out.bias", "conv.weight", "conv.bias"), sparse, dense, ref):
        es, ed = _err(xs.view(r.shape), r), _err(xd.view(r.shape), r)
        print("wgrad %-12s S %4d  err_sparse %.3e  err_dense %.3e  floor %.3e" % (name, S, es, ed, floor))
        assert es <= max(2 * ed, floor), (name, es, ed, floor)


def _head_grads(head):
    g = head.out.arena
    return [g.view(i, "g").clone() for i in (head.out.wi, head.out.bi, head.conv.wi, head.conv.bi)]


@pytest.fixture(scope="module", params=list(CASES))
def run(request, hip):
    """One head, one forward and loss; the dense backward once per accumulate pattern, the sparse one twice."""
    import torch
    from mxdetection_amd.models.rpn_heads import rpn_head as RH
    from mxdetection_amd.models.utils.layers import ParamArena, Workspace
    assert RH.RPN_SPARSE == 1
    dev = "cuda"
    gen = torch.Generator().manual_seed(3)
    arena, ws = ParamArena(dev), Workspace(dev)
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
    assert sp is not None and sp.smax == N * BATCH
    P = [torch.randn(s, generator=gen).to(torch.bfloat16).to(dev) for s in shapes]
    head.forward(P)
    head.tbits[0][0, 20, 12, :] = 0                      # a cell whose ReLU mask is all zero
    lab = CASES[request.param]()
    labels = torch.from_numpy(lab.reshape(N, CT * A)).to(dev)
    targets = (0.5 * torch.randn((N, CT * A, 4), generator=gen)).to(dev)
    head._assigned = (labels, targets)
    sp.build_list(labels)
    head.loss_and_grad(torch.zeros((N, 8, 5), device=dev), None, 0, 0, assigned=True)
    dP0 = [torch.randn(s, generator=gen).to(torch.bfloat16).to(dev) for s in shapes]
    patterns = {"overwrite": [False] * 5, "accumulate": [True] * 5, "mixed": [True, False, True, False, True]}
    out = {"case": request.param, "head": head, "lab": lab, "P": P, "dense": {}, "sparse": {}, "again": {}, "slots": {},
           "slots_again": {}}
    head.sparse = None                                   # today's dense backward
    for k, acc in patterns.items():
        dP = [x.clone() for x in dP0]
        head.backward(dP, acc)
        ws.join()
        out["dense"][k] = (dP, _head_grads(head))
    out["dt"] = [head.bufs[("dt%d" % l, shapes[l], torch.bfloat16)].clone() for l in range(5)]
    head.sparse = sp
    for rep in ("sparse", "again", "slots", "slots_again"):
        head.sparse_wgrad = rep.startswith("slots")      # mode 2: weight gradients over the slots
        for k, acc in patterns.items():
            dP = [x.clone() for x in dP0]
            for i in (head.out.wi, head.out.bi, head.conv.wi, head.conv.bi):
                arena.view(i, "g").fill_(float("nan"))   # the sparse path overwrites every element
            head.backward(dP, acc)
            ws.join()
            out[rep][k] = (dP, _head_grads(head), sp.dts.clone())
        if rep == "sparse":
            out["dt_map"] = [d.clone() for d in head.dt_map]
    head.sparse_wgrad = False
    torch.cuda.synchronize()
    return out


def test_list_count_and_map(run):
    sp = run["head"].sparse
    act = (run["lab"] >= 0).any(2).reshape(-1)
    ids = np.nonzero(act)[0]
    S = int(sp.state[0].item())
    assert S == ids.size
    assert S == {"main": 39, "empty": 0, "full": N * BATCH}[run["case"]]      # "full": the list is at capacity
    lst = sp.list.cpu().numpy()
    assert np.array_equal(lst[:S], ids) and np.all(lst[S:sp.smax] == -1)
    m = -np.ones(N * CT, np.int32)
    m[ids] = np.arange(S)
    assert np.array_equal(sp.map.cpu().numpy(), m)


def test_dt_rows_carry_the_dense_bits(run):
    import torch
    sp = run["head"].sparse
    S = int(sp.state[0].item())
    ids = sp.list.cpu().numpy()[:S].astype(np.int64)
    lv, row = _rows(ids)
    dts = run["sparse"]["overwrite"][2]
    dense = run["dt"]
    seen = [torch.zeros(d.shape[0] * d.shape[1] * d.shape[2], dtype=torch.bool) for d in dense]
    for s in range(S):
        assert torch.equal(_bits(dts[s]), _bits(dense[lv[s]].view(-1, C)[row[s]])), (s, ids[s])
        seen[lv[s]][row[s]] = True
    assert not _bits(dts[S:]).any()                      # rows past S are zero
    for d, sn in zip(dense, seen):                       # ... and so is every dense row that has no slot
        assert not _bits(d.view(-1, C)[~sn.to(d.device)]).any()
    if S:
        assert _bits(dts[:S]).any()
        l0, r0 = _rows(np.array([_cell(0, 0, 20, 12)]))
        if seen[0][r0[0]]:
            assert not _bits(dts[int(np.nonzero(ids == _cell(0, 0, 20, 12))[0][0])]).any()   # masked to zero


@pytest.mark.parametrize("pattern", ["overwrite", "accumulate", "mixed"])
def test_dP_carries_the_dense_bits(run, pattern):
    import torch
    for mode in ("sparse", "slots"):
        dense, sparse = run["dense"][pattern][0], run[mode][pattern][0]
        for l in range(5):
            assert torch.equal(_bits(dense[l]), _bits(sparse[l])), (mode, pattern, l)


def test_default_mode_weight_gradients_carry_the_dense_bits(run):
    """Mode 1: the dense weight-gradient kernels on the scattered dt map -- the map and all four gradients bit for bit."""
    import torch
    for l in range(5):
        assert torch.equal(_bits(run["dt"][l]), _bits(run["dt_map"][l])), l
    for k in run["dense"]:
        for x, y in zip(run["dense"][k][1], run["sparse"][k][1]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k


def test_weight_gradients_against_fp64(run):
    head = run["head"]
    S = int(head.sparse.state[0].item())
    ref = _wgrad_ref64(run["P"], head.t, head.gh, run["dt"])
    _check_wgrad(run["slots"]["overwrite"][1], run["dense"]["overwrite"][1], ref, S)


def test_two_runs_agree_bit_for_bit(run):
    import torch
    for first, second, k in [(f, s_, k) for f, s_ in (("sparse", "again"), ("slots", "slots_again")) for k in run["sparse"]]:
        a, b = run[first][k], run[second][k]
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a[0], b[0]))
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[1], b[1]))
        assert torch.equal(_bits(a[2]), _bits(b[2]))


# ---- model level ------------------------------------------------------------------------------------------------------
def _inputs(H, W, seed):
    import torch
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(1234 + seed)
    image = torch.randn((2, 3, H, W), generator=g).cuda()
    gt = torch.from_numpy(synth_gt(rng, 2, 16, H, W - 5)).cuda()
    im_info = torch.tensor([[H, W - 5, 1.0]] * 2, dtype=torch.float32).cuda()
    return image, gt, im_info


def _model(sparse, monkeypatch):
    from mxdetection_amd.models import FasterRCNN
    from mxdetection_amd.models.rpn_heads import rpn_head as RH
    monkeypatch.setattr(RH, "RPN_SPARSE", int(sparse))   # read when the head plans its buffers
    return FasterRCNN("cuda", seed=7, pre_nms_top_n=1000, post_nms_top_n=1000)


def _rpn_entries(m):
    return [k for k, e in enumerate(m.arena.entries) if e[0].startswith("rpn.")]


def test_model_step_sparse_on_against_off(hip, monkeypatch):
    import torch
    batch = _inputs(256, 320, 5)
    res = {}
    for sparse in (0, 1, 2):
        m = _model(sparse, monkeypatch)
        losses = torch.cat(m.forward_backward(*batch, step=3, image_offset=0)).clone()
        m.ws.join()
        torch.cuda.synchronize()
        assert (m.rpn_head.sparse is not None) == (sparse > 0) and m.rpn_head.sparse_wgrad == (sparse == 2)
        res[sparse] = (m, losses)
    (md, ld), (m1, l1), (ms, ls) = res[0], res[1], res[2]
    assert torch.equal(ld, ls) and torch.equal(ld, l1)
    assert torch.equal(md.arena.g.view(torch.int32), m1.arena.g.view(torch.int32))    # mode 1: every gradient, bit for bit
    rpn = _rpn_entries(md)
    assert [md.arena.entries[k][0] for k in rpn] == ["rpn.out.weight", "rpn.out.bias", "rpn.conv.weight", "rpn.conv.bias"]
    for k, (name, _, _, _) in enumerate(md.arena.entries):    # box head, FPN, backbone: they consume dP, bit for bit
        if k not in rpn:
            assert torch.equal(md.arena.view(k, "g").view(torch.int32), ms.arena.view(k, "g").view(torch.int32)), name
    hd = md.rpn_head
    dt = [hd.bufs[("dt%d" % l, tuple(hd.t[l].shape), torch.bfloat16)] for l in range(5)]
    ref = _wgrad_ref64(hd.P, hd.t, hd.gh, dt)
    S = int(ms.rpn_head.sparse.state[0].item())
    assert 0 < S <= 2 * 256
    _check_wgrad([ms.arena.view(k, "g") for k in rpn], [md.arena.view(k, "g") for k in rpn], ref, S)


@pytest.mark.parametrize("mode", [1, 2])
def test_replayed_step_follows_its_batch(hip, monkeypatch, mode):
    """S, the list and the map are read on the device: a captured step replayed over other batches (lr = 0: fixed weights)
    takes the eager step of each batch. Tolerances: those of the suite's other replay-against-eager checks
    (test_gpu_model.py), with the RPN entries measured against their own largest element."""
    import torch
    m = _model(mode, monkeypatch)
    m.enable_wgrad_stream()
    m.enable_branch_stream()
    m.enable_grouped_wgrad()
    batches = [_inputs(256, 320, 30 + k) for k in range(3)]
    ref, counts = [], []
    for b in batches:
        losses = torch.cat(m.forward_backward(*b, step=7, image_offset=0)).clone()
        m.ws.join()
        torch.cuda.synchronize()
        ref.append((losses, m.arena.g.clone()))
        counts.append(int(m.rpn_head.sparse.state[0].item()))
    m.capture(*batches[0], lr=0.0, image_offset=0, warmup=1)
    rpn = _rpn_entries(m)
    for k in (1, 2, 0):
        got = torch.cat(m.replay(*batches[k], 7)).clone()
        torch.cuda.synchronize()
        assert int(m.rpn_head.sparse.state[0].item()) == counts[k]
        assert torch.allclose(ref[k][0], got, rtol=1e-4, atol=1e-5), (k, ref[k][0], got)
        assert (ref[k][1] - m.arena.g).abs().max().item() <= 1e-3 * ref[k][1].abs().max().item()
        for e in rpn:
            _, shape, off, n = m.arena.entries[e]
            r = ref[k][1][off:off + n]
            assert (r - m.arena.g[off:off + n]).abs().max().item() <= 1e-3 * r.abs().max().item(), (k, m.arena.entries[e][0])
