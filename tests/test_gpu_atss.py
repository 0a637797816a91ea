"""mxdet_atss_assign on the device against the numpy restatement of its definition (tests/_atss_ref.py): labels, matched_gt,
bbox_targets and matched_iou bit for bit -- there is no tolerance anywhere in this file.

Fixture S, the smallest at which each branch can go wrong: a 64 x 96 image (levels of 8x12, 4x6, 2x3, 1x2 and 1x1 cells),
N = 2 (image 1 has no valid GT), G_max = 8:

  row  box                      class  purpose
  0    15.5, 7.5, 47.5, 39.5    3      centre equidistant from four P3 cells: ties at the k-th distance across cells
  1    padding                  -1     padding in the middle of the list
  2    10, 10, 70, 50           1      identical to row 3: IoU ties go to the lower GT
  3    10, 10, 70, 50           2      identical to row 2
  4    20, 16, 60, 44           5      nested in rows 2 / 3: anchors positive for several GTs
  5    40, 30, 41, 31           7      no anchor centre inside: a valid GT with zero positives
  6    60, 20, 95, 63           4      touches the image corner
  7    padding                  -1     padding at the end

with 9 anchors per cell (the head's default base anchors, 1161 anchors) and with 1 (ratio 1, scale 8: 129 anchors, P5..P7
hold 6, 2 and 1 anchors, fewer than k). Fixture M: 256 x 320, N = 2, G_max = 32, every fifth row padding; 15,354 anchors at
9 per cell, so P3 (11,520) spans several passes of the 1024-thread workgroup. tests/test_atss_cpu.py asserts that the
fixtures exercise these branches; the reference of each (fixture, anchors, k) is computed once and shared."""
import functools

import numpy as np
import pytest

import _atss_ref as R
from test_atss_cpu import FIXTURES, ONE, test_host_argument_checks_need_no_device as _host_checks

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name, one, topk=9, seed=None):
    from oracle import oracle
    make, H, W = FIXTURES[name]
    anchors, offs = R.pyramid_anchors(oracle, H, W, **(ONE if one else {}))
    gt = make() if seed is None else make(seed)
    return anchors, offs, gt, R.atss_assign(oracle, anchors, offs, gt, topk)


def _device(anchors, offs, gt, topk, with_iou=True, **kw):
    import torch
    from mxdetection_amd.core.anchor import atss_assign
    a, g = torch.from_numpy(anchors).cuda(), torch.from_numpy(gt).cuda()
    out = None
    if not with_iou:
        N, A = gt.shape[0], anchors.shape[0]
        out = (torch.full((N, A), 7, dtype=torch.int32, device="cuda"), torch.full((N, A), 7, dtype=torch.int32, device="cuda"),
               torch.full((N, A, 4), 7.0, device="cuda"), None)
    res = atss_assign(a, offs, g, topk, out=out, **kw)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in res]


def _same(got, want, what):
    labels, matched, targets, miou = got
    wl, wm, wt, wi = want[:4]
    assert np.array_equal(labels, wl), "%s: labels differ at %s" % (what, np.argwhere(labels != wl)[:5].tolist())
    assert np.array_equal(matched, wm), "%s: matched_gt differs at %s" % (what, np.argwhere(matched != wm)[:5].tolist())
    assert np.array_equal(targets.view(np.uint32), wt.view(np.uint32)), "%s: bbox_targets differ" % what
    if miou is not None:
        assert np.array_equal(miou.view(np.uint32), wi.view(np.uint32)), "%s: matched_iou differs" % what


@pytest.mark.parametrize("one", [False, True], ids=["9", "1"])
@pytest.mark.parametrize("name", ["S", "M"])
def test_atss_assign_bit_exact(hip, name, one):
    anchors, offs, gt, want = _case(name, one)
    assert want[0].sum() > 0
    _same(_device(anchors, offs, gt, 9), want, "fixture %s" % name)


@pytest.mark.parametrize("one", [False, True], ids=["9", "1"])
@pytest.mark.parametrize("topk", [1, 16])
def test_atss_topk_limits(hip, topk, one):
    anchors, offs, gt, want = _case("S", one, topk)
    _same(_device(anchors, offs, gt, topk), want, "topk %d" % topk)


def test_atss_without_matched_iou(hip):
    anchors, offs, gt, want = _case("S", False)
    got = _device(anchors, offs, gt, 9, with_iou=False)
    assert got[3] is None
    _same(got, want, "matched_iou = NULL")           # every element of the three outputs was written (they started at 7)


def test_atss_host_argument_checks(hip):
    """topk 0 and 17, descending offsets, off[L] != A_total, a null output, a short workspace: code and message, no launch."""
    import torch
    from mxdetection_amd._lib import MxdetError
    from mxdetection_amd.core.anchor import AtssWorkspace, atss_assign
    _host_checks()
    anchors, offs, gt, _ = _case("S", True)
    a, g = torch.from_numpy(anchors).cuda(), torch.from_numpy(gt).cuda()
    for bad_offs, topk, match in ((offs, 0, "topk"), (offs, 17, "topk"), (offs[:2] + [offs[1] - 1] + offs[3:], 9, "ascending"),
                                  (offs[:-1] + [offs[-1] + 1], 9, "A_total")):      # still ascending: only off[L] is wrong
        with pytest.raises(MxdetError, match=match):
            atss_assign(a, bad_offs, g, topk)
    with pytest.raises(MxdetError, match="workspace"):
        atss_assign(a, offs, g, 9, workspace=AtssWorkspace(1, anchors.shape[0] // 2, 8, "cuda"))
    torch.cuda.synchronize()


def test_atss_run_to_run(hip):
    anchors, offs, gt, _ = _case("M", False)
    first, second = _device(anchors, offs, gt, 9), _device(anchors, offs, gt, 9)
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()


def test_atss_graph_replay_reads_new_ground_truth(hip):
    """Captured once on fixture M, replayed after gt_boxes was overwritten with a second set: the eager result of the
    second set (nothing of the ground truth or of the host offsets is frozen at capture beyond what the call passed)."""
    import torch
    from mxdetection_amd.core.anchor import AtssWorkspace, atss_assign
    anchors, offs, gt_a, want_a = _case("M", False)
    _, _, gt_b, want_b = _case("M", False, 9, 7)
    assert not np.array_equal(want_a[0], want_b[0])
    N, A = gt_a.shape[0], anchors.shape[0]
    a, g = torch.from_numpy(anchors).cuda(), torch.from_numpy(gt_a).cuda()
    ws = AtssWorkspace(N, A, gt_a.shape[1], "cuda")
    out = (torch.empty((N, A), dtype=torch.int32, device="cuda"), torch.empty((N, A), dtype=torch.int32, device="cuda"),
           torch.empty((N, A, 4), device="cuda"), torch.empty((N, A), device="cuda"))
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap):
        graph.capture_begin(capture_error_mode="thread_local")
        atss_assign(a, offs, g, 9, workspace=ws, out=out)
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(cap)
    for gt, want in ((gt_a, want_a), (gt_b, want_b), (gt_a, want_a)):
        g.copy_(torch.from_numpy(gt))
        for t in out:
            t.fill_(3)
        graph.replay()
        torch.cuda.synchronize()
        _same([t.cpu().numpy() for t in out], want, "replay")
