"""GPU parity of Soft-NMS (csrc/soft_nms.hip): the standalone entry, the two detection entries and the
models' predict against the numpy restatement of tests/_soft_nms_ref.py. Indices, scores and boxes are compared bit for
bit (`view(np.uint32)`): both sides use mxdet_math.h's arithmetic without FMA contraction. Every parity test first asserts,
on the reference alone, that its input is one on which Soft-NMS differs from greedy NMS."""
import numpy as np
import pytest

import _soft_nms_ref as R

pytestmark = pytest.mark.gpu

COUNTS = [300, 187, 65, 64, 63, 1, 0, 300]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def lists():
    rng = np.random.default_rng(17)
    boxes, scores = R.clustered_lists(rng, 8, 300, tie_list=7)
    return boxes, scores, np.asarray(COUNTS, np.int32)


def _same(got, want):
    for g, w in zip(got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))


@pytest.mark.parametrize("method", ["hard", "linear", "gaussian"])
def test_soft_nms_batched_bit_exact(hip, oracle, lists, method):
    from mxdetection_amd.ops import soft_nms_batched
    boxes, scores, counts = lists
    m = R.METHODS[method]
    # max_keep below the live count: the loop ends on max_keep
    want = R.soft_nms_batched(oracle, boxes, scores, counts, m, 0.5, 0.5, 0.001, 40)
    assert want[2].tolist() == [40, 40, 40, 40, 40, 1, 0, 40] if m else want[2][0] > 5
    if m:
        assert np.sum(want[1][0] != scores[0][want[0][0]]) >= 3           # decayed scores among the selections
        tied = want[1][7][:-1] == want[1][7][1:]
        assert tied.sum() >= 1 and np.all(want[0][7][:-1][tied] < want[0][7][1:][tied])     # ties, resolved by position
    _same(soft_nms_batched(_t(boxes), _t(scores), _t(counts), method, 0.5, 0.5, 0.001, 40), want)
    # max_keep = n_max, a high min_score: the loop ends on the threshold; the tail is padding
    want = R.soft_nms_batched(oracle, boxes, scores, counts, m, 0.5, 0.5, 0.3, 300)
    assert 3 < want[2][0] < 300 and want[2][6] == 0 and np.all(want[0][0][want[2][0]:] == -1)
    _same(soft_nms_batched(_t(boxes), _t(scores), _t(counts), method, 0.5, 0.5, 0.3, 300), want)
    # max_keep defaults to n_max
    got = soft_nms_batched(_t(boxes), _t(scores), _t(counts), method, 0.5, 0.5, 0.3)
    _same(got, want)


def test_soft_nms_batched_size_limit(hip, oracle):
    """4096 candidates per list (the 16-slot instantiation), two lists, Gaussian."""
    import torch
    from mxdetection_amd.ops import soft_nms_batched
    rng = np.random.default_rng(19)
    boxes, scores = R.clustered_lists(rng, 2, 4096, G=40)
    counts = np.asarray([4096, 4033], np.int32)
    want = R.soft_nms_batched(oracle, boxes, scores, counts, 2, 0.5, 0.5, 0.001, 100)
    assert want[2].tolist() == [100, 100] and want[0].max() > 4000 and np.sum(want[1][1] != scores[1][want[0][1]]) >= 3
    _same(soft_nms_batched(_t(boxes), _t(scores), _t(counts), "gaussian", 0.5, 0.5, 0.001, 100), want)
    with pytest.raises(hip.MxdetError, match="n_max"):
        soft_nms_batched(torch.zeros((1, 4097, 4), device="cuda"), torch.zeros((1, 4097), device="cuda"),
                         torch.tensor([4097], dtype=torch.int32, device="cuda"), "gaussian")


def test_method0_keeps_what_nms_batched_keeps(hip, lists):
    """Method 0 through the Soft-NMS kernel against the bitmask kernels on the same score-sorted lists."""
    from mxdetection_amd.ops import nms_batched, soft_nms_batched
    boxes, scores, counts = lists
    sb, ss = boxes.copy(), scores.copy()
    for b, n in enumerate(counts):
        order = np.lexsort((np.arange(n), -scores[b, :n]))
        sb[b, :n], ss[b, :n] = boxes[b, :n][order], scores[b, :n][order]
    keep, num = nms_batched(_t(sb), _t(counts), 0.5)
    skeep, sscore, snum = soft_nms_batched(_t(sb), _t(ss), _t(counts), "hard", 0.5, 0.5, 0.001)
    keep, num, skeep, sscore, snum = [x.cpu().numpy() for x in (keep, num, skeep, sscore, snum)]
    assert np.array_equal(num, snum) and 5 < num[0] < 300
    for b in range(len(counts)):
        assert np.array_equal(keep[b, :num[b]], skeep[b, :num[b]])
        assert np.array_equal(sscore[b, :num[b]], ss[b][keep[b, :num[b]]])


@pytest.fixture(scope="module")
def det_case(oracle):
    rng = np.random.default_rng(11)
    N, R_, C = 2, 300, 21
    return (N, R_, C) + R.clustered_case(rng, N, R_, C, [300, 187])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_detection_postprocess_soft_bit_exact(hip, oracle, det_case, method, dtype):
    import torch
    from mxdetection_amd.core.evaluation import DetectionPostprocess
    N, R_, C, cls, reg, rois, nvalid, info = det_case
    stds = (0.1, 0.1, 0.2, 0.2)
    if dtype == "bf16":
        cls, reg = oracle.round_bf16(cls), oracle.round_bf16(reg)
    hard, hnum, _, _ = oracle.detection_postprocess(cls, reg, rois, nvalid, info, (0, 0, 0, 0), stds, 0.05, 0.5, 50)
    want, wnum, orig = R.detection_postprocess(oracle, cls, reg, rois, nvalid, info, (0, 0, 0, 0), stds, 0.05, 0.5, 50,
                                               R.METHODS[method], 0.5)
    assert wnum.tolist() == [50, 50]
    for decayed, absent in R.non_degenerate(want, wnum, orig, hard, hnum):
        assert decayed >= 3 and absent >= 3
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    ld = (C + 4 * C + 63) // 64 * 64                      # fused head layout: one [N*R, ld] tensor, cls | reg | padding
    fused = torch.zeros((N * R_, ld), dtype=tdt, device="cuda")
    fused[:, :C] = _t(cls).to(tdt)
    fused[:, C:5 * C] = _t(reg).to(tdt)
    args = (fused[:, :C], fused[:, C:], _t(rois), _t(nvalid), _t(info))
    post = DetectionPostprocess(C, score_thresh=0.05, nms_thresh=0.5, max_per_image=50, stds=stds, nms_method=method,
                                soft_sigma=0.5)
    dets, num = post(*args)
    assert np.array_equal(num.cpu().numpy(), wnum)
    got = dets.cpu().numpy()
    assert np.array_equal(got[..., 5], want[..., 5])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # "hard" is the existing entry: the default object's output, which is the oracle's
    d0, n0 = DetectionPostprocess(C, score_thresh=0.05, nms_thresh=0.5, max_per_image=50, stds=stds)(*args)
    d1, n1 = DetectionPostprocess(C, score_thresh=0.05, nms_thresh=0.5, max_per_image=50, stds=stds, nms_method="hard")(*args)
    assert torch.equal(d0, d1) and torch.equal(n0, n1)
    assert np.array_equal(d0.cpu().numpy().view(np.uint32), hard.view(np.uint32))


@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_retina_detect_soft_bit_exact(hip, oracle, method):
    import torch
    from mxdetection_amd.core.evaluation import RetinaDetect
    rng = np.random.default_rng(23)
    N, A, Cn = 2, 3, 5
    shapes, strides = [(16, 20), (8, 10), (4, 5)], [8, 16, 32]
    cls, reg, base, info = R.retina_case(oracle, rng, N, A, Cn, shapes, strides)
    cls_o = [c[..., :A * Cn].reshape(N, -1) for c in cls]
    reg_o = [r[..., :A * 4].reshape(N, -1, 4) for r in reg]
    Hs, Ws = [s[0] for s in shapes], [s[1] for s in shapes]
    hard, hnum = oracle.retina_detect(cls_o, reg_o, base, Hs, Ws, strides, info, Cn, pre_n=60, score_thresh=0.05,
                                      nms_thresh=0.5, max_det=30)
    want, wnum, orig = R.retina_detect(oracle, cls_o, reg_o, base, Hs, Ws, strides, info, Cn, 60, 0.05, 0.5, 30,
                                       R.METHODS[method], 0.5)
    assert wnum.tolist() == [30, 30]
    for decayed, absent in R.non_degenerate(want, wnum, orig, hard, hnum):
        assert decayed >= 3 and absent >= 3
    tc = [_t(c).to(torch.bfloat16) for c in cls]
    tr = [_t(r).to(torch.bfloat16) for r in reg]
    tb = [_t(b) for b in base]
    dets, num = RetinaDetect(Cn, strides, tb, pre_nms_top_n=60, score_thresh=0.05, nms_thresh=0.5, max_per_image=30,
                             nms_method=method, soft_sigma=0.5)(tc, tr, _t(info))
    assert np.array_equal(num.cpu().numpy(), wnum)
    assert np.array_equal(dets.cpu().numpy().view(np.uint32), want.view(np.uint32))
    d1, n1 = RetinaDetect(Cn, strides, tb, pre_nms_top_n=60, score_thresh=0.05, nms_thresh=0.5, max_per_image=30,
                          nms_method="hard")(tc, tr, _t(info))
    assert np.array_equal(n1.cpu().numpy(), hnum) and np.array_equal(d1.cpu().numpy().view(np.uint32), hard.view(np.uint32))


def test_faster_rcnn_predict_soft(hip):
    import torch
    from mxdetection_amd.models import FasterRCNN
    m = FasterRCNN("cuda", seed=7, pre_nms_top_n=600, post_nms_top_n=300)
    torch.manual_seed(0)
    img = torch.randn(2, 3, 192, 256).cuda()
    info = torch.tensor([[192.0, 256.0, 1.0]] * 2).cuda()
    d0, n0 = [x.clone() for x in m.predict(img, info, score_thresh=0.0, max_per_image=20)]
    dets, num = [x.clone() for x in m.predict(img, info, score_thresh=0.0, max_per_image=20, nms_method="linear")]
    d, k = dets.cpu().numpy(), num.cpu().numpy()
    assert d.shape == (2, 20, 6) and np.all(np.isfinite(d)) and np.all(k == 20)
    for n in range(2):
        assert np.all(d[n, :, 5] >= 1) and np.all(np.diff(d[n, :, 4]) <= 0)          # foreground classes, sorted by score
        assert np.all(d[n, :, 0] >= 0) and np.all(d[n, :, 2] <= 255) and np.all(d[n, :, 3] <= 191)
    # back to "hard": the cached post-processor is keyed by the method, so this is the default output again
    d1, n1 = m.predict(img, info, score_thresh=0.0, max_per_image=20, nms_method="hard")
    assert torch.equal(d1, d0) and torch.equal(n1, n0)


def test_mask_rcnn_predict_soft_with_masks(hip):
    import torch
    from mxdetection_amd.models import FasterRCNN
    m = FasterRCNN("cuda", seed=7, pre_nms_top_n=600, post_nms_top_n=300, with_mask=True)
    torch.manual_seed(0)
    img = torch.randn(2, 3, 192, 256).cuda()
    info = torch.tensor([[192.0, 256.0, 1.0]] * 2).cuda()
    dets, num, masks = m.predict(img, info, score_thresh=0.0, max_per_image=10, with_masks=True, nms_method="gaussian")
    assert dets.shape == (2, 10, 6) and masks.shape == (2, 10, 192, 256) and masks.dtype == torch.uint8
    assert bool(torch.isfinite(dets).all()) and num.tolist() == [10, 10]
    assert bool((dets[..., 4].diff(dim=1) <= 0).all())
