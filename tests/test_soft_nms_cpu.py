"""Soft-NMS without a GPU: hand-computed answers for the numpy reference (tests/_soft_nms_ref.py) that the GPU tests compare
the kernels against, its agreement with the C oracle's greedy NMS, the order property the per-image merge relies on
(DESIGN.md 5g), the config keys, and the host-side argument checks of the library."""
import os

import numpy as np
import pytest

import _soft_nms_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_reference_known_answers(oracle):
    # (0,0,9,9) and (0,0,9,7), +1 convention: areas 100 and 80, intersection 80, IoU = 80 / 100 -> 0.8f exactly
    boxes = np.array([[0, 0, 9, 9], [0, 0, 9, 7], [100, 100, 120, 130]], f32)
    scores = np.array([0.9, 0.75, 0.6], f32)
    assert oracle.box_iou(boxes[:1], boxes[1:2])[0, 0] == f32(0.8)
    ids = np.arange(3)
    sel, sc = R.soft_nms_list(oracle, boxes, scores, ids, 1, 0.5, 0.5, 0.001, 3)
    want = f32(0.75) * (f32(1.0) - f32(0.8))                       # 0.15: below the disjoint box's 0.6
    assert sel.tolist() == [0, 2, 1] and sc[0] == f32(0.9) and sc[2] == want
    assert sc[1].view(np.uint32) == f32(0.6).view(np.uint32)       # a disjoint box keeps its bits
    for sigma in (0.5, 0.3):
        sel, sc = R.soft_nms_list(oracle, boxes, scores, ids, 2, 0.5, sigma, 0.001, 3)
        t = f32(f32(0.8) * f32(0.8)) / f32(sigma)                  # t = o * o; t = t / sigma, each rounded to fp32
        want = f32(0.75) * oracle.expf(np.array([-t], f32))[0]
        assert sel.tolist() == [0, 2, 1] and sc[2] == want and 0.0 < want < 0.75 * np.exp(-0.64 / sigma) * 1.0001
        assert sc[1].view(np.uint32) == f32(0.6).view(np.uint32)   # expf(-0.0f) == 1.0f exactly
    assert oracle.expf(np.array([-0.0], f32))[0] == f32(1.0)
    # hard: the overlapping box dies; linear below the threshold leaves the score alone
    sel, sc = R.soft_nms_list(oracle, boxes, scores, ids, 0, 0.5, 0.5, 0.001, 3)
    assert sel.tolist() == [0, 2] and sc.tolist() == [f32(0.9), f32(0.6)]
    sel, sc = R.soft_nms_list(oracle, boxes, scores, ids, 1, 0.85, 0.5, 0.001, 3)
    assert sel.tolist() == [0, 1, 2] and sc[1] == f32(0.75)
    # min_score is a strict bound; max_keep cuts the loop
    sel, _ = R.soft_nms_list(oracle, boxes, scores, ids, 1, 0.5, 0.5, float(f32(0.75) * (f32(1.0) - f32(0.8))), 3)
    assert sel.tolist() == [0, 2]
    sel, _ = R.soft_nms_list(oracle, boxes, scores, ids, 1, 0.5, 0.5, 0.001, 1)
    assert sel.tolist() == [0]


def test_reference_ties_resolve_by_id(oracle):
    # identical boxes with equal scores: the lower id goes first, whatever its position
    boxes = np.array([[10, 10, 50, 50]] * 3 + [[200, 200, 240, 260]], f32)
    scores = np.array([0.5, 0.5, 0.5, 0.5], f32)
    sel, sc = R.soft_nms_list(oracle, boxes, scores, np.array([7, 3, 5, 9]), 2, 0.5, 0.5, 0.001, 4)
    w = oracle.expf(np.array([-(f32(1.0) / f32(0.5))], f32))[0]
    assert sel.tolist() == [1, 3, 2, 0]                            # ids 3, 9 (untouched 0.5), then 5, 7 (decayed)
    assert sc[0] == f32(0.5) and sc[1] == f32(0.5) and sc[2] == f32(0.5) * w and sc[3] == f32(0.5) * w * w
    # two different starting scores that meet after a decay tie by id as well, not by position or starting score
    d = f32(0.625) * (f32(1.0) - f32(0.8))
    boxes = np.array([[0, 0, 9, 9], [300, 0, 309, 9], [0, 0, 9, 7]], f32)
    scores = np.array([1.0, d, 0.625], f32)
    sel, sc = R.soft_nms_list(oracle, boxes, scores, np.array([0, 2, 1]), 1, 0.5, 0.5, 0.001, 3)
    assert sel.tolist() == [0, 2, 1] and sc[1] == d and sc[2] == d
    sel, _ = R.soft_nms_list(oracle, boxes, scores, np.array([0, 1, 2]), 1, 0.5, 0.5, 0.001, 3)
    assert sel.tolist() == [0, 1, 2]


def test_reference_method0_is_greedy_nms(oracle):
    rng = np.random.default_rng(3)
    boxes = np.concatenate([R._clustered_boxes(rng, 100, 6)[0], R._clustered_boxes(rng, 100, 40)[0]])
    scores = (np.round(rng.uniform(0.01, 1.0, 200) * 64) / 64 + 1 / 64).astype(f32)          # ties
    order = np.lexsort((np.arange(200), -scores))
    for thr in (0.3, 0.5, 0.7):
        want = oracle.nms(boxes[order], thr)
        sel, sc = R.soft_nms_list(oracle, boxes[order], scores[order], np.arange(200), 0, thr, 0.5, 0.001, 200)
        assert 5 < len(want) < 200 and np.array_equal(sel, want) and np.array_equal(sc, scores[order][want])
        # unsorted input, id = position: the same boxes
        sel2, _ = R.soft_nms_list(oracle, boxes, scores, np.arange(200), 0, thr, 0.5, 0.001, 200)
        assert np.array_equal(sel2, order[want])


@pytest.mark.parametrize("method", [1, 2])
def test_order_property_on_the_clustered_input(oracle, method):
    """Selected (score, id) keys strictly decrease along a list, so a list's output is already sorted for the merge; and
    the clustered input is the non-degenerate one the GPU parity tests assume."""
    rng = np.random.default_rng(11)
    cls, reg, rois, nv, info = R.clustered_case(rng, 2, 300, 21, [300, 187])
    stds = (0.1, 0.1, 0.2, 0.2)
    hard, hnum, sc, bb = oracle.detection_postprocess(cls, reg, rois, nv, info, (0, 0, 0, 0), stds, 0.05, 0.5, 50)
    nlists = 0
    for n in range(2):
        for c in range(1, 21):
            s, b = sc[n * 300:n * 300 + nv[n], c], bb[n * 300:n * 300 + nv[n], c]
            cand = np.flatnonzero(s > f32(0.05))
            sel, ssc = R.soft_nms_list(oracle, b[cand], s[cand], cand, method, 0.5, 0.5, 0.05, 50)
            ids = cand[sel]
            for k in range(1, len(sel)):
                assert ssc[k] < ssc[k - 1] or (ssc[k] == ssc[k - 1] and ids[k] > ids[k - 1])
            assert np.all(ssc > f32(0.05))
            nlists += len(sel) > 1
    assert nlists >= 10
    dets, num, orig = R.detection_postprocess(oracle, cls, reg, rois, nv, info, (0, 0, 0, 0), stds, 0.05, 0.5, 50, method, 0.5)
    assert num.tolist() == [50, 50]
    for decayed, absent in R.non_degenerate(dets, num, orig, hard, hnum):
        assert decayed >= 3 and absent >= 3
    for n in range(2):
        assert np.all(np.diff(dets[n, :, 4]) <= 0)


def test_config_keys_and_files():
    from mxdetection_amd.utils import load_config
    cfg = load_config()
    assert cfg.TEST.nms_method == "hard" and cfg.TEST.soft_sigma == 0.5
    a = load_config(os.path.join(ROOT, "configs", "faster_rcnn_r50_fpn_softnms.yaml"))
    assert a.TEST.nms_method == "linear" and a.network.type == "faster_rcnn"
    b = load_config(os.path.join(ROOT, "configs", "retinanet_r101_fpn_softnms.yaml"))
    assert b.TEST.nms_method == "gaussian" and b.TEST.soft_sigma == 0.5 and b.network.type == "retinanet"
    assert load_config(None, ["TEST.nms_method=gaussian", "TEST.soft_sigma=0.3"]).TEST.soft_sigma == 0.3


def test_unknown_method_raises_when_the_postprocessor_is_built():
    from mxdetection_amd.core.evaluation import DetectionPostprocess, RetinaDetect
    for name in ("linear", "gaussian", "hard"):
        DetectionPostprocess(21, nms_method=name)
    with pytest.raises(ValueError, match="nms_method"):
        DetectionPostprocess(21, nms_method="soft")
    with pytest.raises(ValueError, match="nms_method"):
        RetinaDetect(5, [8, 16, 32], [None] * 3, nms_method="Linear")


def test_library_checks_arguments_before_any_launch():
    """As tests/test_abi.py does for mxdet_nms_batched: no GPU needed, the checks come before any device work."""
    from mxdetection_amd import _lib
    lib = _lib.load()

    def call(n_max, method, sigma, B=1):
        return lib.mxdet_soft_nms_batched(None, None, None, B, n_max, method, 0.5, sigma, 0.001, 10, None, None, None, None)

    assert call(5000, 1, 0.5) == -2 and b"n_max" in lib.mxdet_last_error()
    assert call(100, 7, 0.5) == -1 and b"method" in lib.mxdet_last_error()
    assert call(100, -1, 0.5) == -1
    assert call(100, 2, 0.0) == -1 and b"sigma" in lib.mxdet_last_error()
    assert call(100, 2, -1.0) == -1
    assert call(100, 1, 0.0) == -1 and b"null" in lib.mxdet_last_error()      # sigma is unused by linear: next check
    assert call(100, 1, 0.5, B=0) == 0 and lib.mxdet_last_error() == b""
    # the two detection entries reject the same method / sigma values
    m, s = (_lib.c_f32 * 4)(), (_lib.c_f32 * 4)()
    args = (None, None, 0, 32, 128, None, None, None, 1, 64, 5, m, s, 0.05, 0.5, 10, None, None, None, 0)
    assert lib.mxdet_detection_postprocess_soft(*args, 3, 0.5, None) == -1 and b"method" in lib.mxdet_last_error()
    assert lib.mxdet_detection_postprocess_soft(*args, 2, 0.0, None) == -1 and b"sigma" in lib.mxdet_last_error()
    assert lib.mxdet_detection_postprocess_soft(*args, 1, 0.5, None) == -1 and b"null" in lib.mxdet_last_error()
    rargs = (None, 1, None, 100, 0.05, 0.5, 10, None, None, None, 0)
    assert lib.mxdet_retina_detect_soft(*rargs, 9, 0.5, None) == -1 and b"method" in lib.mxdet_last_error()
    assert lib.mxdet_retina_detect_soft(*rargs, 2, 0.0, None) == -1 and b"sigma" in lib.mxdet_last_error()
