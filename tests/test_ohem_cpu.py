"""OHEM without a GPU: the selection reference (tests/_ohem_ref.py) against hand-checked answers, the pool assignment on the
C oracle's proposal-target (rois_per_image >= candidates, fg_fraction 1: every candidate, foreground first, ascending, whatever
the seed), option validation in the model / builder / config, and the entries' host argument checks."""
import os

import numpy as np
import pytest

import _ohem_ref as ref
from conftest import synth_boxes, synth_gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _disjoint(n):
    """n boxes of 10 x 10 that do not touch."""
    x = 20.0 * np.arange(n, dtype=np.float32)
    return np.stack([x, np.zeros_like(x), x + 9, np.full_like(x, 9)], 1)


def test_iou_restatement_known_answers():
    a = np.array([0, 0, 99, 99], np.float32)
    b = np.array([[10, 0, 109, 99], [20, 0, 119, 99], [100, 0, 199, 99], [0, 0, 99, 99], [99, 99, 120, 120]], np.float32)
    got = ref.iou_one_to_many(a, b)
    want = np.array([9000 / 11000, 8000 / 12000, 0.0, 1.0, 1.0 / (10000 + 484 - 1)])
    assert got.dtype == np.float32 and np.allclose(got, want, rtol=1e-6)


def test_iou_restatement_is_the_oracle_bit_for_bit(oracle):
    rng = np.random.default_rng(0)
    boxes = synth_boxes(rng, 300)
    boxes[100:200] = boxes[:100] + rng.uniform(-4, 4, (100, 4)).astype(np.float32)
    want = oracle.box_iou(boxes[:50], boxes)
    for i in range(50):
        assert np.array_equal(ref.iou_one_to_many(boxes[i], boxes), want[i])


def test_ties_fall_to_the_pool_slot():
    labels = np.array([1, 0, -1, 0, 2, 0], np.int32)
    score = np.full(6, 0.5, np.float32)
    sel, num, nfg, sup = ref.select_image(score, labels, _disjoint(6), 3, 0.7)
    assert ref.order_image(score, labels).tolist() == [0, 1, 3, 4, 5]
    assert sel.tolist() == [0, 1, 3] and (num, nfg, sup) == (3, 1, 0)


def test_more_slots_than_candidates_pads():
    labels = np.array([1, 0, -1, 0, 2, 0], np.int32)
    score = np.array([0.1, 0.9, 7.0, 0.2, 0.3, 0.4], np.float32)       # slot 2 is no candidate, whatever its score
    sel, num, nfg, sup = ref.select_image(score, labels, _disjoint(6), 8, 0.7)
    assert sel.tolist() == [0, 4, 1, 3, 5, -1, -1, -1] and (num, nfg, sup) == (5, 2, 0)
    # R = 2: the two highest scores (slots 1 and 5), both background
    assert ref.select_image(score, labels, _disjoint(6), 2, 0.7)[0].tolist() == [1, 5]
    # R = 3 adds slot 4, a foreground roi: it is written first
    sel, num, nfg, _ = ref.select_image(score, labels, _disjoint(6), 3, 0.7)
    assert sel.tolist() == [4, 1, 5] and (num, nfg) == (3, 1)


def test_nms_chain_a_suppresses_b_so_c_survives():
    # IoU(A,B) = IoU(B,C) = 0.818 > 0.7 > IoU(A,C) = 0.667; scores A > B > C
    boxes = np.array([[20, 0, 119, 99], [0, 0, 99, 99], [10, 0, 109, 99]], np.float32)     # slots: C, A, B
    score = np.array([1.0, 3.0, 2.0], np.float32)
    labels = np.array([0, 3, 0], np.int32)
    sel, num, nfg, sup = ref.select_image(score, labels, boxes, 3, 0.7)
    assert sel.tolist() == [1, 0, -1] and (num, nfg, sup) == (2, 1, 1)
    # with B first it is A and C that go
    sel, num, nfg, sup = ref.select_image(np.array([1.0, 2.0, 3.0], np.float32), labels, boxes, 3, 0.7)
    assert sel.tolist() == [2, -1, -1] and (num, nfg, sup) == (1, 0, 2)
    # no dedup at 1.0, and strict `>`: a threshold equal to the IoU suppresses nothing
    assert ref.select_image(score, labels, boxes, 3, 1.0)[0].tolist() == [1, 0, 2]
    thr = float(ref.iou_one_to_many(boxes[1], boxes[2:3])[0])
    assert ref.select_image(score, labels, boxes, 3, thr)[0].tolist() == [1, 0, 2]


def test_no_candidates():
    sel, num, nfg, sup = ref.select_image(np.ones(5, np.float32), -np.ones(5, np.int32), _disjoint(5), 4, 0.7)
    assert sel.tolist() == [-1] * 4 and (num, nfg, sup) == (0, 0, 0)


def test_a_nan_score_comes_first():
    score = np.array([0.1, np.nan, 5.0, np.inf], np.float32)
    labels = np.zeros(4, np.int32)
    assert ref.order_image(score, labels).tolist() == [1, 3, 2, 0]
    assert ref.select_image(score, labels, _disjoint(4), 1, 0.7)[0].tolist() == [1]


def test_batched_select_and_gather():
    labels = np.array([[1, 0, -1, 0], [-1, -1, -1, -1]], np.int32)
    score = np.array([[0.1, 0.9, 7.0, 0.2], [1, 1, 1, 1]], np.float32)
    rois = np.zeros((2, 4, 5), np.float32)
    rois[:, :, 1:] = _disjoint(4)
    rois[1, :, 0] = 1
    sel, num, nfg, _ = ref.select(score, labels, rois, 3, 0.7)
    assert sel.tolist() == [[0, 1, 3], [-1, -1, -1]] and num.tolist() == [3, 0] and nfg.tolist() == [1, 0]
    matched = np.array([[5, 6, 7, 8], [0, 0, 0, 0]], np.int32)
    tgt = np.arange(2 * 4 * 8, dtype=np.float32).reshape(2, 4, 8)
    o_rois, o_lab, o_t, o_w, o_m = ref.gather(sel, rois, labels, matched, tgt, tgt + 1)
    assert o_lab.tolist() == [[1, 0, 0], [-1, -1, -1]] and o_m.tolist() == [[5, 6, 8], [-1, -1, -1]]
    assert np.array_equal(o_rois[0], rois[0, [0, 1, 3]]) and np.array_equal(o_rois[1], [[1, 0, 0, 0, 0]] * 3)
    assert np.array_equal(o_t[0], tgt[0, [0, 1, 3]]) and not o_t[1].any() and not o_w[1].any()
    assert ref.gather(sel, rois, labels, matched)[2] is None


@pytest.mark.parametrize("seed", [0, 1])
def test_pool_assignment_returns_every_candidate_foreground_first(oracle, seed):
    """The oracle's proposal-target with rois_per_image >= candidates and fg_fraction 1: all foreground candidates, then all
    background ones, each ascending, then padding -- and the sampling seed / step decide nothing."""
    rng = np.random.default_rng(seed)
    N, S, G = 2, 150, 8
    gt = synth_gt(rng, N, g_max=G, g_lo=2, g_hi=6)
    rois = np.zeros((N, S, 5), np.float32)
    num_rois = np.array([150, 97], np.int32)
    for n in range(N):
        valid = gt[n][gt[n, :, 4] >= 0]
        near = valid[rng.integers(0, len(valid), 60), :4] + rng.uniform(-6, 6, (60, 4)).astype(np.float32)
        rois[n, :, 0] = n
        rois[n, :60, 1:] = near
        rois[n, 60:, 1:] = synth_boxes(rng, S - 60)
    P = (S + G + 63) // 64 * 64
    outs = [oracle.proposal_target(rois, num_rois, gt, R=R, fg_fraction=1.0, seed=sd, step=st)
            for R, sd, st in ((P, 99, 0), (P, 5, 17), (S + G, 99, 3))]
    for o_rois, labels, tgt, wgt, matched, nfg in outs:
        R = labels.shape[1]
        for n in range(N):
            valid = np.flatnonzero(gt[n, :, 4] >= 0)
            cand = np.concatenate([rois[n, :num_rois[n], 1:], gt[n, valid, :4]])
            iou = oracle.box_iou(cand, gt[n, valid, :4])
            best, arg = iou.max(1), valid[iou.argmax(1)]
            fg, bg = np.flatnonzero(best >= 0.5), np.flatnonzero(best < 0.5)
            assert len(fg) >= len(valid) and len(bg) > 20 and len(fg) + len(bg) == len(cand) <= R
            k = len(cand)
            assert nfg[n] == len(fg)
            assert np.array_equal(o_rois[n, :k, 1:], cand[np.concatenate([fg, bg])])
            assert np.array_equal(labels[n, :len(fg)], gt[n, arg[fg], 4].astype(np.int32)) and (labels[n, :len(fg)] > 0).all()
            assert not labels[n, len(fg):k].any() and (labels[n, k:] == -1).all() and (matched[n, k:] == -1).all()
            assert np.array_equal(matched[n, :k], arg[np.concatenate([fg, bg])])
            assert not o_rois[n, k:, 1:].any() and not wgt[n, len(fg):].any() and (wgt[n, :len(fg)].sum(1) == 4).all()
    k = S + G
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)                            # another seed and step: the same pool
    for a, b in zip(outs[0][:5], outs[2][:5]):
        assert np.array_equal(a[:, :k], b[:, :k])              # another R >= candidates: the same rows


def test_option_validation():
    from mxdetection_amd.core.bbox import check_ohem, ohem_pool_size
    from mxdetection_amd.models import FasterRCNN
    for ok in (0.7, 1, 1.0, 1e-3):
        check_ohem(ok)
    for bad in (0, 0.0, -0.5, 1.5, True, "0.7", None, float("nan")):
        with pytest.raises(ValueError, match="ohem_nms"):
            check_ohem(bad)
        with pytest.raises(ValueError, match="ohem_nms"):        # before anything is allocated: no device needed
            FasterRCNN("cpu", ohem=True, ohem_nms=bad)
    with pytest.raises(ValueError, match="ohem must be a bool"):
        FasterRCNN("cpu", ohem="yes")
    assert ohem_pool_size(2000, 100) == 2112 and ohem_pool_size(300, 20) == 320 and ohem_pool_size(60, 4) == 64


def test_config_keys_and_file():
    from mxdetection_amd.utils import load_config
    cfg = load_config()
    assert cfg.network.ohem is False and cfg.network.ohem_nms == 0.7
    a = load_config(os.path.join(ROOT, "configs", "faster_rcnn_r50_fpn_ohem.yaml"))     # only known keys load
    assert a.network.type == "faster_rcnn" and a.network.ohem is True and a.network.ohem_nms == 0.7
    assert load_config(None, ["network.ohem=true", "network.ohem_nms=0.5"]).network.ohem_nms == 0.5


def test_builder_refuses_ohem_for_retinanet_and_checks_the_threshold():
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils import load_config
    with pytest.raises(ValueError, match="network.ohem.*no box head"):
        build_detector(load_config(None, ["network.type=retinanet", "network.ohem=true"]), device="cpu")
    for net_type in ("faster_rcnn", "mask_rcnn"):
        with pytest.raises(ValueError, match="ohem_nms"):
            build_detector(load_config(None, ["network.type=%s" % net_type, "network.ohem=true", "network.ohem_nms=1.5"]),
                           device="cpu")


def test_abi_argument_checks():
    """Argument validation happens on the host before any launch: no GPU needed."""
    from mxdetection_amd import _lib
    lib = _lib.load()
    assert lib.mxdet_ohem_select_workspace_bytes(2, 2112) >= 2 * 2112 * (16 + 4 + 4)
    assert lib.mxdet_ohem_select_workspace_bytes(2, 17409) == 0 and lib.mxdet_ohem_select_workspace_bytes(0, 64) == 0
    sel = (None, None, None)
    assert lib.mxdet_ohem_select(*sel, 2, 17409, 16, 0.7, None, None, None, None, 0, None) == -2
    assert b"P 17409" in lib.mxdet_last_error()
    assert lib.mxdet_ohem_select(*sel, 2, 64, 0, 0.7, None, None, None, None, 0, None) == -2 and b"R" in lib.mxdet_last_error()
    assert lib.mxdet_ohem_select(*sel, 2, 5000, 16, 0.7, None, None, None, None, 0, None) == -2
    assert b"nms_thresh >= 1" in lib.mxdet_last_error()
    assert lib.mxdet_ohem_select(*sel, 2, 5000, 16, 1.0, None, None, None, None, 0, None) == -1      # allowed: null pointers next
    assert lib.mxdet_ohem_select(*sel, 2, 64, 16, 0.0, None, None, None, None, 0, None) == -1
    assert b"nms_thresh" in lib.mxdet_last_error()
    assert lib.mxdet_ohem_select(*sel, 2, 64, 16, 0.7, None, None, None, None, 0, None) == -1 and b"null" in lib.mxdet_last_error()
    g = (None,) * 6
    assert lib.mxdet_ohem_gather(*g, 2, 64, 0, 324, None, None, None, None, None, None) == -2
    assert lib.mxdet_ohem_gather(*g, 2, 20000, 16, 324, None, None, None, None, None, None) == -2
    assert lib.mxdet_ohem_gather(*g, 2, 64, 16, 324, None, None, None, None, None, None) == -1 and b"null" in lib.mxdet_last_error()
    s = (None, None)
    tail = (None,) * 5
    assert lib.mxdet_ohem_roi_score(*s, 1, 448, 448, None, *tail, 2, 8, 0, 81, 324, -1, 1.0, .1, .1, .2, .2, 1.0, None, None) == -2
    assert lib.mxdet_ohem_roi_score(*s, 1, 448, 448, None, *tail, 2, 8, 64, 81, 324, 7, 1.0, .1, .1, .2, .2, 1.0, None, None) == -1
    assert b"kind" in lib.mxdet_last_error()
    assert lib.mxdet_ohem_roi_score(*s, 1, 448, 448, None, *tail, 2, 8, 64, 81, 320, 1, 1.0, .1, .1, .2, .2, 1.0, None, None) == -1
    assert b"null" in lib.mxdet_last_error()
