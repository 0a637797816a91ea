"""Mask Scoring R-CNN without a GPU: the reference restatement (tests/_mask_iou_ref.py) against known answers, the loss
against a float64 formula, the config keys, the builder's refusals and the C-ABI's argument checks."""
import os

import numpy as np
import pytest

import _mask_iou_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 28


def _case(roi, logit=8.0, frame=(64, 64), tg=None):
    """One roi on a 64x64 frame whose GT mask is the rectangle x 20..59, y 10..49 (1600 pixels); mask targets all ones and
    logits `logit` everywhere unless given."""
    H, W = frame
    masks = np.zeros((1, 1, H, W), np.uint8)
    masks[0, 0, 10:50, 20:60] = 1
    gt = np.array([[[20, 10, 59, 49, 3]]], np.float32)
    rois = np.array([[0, *roi]], np.float32)
    logits = np.full((1, S, S, 8), logit, np.float32)
    tg = np.ones((1, S, S), np.uint8) if tg is None else tg
    cls = np.array([3], np.int32)
    matched = np.array([0], np.int32)
    return rois, matched, cls, gt, masks, logits, tg


def test_known_answer_exact():
    """Half of the instance in the box, a perfect prediction of that half: the paper's target is 0.5."""
    a = _case((20, 10, 39, 49))
    assert ref.target_counts(*a) == [(1600, 800, S * S, S * S, S * S)]
    t = ref.maskiou_target(*a)
    assert t.dtype == np.float32 and t[0] == np.float32(0.5)


def test_box_variations():
    a = _case((20, 15, 39, 44))
    assert ref.target_counts(*a)[0][:2] == (1600, 600)
    assert abs(float(ref.maskiou_target(*a)[0]) - 0.375) <= 1e-6
    # clipped by the frame: x 40..63 of the box (-> 40..59 of the mask), y 0..49 (-> 10..49)
    a = _case((40, -30, 90, 49))
    assert ref.target_counts(*a)[0][:2] == (1600, 20 * 40)
    assert ref.maskiou_target(*a)[0] == np.float32(0.5)
    # fractional corners: floor(20.5) = 20, ceil(38.2) = 39, floor(10.7) = 10, ceil(48.1) = 49
    a = _case((20.5, 10.7, 38.2, 48.1))
    assert ref.target_counts(*a)[0][:2] == (1600, 800)
    # ... and the same corners moved across an integer: floor(21.0) = 21, ceil(39.01) = 40 -> x 21..40
    a = _case((21.0, 10.0, 39.01, 49.0))
    assert ref.target_counts(*a)[0][1] == 20 * 40
    # a box that misses the mask: no in-box pixels, target 0
    a = _case((0, 0, 15, 8))
    assert ref.target_counts(*a)[0][1] == 0 and ref.maskiou_target(*a)[0] == 0.0
    # a box entirely outside the frame
    a = _case((70, 70, 90, 90))
    assert ref.target_counts(*a)[0][1] == 0 and ref.maskiou_target(*a)[0] == 0.0
    # all-negative logits: empty prediction, IoU 0; half of the map predicted: a_ovr / (a_pred + gt_s - a_ovr)
    a = _case((20, 10, 39, 49), logit=-8.0)
    assert ref.maskiou_target(*a)[0] == 0.0
    lg = np.full((1, S, S, 8), -8.0, np.float32)
    lg[:, :, :S // 2, 2] = 8.0
    a = list(_case((20, 10, 59, 49)))
    a[5] = lg
    assert ref.maskiou_target(*a)[0] == np.float32(392.0) / np.float32(784.0)


def test_rows_that_read_nothing():
    rois, matched, cls, gt, masks, logits, tg = _case((20, 10, 39, 49))
    for c, g in ((-1, -1), (0, 0), (3, -1), (9, 0), (3, 1)):        # not fg / unmatched / class past Cpad / g past G
        assert ref.target_counts(rois, np.array([g], np.int32), np.array([c], np.int32), gt, masks, logits, tg) == [None]
        assert ref.maskiou_target(rois, np.array([g], np.int32), np.array([c], np.int32), gt, masks, logits, tg)[0] == 0.0
    rois[0, 0] = 1                                                   # image index past N
    assert ref.maskiou_target(rois, matched, cls, gt, masks, logits, tg)[0] == 0.0


def test_loss_against_float64(oracle):
    pred = oracle.round_bf16(np.array([[0.25, 0.75, 0.5, 0, 0, 0, 0, 0],
                                       [0.1, 0.2, 0.3, 0, 0, 0, 0, 0],
                                       [0.9, 0.8, 0.7, 0, 0, 0, 0, 0],
                                       [0.4, 0.4, 0.4, 0, 0, 0, 0, 0]], np.float32))
    cls = np.array([2, -1, 1, 3], np.int32)
    t = np.array([0.5, 0.9, 0.0, 0.625], np.float32)          # row 1: ignored roi; row 2: target 0 -> not positive
    loss, grad = ref.maskiou_loss(oracle, pred, cls, t, loss_scale=2.0, weight=0.5)
    p0, p3 = float(pred[0, 1]), float(pred[3, 2])
    want = (2.0 * 0.5 / 2.0) * (0.5 * (p0 - 0.5) ** 2 + 0.5 * (p3 - 0.625) ** 2)
    assert abs(loss - want) <= 1e-12
    g = oracle.bf16_bits_to_f32(grad)
    assert np.count_nonzero(g) == 2
    assert g[0, 1] == oracle.round_bf16(np.float32((np.float32(pred[0, 1]) - np.float32(0.5)) * np.float32(0.5)))
    assert g[3, 2] == oracle.round_bf16(np.float32((np.float32(pred[3, 2]) - np.float32(0.625)) * np.float32(0.5)))
    loss0, grad0 = ref.maskiou_loss(oracle, pred, np.full(4, -1, np.int32), t)
    assert loss0 == 0.0 and not grad0.any()


def test_input_and_score_reference(oracle):
    rng = np.random.default_rng(3)
    mp = oracle.round_bf16(rng.standard_normal((2, 2, 2, 16)).astype(np.float32))
    lg = np.zeros((2, 4, 4, 8), np.float32)
    lg[0, :2, :2, 4] = [[-3.0, 0.5], [2.0, -1.0]]             # window (0,0) of channel 4: max 2.0
    x = ref.maskiou_input(oracle, mp, lg, np.array([5, -1], np.int32), cin=64)
    assert x.shape == (2, 2, 2, 64) and np.array_equal(x[..., :16], oracle.f32_to_bf16_bits(mp))
    sig2 = np.float32(1.0) / (np.float32(1.0) + oracle.expf(np.float32(-2.0)))
    assert x[0, 0, 0, 16] == oracle.f32_to_bf16_bits(sig2) and abs(float(sig2) - 1 / (1 + np.exp(-2.0))) < 1e-6
    assert x[0, 1, 1, 16] == oracle.f32_to_bf16_bits(np.float32(0.5))      # all-zero window: sigmoid(0)
    assert not x[1, :, :, 16].any() and not x[..., 17:].any()
    dets = np.array([[0, 0, 9, 9, 0.5, 2], [0, 0, 0, 0, 0, -1], [0, 0, 9, 9, 0.25, 9]], np.float32)
    pred = np.zeros((3, 8), np.float32)
    pred[0, 1], pred[1, 0], pred[2, 7] = 0.75, 0.5, 0.5
    assert np.array_equal(ref.maskiou_score(dets, pred), np.array([0.375, 0.0, 0.0], np.float32))


def test_config_keys_and_file():
    from mxdetection_amd.utils import load_config
    cfg = load_config()
    assert cfg.network.mask_iou is False and cfg.network.mask_iou_weight == 1.0
    a = load_config(os.path.join(ROOT, "configs", "mask_scoring_rcnn_r50_fpn.yaml"))     # only known keys load
    assert a.network.type == "mask_rcnn" and a.network.mask_iou is True and a.network.mask_iou_weight == 1.0
    assert load_config(None, ["network.mask_iou=true", "network.mask_iou_weight=0.5"]).network.mask_iou_weight == 0.5


@pytest.mark.parametrize("net_type", ["faster_rcnn", "retinanet"])
def test_builder_refuses_mask_iou_without_a_mask_branch(net_type):
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils import load_config
    cfg = load_config(None, ["network.type=%s" % net_type, "network.mask_iou=true"])
    with pytest.raises(ValueError, match="mask_iou.*no mask branch"):
        build_detector(cfg, device="cpu")


def test_abi_argument_checks():
    """Argument validation happens on the host before any launch: no GPU needed."""
    from mxdetection_amd import _lib
    lib = _lib.load()
    assert lib.mxdet_maskiou_target_workspace_bytes(2, 16) >= 2 * 16 * 4
    rc = lib.mxdet_maskiou_target(None, None, None, None, None, None, None, 4, 2, 16, 8, 96, 128, 28, 128, None, None, 0, None)
    assert rc == -2 and b"G_boxes >= G" in lib.mxdet_last_error()
    rc = lib.mxdet_maskiou_target(None, None, None, None, None, None, None, 4, 2, 16, 16, 96, 128, 28, 128, None, None, 0, None)
    assert rc == -1 and b"null" in lib.mxdet_last_error()
    assert lib.mxdet_maskiou_input(None, None, None, 4, 27, 256, 128, 320, None, None) == -2
    assert lib.mxdet_maskiou_input(None, None, None, 4, 28, 256, 128, 256, None, None) == -2      # Ctot must exceed C
    assert lib.mxdet_maskiou_input(None, None, None, 4, 28, 256, 128, 320, None, None) == -1
    assert lib.mxdet_maskiou_input_bwd(None, 10, 256, 252, None, None) == -2
    assert lib.mxdet_maskiou_loss(None, None, None, 4, 100, 1.0, 1.0, None, None, None) == -2
    assert lib.mxdet_maskiou_loss(None, None, None, 4, 128, 1.0, 1.0, None, None, None) == -1
    assert lib.mxdet_maskiou_score(None, None, 4, 0, None, None) == -2
    assert lib.mxdet_maskiou_score(None, None, 0, 128, None, None) == 0
