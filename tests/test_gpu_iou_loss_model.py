"""reg_loss = "giou" in the assembled models, at the small shapes of tests/test_gpu_gn_heads.py: the reported regression loss
and the gradient the head receives against the float64 reference of tests/test_iou_loss_cases_cpu.py (evaluated on the head
output, rois / anchors, matches and ground truth copied to the host; tolerances as in tests/test_gpu_iou_loss.py), replayed
steps that read the ground truth from device buffers, inference that does not depend on the option, and the default models
still on the smooth-L1 entries."""
import functools

import numpy as np
import pytest

import test_iou_loss_cases_cpu as T
from test_gpu_gn_heads import _inputs
from test_gpu_iou_loss import _grad_ok, _sum_ok

pytestmark = pytest.mark.gpu

N, H, W = 2, 256, 320
FRCNN_KW = dict(seed=7, pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=128)
RETINA_KW = dict(depth=50, seed=7)
FRCNN_WEIGHT, RETINA_WEIGHT = 10.0, 2.0


@functools.lru_cache(maxsize=None)
def _model(which, reg_loss):
    from mxdetection_amd.models import FasterRCNN, RetinaNet
    w = {} if reg_loss == "smooth_l1" else dict(reg_loss=reg_loss, reg_loss_weight=FRCNN_WEIGHT if which == "frcnn" else RETINA_WEIGHT)
    return FasterRCNN("cuda", **FRCNN_KW, **w) if which == "frcnn" else RetinaNet("cuda", **RETINA_KW, **w)


def _f64(t):
    return t.double().cpu().numpy()


def test_faster_rcnn_giou_step_matches_fp64(hip):
    import torch
    m = _model("frcnn", "giou")
    image, gt, im_info = _inputs(N, H, W, seed=1)
    losses = m.forward_backward(image, gt, im_info, step=2)
    torch.cuda.synchronize()
    h = m.bbox_head
    assert h.reg_loss == "giou" and h.reg_loss_weight == FRCNN_WEIGHT and h.gt_boxes is gt
    R, nc = h.o.shape[0], h.nc
    o, go = _f64(h.o.view(R, h.ld)), _f64(h.go.view(R, h.ld))
    labels = h.labels.view(-1).cpu().numpy()
    ref = T.ref_rcnn_iou(o[:, :nc], o[:, nc:nc + 4 * nc], labels, h.rois.view(-1, 5).cpu().numpy(), h.matched.view(-1).cpu().numpy(),
                         gt.cpu().numpy(), nc, "giou", h.stds, FRCNN_WEIGHT, 1.0 / R, 1.0)
    assert ref["nfg"] >= 8 and R == N * FRCNN_KW["rois_per_image"]
    rcnn = losses[1].cpu().numpy()
    assert abs(rcnn[0] - ref["loss"][0]) <= T.LOSS_RTOL * ref["loss"][0]
    assert _sum_ok("box-head giou loss", rcnn[1], ref["loss"][1], FRCNN_WEIGHT / R, ref["nfg"]) and rcnn[1] > 0
    assert _grad_ok("grad_reg", go[:, nc:nc + 4 * nc], ref["grad_reg"], ref["unit_reg"], T.ATOL_GRAD["head"], True)
    assert _grad_ok("grad_cls", go[:, :nc], ref["grad_cls"], ref["unit"], 2.0 ** -20, True)
    assert not go[:, nc + 4 * nc:].any()
    assert torch.isfinite(m.arena.g).all() and m.export_grads()["bbox.fc_out.weight"].abs().sum().item() > 0


def test_retinanet_giou_step_matches_fp64(hip):
    import torch
    m = _model("retina", "giou")
    image, gt, im_info = _inputs(N, H, W, seed=1)
    (loss,) = m.forward_backward(image, gt, im_info, step=0)
    torch.cuda.synchronize()
    h = m.head
    assert h.reg_loss == "giou" and h.reg_loss_weight == RETINA_WEIGHT
    num_fg = int(h.num_fg.item())
    anchors, matched, cls_labels, gtn = h.anchors.cpu().numpy(), h.matched.cpu().numpy(), h.cls_labels.cpu().numpy(), gt.cpu().numpy()
    total, nfg = np.zeros(2), 0
    for l, (co, bo, gb) in enumerate(zip(h.co, h.bo, h.gbo)):
        ref = T.ref_retina_iou(_f64(co), _f64(bo), h.A, h.Cn, cls_labels, anchors, matched, gtn, h.level_offsets[l], h.alpha, h.gamma,
                               "giou", T.STDS["unit"], RETINA_WEIGHT, num_fg, 1.0)
        total += ref["loss"]
        nfg += ref["nfg"]
        assert _grad_ok("level %d grad_reg" % l, _f64(gb), ref["grad_reg"], ref["unit_reg"], T.ATOL_GRAD["unit"], True)
    assert nfg == num_fg >= 8
    got = loss.cpu().numpy()
    assert abs(got[0] - total[0]) <= T.LOSS_RTOL * total[0]
    assert _sum_ok("retinanet giou loss", got[1], total[1], RETINA_WEIGHT / num_fg, nfg) and got[1] > 0
    assert torch.isfinite(m.arena.g).all()


@pytest.mark.parametrize("which", ["frcnn", "retina"])
def test_replayed_steps_read_the_ground_truth_from_the_device(hip, which):
    """Two replays with different ground truth give the eager losses of each: nothing of the GT is frozen at capture."""
    import torch
    from mxdetection_amd.models import FasterRCNN, RetinaNet
    kw = dict(FRCNN_KW, reg_loss="giou", reg_loss_weight=FRCNN_WEIGHT) if which == "frcnn" else \
        dict(RETINA_KW, reg_loss="giou", reg_loss_weight=RETINA_WEIGHT)
    cls = FasterRCNN if which == "frcnn" else RetinaNet
    image, gt_a, im_info = _inputs(N, H, W, seed=2)
    _, gt_b, _ = _inputs(N, H, W, seed=3)
    assert not torch.equal(gt_a, gt_b)
    eager = _model(which, "giou")
    want = []
    for gt in (gt_a, gt_b):
        want.append(torch.cat(list(eager.forward_backward(image, gt, im_info, step=4))).clone())
    torch.cuda.synchronize()
    assert not torch.allclose(want[0], want[1], rtol=1e-3)
    m = cls("cuda", **kw)
    m.capture(image, gt_a, im_info, lr=0.0, image_offset=0, warmup=1)
    for gt, w in zip((gt_a, gt_b, gt_a), want + want[:1]):
        got = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
        torch.cuda.synchronize()
        assert torch.allclose(got, w, rtol=1e-4, atol=1e-5), (got, w)


@pytest.mark.parametrize("which", ["frcnn", "retina"])
def test_detect_does_not_depend_on_reg_loss(hip, which):
    import torch
    image, _, im_info = _inputs(N, H, W, seed=5)
    outs = []
    for reg_loss in ("smooth_l1", "giou"):
        m = _model(which, reg_loss)
        dets, num = m.predict(image, im_info, score_thresh=0.0)
        torch.cuda.synchronize()
        outs.append((dets.clone(), num.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(_model(which, "smooth_l1").arena.w, _model(which, "giou").arena.w)


@pytest.mark.parametrize("which", ["frcnn", "retina"])
def test_default_models_call_the_smooth_l1_entries(hip, which, monkeypatch):
    import torch
    from mxdetection_amd.core import loss as L
    calls = []
    for name in ("rcnn_loss", "rcnn_loss_iou", "retina_loss_level", "retina_loss_level_iou"):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _fn=fn, _name=name, **k: calls.append(_name) or _fn(*a, **k))
    image, gt, im_info = _inputs(N, H, W, seed=1)
    old, new = ("rcnn_loss", "rcnn_loss_iou") if which == "frcnn" else ("retina_loss_level", "retina_loss_level_iou")
    m = _model(which, "smooth_l1")
    assert (m.bbox_head if which == "frcnn" else m.head).reg_loss == "smooth_l1"
    m.forward_backward(image, gt, im_info, step=1)
    torch.cuda.synchronize()
    assert calls.count(old) == (1 if which == "frcnn" else 5) and new not in calls
    calls.clear()
    _model(which, "giou").forward_backward(image, gt, im_info, step=1)
    torch.cuda.synchronize()
    assert calls.count(new) == (1 if which == "frcnn" else 5) and old not in calls
