"""RetinaNet with a quality-aware class loss (QFL / Varifocal) at a small shape (128 x 192, ResNet-50), on the
one-anchor ATSS model of tests/test_gpu_atss_model.py: a training step whose class loss is the float64 reference
(tests/_quality_loss_ref.py) evaluated on the head's own outputs, a captured step replayed with new ground truth, inference
and a checkpoint round trip into a focal model, and cls_loss="focal" being today's model bit for bit."""
import functools

import numpy as np
import pytest

import _quality_loss_ref as Q
import test_quality_loss_cases_cpu as QT
from test_gpu_atss_model import CELLS, H, N, ONE, W
from test_gpu_gn_heads import _inputs

pytestmark = pytest.mark.gpu

PUBLISHED = {"qfl": (0.0, 2.0), "vfl": (0.75, 2.0)}


@functools.lru_cache(maxsize=None)
def _model(cls_loss, seed=7):
    from mxdetection_amd.models import RetinaNet
    return RetinaNet("cuda", depth=50, seed=seed, **ONE, **({} if cls_loss is None else {"cls_loss": cls_loss}))


@pytest.mark.parametrize("cls_loss", ["qfl", "vfl"])
def test_quality_training_step(hip, cls_loss):
    import torch
    m = _model(cls_loss)
    image, gt, im_info = _inputs(N, H, W, seed=1)
    (loss,) = m.forward_backward(image, gt, im_info, step=0)
    torch.cuda.synchronize()
    h = m.head
    assert (h.cls_loss, h.cls_alpha, h.cls_gamma) == (cls_loss,) + PUBLISHED[cls_loss]
    assert h.A == 1 and h.anchors.shape[0] == CELLS and (h.ld_cls, h.ld_reg) == (128, 64) and h.reg_loss == "giou"
    nfg = int(h.num_fg.item())
    assert nfg >= 8
    # the reference on the head's own outputs, level by level
    anchors, matched, gtn = h.anchors.cpu().numpy(), h.matched.cpu().numpy(), gt.cpu().numpy()
    cls_labels = h.cls_labels.cpu().numpy()
    want, n_valid, qs = 0.0, 0, []
    for l, (co, bo) in enumerate(zip(h.co, h.bo)):
        r = Q.ref_retina_quality(co.float().cpu().numpy(), bo.float().cpu().numpy(), h.A, h.Cn, cls_labels, anchors, matched, gtn,
                                 h.level_offsets[l], cls_loss, h.cls_alpha, h.cls_gamma, (1.0, 1.0, 1.0, 1.0), nfg, 1.0)
        want += r["loss"]
        n_valid += r["n_valid"]
        qs.append(r["q"].reshape(-1))
    qs = np.concatenate(qs)
    assert np.count_nonzero(qs > 0) >= 8 and qs.max() <= 1.0
    got = loss.cpu().numpy()
    print("%s class loss: got %.9g ref %.9g over %d anchors, %d foreground" % (cls_loss, got[0], want, n_valid, nfg))
    assert abs(got[0] - want) <= QT.LOSS_RTOL * abs(want) + n_valid * QT.ATOL_CLS_LOSS / nfg
    assert np.all(np.isfinite(got)) and got[0] > 0 and got[1] > 0
    assert torch.isfinite(m.arena.g).all()
    grads = m.export_grads()
    for name in ("retina.cls_out.weight", "retina.box_out.weight", "retina.cls0.weight", "retina.box0.weight"):
        assert grads[name].abs().sum().item() > 0, name


def test_quality_step_differs_from_focal_only_in_the_class_half(hip):
    """Same seed, same inputs: the box loss is the focal model's bit for bit (the box half does not see the class loss)."""
    import torch
    image, gt, im_info = _inputs(N, H, W, seed=1)
    out = {}
    for k in (None, "qfl", "vfl"):
        out[k] = _model(k).forward_backward(image, gt, im_info, step=0)[0].clone()
    torch.cuda.synchronize()
    for k in ("qfl", "vfl"):
        assert torch.equal(out[k][1], out[None][1]) and not torch.equal(out[k][0], out[None][0])
    assert not torch.equal(out["qfl"][0], out["vfl"][0])


def test_focal_argument_is_todays_model(hip):
    import torch
    from mxdetection_amd.models import RetinaNet
    image, gt, im_info = _inputs(N, H, W, seed=1)
    a = _model(None)
    b = RetinaNet("cuda", depth=50, seed=7, **ONE, cls_loss="focal", cls_loss_alpha=None, cls_loss_gamma=None)
    assert (b.head.cls_loss, b.head.alpha, b.head.gamma) == ("focal", a.head.alpha, a.head.gamma) == ("focal", 0.25, 2.0)
    la = a.forward_backward(image, gt, im_info, step=0)[0].clone()
    lb = b.forward_backward(image, gt, im_info, step=0)[0].clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(a.arena.g, b.arena.g)
    ga, gb = a.export_grads(), b.export_grads()
    assert list(ga) == list(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)


def test_quality_replayed_step_equals_the_eager_step(hip):
    """Two replays with different ground truth give the eager losses of each: assignment, quality and loss run inside the
    graph on what gt_boxes holds at replay."""
    import torch
    from mxdetection_amd.models import RetinaNet
    image, gt_a, im_info = _inputs(N, H, W, seed=2)
    _, gt_b, _ = _inputs(N, H, W, seed=3)
    eager = _model("qfl")
    want = []
    for gt in (gt_a, gt_b):
        want.append(torch.cat(list(eager.forward_backward(image, gt, im_info, step=4))).clone())
    torch.cuda.synchronize()
    assert not torch.allclose(want[0], want[1], rtol=1e-3)
    m = RetinaNet("cuda", depth=50, seed=7, **ONE, cls_loss="qfl")
    m.capture(image, gt_a, im_info, lr=0.0, image_offset=0, warmup=1)
    for gt, w in zip((gt_a, gt_b, gt_a), want + want[:1]):
        got = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
        torch.cuda.synchronize()
        assert torch.allclose(got, w, rtol=1e-4, atol=1e-5), (got, w)


def test_quality_predict_and_checkpoint_into_a_focal_model(hip, tmp_path):
    """The parameter layout does not depend on the class loss: a qfl checkpoint loads into a focal model, and inference
    (score = sigmoid(cls), untouched) gives the same detections from both."""
    import torch
    from mxdetection_amd.models import RetinaNet
    image, gt, im_info = _inputs(N, H, W, seed=4)
    a = RetinaNet("cuda", depth=50, seed=5, **ONE, cls_loss="vfl")
    a.train_step(image, gt, im_info, step=0, lr=0.01)
    a.train_step(image, gt, im_info, step=1, lr=0.01)
    fn = str(tmp_path / "vfl-0001.params")
    a.save_checkpoint(fn)
    b = RetinaNet("cuda", depth=50, seed=11, **ONE)
    assert b.head.cls_loss == "focal" and b.load_checkpoint(fn) == []
    for (na, _, ta, _), (nb, _, tb, _) in zip(a._named_tensors(), b._named_tensors()):
        assert na == nb and torch.equal(ta, tb), na
    assert torch.equal(a.arena.w, b.arena.w) and torch.equal(a.arena.m, b.arena.m)
    outs = []
    for m in (a, b):
        dets, num = m.predict(image, im_info, score_thresh=0.0, max_per_image=50)
        torch.cuda.synchronize()
        outs.append((dets.clone(), num.clone()))
    dets, num = outs[0]
    assert torch.equal(dets, outs[1][0]) and torch.equal(num, outs[1][1])
    assert dets.shape == (N, 50, 6) and torch.isfinite(dets).all()
    for n in range(N):
        k = int(num[n])
        d = dets[n].cpu().numpy()
        assert 0 < k <= 50 and np.all(np.diff(d[:k, 4]) <= 0) and np.all((d[:k, 5] >= 1) & (d[:k, 5] <= 80))
