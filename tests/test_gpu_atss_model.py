"""RetinaNet with ATSS targets at a small shape (128 x 192, ResNet-50): a training step of the published setting (one square
anchor per cell, GIoU) and of the 9-anchor head with smooth-L1, whose positive count is the reference's
(tests/_atss_ref.py on the head's own anchors); a captured step replayed with new ground truth; inference and a checkpoint
round trip of the one-anchor model."""
import functools

import numpy as np
import pytest

import _atss_ref as R
from test_gpu_gn_heads import _inputs

pytestmark = pytest.mark.gpu

N, H, W = 2, 128, 192
ONE = dict(assigner="atss", anchor_ratios=(1.0,), anchor_scales_per_octave=1, anchor_scale=8.0, reg_loss="giou", reg_loss_weight=2.0)
NINE = dict(assigner="atss")
CELLS = 16 * 24 + 8 * 12 + 4 * 6 + 2 * 3 + 1 * 2


@functools.lru_cache(maxsize=None)
def _model(which, seed=7):
    from mxdetection_amd.models import RetinaNet
    return RetinaNet("cuda", depth=50, seed=seed, **(ONE if which == "one" else NINE))


@pytest.mark.parametrize("which", ["one", "nine"])
def test_atss_training_step(hip, oracle, which):
    import torch
    m = _model(which)
    image, gt, im_info = _inputs(N, H, W, seed=1)
    (loss,) = m.forward_backward(image, gt, im_info, step=0)
    torch.cuda.synchronize()
    h = m.head
    A = 1 if which == "one" else 9
    assert h.assigner == "atss" and h.A == A and h.anchors.shape[0] == A * CELLS and h.level_offsets[-1] == A * CELLS
    assert (h.ld_cls, h.ld_reg) == ((128, 64) if which == "one" else (768, 64))
    assert h.reg_loss == ("giou" if which == "one" else "smooth_l1")
    labels, matched, _, _, _ = R.atss_assign(oracle, h.anchors.cpu().numpy(), h.level_offsets, gt.cpu().numpy(), 9)
    assert int(h.num_fg.item()) == int(labels.sum()) >= 8
    assert np.array_equal(h.matched.cpu().numpy(), matched)
    cls_labels = h.cls_labels.cpu().numpy()
    assert cls_labels.min() == 0 and np.array_equal(cls_labels > 0, labels == 1)       # no ignore band
    got = loss.cpu().numpy()
    assert np.all(np.isfinite(got)) and got[0] > 0 and got[1] > 0
    assert torch.isfinite(m.arena.g).all()
    grads = m.export_grads()
    c5 = m.backbone.stages[3][0].layers()[-1].name + ".weight"
    for name in ("retina.cls_out.weight", "retina.box_out.weight", "retina.cls0.weight", "retina.box0.weight", c5):
        assert grads[name].abs().sum().item() > 0, name


def test_atss_replayed_step_equals_the_eager_step(hip):
    """Two replays with different ground truth give the eager losses of each: the assignment runs inside the graph."""
    import torch
    from mxdetection_amd.models import RetinaNet
    image, gt_a, im_info = _inputs(N, H, W, seed=2)
    _, gt_b, _ = _inputs(N, H, W, seed=3)
    eager = _model("one")
    want = []
    for gt in (gt_a, gt_b):
        want.append(torch.cat(list(eager.forward_backward(image, gt, im_info, step=4))).clone())
    torch.cuda.synchronize()
    assert not torch.allclose(want[0], want[1], rtol=1e-3)
    m = RetinaNet("cuda", depth=50, seed=7, **ONE)
    m.capture(image, gt_a, im_info, lr=0.0, image_offset=0, warmup=1)
    for gt, w in zip((gt_a, gt_b, gt_a), want + want[:1]):
        got = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
        torch.cuda.synchronize()
        assert torch.allclose(got, w, rtol=1e-4, atol=1e-5), (got, w)


def test_atss_one_anchor_predict_and_checkpoint(hip, tmp_path):
    import torch
    from mxdetection_amd.models import RetinaNet
    from mxdetection_amd.utils import load_params
    image, gt, im_info = _inputs(N, H, W, seed=4)
    a = RetinaNet("cuda", depth=50, seed=5, **ONE)
    a.train_step(image, gt, im_info, step=0, lr=0.01)
    a.train_step(image, gt, im_info, step=1, lr=0.01)
    fn = str(tmp_path / "atss-0001.params")
    a.save_checkpoint(fn)
    blob = load_params(fn)
    assert blob["arg:retina.cls_out.weight"].shape == (80, 256, 3, 3) and blob["arg:retina.box_out.weight"].shape == (4, 256, 3, 3)
    b = RetinaNet("cuda", depth=50, seed=11, **ONE)
    assert b.load_checkpoint(fn) == []
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
    assert dets.shape == (N, 50, 6) and num.shape == (N,) and torch.isfinite(dets).all()
    for n in range(N):
        k = int(num[n])
        d = dets[n].cpu().numpy()
        assert 0 < k <= 50 and np.all(np.diff(d[:k, 4]) <= 0) and np.all((d[:k, 5] >= 1) & (d[:k, 5] <= 80))
        assert np.all(d[:k, 2] <= W - 1) and np.all(d[:k, 3] <= H - 1) and np.all(d[k:, 5] == -1)
