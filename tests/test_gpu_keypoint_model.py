"""Keypoint R-CNN assembled (FasterRCNN(with_keypoints=True)): the training step beside the model without the head, the
replayed step, training on a fixed batch, predict's keypoints, checkpoints, and the head next to the mask branch (small
images, the shapes of tests/test_gpu_mask_iou_model.py)."""
import numpy as np
import pytest

from _mask_iou_ref import ellipse_masks
from conftest import synth_gt

pytestmark = pytest.mark.gpu

N, H, W, K = 2, 192, 256, 17
KW = dict(seed=7, pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=128)
NAMES = sorted("kpt.%s.%s" % (l, p) for l in ["deconv"] + ["conv%d" % i for i in range(8)] for p in ("weight", "bias"))


def _inputs(seed=24):
    """image, gt_boxes, im_info, gt_masks, gt_keypoints: 17 labelled points inside every box (one in five unlabelled)."""
    import torch
    rng = np.random.default_rng(seed)
    gt = synth_gt(rng, N, 8, H, W - 4, 2, 5)
    masks = torch.from_numpy(ellipse_masks(gt, H, W)).cuda()
    krng = np.random.default_rng(seed + 1)
    u = krng.uniform(0.05, 0.95, (N, 8, K, 2)).astype(np.float32)
    kp = np.zeros((N, 8, K, 3), np.float32)
    kp[..., 0] = gt[:, :, None, 0] + u[..., 0] * (gt[:, :, None, 2] - gt[:, :, None, 0])
    kp[..., 1] = gt[:, :, None, 1] + u[..., 1] * (gt[:, :, None, 3] - gt[:, :, None, 1])
    kp[..., 2] = krng.integers(1, 3, (N, 8, K))
    kp[krng.uniform(size=(N, 8, K)) < 0.2] = 0
    kp[gt[..., 4] < 0] = 0                                   # padding instances are all zero
    img = torch.randn((N, 3, H, W), generator=torch.Generator().manual_seed(5)).cuda()
    info = torch.tensor([[H, W - 4, 1.0]] * N).cuda()
    return img, torch.from_numpy(gt).cuda(), info, masks, torch.from_numpy(kp).cuda()


def test_step_beside_the_plain_model_replay_and_training(hip):
    """Step 0 of the model with the head computes the plain model's RPN / R-CNN losses bit for bit (the head has a weight
    generator of its own and reads the box head's rois only); the keypoint loss is the last one and starts near
    log(56*56) = 8.05 (a uniform softmax); the captured + replayed step gives the eager step's losses bit for bit; on one
    repeated batch the keypoint loss falls. The learning rate is 1e-4, not the 2e-3 of test_mask_rcnn_step: on this randomly
    initialised backbone the R-CNN class loss starts at 5.2 (above log 81 = 4.4: logits of several units) and at 2e-3 the box
    head overshoots from the first step (measured: 5.2, 3.5, 7.4, 10.4, ...), which shakes the FPN features all heads share;
    the keypoint head's deconvolution starts at std 0.001, so its own step is small at any of these rates."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    img, gt, info, _, kp = _inputs()
    plain = FasterRCNN("cuda", **KW)
    l_plain = torch.cat(plain.forward_backward(img, gt, info, step=4, image_offset=0)).clone()
    m = FasterRCNN("cuda", with_keypoints=True, **KW)
    assert [l.name for l in m.layers[:9]] == ["kpt.deconv"] + ["kpt.conv%d" % i for i in reversed(range(8))]
    with pytest.raises(ValueError, match="gt_keypoints"):
        m.forward_backward(img, gt, info, step=4, image_offset=0)
    m.enable_wgrad_stream()
    m.enable_branch_stream()
    m.enable_grouped_wgrad()
    l_eager = torch.cat(m.forward_backward(img, gt, info, step=4, image_offset=0, gt_keypoints=kp)).clone()
    m.ws.join()
    torch.cuda.synchronize()
    print("plain", l_plain.tolist(), "with keypoints", l_eager.tolist())
    assert l_plain.shape == (4,) and l_eager.shape == (5,) and torch.equal(l_eager[:4], l_plain)
    assert 6.0 < float(l_eager[4]) < 10.0
    tg = m.keypoint_head.tg
    assert tg.shape == (N * 32, K) and int((tg >= 0).sum()) > K and int(tg.max()) < 56 * 56
    for l in m.keypoint_head.layers():
        g = m.arena.view(l.wi, "g")
        assert torch.isfinite(g).all() and g.abs().sum() > 0, l.name
    gd = m.arena.view(m.keypoint_head.deconv.wi, "g").view(4, m.keypoint_head.kpad, -1)
    assert not gd[:, K:].any() and not m.arena.view(m.keypoint_head.deconv.wi, "w").view(4, 32, -1)[:, K:].any()
    m.capture(img, gt, info, lr=0.0, image_offset=0, warmup=1, gt_keypoints=kp)
    l_graph = torch.cat(m.replay(img, gt, info, 4, gt_keypoints=kp)).clone()
    torch.cuda.synchronize()
    print("replayed", l_graph.tolist())
    assert torch.equal(l_graph, l_eager), (l_eager, l_graph)
    hist = [l_graph.cpu().numpy()]
    for it in range(5):
        hist.append(torch.cat(m.replay(img, gt, info, 4, gt_keypoints=kp, lr=1e-4)).clone().cpu().numpy())
    hist = np.array(hist)
    print("losses per step:\n", hist)
    assert np.isfinite(hist).all() and hist[-1, 4] < hist[0, 4]


def test_predict_keypoints(hip):
    """Keypoints lie inside their boxes (bin centres of the box's 56x56 grid), padding rows are zero, and the boxes are
    the plain call's."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    img, _, info, _, _ = _inputs()
    m = FasterRCNN("cuda", with_keypoints=True, **KW)
    M = 20
    dets0, num0 = m.predict(img, info, score_thresh=0.0, max_per_image=M)
    dets0, num0 = dets0.clone(), num0.clone()
    out = m.predict(img, info, score_thresh=0.0, max_per_image=M, with_keypoints=True)
    assert len(out) == 3 and torch.equal(out[0], dets0) and torch.equal(out[1], num0)
    kp = out[2]
    assert kp.shape == (N, M, K, 3) and kp.dtype == torch.float32 and torch.isfinite(kp).all() and int(num0.min()) > 0
    d, k = out[0].cpu().numpy(), kp.cpu().numpy()
    real = d[..., 5] > 0
    assert real.any()
    x1, y1 = d[..., None, 0], d[..., None, 1]
    x2, y2 = np.maximum(d[..., None, 2], x1 + 1), np.maximum(d[..., None, 3], y1 + 1)
    inside = (k[..., 0] > x1) & (k[..., 0] < x2) & (k[..., 1] > y1) & (k[..., 1] < y2)
    assert inside[real].all()
    # the decode kernel against the logits the head left behind
    import _keypoint_ref as ref
    lg = m.keypoint_head.o.float().cpu().numpy()
    want = ref.keypoint_decode(lg, d.reshape(N * M, 6), K)
    assert np.array_equal(k.reshape(N * M, K, 3).view(np.uint32), want.view(np.uint32))
    # a threshold no untrained score reaches: (nearly) every row is padding (class -1, zero box) and decodes to zeros
    dets, num, kp = m.predict(img, info, score_thresh=0.9999, max_per_image=M, with_keypoints=True)
    pad = (dets[..., 5] <= 0).cpu().numpy()
    assert pad.any() and not kp.cpu().numpy()[pad].any()
    with pytest.raises(AssertionError, match="keypoint head"):
        FasterRCNN("cuda", **KW).predict(img, info, with_keypoints=True)


def test_checkpoints(hip, tmp_path):
    """The head's layers save and load like the others; a plain checkpoint loaded with strict=False reports exactly the
    kpt.* names as missing and leaves the head at its initialisation."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    from mxdetection_amd.utils import load_params
    img, gt, info, _, kp = _inputs()
    a = FasterRCNN("cuda", with_keypoints=True, **KW)
    a.train_step(img, gt, info, step=0, lr=1e-4, gt_keypoints=kp)         # non-trivial weights and momentum
    a.train_step(img, gt, info, step=1, lr=1e-4, gt_keypoints=kp)
    fn = str(tmp_path / "kprcnn-0001.params")
    a.save_checkpoint(fn)
    blob = load_params(fn)
    assert blob["arg:kpt.conv0.weight"].shape == (512, 256, 3, 3) and blob["arg:kpt.conv7.weight"].shape == (512, 512, 3, 3)
    assert blob["arg:kpt.deconv.weight"].shape == (128, 512, 1, 1) and blob["arg:kpt.deconv.bias"].shape == (128,)
    assert blob["aux:momentum:kpt.deconv.weight"].shape == (128, 512, 1, 1)
    kw = dict(KW, seed=11)
    b = FasterRCNN("cuda", with_keypoints=True, **kw)
    assert b.load_checkpoint(fn) == []
    assert torch.equal(a.arena.w, b.arena.w) and torch.equal(a.arena.m, b.arena.m) and torch.equal(a.arena.wb, b.arena.wb)
    for l in a.keypoint_head.layers():
        assert torch.equal(a.arena.view(l.wi, "w"), b.arena.view(l.wi, "w")) and a.arena.view(l.wi, "w").any(), l.name
    plain = FasterRCNN("cuda", **kw)
    fn2 = str(tmp_path / "plain-0001.params")
    plain.save_checkpoint(fn2)
    with pytest.raises(KeyError):
        b.load_checkpoint(fn2)
    c = FasterRCNN("cuda", with_keypoints=True, **KW)
    before = {l.name: c.arena.view(l.wi, "w").clone() for l in c.keypoint_head.layers()}
    missing = c.load_checkpoint(fn2, strict=False)
    assert sorted(missing) == NAMES
    assert torch.equal(c.arena.view(c.bbox_head.layers()[0].wi, "w"), plain.arena.view(plain.bbox_head.layers()[0].wi, "w"))
    for l in c.keypoint_head.layers():            # the fine-tuning route: the head keeps its initialisation
        assert torch.equal(c.arena.view(l.wi, "w"), before[l.name])


def test_mask_and_keypoints_together(hip):
    """Mask R-CNN with the keypoint head: the first five losses are Mask R-CNN's bit for bit, the keypoint loss is the
    last, every other parameter starts as in the model without the head, and predict returns masks and keypoints."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    img, gt, info, masks, kp = _inputs()
    mask_only = FasterRCNN("cuda", with_mask=True, **KW)
    m = FasterRCNN("cuda", with_mask=True, with_keypoints=True, **KW)
    mine = {n: t for n, _, t, _ in m._named_tensors()}
    for name, _, t, _ in mask_only._named_tensors():
        assert torch.equal(mine[name], t), name
    assert sorted(set(mine) - {n for n, _, _, _ in mask_only._named_tensors()}) == NAMES
    l_mask = torch.cat(mask_only.train_step(img, gt, info, step=0, lr=1e-4, gt_masks=masks)).clone()
    l_both = torch.cat(m.train_step(img, gt, info, step=0, lr=1e-4, gt_masks=masks, gt_keypoints=kp)).clone()
    print("mask", l_mask.tolist(), "mask + keypoints", l_both.tolist())
    assert l_mask.shape == (5,) and l_both.shape == (6,) and torch.equal(l_both[:5], l_mask)
    assert 6.0 < float(l_both[5]) < 10.0
    l2 = torch.cat(m.train_step(img, gt, info, step=0, lr=1e-4, gt_masks=masks, gt_keypoints=kp))
    assert torch.isfinite(l2).all()
    out = m.predict(img, info, score_thresh=0.0, max_per_image=10, with_masks=True, with_keypoints=True)
    assert len(out) == 4 and out[2].shape == (N, 10, H, W) and out[3].shape == (N, 10, K, 3)
    assert len(m.predict(img, info, score_thresh=0.0, max_per_image=10, with_masks=True)) == 3
