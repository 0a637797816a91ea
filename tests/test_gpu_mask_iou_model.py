"""Mask Scoring R-CNN assembled (FasterRCNN(with_mask=True, mask_iou=True)): the training step and its gradients, the
replayed step, the model without the head, predict's mask scores and checkpoints (small images, the shapes of
tests/test_gpu_mask.py::test_mask_rcnn_step)."""
import numpy as np
import pytest

from _mask_iou_ref import ellipse_masks
from conftest import synth_gt

pytestmark = pytest.mark.gpu

N, H, W = 2, 192, 256
KW = dict(seed=7, pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=128, with_mask=True)


def _inputs(seed=24):
    import torch
    rng = np.random.default_rng(seed)
    gt = synth_gt(rng, N, 8, H, W - 4, 2, 5)
    masks = torch.from_numpy(ellipse_masks(gt, H, W)).cuda()
    img = torch.randn((N, 3, H, W), generator=torch.Generator().manual_seed(5)).cuda()
    info = torch.tensor([[H, W - 4, 1.0]] * N).cuda()
    return img, torch.from_numpy(gt).cuda(), info, masks


def test_mask_scoring_rcnn_training(hip):
    """Eight steps on a fixed batch. The learning rate is 2e-5, not the 2e-3 of test_mask_rcnn_step: the MaskIoU loss is an
    L2 regression, which (unlike the saturating CE / BCE heads) has a hard step-size limit. One SGD step moves a positive
    row's prediction by about lr / n_pos * (p - t) * sum over layers |dp/dW|^2, and fc_out alone contributes |h2|^2: 1,024
    entries of rms about 6 on this randomly initialised backbone = 3.7e4, with n_pos about 7: lr * 5e3 from the last layer,
    several times that through fc2 / fc1 / the convs, so lr * lambda ~ 1e4..3e4 * lr. Heavy-ball SGD with momentum 0.9
    contracts below lr * lambda = 2 * 1.9; at 2e-3 the product is 20..60 (the step diverges), at 2e-5 it is 0.2..0.6."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    img, gt, info, masks = _inputs()
    m = FasterRCNN("cuda", mask_iou=True, **KW)
    hist = []
    for it in range(8):
        losses = m.train_step(img, gt, info, step=0, lr=2e-5, gt_masks=masks)
        assert len(losses) == 4 and losses[3].shape == (1,)
        hist.append([float(v) for v in torch.cat(list(losses)).cpu()])
    hist = np.array(hist)                     # columns: rpn cls, rpn box, rcnn cls, rcnn box, mask, maskiou
    print("losses per step:\n", hist)
    assert hist.shape == (8, 6) and np.all(np.isfinite(hist))
    assert hist[0, 5] > 0 and hist[-1, 5] < hist[0, 5]          # the MaskIoU loss goes down on a fixed batch
    assert hist[-1, 4] < hist[0, 4] and hist[-1, 0] < hist[0, 0]   # ... and the mask / RPN losses still do
    c0 = m.mask_iou_head.convs[0]
    g = m.arena.view(c0.wi, "g")
    assert g.shape == (256, 3, 3, 320) and torch.isfinite(g).all() and g[..., :257].abs().sum() > 0
    assert g[..., 256].abs().sum() > 0                            # the mask channel's filter column learns
    assert not g[..., 257:].any() and not m.arena.view(c0.wi, "w")[..., 257:].any()    # the alignment channels stay zero
    t = m.mask_iou_head.t
    assert ((t >= 0) & (t <= 1)).all() and (t > 0).any()


def test_replayed_and_eager_steps_agree(hip):
    """Grouped weight gradients on a side stream, the RPN branch on its own stream and the replayed hipGraph step compute
    the same step as plain eager launches (tests/test_gpu_dpool_model.py checks the same for its option)."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    img, gt, info, masks = _inputs()
    ref = FasterRCNN("cuda", mask_iou=True, **KW)
    l_ref = torch.cat(ref.forward_backward(img, gt, info, step=4, image_offset=0, gt_masks=masks)).clone()
    g_ref = ref.arena.g.clone()
    assert l_ref.shape == (6,) and l_ref[5] > 0
    m = FasterRCNN("cuda", mask_iou=True, **KW)
    m.enable_wgrad_stream()
    m.enable_branch_stream()
    m.enable_grouped_wgrad()
    l_side = torch.cat(m.forward_backward(img, gt, info, step=4, image_offset=0, gt_masks=masks)).clone()
    m.ws.join()
    torch.cuda.synchronize()
    assert torch.equal(l_ref, l_side)
    denom = g_ref.abs().max().item()
    assert (g_ref - m.arena.g).abs().max().item() <= 1e-3 * denom
    m.capture(img, gt, info, lr=0.0, image_offset=0, warmup=1, gt_masks=masks)
    l_graph = torch.cat(m.replay(img, gt, info, 4, gt_masks=masks)).clone()
    torch.cuda.synchronize()
    assert torch.allclose(l_ref, l_graph, rtol=1e-4, atol=1e-5), (l_ref, l_graph)
    assert (g_ref - m.arena.g).abs().max().item() <= 1e-3 * denom
    for l in m.mask_iou_head.layers():
        a, r = m.arena.view(l.wi, "g"), ref.arena.view(l.wi, "g")
        assert r.abs().sum().item() > 0 and (a - r).abs().max().item() <= 1e-2 * r.abs().max().item(), l.name


def test_mask_iou_needs_the_mask_branch():
    from mxdetection_amd.models import FasterRCNN
    with pytest.raises(ValueError, match="mask_iou needs the mask branch"):
        FasterRCNN("cuda", mask_iou=True)
    with pytest.raises(ValueError, match="mask_iou_weight"):
        FasterRCNN("cuda", with_mask=True, mask_iou=True, mask_iou_weight=0.0)


def test_predict_mask_scores_and_the_model_without_the_head(hip):
    """The plain model has no head, three predict values and the same parameters; with the head the boxes and masks are
    the plain model's, and the scores are det score x predicted IoU of the detection's class, bit for bit."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    img, _, info, _ = _inputs()
    plain = FasterRCNN("cuda", **KW)
    m = FasterRCNN("cuda", mask_iou=True, **KW)
    assert plain.mask_iou_head is None and m.mask_iou_head is not None
    mine = {n: t for n, _, t, _ in m._named_tensors()}
    for name, _, t, _ in plain._named_tensors():
        assert torch.equal(mine[name], t), name
    assert sorted(set(mine) - {n for n, _, _, _ in plain._named_tensors()}) == sorted(
        "maskiou.%s.%s" % (l, p) for l in ("conv0", "conv1", "conv2", "conv3", "fc1", "fc2", "fc_out") for p in ("weight", "bias"))
    assert [l.name for l in m.layers[:7]] == ["maskiou.fc_out", "maskiou.fc2", "maskiou.fc1", "maskiou.conv3", "maskiou.conv2",
                                              "maskiou.conv1", "maskiou.conv0"]
    M = 20
    out_p = plain.predict(img, info, score_thresh=0.0, max_per_image=M, with_masks=True)
    out_m = m.predict(img, info, score_thresh=0.0, max_per_image=M, with_masks=True)
    torch.cuda.synchronize()
    assert len(out_p) == 3 and len(out_m) == 4
    for a, b in zip(out_p, out_m[:3]):
        assert torch.equal(a, b)
    dets, num, _, scores = out_m
    assert scores.shape == (N, M) and scores.dtype == torch.float32 and int(num.min()) > 0
    d = dets.view(N * M, 6).cpu().numpy()
    pred = m.mask_iou_head.o.view(N * M, -1).float().cpu().numpy()
    want = np.zeros((N * M,), np.float32)
    for r in range(N * M):
        c = int(d[r, 5])
        if c > 0:
            want[r] = np.float32(d[r, 4]) * np.float32(pred[r, c - 1])
    got = scores.view(-1).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isfinite(got).all() and not got[d[:, 5] <= 0].any()
    # a threshold no untrained score reaches: (nearly) every row is padding (class -1, zero box) and scores 0
    dets, num, _, scores = m.predict(img, info, score_thresh=0.9999, max_per_image=M, with_masks=True)
    pad = (dets[..., 5] <= 0).cpu().numpy()
    assert pad.any() and not scores.cpu().numpy()[pad].any() and torch.isfinite(scores).all()
    assert len(m.predict(img, info)) == 2          # without masks: boxes only, as before


def test_checkpoints(hip, tmp_path):
    """The new layers save and load like the others (conv0 with all 320 input channels, FCs 2-D); a plain Mask R-CNN
    checkpoint loaded with strict=False reports exactly the maskiou.* names as missing."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    from mxdetection_amd.utils import load_params
    img, gt, info, masks = _inputs()
    a = FasterRCNN("cuda", mask_iou=True, **KW)
    a.train_step(img, gt, info, step=0, lr=2e-5, gt_masks=masks)         # non-trivial weights and momentum
    a.train_step(img, gt, info, step=1, lr=2e-5, gt_masks=masks)
    fn = str(tmp_path / "msrcnn-0001.params")
    a.save_checkpoint(fn)
    blob = load_params(fn)
    assert blob["arg:maskiou.conv0.weight"].shape == (256, 320, 3, 3) and blob["arg:maskiou.conv3.weight"].shape == (256, 256, 3, 3)
    assert blob["arg:maskiou.fc1.weight"].shape == (1024, 12544) and blob["arg:maskiou.fc2.weight"].shape == (1024, 1024)
    assert blob["arg:maskiou.fc_out.weight"].shape == (80, 1024) and blob["arg:maskiou.fc_out.bias"].shape == (80,)
    assert blob["aux:momentum:maskiou.fc_out.weight"].shape == (80, 1024)
    assert not blob["arg:maskiou.conv0.weight"][:, 257:].any() and blob["arg:maskiou.conv0.weight"][:, 256].any()
    kw = dict(KW, seed=11)
    b = FasterRCNN("cuda", mask_iou=True, **kw)
    assert b.load_checkpoint(fn) == []
    assert torch.equal(a.arena.w, b.arena.w) and torch.equal(a.arena.m, b.arena.m) and torch.equal(a.arena.wb, b.arena.wb)
    for l in a.mask_iou_head.layers():
        assert torch.equal(a.arena.view(l.wi, "w"), b.arena.view(l.wi, "w")) and a.arena.view(l.wi, "w").any(), l.name
    plain = FasterRCNN("cuda", **kw)
    fn2 = str(tmp_path / "mask-0001.params")
    plain.save_checkpoint(fn2)
    with pytest.raises(KeyError):
        b.load_checkpoint(fn2)
    c = FasterRCNN("cuda", mask_iou=True, **KW)
    before = {l.name: c.arena.view(l.wi, "w").clone() for l in c.mask_iou_head.layers()}
    missing = c.load_checkpoint(fn2, strict=False)
    assert sorted(missing) == sorted("maskiou.%s.%s" % (l, p) for l in ("conv0", "conv1", "conv2", "conv3", "fc1", "fc2", "fc_out")
                                     for p in ("weight", "bias"))
    assert torch.equal(c.arena.view(c.mask_head.convs[0].wi, "w"), plain.arena.view(plain.mask_head.convs[0].wi, "w"))
    for l in c.mask_iou_head.layers():            # the fine-tuning route: the head keeps its initialisation
        assert torch.equal(c.arena.view(l.wi, "w"), before[l.name])
