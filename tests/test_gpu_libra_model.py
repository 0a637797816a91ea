"""Libra R-CNN in the assembled Faster R-CNN, at the small shapes of tests/test_gpu_ohem_model.py: a Balanced Feature Pyramid
whose refine convolution is zero is the plain FPN bit for bit (Q = P, dB = 0); with refine 'none' and 'conv' the step runs and
its captured replay reproduces the eager step's bits; the IoU-balanced sampler with one bin is the plain model; the model of
configs/libra_faster_rcnn_r50_fpn.yaml trains, round-trips a checkpoint, loads a plain one, predicts, and steps with the mask
branch."""
import functools
import os

import numpy as np
import pytest

from test_gpu_gn_heads import _inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 256, 320
KW = dict(seed=7, pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=64)
REFINE = ("bfp.refine.weight", "bfp.refine.bias")


@functools.lru_cache(maxsize=None)
def _plain_step():
    """One eager step of the default model (step 2, inputs of seed 1): losses, gradients by name, the gradient arena."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    m = FasterRCNN("cuda", **KW)
    image, gt, im_info = _inputs(N, H, W, seed=1)
    losses = torch.cat(list(m.forward_backward(image, gt, im_info, step=2))).clone()
    torch.cuda.synchronize()
    return losses, m.export_grads(), m.arena.g.clone(), m.arena.w.clone(), m.export_params()


def _libra_model():
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils.config import load_config
    cfg = load_config(os.path.join(ROOT, "configs", "libra_faster_rcnn_r50_fpn.yaml"),
                      ["TRAIN.batch_rois=64", "TRAIN.rpn_pre_nms_top_n=600", "TRAIN.rpn_post_nms_top_n=300"])
    return build_detector(cfg, "cuda")


def test_bfp_with_a_zero_refine_convolution_is_the_fpn(hip):
    import torch
    from mxdetection_amd.models import FasterRCNN
    l_plain, g_plain, _, _, p_plain = _plain_step()
    m = FasterRCNN("cuda", **KW, neck="bfp")
    names = [l.name for l in m.layers]
    assert names.index("bfp.refine") + 1 == names.index("fpn.out2")     # first among the neck's layers
    c = m.bfp.refine
    off = m.arena.offset_of(c.wi)
    assert m.mark_rpn <= off < m.mark_fpn                             # inside the FPN bucket, first
    # every other parameter starts as in the plain model: the refine convolution draws from a generator of its own
    mine = m.export_params()
    assert float(mine["bfp.refine.weight"].abs().sum()) > 0 and set(mine) - set(p_plain) == set(REFINE)
    for name, v in p_plain.items():
        assert torch.equal(mine[name], v), name
    m.arena.view(c.wi, "w").zero_()
    m.arena.view(c.bi, "w").zero_()
    m.arena.refresh_bf16()
    m.refresh_transposed()
    image, gt, im_info = _inputs(N, H, W, seed=1)
    losses = torch.cat(list(m.forward_backward(image, gt, im_info, step=2))).clone()
    torch.cuda.synchronize()
    assert torch.equal(losses, l_plain), (losses, l_plain)
    grads = m.export_grads()
    assert set(grads) - set(g_plain) == set(REFINE)
    for name, g in g_plain.items():
        assert torch.equal(grads[name], g), name
    assert float(grads["bfp.refine.weight"].abs().sum()) > 0 and float(grads["bfp.refine.bias"].abs().sum()) > 0
    for a, b in zip(m.bfp.Q, m.neck.P):
        assert torch.equal(a, b)


@pytest.mark.parametrize("refine", ["none", "conv"])
def test_bfp_step_and_its_captured_replay(hip, refine):
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, gt, im_info = _inputs(N, H, W, seed=1)
    m = FasterRCNN("cuda", **KW, neck="bfp", bfp_refine=refine)
    assert (m.bfp.refine is None) == (refine == "none")
    m.enable_wgrad_stream()
    m.enable_branch_stream()
    m.enable_grouped_wgrad()
    l_eager = torch.cat(list(m.forward_backward(image, gt, im_info, step=4))).clone()
    m.ws.join()
    torch.cuda.synchronize()
    l_plain = _plain_step()[0]
    print("plain", l_plain.tolist(), "bfp", refine, l_eager.tolist())
    assert torch.isfinite(l_eager).all() and torch.isfinite(m.arena.g).all() and (l_eager > 0).all()
    assert not torch.equal(m.bfp.Q[0], m.neck.P[0])                    # the balanced map reached the finest level
    if refine == "conv":
        assert float(m.arena.view(m.bfp.refine.wi, "g").abs().sum()) > 0
    m.capture(image, gt, im_info, lr=0.0, image_offset=0, warmup=1)
    l_graph = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
    torch.cuda.synchronize()
    assert torch.equal(l_graph, l_eager), (l_eager, l_graph)
    again = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
    torch.cuda.synchronize()
    assert torch.equal(again, l_eager)


def test_iou_balanced_with_one_bin_is_the_plain_model(hip):
    import torch
    from mxdetection_amd.models import FasterRCNN
    l_plain, _, g_plain, w_plain, _ = _plain_step()
    m = FasterRCNN("cuda", **KW, sampler="iou_balanced", sampler_bins=1)
    assert torch.equal(m.arena.w, w_plain)
    image, gt, im_info = _inputs(N, H, W, seed=1)
    losses = torch.cat(list(m.forward_backward(image, gt, im_info, step=2))).clone()
    torch.cuda.synchronize()
    assert torch.equal(losses, l_plain) and torch.equal(m.arena.g, g_plain)
    # three bins draw other background RoIs
    m3 = FasterRCNN("cuda", **KW, sampler="iou_balanced", sampler_bins=3)
    l3 = torch.cat(list(m3.forward_backward(image, gt, im_info, step=2))).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(l3).all() and torch.equal(l3[:2], l_plain[:2]) and not torch.equal(m3.bbox_head.rois, m.bbox_head.rois)
    assert torch.equal(m3.bbox_head.num_fg, m.bbox_head.num_fg)


def test_default_model_never_calls_the_new_bindings(hip, monkeypatch):
    import torch
    from mxdetection_amd import _lib
    from mxdetection_amd.models import FasterRCNN
    lib = _lib.load()
    calls = []
    new = ("mxdet_proposal_target_balanced", "mxdet_rcnn_loss_balanced", "mxdet_bfp_gather_fwd", "mxdet_bfp_scatter_fwd",
           "mxdet_bfp_scatter_bwd", "mxdet_bfp_gather_bwd")
    for name in new:
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _name=name: calls.append(_name) or _fn(*a))
    image, gt, im_info = _inputs(N, H, W, seed=1)
    FasterRCNN("cuda", **KW).forward_backward(image, gt, im_info, step=1)
    torch.cuda.synchronize()
    assert calls == []
    _libra_model().forward_backward(image, gt, im_info, step=1)
    torch.cuda.synchronize()
    assert sorted(calls) == sorted(new)


def test_libra_config_model_trains_checkpoints_and_predicts(hip, tmp_path):
    """Six steps on a fixed batch at the learning rate 1e-4 of tests/test_gpu_keypoint_model.py (the randomly initialised
    backbone overshoots at 2e-3): the summed loss falls."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, gt, im_info = _inputs(N, H, W, seed=1)
    m = _libra_model()
    h = m.bbox_head
    assert (h.sampler, h.sampler_bins, h.reg_loss, h.bl1, h.reg_loss_weight) == ("iou_balanced", 3, "balanced_l1", (0.5, 1.5, 1.0), 1.0)
    assert m.bfp is not None and m.bfp.refine is not None
    hist = []
    for it in range(6):
        hist.append(torch.cat(list(m.train_step(image, gt, im_info, step=0, lr=1e-4))).cpu().numpy())
    hist = np.array(hist)
    print("losses per step:\n", hist)
    assert hist.shape == (6, 4) and np.isfinite(hist).all() and (hist[0] > 0).all()
    assert hist[-1].sum() < hist[0].sum()
    # checkpoint round trip
    path = str(tmp_path / "libra.params")
    m.save_checkpoint(path)
    m2 = _libra_model()
    assert not torch.equal(m2.arena.w, m.arena.w)
    assert m2.load_checkpoint(path) == []
    assert torch.equal(m2.arena.w, m.arena.w) and torch.equal(m2.arena.m, m.arena.m) and torch.equal(m2.arena.wb, m.arena.wb)
    # a plain checkpoint: strict refuses, strict=False leaves the refine convolution at its init
    plain = FasterRCNN("cuda", **KW)
    ppath = str(tmp_path / "plain.params")
    plain.save_checkpoint(ppath)
    m3 = _libra_model()
    init = {k: v.clone() for k, v in m3.export_params().items() if k in REFINE}
    with pytest.raises(KeyError):
        _libra_model().load_checkpoint(ppath)
    assert sorted(m3.load_checkpoint(ppath, strict=False)) == sorted(REFINE)
    got, want = m3.export_params(), plain.export_params()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    for k in REFINE:
        assert torch.equal(got[k], init[k])
    # predict
    dets, num = m.predict(image, im_info, score_thresh=0.0)
    torch.cuda.synchronize()
    assert dets.shape == (N, 100, 6) and int(num.min()) > 0 and torch.isfinite(dets).all()


def test_libra_with_the_mask_branch(hip):
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, gt, im_info, masks = _inputs(N, H, W, seed=1, masks=True)
    m = FasterRCNN("cuda", **dict(KW, rois_per_image=32), with_mask=True, neck="bfp", sampler="iou_balanced", reg_loss="balanced_l1")
    losses = m.forward_backward(image, gt, im_info, step=0, gt_masks=masks)
    torch.cuda.synchronize()
    assert len(losses) == 3 and torch.isfinite(torch.cat(list(losses))).all() and torch.isfinite(m.arena.g).all()
    assert m.export_grads()["bfp.refine.weight"].abs().sum().item() > 0
    labels, num_fg = m.bbox_head.labels.cpu().numpy(), m.bbox_head.num_fg.cpu().numpy()
    for n in range(N):        # foreground first: what FCNMaskHead.select_rois relies on
        assert (labels[n, :num_fg[n]] > 0).all() and (labels[n, num_fg[n]:] <= 0).all()
