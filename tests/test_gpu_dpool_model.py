"""Deformable RoI pooling in the Faster R-CNN box branch (network.roi_pool = dpool / mdpool): the assembled training
step, its offset head's initial state and gradients, grouped / replayed steps, checkpoints and predict (small images, as
tests/test_gpu_dcn_model.py)."""
import numpy as np
import pytest

from conftest import synth_gt

pytestmark = pytest.mark.gpu


def _inputs(N, H, W, seed=0):
    import torch
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(1234 + seed)
    image = torch.randn((N, 3, H, W), generator=g).cuda()
    gt = torch.from_numpy(synth_gt(rng, N, 16, H, W - 5)).cuda()
    im_info = torch.tensor([[H, W - 5, 1.0]] * N, dtype=torch.float32).cuda()
    return image, gt, im_info


def _head(m):
    e = m.roi_extractor
    return e.offset_fc, e.mask_fc


def test_mdpool_step_initial_state_and_gradients(hip):
    """Every parameter of the plain model is bit-identical in the mdpool model; the step is finite; at step 1 the zero
    last FCs get non-zero weight gradients and the hidden FCs zero ones (their gradient passes through a zero weight);
    after one SGD step every offset-head FC gets a non-zero gradient."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    N, H, W = 2, 256, 320
    image, gt, im_info = _inputs(N, H, W, seed=1)
    kw = dict(seed=7, pre_nms_top_n=1000, post_nms_top_n=1000)
    ref = FasterRCNN("cuda", **kw)
    m = FasterRCNN("cuda", roi_pool="mdpool", **kw)
    mine = {n: t for n, _, t, _ in m._named_tensors()}
    for name, _, t, _ in ref._named_tensors():
        assert torch.equal(mine[name], t), name
    offs, masks = _head(m)
    assert [l.name for l in offs] == ["bbox.offset_fc1", "bbox.offset_fc2", "bbox.offset_fc3"]
    assert [l.name for l in masks] == ["bbox.mask_fc1", "bbox.mask_fc2"]
    assert not m.arena.view(offs[-1].wi, "w").any() and not m.arena.view(masks[-1].wi, "w").any()
    losses = torch.cat(m.forward_backward(image, gt, im_info, step=2)).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all()
    g = lambda l: m.arena.view(l.wi, "g")    # noqa: E731
    for l in (offs[-1], masks[-1]):
        assert g(l)[:l.cout_real].abs().sum().item() > 0, l.name
        assert not g(l)[l.cout_real:].any(), l.name                   # padding rows stay zero
    for l in offs[:-1] + masks[:-1]:
        assert not g(l).any(), l.name
    m.train_step(image, gt, im_info, step=3, lr=0.02)
    m.forward_backward(image, gt, im_info, step=4)
    torch.cuda.synchronize()
    for l in offs + masks:
        assert g(l).abs().sum().item() > 0, l.name
    assert torch.isfinite(m.arena.g).all()


@pytest.mark.parametrize("roi_pool", ["dpool", "mdpool"])
def test_dpool_zero_offsets_match_roi_pooling_pass0(hip, roi_pool):
    """At the start, pass 1 equals pass 0 (v1) or half of it (v2): the box head sees exactly that."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    N, H, W = 1, 192, 256
    image, gt, im_info = _inputs(N, H, W, seed=3)
    m = FasterRCNN("cuda", seed=7, pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=128, roi_pool=roi_pool,
                   dpool_offset_fcs=1)
    assert len(m.roi_extractor.offset_fc) == 1 and m.roi_extractor.offset_fc[0].cin == 7 * 7 * 256
    m.forward_backward(image, gt, im_info, step=0)
    torch.cuda.synchronize()
    e = m.roi_extractor
    x1 = e.bufs[("x1", tuple(e.x0.shape), torch.bfloat16)]
    want = e.x0.float() * (0.5 if roi_pool == "mdpool" else 1.0)
    assert torch.equal(x1.float(), want)


def test_mdpool_grouped_replayed_and_eager_steps_agree(hip):
    """Grouped weight gradients on a side stream, the RPN branch on its own stream and the replayed hipGraph step
    compute the same step as plain eager launches (the offset head included)."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    N, H, W = 2, 256, 320
    image, gt, im_info = _inputs(N, H, W, seed=2)
    kw = dict(seed=7, pre_nms_top_n=1000, post_nms_top_n=1000, roi_pool="mdpool")
    ref = FasterRCNN("cuda", **kw)
    l_ref = torch.cat(ref.forward_backward(image, gt, im_info, step=4, image_offset=0)).clone()
    g_ref = ref.arena.g.clone()
    m = FasterRCNN("cuda", **kw)
    m.enable_wgrad_stream()
    m.enable_branch_stream()
    m.enable_grouped_wgrad()
    l_side = torch.cat(m.forward_backward(image, gt, im_info, step=4, image_offset=0)).clone()
    m.ws.join()
    torch.cuda.synchronize()
    assert torch.equal(l_ref, l_side)
    denom = g_ref.abs().max().item()
    assert (g_ref - m.arena.g).abs().max().item() <= 1e-3 * denom
    offs, masks = _head(m)
    for l in (offs[-1], masks[-1]):
        a, r = m.arena.view(l.wi, "g"), ref.arena.view(l.wi, "g")
        assert r.abs().sum().item() > 0 and (a - r).abs().max().item() <= 1e-2 * r.abs().max().item(), l.name
    m.capture(image, gt, im_info, lr=0.0, image_offset=0, warmup=1)
    l_graph = torch.cat(m.replay(image, gt, im_info, 4)).clone()
    torch.cuda.synchronize()
    assert torch.allclose(l_ref, l_graph, rtol=1e-4, atol=1e-5), (l_ref, l_graph)
    assert (g_ref - m.arena.g).abs().max().item() <= 1e-3 * denom


@pytest.mark.parametrize("kw", [dict(roi_pool="dpool"), dict(roi_pool="mdpool", dcn_stages=(3, 4, 5))])
def test_dpool_checkpoint_round_trip_and_predict(hip, tmp_path, kw):
    """The offset head survives save / load (FC weights 2-D, the pooled-input ones in (C, H, W) order, padding
    stripped); the loaded model computes the same step; predict runs both passes."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    from mxdetection_amd.utils import load_params
    N, H, W = 1, 192, 256
    image, gt, im_info = _inputs(N, H, W, seed=4)
    kw = dict(pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=128, **kw)
    a = FasterRCNN("cuda", seed=7, **kw)
    a.train_step(image, gt, im_info, step=0, lr=0.01)           # non-zero offset FCs and momentum
    a.train_step(image, gt, im_info, step=1, lr=0.01)
    fn = str(tmp_path / "dpool-0001.params")
    a.save_checkpoint(fn)
    blob = load_params(fn)
    assert blob["arg:bbox.offset_fc1.weight"].shape == (1024, 12544)
    assert blob["arg:bbox.offset_fc3.weight"].shape == (98, 1024) and blob["arg:bbox.offset_fc3.bias"].shape == (98,)
    w_here = a.arena.view(a.roi_extractor.offset_fc[0].wi, "w").float().cpu().numpy().reshape(1024, 7, 7, 256)
    assert np.array_equal(blob["arg:bbox.offset_fc1.weight"].reshape(1024, 256, 7, 7)[5, 17, 2, 1], w_here[5, 2, 1, 17])
    if kw["roi_pool"] == "mdpool":
        assert blob["arg:bbox.mask_fc1.weight"].shape == (1024, 12544)
        assert blob["arg:bbox.mask_fc2.weight"].shape == (49, 1024)
        assert blob["aux:momentum:bbox.mask_fc2.weight"].shape == (49, 1024)
    b = FasterRCNN("cuda", seed=11, **kw)
    assert b.load_checkpoint(fn) == []
    assert torch.equal(a.arena.w, b.arena.w) and torch.equal(a.arena.m, b.arena.m) and torch.equal(a.arena.wb, b.arena.wb)
    la = torch.cat(a.forward_backward(image, gt, im_info, step=2)).clone()
    lb = torch.cat(b.forward_backward(image, gt, im_info, step=2)).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    dets, num = b.predict(image, im_info)
    torch.cuda.synchronize()
    assert dets.shape == (N, 100, 6) and torch.isfinite(dets).all() and int(num[0]) >= 0
