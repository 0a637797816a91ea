"""Deformable convolutions in the ResNet backbone (network.dcn_stages): the assembled Faster R-CNN training step with
DCN in C3-C5 (small image, as tests/test_gpu_model.py)."""
import numpy as np
import pytest

from conftest import synth_gt

pytestmark = pytest.mark.gpu

DCN = (3, 4, 5)


def _inputs(N, H, W, seed=0):
    import torch
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(1234 + seed)
    image = torch.randn((N, 3, H, W), generator=g).cuda()
    gt = torch.from_numpy(synth_gt(rng, N, 16, H, W - 5)).cuda()
    im_info = torch.tensor([[H, W - 5, 1.0]] * N, dtype=torch.float32).cuda()
    return image, gt, im_info


def _dcn_blocks(m):
    return [b for st in m.backbone.stages for b in st if b.dcn]


def test_zero_offset_dcn_v1_matches_the_plain_model(hip):
    """v1 with zero-initialised offset convs samples exactly the plain 3x3 taps: same filters (same random draws), and
    first-step losses equal to the plain model's within tolerance; the offset convs receive non-zero gradients."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    N, H, W = 2, 256, 320
    image, gt, im_info = _inputs(N, H, W, seed=1)
    ref = FasterRCNN("cuda", seed=7, pre_nms_top_n=1000, post_nms_top_n=1000)
    l_ref = torch.cat(ref.forward_backward(image, gt, im_info, step=2)).clone()
    m = FasterRCNN("cuda", seed=7, pre_nms_top_n=1000, post_nms_top_n=1000, dcn_stages=DCN, dcn_modulated=False)
    blocks = _dcn_blocks(m)
    assert len(blocks) == 4 + 6 + 3
    for si in (1, 2, 3):
        for b, rb in zip(m.backbone.stages[si], ref.backbone.stages[si]):
            w = m.arena.view(b.conv2.conv.wi, "w")
            assert torch.equal(w.reshape(rb.conv2.cout, 3, 3, rb.conv2.cin), ref.arena.view(rb.conv2.wi, "w"))
            assert not m.arena.view(b.conv2.offset.wi, "w").any()
    assert torch.equal(m.arena.view(m.bbox_head.fc1.wi, "w"), ref.arena.view(ref.bbox_head.fc1.wi, "w"))
    l_dcn = torch.cat(m.forward_backward(image, gt, im_info, step=2)).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(l_dcn).all()
    # bf16 column tensor vs direct 3x3 tiles: the features differ in the last bits, which may move a proposal / sample
    assert torch.allclose(l_dcn, l_ref, rtol=5e-2, atol=1e-3), (l_dcn, l_ref)
    nz = [b for b in blocks if m.arena.view(b.conv2.offset.wi, "g").abs().sum().item() > 0]
    assert len(nz) == len(blocks), "offset convs without gradient: %d of %d" % (len(blocks) - len(nz), len(blocks))
    assert all(m.arena.view(b.conv2.offset.bi, "g")[:18].abs().sum().item() > 0 for b in blocks)
    # the padding output channels of the offset convs stay zero
    assert all(not m.arena.view(b.conv2.offset.wi, "g")[18:].any() for b in blocks)


def test_dcn_grouped_replayed_and_eager_steps_agree(hip):
    """v2 in C3-C5: grouped weight gradients on a side stream, the RPN branch on its own stream and the replayed hipGraph
    step compute the same step as plain eager launches."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    N, H, W = 2, 256, 320
    image, gt, im_info = _inputs(N, H, W, seed=2)
    kw = dict(seed=7, pre_nms_top_n=1000, post_nms_top_n=1000, dcn_stages=DCN, dcn_modulated=True)
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
    for b in _dcn_blocks(m):           # the DCN tensors take part in the grouped launches
        for l in b.conv2.layers():
            a, r = m.arena.view(l.wi, "g"), ref.arena.view(l.wi, "g")
            assert (a - r).abs().max().item() <= 1e-2 * (r.abs().max().item() + 1e-30), l.name
    m.capture(image, gt, im_info, lr=0.0, image_offset=0, warmup=1)
    l_graph = torch.cat(m.replay(image, gt, im_info, 4)).clone()
    torch.cuda.synchronize()
    assert torch.allclose(l_ref, l_graph, rtol=1e-4, atol=1e-5), (l_ref, l_graph)
    assert (g_ref - m.arena.g).abs().max().item() <= 1e-3 * denom


def test_dcn_checkpoint_round_trip_and_predict(hip, tmp_path):
    """Every DCN tensor survives save / load (deformable filter OIHW under the plain conv2 name, offset convs as
    conv2_offset with their padding stripped); the loaded model computes the same step; predict runs."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    from mxdetection_amd.utils import load_params
    N, H, W = 1, 192, 256
    image, gt, im_info = _inputs(N, H, W, seed=4)
    kw = dict(pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=128, dcn_stages=DCN, dcn_modulated=True)
    a = FasterRCNN("cuda", seed=7, **kw)
    a.train_step(image, gt, im_info, step=0, lr=0.01)           # non-zero offset convs and momentum
    off = a.arena.view(a.backbone.stages[1][0].conv2.offset.wi, "w")
    assert off.abs().sum().item() > 0
    fn = str(tmp_path / "dcn-0001.params")
    a.save_checkpoint(fn)
    blob = load_params(fn)
    assert blob["arg:layer2.0.conv2.weight"].shape == (128, 128, 3, 3)
    assert blob["arg:layer2.0.conv2_offset.weight"].shape == (27, 128, 3, 3)
    assert blob["arg:layer2.0.conv2_offset.bias"].shape == (27,)
    assert blob["aux:momentum:layer4.2.conv2_offset.weight"].shape == (27, 512, 3, 3)
    w_here = a.arena.view(a.backbone.stages[2][1].conv2.conv.wi, "w").float().cpu().numpy().reshape(256, 3, 3, 256)
    assert np.array_equal(blob["arg:layer3.1.conv2.weight"][5, 17, 2, 1], w_here[5, 2, 1, 17])
    b = FasterRCNN("cuda", seed=11, **kw)
    assert b.load_checkpoint(fn) == []
    assert torch.equal(a.arena.w, b.arena.w) and torch.equal(a.arena.m, b.arena.m) and torch.equal(a.arena.wb, b.arena.wb)
    la = torch.cat(a.forward_backward(image, gt, im_info, step=1)).clone()
    lb = torch.cat(b.forward_backward(image, gt, im_info, step=1)).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    dets, num = b.predict(image, im_info)
    torch.cuda.synchronize()
    assert dets.shape == (N, 100, 6) and torch.isfinite(dets).all() and int(num[0]) >= 0


def test_pretrained_import_fills_dcn_conv2(hip):
    """load_pretrained_backbone fills a deformable conv2 from stageS_unitU_conv2_weight exactly as a plain conv2 and
    leaves the offset convs at zero."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    from mxdetection_amd.utils import load_pretrained_backbone, resnet_v1_names
    rng = np.random.default_rng(5)
    plain = FasterRCNN("cuda", seed=1)
    dcn = FasterRCNN("cuda", seed=2, dcn_stages=DCN, dcn_modulated=False)
    shapes = {n: tuple(t.shape) for n, _, t, _ in plain._named_tensors()}
    blob = {}
    for ours, wname, bn in resnet_v1_names(50):
        co, kh, kw_, ci = shapes[ours + ".weight"]
        blob["arg:" + wname] = (rng.standard_normal((co, ci, kh, kw_)) * (2.0 / (ci * kh * kw_)) ** 0.5 * 0.5).astype(np.float32)
        blob["arg:" + bn + "_gamma"] = rng.uniform(0.5, 1.5, co).astype(np.float32)
        blob["arg:" + bn + "_beta"] = rng.uniform(-0.2, 0.2, co).astype(np.float32)
        blob["aux:" + bn + "_moving_mean"] = rng.uniform(-0.3, 0.3, co).astype(np.float32)
        blob["aux:" + bn + "_moving_var"] = rng.uniform(0.5, 2.0, co).astype(np.float32)
    assert load_pretrained_backbone(plain, blob, depth=50) == []
    assert load_pretrained_backbone(dcn, blob, depth=50) == []
    for si in (1, 2, 3):
        for b, pb in zip(dcn.backbone.stages[si], plain.backbone.stages[si]):
            w = dcn.arena.view(b.conv2.conv.wi, "w").reshape(pb.conv2.cout, 3, 3, pb.conv2.cin)
            assert torch.equal(w, plain.arena.view(pb.conv2.wi, "w")), b.conv2.name
            assert torch.equal(b.conv2.conv.bias_f32, pb.conv2.bias_f32)
            assert not dcn.arena.view(b.conv2.offset.wi, "w").any() and not dcn.arena.view(b.conv2.offset.bi, "w").any()
    x = torch.from_numpy(rng.standard_normal((2, 3, 64, 96)).astype(np.float32)).cuda()
    plain.backbone.plan(tuple(x.shape))
    dcn.backbone.plan(tuple(x.shape))
    want = [t.float().clone() for t in plain.backbone.forward(x)]
    got = [t.float() for t in dcn.backbone.forward(x)]
    for lvl, (g, w) in enumerate(zip(got, want)):
        rel = float((g - w).norm() / w.norm())
        assert rel < 3e-2, "C%d relative error %.4f" % (lvl + 2, rel)
