"""Global context blocks in the assembled detectors at the shapes of tests/test_gpu_carafe_model.py (N = 2, 256 x 320): a step
of FasterRCNN(gcb_stages=(3, 4, 5)) and its gradients, the eager step against the grouped / side-stream step and the captured
replay, the model of configs/mask_rcnn_r50_fpn_gcb.yaml trains, round-trips a checkpoint, loads a plain checkpoint and predicts;
the option composes with deformable conv2 and with RetinaNet; the default model never calls the new bindings and a model with the
option starts with every other parameter as the default model's."""
import os

import numpy as np
import pytest

from test_gpu_gn_heads import _inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 256, 320
KW = dict(seed=7, pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=64)
SMALL = ["TRAIN.batch_rois=64", "TRAIN.rpn_pre_nms_top_n=600", "TRAIN.rpn_post_nms_top_n=300"]
PARTS = ("fc2.weight", "fc2.bias", "ln.gamma", "ln.beta", "fc1.weight", "fc1.bias", "mask.weight")
BLOCKS = {3: 4, 4: 6, 5: 3}                      # bottlenecks per stage of a ResNet-50
ENTRIES = ("mxdet_gc_pool_fwd", "mxdet_gc_transform_fwd", "mxdet_gc_fuse_fwd", "mxdet_gc_reduce_bwd", "mxdet_gc_transform_bwd",
           "mxdet_gc_pool_bwd")


def _names(stages=(3, 4, 5)):
    return sorted("layer%d.%d.gc.%s" % (s - 1, b, p) for s in stages for b in range(BLOCKS[s]) for p in PARTS)


def _config_model(overrides=()):
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils.config import load_config
    return build_detector(load_config(os.path.join(ROOT, "configs", "mask_rcnn_r50_fpn_gcb.yaml"), SMALL + list(overrides)), "cuda")


def _visible_fc2(m, seed=3):
    """fc2 starts at zero (the block is the identity and only fc2 itself has a gradient): give it values of visible size so
    that every path of the block carries signal."""
    import torch
    g = torch.Generator().manual_seed(seed)
    for blk in m.backbone.norm_layers():
        w = m.arena.view(blk.idx["fc2.weight"], "w")
        w.copy_((torch.randn(tuple(w.shape), generator=g) * (0.5 / blk.P) ** 0.5).cuda())
    m.arena.refresh_bf16()


def _gc_grads(m):
    return {name: m.arena.view(idx, "g").clone() for blk in m.backbone.norm_layers() for name, idx in blk.named_params()}


def test_initial_state_and_only_the_new_model_calls_the_new_bindings(hip, monkeypatch):
    """The blocks draw from a generator of their own, so every parameter outside gc.* starts bit-identical to the plain
    model's. At the zero start of fc2 the block is the identity: add = 0, so the losses are the plain model's up to the extra
    bf16 rounding of t; d_u = d_add W2 = 0, so NOTHING flows back into the block: fc2.weight and fc2.bias have a gradient
    (d_add^T u, sum d_add) and the gradients of ln.gamma, ln.beta, fc1.weight, fc1.bias AND mask.weight are exactly zero --
    mask.weight too: d_wk is a sum of dl = att (e - S) with e = d_ctx . t and d_ctx = dh W1 = 0."""
    import torch
    from mxdetection_amd import _lib
    from mxdetection_amd.models import FasterRCNN
    lib = _lib.load()
    calls = []
    for name in ENTRIES:
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _name=name: calls.append(_name) or _fn(*a))
    image, gt, im_info = _inputs(N, H, W, seed=1)
    plain = FasterRCNN("cuda", **KW)
    l_plain = torch.cat(list(plain.forward_backward(image, gt, im_info, step=1))).clone()
    torch.cuda.synchronize()
    assert calls == [] and plain.backbone.norm_layers() == []
    m = FasterRCNN("cuda", **KW, gcb_stages=(3, 4, 5))
    mine, theirs = m.export_params(), plain.export_params()
    assert sorted(set(mine) - set(theirs)) == _names() and set(theirs) <= set(mine)
    for name, v in theirs.items():
        assert torch.equal(mine[name], v), name
    for name in _names():
        v = mine[name]
        if name.endswith(("fc2.weight", "fc2.bias", "fc1.bias", "ln.beta")):
            assert not v.any(), name
        elif name.endswith("ln.gamma"):
            assert bool((v == 1).all()), name
        else:
            assert v.any(), name
    # registered before the block's conv3, inside the backbone's buckets
    entries = [e[0] for e in m.arena.entries]
    i = entries.index("layer4.2.gc.fc2.weight")
    assert entries[i:i + 8] == ["layer4.2.gc." + p for p in PARTS] + ["layer4.2.conv3.weight"]
    assert m.arena.offset_of(i) == m.mark_fpn
    losses = torch.cat(list(m.forward_backward(image, gt, im_info, step=1))).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and torch.isfinite(m.arena.g).all()
    assert torch.allclose(losses, l_plain, rtol=5e-2, atol=1e-3), (losses, l_plain)
    assert sorted(set(calls)) == sorted(ENTRIES) and all(calls.count(e) == 13 for e in ENTRIES)
    for name, g in _gc_grads(m).items():
        if name.endswith(("fc2.weight", "fc2.bias")):
            assert float(g.abs().sum()) > 0, name
        else:
            assert not g.any(), name


def test_step_its_grouped_form_and_its_captured_replay(hip):
    """With fc2 of visible size every gc.* entry has a non-zero gradient. The blocks' kernels are deterministic and sit on the
    data-gradient chain, which weight-gradient grouping and the side streams do not touch: the grouped / side-stream step gives
    the plain eager step's losses and gc.* gradients bit for bit, and so does the captured replay."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, gt, im_info = _inputs(N, H, W, seed=1)
    ref = FasterRCNN("cuda", **KW, gcb_stages=(3, 4, 5))
    _visible_fc2(ref)
    l_ref = torch.cat(list(ref.forward_backward(image, gt, im_info, step=4))).clone()
    torch.cuda.synchronize()
    g_ref = _gc_grads(ref)
    assert torch.isfinite(l_ref).all() and torch.isfinite(ref.arena.g).all() and (l_ref > 0).all()
    assert sorted(g_ref) == _names()
    for name, g in g_ref.items():
        assert float(g.abs().sum()) > 0, name
    m = FasterRCNN("cuda", **KW, gcb_stages=(3, 4, 5))
    _visible_fc2(m)
    assert torch.equal(m.arena.w, ref.arena.w)
    m.enable_wgrad_stream()
    m.enable_branch_stream()
    m.enable_grouped_wgrad()
    l_eager = torch.cat(list(m.forward_backward(image, gt, im_info, step=4))).clone()
    m.ws.join()
    torch.cuda.synchronize()
    assert torch.equal(l_eager, l_ref), (l_ref, l_eager)
    for name, g in _gc_grads(m).items():
        assert torch.equal(g, g_ref[name]), name
    denom = float(ref.arena.g.abs().max())
    assert float((ref.arena.g - m.arena.g).abs().max()) <= 1e-3 * denom        # the grouped split-K order differs: the dcn test's bound
    m.capture(image, gt, im_info, lr=0.0, image_offset=0, warmup=1)
    l_graph = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
    torch.cuda.synchronize()
    assert torch.equal(l_graph, l_eager), (l_eager, l_graph)
    again = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
    torch.cuda.synchronize()
    assert torch.equal(again, l_eager)
    for name, g in _gc_grads(m).items():
        assert torch.equal(g, g_ref[name]), name


def test_config_model_trains_checkpoints_and_predicts(hip, tmp_path):
    """Mask R-CNN with the option (configs/mask_rcnn_r50_fpn_gcb.yaml): six steps on a fixed batch at the learning rate 1e-4 of
    tests/test_gpu_carafe_model.py lower the summed loss; fc2 leaves zero in the first step, every gc.* entry moves after."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, gt, im_info, gm = _inputs(N, H, W, seed=1, masks=True)
    m = _config_model()
    assert m.with_mask and m.backbone.gcb_stages == [3, 4, 5] and len(m.backbone.norm_layers()) == 13
    assert sorted(b.P for b in m.backbone.norm_layers()) == [32] * 4 + [64] * 6 + [128] * 3
    init = m.export_params()
    hist = []
    for it in range(6):
        hist.append(torch.cat(list(m.train_step(image, gt, im_info, step=0, lr=1e-4, gt_masks=gm))).cpu().numpy())
    hist = np.array(hist)
    print("losses per step:\n", hist)
    assert np.isfinite(hist).all() and (hist[0] > 0).all()
    assert hist[-1].sum() < hist[0].sum()
    after = m.export_params()
    for name in _names():
        assert not torch.equal(after[name], init[name]), name                # every entry of every block trains
    # checkpoint round trip
    path = str(tmp_path / "gcb.params")
    m.save_checkpoint(path)
    m2 = _config_model()
    assert not torch.equal(m2.arena.w, m.arena.w)
    assert m2.load_checkpoint(path) == []
    assert torch.equal(m2.arena.w, m.arena.w) and torch.equal(m2.arena.m, m.arena.m) and torch.equal(m2.arena.wb, m.arena.wb)
    # a plain checkpoint: strict refuses, strict=False leaves the blocks at their init -- the identity
    src = FasterRCNN("cuda", **KW, with_mask=True)
    spath = str(tmp_path / "plain.params")
    src.save_checkpoint(spath)
    m3 = _config_model()
    init3 = {k: v.clone() for k, v in m3.export_params().items() if k in set(_names())}
    with pytest.raises(KeyError):
        _config_model().load_checkpoint(spath)
    assert sorted(m3.load_checkpoint(spath, strict=False)) == _names()
    got, want = m3.export_params(), src.export_params()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    for k in _names():
        assert torch.equal(got[k], init3[k]), k
    # predict
    dets, num = m.predict(image, im_info, score_thresh=0.0)[:2]
    torch.cuda.synchronize()
    assert dets.shape == (N, 100, 6) and int(num.min()) > 0 and torch.isfinite(dets).all()


def test_composes_with_deformable_conv2(hip):
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, gt, im_info = _inputs(N, H, W, seed=1)
    m = FasterRCNN("cuda", **KW, dcn_stages=(5,), gcb_stages=(5,))
    assert [n for n, _ in m.backbone.norm_layers()[0].named_params()][0].startswith("layer4.")
    assert len(m.backbone.norm_layers()) == 3 and all(b.dcn and b.gcb is not None for b in m.backbone.stages[3])
    assert all(b.gcb is None for st in m.backbone.stages[:3] for b in st)
    _visible_fc2(m)
    m.forward_backward(image, gt, im_info, step=0)
    torch.cuda.synchronize()
    for name, g in _gc_grads(m).items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0, name
    losses = torch.cat(list(m.train_step(image, gt, im_info, step=0, lr=1e-4)))
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and (losses > 0).all() and torch.isfinite(m.arena.w).all()


def test_retinanet_with_the_option_trains_a_step(hip):
    import torch
    from mxdetection_amd.models import RetinaNet
    image, gt, im_info = _inputs(N, H, W, seed=1)
    m = RetinaNet("cuda", depth=50, seed=7, gcb_stages=(4, 5), gcb_reduction=4)
    assert sorted(b.P for b in m.backbone.norm_layers()) == [256] * 6 + [512] * 3
    assert sorted(n for blk in m.norm_layers for n, _ in blk.named_params()) == _names((4, 5))
    _visible_fc2(m)
    m.forward_backward(image, gt, im_info, step=0)
    torch.cuda.synchronize()
    for name, g in _gc_grads(m).items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0, name
    losses = torch.cat(list(m.train_step(image, gt, im_info, step=0, lr=1e-4)))
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and (losses > 0).all() and torch.isfinite(m.arena.w).all()
