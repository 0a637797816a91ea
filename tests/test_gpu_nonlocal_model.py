"""The embedded-Gaussian non-local refine of the Balanced Feature Pyramid in the assembled Faster R-CNN, at the shapes of
tests/test_gpu_libra_model.py (N = 2, 256 x 320: the refine level is 16 x 20 = 320 positions): the zero-initialised block is
the identity bit for bit; the neck's forward and backward against the fp64 reference of tests/_nonlocal_ref.py; the eager step
against its captured replay; the model of configs/libra_faster_rcnn_r50_fpn_nonlocal.yaml trains, round-trips a checkpoint,
loads a `conv` Libra and a plain checkpoint, predicts; only that model calls the attention bindings."""
import functools
import os

import numpy as np
import pytest

import _nonlocal_ref as ref
from test_gpu_gn_heads import _inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 256, 320
KW = dict(seed=7, pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=64)
NL = ("bfp.nl.out.weight", "bfp.nl.out.bias", "bfp.nl.qkv.weight", "bfp.nl.qkv.bias")
SMALL = ["TRAIN.batch_rois=64", "TRAIN.rpn_pre_nms_top_n=600", "TRAIN.rpn_post_nms_top_n=300"]


def _config_model(name="libra_faster_rcnn_r50_fpn_nonlocal.yaml"):
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils.config import load_config
    return build_detector(load_config(os.path.join(ROOT, "configs", name), SMALL), "cuda")


@functools.lru_cache(maxsize=None)
def _step_without_refine():
    """One eager step (step 2, inputs of seed 1) of the Balanced Feature Pyramid with refine 'none'."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    m = FasterRCNN("cuda", **KW, neck="bfp", bfp_refine="none")
    image, gt, im_info = _inputs(N, H, W, seed=1)
    losses = torch.cat(list(m.forward_backward(image, gt, im_info, step=2))).clone()
    torch.cuda.synchronize()
    return losses, m.export_grads(), [q.clone() for q in m.bfp.Q], m.export_params()


def test_the_block_is_the_identity_at_init(hip):
    import torch
    from mxdetection_amd.models import FasterRCNN
    l_none, g_none, q_none, p_none = _step_without_refine()
    m = FasterRCNN("cuda", **KW, neck="bfp", bfp_refine="embedded_gaussian")
    names = [l.name for l in m.layers]
    assert names.index("bfp.nl.out") + 1 == names.index("bfp.nl.qkv") and names.index("bfp.nl.qkv") + 1 == names.index("fpn.out2")
    for l in (m.bfp.nl_out, m.bfp.nl_qkv):
        assert m.mark_rpn <= m.arena.offset_of(l.wi) < m.mark_fpn        # inside the FPN bucket, before the FPN's layers
    mine = m.export_params()
    assert set(mine) - set(p_none) == set(NL)
    for name, v in p_none.items():                                       # the block draws from the BFP's own generator
        assert torch.equal(mine[name], v), name
    assert not mine["bfp.nl.out.weight"].any() and not mine["bfp.nl.out.bias"].any() and not mine["bfp.nl.qkv.bias"].any()
    assert abs(float(mine["bfp.nl.qkv.weight"].std()) - 0.01) < 1e-3 and tuple(mine["bfp.nl.qkv.weight"].shape)[0] == 384
    image, gt, im_info = _inputs(N, H, W, seed=1)
    losses = torch.cat(list(m.forward_backward(image, gt, im_info, step=2))).clone()
    torch.cuda.synchronize()
    assert torch.equal(losses, l_none), (losses, l_none)
    for a, b in zip(m.bfp.Q, q_none):
        assert torch.equal(a, b)
    grads = m.export_grads()
    assert set(grads) - set(g_none) == set(NL)
    for name, g in g_none.items():
        assert torch.equal(grads[name], g), name
    assert float(grads["bfp.nl.out.weight"].abs().sum()) > 0 and float(grads["bfp.nl.out.bias"].abs().sum()) > 0
    assert not grads["bfp.nl.qkv.weight"].any()                         # dY = W_out^T dRf is exactly zero
    assert float(m.bfp.O.float().abs().sum()) > 0                       # ... although the attention ran


@pytest.mark.parametrize("reduction,use_scale", [(2, False), (4, True)])
def test_neck_forward_and_backward_against_fp64(hip, reduction, use_scale):
    """The neck on its own on a tiny pyramid (refine level 9 x 8 = 72 positions: one key tile and a tail), bfp.nl.out given
    random weights. Rf and dB follow the kernel test's rule: within 2 E + 2^-9 max |exact| of the exact fp64 composition,
    E = max |emulated - exact| from the CPU reference alone; so do the four parameter gradients."""
    import torch
    from mxdetection_amd.models.necks import BFP
    from mxdetection_amd.models.utils.layers import ParamArena, Workspace
    shapes = [(N, 36, 32, 256), (N, 18, 16, 256), (N, 9, 8, 256), (N, 5, 4, 256), (N, 3, 2, 256)]
    arena = ParamArena("cuda")
    bfp = BFP(256, arena, Workspace("cuda"), "cuda", torch.Generator().manual_seed(3), refine="embedded_gaussian",
              nl_reduction=reduction, nl_use_scale=use_scale)
    arena.finalize()
    g = torch.Generator().manual_seed(11)
    for l, std in ((bfp.nl_out, 0.05), (bfp.nl_qkv, 0.03)):
        l.materialize()
        arena.view(l.wi, "w").copy_(torch.randn(arena.view(l.wi, "w").shape, generator=g) * std)
        arena.view(l.bi, "w").copy_(torch.randn((l.cout,), generator=g) * 0.1)
    arena.refresh_bf16()
    for l in bfp.layers():
        l.refresh_transposed()
    P = [(torch.randn(s, generator=g)).to(torch.bfloat16).cuda() for s in shapes]
    dQ = [(torch.randn(s, generator=g) * 0.5).to(torch.bfloat16).cuda() for s in shapes]
    bfp.forward(P)
    bfp.backward(dQ)
    torch.cuda.synchronize()
    rs = shapes[2]
    buf = lambda k, s=rs: bfp.bufs[(k, tuple(s), torch.bfloat16)].double().cpu()   # noqa: E731
    B, Rf, dRf, dB = buf("B"), buf("Rf"), buf("dRf"), buf("dB")
    w = lambda l: (arena.view(l.wi, "wb").double().cpu().reshape(l.cout, l.cin), arena.view(l.bi, "w").double().cpu())  # noqa: E731
    (w_out, b_out), (w_qkv, b_qkv) = w(bfp.nl_out), w(bfp.nl_qkv)
    got = dict(Rf=Rf, dB=dB)
    for name, l in (("out", bfp.nl_out), ("qkv", bfp.nl_qkv)):
        got["dw_" + name] = arena.view(l.wi, "g").double().cpu().reshape(l.cout, l.cin)
        got["db_" + name] = arena.view(l.bi, "g").double().cpu()
    want = {}
    for emulate in (False, True):
        r, cache = ref.refine_forward(B, w_qkv, b_qkv, w_out, b_out, bfp.nl_scale, emulate)
        want[emulate] = dict(ref.refine_backward(B, dRf, w_qkv, w_out, bfp.nl_scale, cache, emulate), Rf=r)
    assert float((want[False]["Rf"] - B).abs().max()) > 0.05             # the block does something
    for name in ("Rf", "dB", "dw_out", "db_out", "dw_qkv", "db_qkv"):
        exact = want[False][name]
        E = float((want[True][name] - exact).abs().max())
        tol = 2.0 * E + 2.0 ** -9 * float(exact.abs().max())
        err = float((got[name] - exact).abs().max())
        print("Ci=%d %s: E %.3e  tolerance %.3e  achieved %.3e  (max |exact| %.3e)" % (bfp.Ci, name, E, tol, err,
                                                                                     float(exact.abs().max())))
        assert err <= tol, "%s off by %.3e > %.3e" % (name, err, tol)


def test_step_and_its_captured_replay(hip):
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, gt, im_info = _inputs(N, H, W, seed=1)
    m = FasterRCNN("cuda", **KW, neck="bfp", bfp_refine="embedded_gaussian")
    c = m.bfp.nl_out                                                     # a non-zero block: the gradients reach theta, phi, g
    m.arena.view(c.wi, "w").copy_(torch.randn(m.arena.view(c.wi, "w").shape, generator=torch.Generator().manual_seed(5)) * 0.05)
    m.arena.refresh_bf16()
    m.refresh_transposed()
    m.enable_wgrad_stream()
    m.enable_branch_stream()
    m.enable_grouped_wgrad()
    l_eager = torch.cat(list(m.forward_backward(image, gt, im_info, step=4))).clone()
    m.ws.join()
    torch.cuda.synchronize()
    assert torch.isfinite(l_eager).all() and torch.isfinite(m.arena.g).all() and (l_eager > 0).all()
    assert float(m.arena.view(m.bfp.nl_qkv.wi, "g").abs().sum()) > 0 and float(m.arena.view(c.wi, "g").abs().sum()) > 0
    g_eager = m.arena.g.clone()
    m.capture(image, gt, im_info, lr=0.0, image_offset=0, warmup=1)
    l_graph = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
    torch.cuda.synchronize()
    assert torch.equal(l_graph, l_eager), (l_eager, l_graph)
    again = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
    torch.cuda.synchronize()
    assert torch.equal(again, l_eager)
    for l in (m.bfp.nl_out, m.bfp.nl_qkv):                               # the block's own gradients too, bit for bit
        lo = m.arena.offset_of(l.wi)
        n = m.arena.view(l.wi, "g").numel()
        assert torch.equal(m.arena.g[lo:lo + n], g_eager[lo:lo + n]), l.name


def test_config_model_trains_checkpoints_and_predicts(hip, tmp_path):
    """Six steps on a fixed batch at the learning rate 1e-4 of tests/test_gpu_libra_model.py: the summed loss falls."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, gt, im_info = _inputs(N, H, W, seed=1)
    m = _config_model()
    assert m.bfp is not None and m.bfp.refine is None and m.bfp.Ci == 128 and m.bfp.nl_scale == 1.0
    assert (m.bbox_head.sampler, m.bbox_head.reg_loss) == ("iou_balanced", "balanced_l1")
    hist = []
    for it in range(6):
        hist.append(torch.cat(list(m.train_step(image, gt, im_info, step=0, lr=1e-4))).cpu().numpy())
    hist = np.array(hist)
    print("losses per step:\n", hist)
    assert hist.shape == (6, 4) and np.isfinite(hist).all() and (hist[0] > 0).all()
    assert hist[-1].sum() < hist[0].sum()
    assert float(m.export_params()["bfp.nl.out.weight"].abs().sum()) > 0        # the block left the identity
    # checkpoint round trip
    path = str(tmp_path / "nonlocal.params")
    m.save_checkpoint(path)
    m2 = _config_model()
    assert not torch.equal(m2.arena.w, m.arena.w)
    assert m2.load_checkpoint(path) == []
    assert torch.equal(m2.arena.w, m.arena.w) and torch.equal(m2.arena.m, m.arena.m) and torch.equal(m2.arena.wb, m.arena.wb)
    # a `conv` Libra checkpoint and a plain one: strict refuses, strict=False leaves the block at its init
    for src in (_config_model("libra_faster_rcnn_r50_fpn.yaml"), FasterRCNN("cuda", **KW)):
        spath = str(tmp_path / "other.params")
        src.save_checkpoint(spath)
        m3 = _config_model()
        init = {k: v.clone() for k, v in m3.export_params().items() if k in NL}
        with pytest.raises(KeyError):
            _config_model().load_checkpoint(spath)
        assert sorted(m3.load_checkpoint(spath, strict=False)) == sorted(NL)
        got, want = m3.export_params(), src.export_params()
        for k, v in want.items():
            if not k.startswith("bfp.refine."):
                assert torch.equal(got[k], v), k
        for k in NL:
            assert torch.equal(got[k], init[k]), k
    # predict
    dets, num = m.predict(image, im_info, score_thresh=0.0)
    torch.cuda.synchronize()
    assert dets.shape == (N, 100, 6) and int(num.min()) > 0 and torch.isfinite(dets).all()


def test_only_the_new_model_calls_the_new_bindings(hip, monkeypatch):
    import torch
    from mxdetection_amd import _lib
    from mxdetection_amd.models import FasterRCNN
    lib = _lib.load()
    calls = []
    new = ("mxdet_attention_workspace_bytes", "mxdet_attention_fwd", "mxdet_attention_bwd")
    for name in new:
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _name=name: calls.append(_name) or _fn(*a))
    image, gt, im_info = _inputs(N, H, W, seed=1)
    for kw in (dict(), dict(neck="bfp", bfp_refine="conv")):
        FasterRCNN("cuda", **KW, **kw).forward_backward(image, gt, im_info, step=1)
        torch.cuda.synchronize()
        assert calls == []
    _config_model().forward_backward(image, gt, im_info, step=1)
    torch.cuda.synchronize()
    assert sorted(calls) == sorted(new)
