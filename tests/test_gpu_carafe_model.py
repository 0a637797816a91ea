"""CARAFE in the FPN's top-down path, in the neck alone and in the assembled Faster R-CNN at the shapes of
tests/test_gpu_libra_model.py (N = 2, 256 x 320): the neck's forward and backward against the fp64 composition of
tests/_carafe_ref.py; the eager step against its captured replay; the model of configs/faster_rcnn_r50_fpn_carafe.yaml trains,
round-trips a checkpoint, loads a plain checkpoint, predicts, and composes with the Balanced Feature Pyramid; the default model
never calls the new bindings and a CARAFE model's other parameters start as the default model's."""
import os

import numpy as np
import pytest

import _carafe_ref as ref
from test_gpu_gn_heads import _inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 256, 320
KW = dict(seed=7, pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=64)
SMALL = ["TRAIN.batch_rois=64", "TRAIN.rpn_pre_nms_top_n=600", "TRAIN.rpn_post_nms_top_n=300"]
NEW = sorted("fpn.carafe%d.%s.%s" % (l, part, p) for l in (2, 3, 4) for part in ("comp", "enc") for p in ("weight", "bias"))


def _config_model(overrides=()):
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils.config import load_config
    return build_detector(load_config(os.path.join(ROOT, "configs", "faster_rcnn_r50_fpn_carafe.yaml"), SMALL + list(overrides)),
                          "cuda")


def _visible_encoders(m_or_neck, arena, scale=50.0):
    """The encoders start at std 0.001 (near-uniform kernels): scale their real rows so that the kernels depend on content."""
    for mod in m_or_neck.carafe:
        arena.view(mod.enc.wi, "w")[:mod.enc.cout_real].mul_(scale)


@pytest.mark.parametrize("k,enc_kernel", [(5, 3), (3, 1)])
def test_neck_forward_and_backward_against_fp64(hip, k, enc_kernel):
    """The neck on its own on a tiny pyramid with odd sizes (C maps 13 x 10, 7 x 5, 4 x 3, 2 x 2: the merges crop a column, a
    row and a column, and nothing), every layer's bias random and the encoders' weights of visible size. Every map and gradient
    follows the kernel tests' rule: within 2 E + 2^-9 max |exact| of the exact fp64 composition, E = max |emulated - exact|
    from the CPU reference alone (tests/_carafe_ref.py fpn_reference: every stored map and gradient map rounded to bf16)."""
    import torch
    from mxdetection_amd.models.necks import FPN
    from mxdetection_amd.models.utils.layers import ParamArena, Workspace
    chans = [256, 512, 1024, 2048]
    sizes = [(13, 10), (7, 5), (4, 3), (2, 2)]
    c_shapes = [(N, h, w, c) for (h, w), c in zip(sizes, chans)]
    arena = ParamArena("cuda")
    neck = FPN(chans, 256, arena, Workspace("cuda"), "cuda", torch.Generator().manual_seed(3), extra_p6=False, upsample="carafe",
               carafe_k=k, carafe_compress=64, carafe_enc_kernel=enc_kernel, carafe_gen=torch.Generator().manual_seed(4))
    arena.finalize()
    g = torch.Generator().manual_seed(11)
    for l in neck.layers():
        l.materialize()
        b = arena.view(l.bi, "w")
        b[:l.cout_real] = (torch.randn((l.cout_real,), generator=g) * 0.1).cuda()
    _visible_encoders(neck, arena, 100.0)
    arena.refresh_bf16()
    for l in neck.layers():
        l.refresh_transposed()
    neck.plan(c_shapes)
    feats = [torch.randn(s, generator=g).to(torch.bfloat16).cuda() for s in c_shapes]
    dP = [(torch.randn((N, h, w, 256), generator=g) * 0.5).to(torch.bfloat16).cuda() for h, w in sizes]
    dP_ref = [t.double().cpu() for t in dP]
    dC = [torch.full(s, float("nan"), dtype=torch.bfloat16, device="cuda") for s in c_shapes]
    neck.forward(feats)
    neck.backward(dP, dC, [True] * 4)
    neck.lats[0].ws.join()
    torch.cuda.synchronize()
    params = {}
    for l in neck.layers():
        params[l.name + ".weight"] = arena.view(l.wi, "wb").double().cpu()[:l.cout_real]
        params[l.name + ".bias"] = arena.view(l.bi, "w").double().cpu()[:l.cout_real]
        assert not arena.view(l.wi, "wb")[l.cout_real:].any() and not arena.view(l.bi, "w")[l.cout_real:].any()
    f64 = [f.double().cpu() for f in feats]
    want = {e: ref.fpn_reference(f64, params, dP_ref, k, emulate=e) for e in (False, True)}
    mask = (f64[-1] > 0).double()            # FPN.backward masks the top level's gradient by C5 > 0
    for e in want:
        want[e]["dC"][-1] = want[e]["dC"][-1] * mask
    rows = []
    for i in range(4):
        rows.append(("inner%d" % i, neck.inner[i].double().cpu(), "inner", i))
        rows.append(("P%d" % i, neck.P[i].double().cpu(), "P", i))
        rows.append(("dC%d" % i, dC[i].double().cpu(), "dC", i))
    for l in neck.layers():
        gw, gb = arena.view(l.wi, "g").double().cpu(), arena.view(l.bi, "g").double().cpu()
        assert not gw[l.cout_real:].any() and not gb[l.cout_real:].any(), "%s: gradient in a padding row" % l.name
        rows.append((l.name + ".weight", gw[:l.cout_real], "grads", l.name + ".weight"))
        rows.append((l.name + ".bias", gb[:l.cout_real], "grads", l.name + ".bias"))
    u = neck.bufs[("cu0", (N, 13, 10, 256), torch.bfloat16)].double().cpu()
    near = ref.nearest_up(neck.inner[1].double().cpu(), (13, 10))
    assert float((u - near).abs().max()) > 0.05                           # the reassembly is not nearest upsampling
    for name, got, kind, key in rows:
        exact = want[False][kind][key]
        E = float((want[True][kind][key] - exact).abs().max())
        tol = 2.0 * E + 2.0 ** -9 * float(exact.abs().max())
        err = float((got - exact).abs().max())
        print("k=%d %s: E %.3e  tolerance %.3e  achieved %.3e  (max |exact| %.3e)" % (k, name, E, tol, err, float(exact.abs().max())))
        assert torch.isfinite(got).all() and err <= tol, "%s off by %.3e > %.3e" % (name, err, tol)
    for name in NEW:                                                     # the gradients reach the new layers
        assert float(want[False]["grads"][name].abs().max()) > 0, name


def test_step_and_its_captured_replay(hip):
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, gt, im_info = _inputs(N, H, W, seed=1)
    m = FasterRCNN("cuda", **KW, fpn_upsample="carafe")
    _visible_encoders(m.neck, m.arena)
    m.arena.refresh_bf16()
    m.refresh_transposed()
    m.enable_wgrad_stream()
    m.enable_branch_stream()
    m.enable_grouped_wgrad()
    l_eager = torch.cat(list(m.forward_backward(image, gt, im_info, step=4))).clone()
    m.ws.join()
    torch.cuda.synchronize()
    assert torch.isfinite(l_eager).all() and torch.isfinite(m.arena.g).all() and (l_eager > 0).all()
    new = [l for mod in m.neck.carafe for l in mod.layers()]
    for l in new:
        assert float(m.arena.view(l.wi, "g").abs().sum()) > 0, l.name
    g_eager = m.arena.g.clone()
    m.capture(image, gt, im_info, lr=0.0, image_offset=0, warmup=1)
    l_graph = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
    torch.cuda.synchronize()
    assert torch.equal(l_graph, l_eager), (l_eager, l_graph)
    again = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
    torch.cuda.synchronize()
    assert torch.equal(again, l_eager)
    for l in new:                                                        # the new layers' own gradients too, bit for bit
        lo = m.arena.offset_of(l.wi)
        n = m.arena.view(l.wi, "g").numel()
        assert torch.equal(m.arena.g[lo:lo + n], g_eager[lo:lo + n]), l.name


def test_config_model_trains_checkpoints_and_predicts(hip, tmp_path):
    """Six steps on a fixed batch at the learning rate 1e-4 of tests/test_gpu_libra_model.py: the summed loss falls."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, gt, im_info = _inputs(N, H, W, seed=1)
    m = _config_model()
    assert m.neck.carafe is not None and len(m.neck.carafe) == 3 and m.neck.carafe[0].k == 5 and m.bfp is None
    assert (m.neck.carafe[0].enc.cout, m.neck.carafe[0].enc.cout_real, m.neck.carafe[0].enc.k) == (128, 100, 3)
    names = [l.name for l in m.layers]
    order = ["fpn.out5", "fpn.carafe2.enc", "fpn.carafe2.comp", "fpn.carafe3.enc", "fpn.carafe3.comp", "fpn.carafe4.enc",
             "fpn.carafe4.comp", "fpn.lat2"]
    first = names.index("fpn.out5")
    assert names[first:first + len(order)] == order                      # backward completion order
    for mod in m.neck.carafe:
        for l in mod.layers():
            assert m.mark_rpn <= m.arena.offset_of(l.wi) < m.mark_fpn        # inside the FPN bucket
    init = m.export_params()
    assert abs(float(init["fpn.carafe2.enc.weight"][:100].std()) - 0.001) < 1e-4
    hist = []
    for it in range(6):
        hist.append(torch.cat(list(m.train_step(image, gt, im_info, step=0, lr=1e-4))).cpu().numpy())
    hist = np.array(hist)
    print("losses per step:\n", hist)
    assert hist.shape == (6, 4) and np.isfinite(hist).all() and (hist[0] > 0).all()
    assert hist[-1].sum() < hist[0].sum()
    after = m.export_params()
    for name in NEW:
        if name.endswith("weight"):
            assert not torch.equal(after[name], init[name]), name        # the new layers train
    assert not after["fpn.carafe2.enc.weight"][100:].any() and not after["fpn.carafe2.enc.bias"][100:].any()
    # checkpoint round trip
    path = str(tmp_path / "carafe.params")
    m.save_checkpoint(path)
    m2 = _config_model()
    assert not torch.equal(m2.arena.w, m.arena.w)
    assert m2.load_checkpoint(path) == []
    assert torch.equal(m2.arena.w, m.arena.w) and torch.equal(m2.arena.m, m.arena.m) and torch.equal(m2.arena.wb, m.arena.wb)
    # a plain checkpoint: strict refuses, strict=False leaves the new layers at their init
    src = FasterRCNN("cuda", **KW)
    spath = str(tmp_path / "plain.params")
    src.save_checkpoint(spath)
    m3 = _config_model()
    init3 = {k: v.clone() for k, v in m3.export_params().items() if k in NEW}
    with pytest.raises(KeyError):
        _config_model().load_checkpoint(spath)
    assert sorted(m3.load_checkpoint(spath, strict=False)) == NEW
    got, want = m3.export_params(), src.export_params()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    for k in NEW:
        assert torch.equal(got[k], init3[k]), k
    # predict
    dets, num = m.predict(image, im_info, score_thresh=0.0)
    torch.cuda.synchronize()
    assert dets.shape == (N, 100, 6) and int(num.min()) > 0 and torch.isfinite(dets).all()


def test_composes_with_the_balanced_feature_pyramid(hip):
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, gt, im_info = _inputs(N, H, W, seed=1)
    m = FasterRCNN("cuda", **KW, neck="bfp", fpn_upsample="carafe", carafe_k=3, carafe_enc_kernel=1)
    assert m.bfp is not None and m.neck.carafe[0].enc.cout == 64
    losses = torch.cat(list(m.train_step(image, gt, im_info, step=0, lr=1e-4)))
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and (losses > 0).all() and torch.isfinite(m.arena.w).all()


def test_only_the_new_model_calls_the_new_bindings(hip, monkeypatch):
    import torch
    from mxdetection_amd import _lib
    from mxdetection_amd.models import FasterRCNN
    lib = _lib.load()
    calls = []
    new = ("mxdet_carafe_fwd", "mxdet_carafe_bwd")
    for name in new:
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _name=name: calls.append(_name) or _fn(*a))
    image, gt, im_info = _inputs(N, H, W, seed=1)
    plain = FasterRCNN("cuda", **KW)
    plain.forward_backward(image, gt, im_info, step=1)
    torch.cuda.synchronize()
    assert calls == []
    m = _config_model()
    # the new layers draw from a generator of their own: every other parameter starts bit-identical
    mine, theirs = m.export_params(), plain.export_params()
    assert sorted(set(mine) - set(theirs)) == NEW and set(theirs) <= set(mine)
    for name, v in theirs.items():
        assert torch.equal(mine[name], v), name
    m.forward_backward(image, gt, im_info, step=1)
    torch.cuda.synchronize()
    assert sorted(set(calls)) == sorted(new) and calls.count("mxdet_carafe_fwd") == 3 and calls.count("mxdet_carafe_bwd") == 3
