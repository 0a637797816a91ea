"""The global context block without a GPU: the fp64 reference (tests/_gc_ref.py) against torch.autograd and against the
composition of torch's own building blocks, its known answers, and the option checks of the backbone, the models, the builder,
the config and the bindings.

The tests above the "options" line exercise tests/_gc_ref.py alone: they pin the reference that the GPU tests trust, and they
pass wherever that file exists, with or without the kernels. The tests below it need the feature."""
import ctypes as C
import os

import pytest
import torch

import _backbone_ref as bref
import _gc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1, 8, 8), (2, 5, 72, 8), (3, 70, 64, 16), (2, 130, 128, 32))          # N, HW, C, P


@pytest.mark.parametrize("shape", SHAPES)
def test_explicit_backward_agrees_with_autograd(shape):
    N, HW, Cc, P = shape
    t, sc, _, p = ref.random_case(N, HW, Cc, P, seed=sum(shape))
    f = ref.forward(t, sc, p)
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(N, HW, Cc, generator=g, dtype=ref.F64)
    ds = dy * (f["y"] > 0)
    d_t, d_sc, grads = ref.autograd_backward(t, sc, p, dy)
    r = ref.backward(t, p, f, ds)
    assert float((d_sc - ds).abs().max()) == 0.0                              # the shortcut receives ds itself
    scale = max(1.0, float(d_t.abs().max()))
    assert float((r["d_t"] - d_t).abs().max()) <= 1e-10 * scale
    for name in ref.PARAMS:
        err = float((r["grads"][name] - grads[name]).abs().max())
        assert err <= 1e-10 * max(1.0, float(grads[name].abs().max())), (name, err)
        if HW > 1:
            assert float(grads[name].abs().max()) > 0, name


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_agrees_with_the_composition(shape):
    N, HW, Cc, P = shape
    t, sc, _, p = ref.random_case(N, HW, Cc, P, seed=7 + sum(shape))
    f = ref.forward(t, sc, p)
    y, add, ctx = ref.composition(t, sc, p)
    assert float((f["y"] - y).abs().max()) <= 1e-12 and float((f["add"] - add).abs().max()) <= 1e-12
    assert float((f["ctx"] - ctx).abs().max()) <= 1e-12
    assert torch.allclose(f["att"].sum(dim=1), torch.ones(N, dtype=ref.F64), atol=1e-14)


def test_a_single_position_attends_to_itself():
    t, sc, ds, p = ref.random_case(3, 1, 72, 8, seed=1)
    f = ref.forward(t, sc, p)
    assert torch.equal(f["att"], torch.ones(3, 1, dtype=ref.F64)) and torch.equal(f["ctx"], t[:, 0])
    r = ref.backward(t, p, f, ds)
    assert not r["dl"].any() and not r["grads"]["mask.weight"].any()


def test_a_zero_mask_filter_gives_mean_pooling():
    t, sc, _, p = ref.random_case(2, 37, 64, 8, seed=2)
    p["mask.weight"].zero_()
    f = ref.forward(t, sc, p)
    assert float((f["ctx"] - t.mean(dim=1)).abs().max()) <= 1e-14
    assert float((f["lse"] - torch.log(torch.tensor(37.0, dtype=ref.F64))).abs().max()) <= 1e-14


def test_a_constant_added_to_the_logits_changes_nothing():
    """Why the mask filter has no bias: att and everything behind it ignore a shift of the logits."""
    t, sc, _, p = ref.random_case(2, 37, 64, 8, seed=3)
    f = ref.forward(t, sc, p)
    shifted = torch.softmax(f["logits"] + 12.5, dim=1)
    assert float((shifted - f["att"]).abs().max()) <= 1e-15
    assert float((torch.softmax(f["logits"], dim=1) - f["att"]).abs().max()) <= 1e-15


def test_zero_fc2_is_the_plain_residual_sum():
    t, sc, ds, p = ref.random_case(2, 37, 64, 8, seed=4)
    p["fc2.weight"].zero_()
    p["fc2.bias"].zero_()
    f = ref.forward(t, sc, p)
    assert not f["add"].any() and torch.equal(f["y"], torch.relu(t + sc))
    r = ref.backward(t, p, f, ds)
    # nothing flows back through a zero fc2: d_t = ds, and only fc2 itself has a gradient
    assert torch.equal(r["d_t"], ds)
    for name in ("mask.weight", "fc1.weight", "fc1.bias", "ln.gamma", "ln.beta"):
        assert not r["grads"][name].any(), name
    assert r["grads"]["fc2.weight"].any() and r["grads"]["fc2.bias"].any()


@pytest.mark.parametrize("shape", ((2, 200, 512, 32), (3, 65, 1024, 64), (1, 201, 2048, 512), (3, 65, 2048, 128), (3, 70, 72, 8)))
def test_bounds_are_a_small_fraction_of_the_outputs(shape):
    """The fp32 bounds of the GPU test are the rule (D + 4) 2^-23 A with nothing added and come from the reference alone. A
    bound that is no small fraction of its output checks nothing: at every width, the largest element of every bound is at most
    ref.fraction_limit (2^-8; 2^-3 for the outputs two or three cancelling sums deep) of max |exact| (mean: of max |h|) -- the
    assertion tests/test_gpu_gc.py repeats at each of its cases."""
    N, HW, Cc, P = shape
    t, sc, ds, p = ref.random_case(N, HW, Cc, P, seed=6 + sum(shape))
    f = ref.forward(t, sc, p)
    r = ref.backward(t, p, f, ds)
    bf, bb = ref.bounds_forward(t, p, f), ref.bounds_backward(t, p, f, r, ds)
    assert sorted(bf) == sorted(("logits", "lse", "ctx", "h", "mean", "rstd", "add"))
    assert sorted(bb) == sorted(("d_add", "d_ctx") + ref.PARAMS)
    want = dict(r["grads"], d_add=r["d_add"], d_ctx=r["d_ctx"], **{k: f[k] for k in bf})
    for name, bound in dict(bf, **bb).items():
        exact = want[name]
        scale = float((f["h"] if name == "mean" else exact).abs().max())
        assert bound.shape == exact.shape and bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), name
        assert 0 < float(bound.max()) <= ref.fraction_limit(name) * scale, (name, float(bound.max()), scale)
    # what the rule must catch at the widest shape: add = 0, a dropped b2, a dropped or doubled W2 u
    u_w2 = f["u"] @ p["fc2.weight"].T
    for wrong in (torch.zeros_like(f["add"]), u_w2, p["fc2.bias"].expand_as(u_w2), 2 * u_w2 + p["fc2.bias"]):
        assert bool(((wrong - f["add"]).abs() > bf["add"]).any())


def test_block_reference_with_zero_fc2_is_the_plain_bottleneck():
    """The block-level reference reduces to tests/_backbone_ref.py's bottleneck when fc2 is zero (exact mode)."""
    g = torch.Generator().manual_seed(8)
    cin, planes, stride = 16, 8, 2
    x = torch.relu(torch.randn(2, 5, 4, cin, generator=g, dtype=ref.F64))
    r = lambda *s: torch.randn(*s, generator=g, dtype=ref.F64) * 0.2      # noqa: E731
    p = {"conv1.weight": r(planes, 1, 1, cin), "conv1.bias": r(planes), "conv2.weight": r(planes, 3, 3, planes),
         "conv2.bias": r(planes), "conv3.weight": r(4 * planes, 1, 1, planes), "conv3.bias": r(4 * planes),
         "down.weight": r(4 * planes, 1, 1, cin), "down.bias": r(4 * planes)}
    gc = ref.random_params(4 * planes, 8, g, zero_fc2=True)
    f = ref.bottleneck_forward(x, p, gc, stride)
    plain = bref.bottleneck_forward(x, p, stride)
    assert float((f["y"] - plain["y"]).abs().max()) <= 1e-14
    ds = torch.randn(f["y"].shape, generator=g, dtype=ref.F64) * (f["y"] > 0)
    masks = bref.block_masks(x, plain)
    got = ref.bottleneck_backward(x, f, p, gc, stride, ds, masks)
    want = bref.bottleneck_backward(x, plain, p, stride, ds, masks)
    assert float((got["dx"] - want["dx"]).abs().max()) <= 1e-13
    for k, v in want["grads"].items():
        assert float((got["grads"][k] - v).abs().max()) <= 1e-12, k
    # ... and the deformable variant's per-tap restatement of conv2's data gradient is that data gradient
    taps = sum(ref._tap_dgrad(got["d_a2"], p["conv2.weight"], ky, kx, f["a1"].shape, stride) for ky in range(3) for kx in range(3))
    assert float((taps - bref.conv_dgrad(got["d_a2"], p["conv2.weight"], f["a1"].shape, stride)).abs().max()) <= 2.0 ** -8 * \
        float(got["d_a2"].abs().max()) * float(p["conv2.weight"].abs().sum(dim=(0, 1, 2)).max())


# ---- options ----------------------------------------------------------------------------------------------------------------------
def test_option_checks_refuse_bad_values():
    from mxdetection_amd.models import FasterRCNN, RetinaNet
    from mxdetection_amd.models.backbones.resnet import ResNet, check_gcb
    assert check_gcb((5, 3), 16) == [3, 5] and check_gcb((), 3) == [] and check_gcb([3, 4, 5], 4) == [3, 4, 5]
    assert check_gcb((3,), 2) == [3]                                        # 512 / 2 = 256 <= 512
    assert check_gcb((), 16.0) == [] and check_gcb([], None) == []          # no stage chosen: the reduction is not looked at
    for make in (lambda **kw: FasterRCNN("cuda", **kw), lambda **kw: RetinaNet("cuda", **kw),
                 lambda **kw: ResNet(50, None, None, "cuda", None, **kw)):
        for kw, what in ((dict(gcb_stages=(2,)), r"gcb_stages \[2\]"), (dict(gcb_stages=(3, 6)), r"gcb_stages \[6\]"),
                         (dict(gcb_stages=(5,), gcb_reduction=2), "gcb_reduction = 2"),      # 2048 / 2 = 1024 > 512
                         (dict(gcb_stages=(3,), gcb_reduction=128), "gcb_reduction = 128"),   # 512 / 128 = 4 < 8
                         (dict(gcb_stages=(3,), gcb_reduction=48), "gcb_reduction = 48"),     # does not divide
                         (dict(gcb_stages=(4,), gcb_reduction=0), "got 0"), (dict(gcb_stages=(4,), gcb_reduction=4.0), "got 4.0"),
                         (dict(gcb_stages=(4,), gcb_reduction=True), "got True"), (dict(gcb_stages=("x",)), "gcb_stages")):
            with pytest.raises(ValueError, match=what):        # before anything is allocated: no device is touched
                make(**kw)
    with pytest.raises(ValueError, match=r"gcb_stages \[3\]"):               # stage 3 frozen
        check_gcb((3, 4), 16, frozen_stages=2)
    with pytest.raises(ValueError, match="gcb_gen"):
        ResNet(50, None, None, "cuda", None, gcb_stages=(3,))


def test_context_block_registers_its_seven_entries():
    from mxdetection_amd.models.utils.layers import ContextBlock, ParamArena
    arena = ParamArena("cpu")
    b = ContextBlock("layer2.0.gc", 512, 16, arena, "cpu", torch.Generator().manual_seed(1))
    names = [e[0] for e in arena.entries]
    assert names == ["layer2.0.gc." + s for s in ("fc2.weight", "fc2.bias", "ln.gamma", "ln.beta", "fc1.weight", "fc1.bias",
                                                  "mask.weight")]
    assert [e[1] for e in arena.entries] == [(512, 32), (512,), (32,), (32,), (32, 512), (32,), (512,)]
    assert [n for n, _ in b.named_params()] == names and b.trainable
    arena.w = torch.full((arena.size,), 7.0)
    b.materialize()
    v = lambda part: arena.view(b.idx[part], "w")      # noqa: E731
    assert not v("fc2.weight").any() and not v("fc2.bias").any() and not v("fc1.bias").any() and not v("ln.beta").any()
    assert bool((v("ln.gamma") == 1).all())
    he = (2.0 / 512) ** 0.5
    assert abs(float(v("fc1.weight").std()) / he - 1) < 0.05 and abs(float(v("mask.weight").std()) / he - 1) < 0.15
    for bad in (3, 0, 1024, True, 16.0):                                     # 512 / 3; 0; P = 0; not an integer
        with pytest.raises(ValueError):
            ContextBlock("x", 512, bad, ParamArena("cpu"), "cpu", torch.Generator())


def test_config_parses_and_the_builder_passes_the_keys(monkeypatch):
    from mxdetection_amd import models
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils.config import load_config
    cfg = load_config(os.path.join(ROOT, "configs", "mask_rcnn_r50_fpn_gcb.yaml"))
    assert (cfg.network.type, list(cfg.network.gcb_stages), cfg.network.gcb_reduction) == ("mask_rcnn", [3, 4, 5], 16)
    plain = load_config(os.path.join(ROOT, "configs", "mask_rcnn_r50_fpn.yaml"))
    assert list(plain.network.gcb_stages) == [] and plain.network.gcb_reduction == 16
    seen = {}

    def fake(name):
        def make(device, **kw):
            seen[name] = kw
            raise RuntimeError("stop here")
        return make
    monkeypatch.setattr(models, "FasterRCNN", fake("rcnn"))
    monkeypatch.setattr(models, "RetinaNet", fake("retina"))
    with pytest.raises(RuntimeError, match="stop here"):
        build_detector(cfg, "cuda")
    assert seen["rcnn"]["gcb_stages"] == (3, 4, 5) and seen["rcnn"]["gcb_reduction"] == 16 and seen["rcnn"]["with_mask"]
    rcfg = load_config(os.path.join(ROOT, "configs", "retinanet_r101_fpn.yaml"), ["network.gcb_stages=[4,5]", "network.gcb_reduction=4"])
    with pytest.raises(RuntimeError, match="stop here"):
        build_detector(rcfg, "cuda")
    assert seen["retina"]["gcb_stages"] == (4, 5) and seen["retina"]["gcb_reduction"] == 4
    monkeypatch.undo()
    for over, what in ((["network.gcb_stages=[2]"], "gcb_stages"), (["network.gcb_reduction=3"], "gcb_reduction = 3")):
        with pytest.raises(ValueError, match=what):
            build_detector(load_config(os.path.join(ROOT, "configs", "mask_rcnn_r50_fpn_gcb.yaml"), over), "cuda")


def test_bindings_refuse_bad_descriptors_on_the_host():
    """The argument checks run before any launch: no GPU needed."""
    from mxdetection_amd import _lib
    from mxdetection_amd.ops import context
    lib = _lib.load()

    def desc(**kw):
        d = context.make_desc(2, 100, 512, 32)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    good = desc()
    need = lib.mxdet_gc_workspace_bytes(C.byref(good))
    K = -(-100 // context.CHUNK)
    assert need >= 4 * (2 * K * (512 + 3) + 3 * 2 * 32 + 2 * 100) and need % 16 == 0
    assert context.workspace_bytes(2, 100, 512, 32) == need
    for kw, text in ((dict(C=12), b"C 12"), (dict(C=4096), b"C 4096"), (dict(C=0), b"C 0"), (dict(P=4), b"P 4"), (dict(P=520), b"P 520"),
                     (dict(P=36), b"P 36"), (dict(HW=0), b"HW 0"), (dict(HW=1 << 20), b"HW 1048576"), (dict(N=0), b"N 0"),
                     (dict(N=65536), b"N 65536"), (dict(N=4000, HW=(1 << 20) - 1), b"too large")):
        d = desc(**kw)
        assert lib.mxdet_gc_workspace_bytes(C.byref(d)) == 0 and text in lib.mxdet_last_error(), kw
        calls = (lib.mxdet_gc_pool_fwd(C.byref(d), None, None, None, None, 0, None),
                 lib.mxdet_gc_transform_fwd(C.byref(d), *[None] * 13, 0, None),
                 lib.mxdet_gc_fuse_fwd(C.byref(d), None, None, None, None, None, None),
                 lib.mxdet_gc_reduce_bwd(C.byref(d), None, None, 0, None),
                 lib.mxdet_gc_transform_bwd(C.byref(d), *[None] * 16, 0, None, 0, None),
                 lib.mxdet_gc_pool_bwd(C.byref(d), *[None] * 8, 0, None, 0, None))
        assert calls == (-2,) * 6 and text in lib.mxdet_last_error(), (kw, calls)
    assert lib.mxdet_gc_pool_fwd(C.byref(desc(eps=0.0)), None, None, None, None, 0, None) == -1 and b"eps" in lib.mxdet_last_error()
    assert lib.mxdet_gc_pool_fwd(None, None, None, None, None, 0, None) == -1 and b"null descriptor" in lib.mxdet_last_error()
    assert lib.mxdet_gc_pool_fwd(C.byref(good), None, None, None, None, 0, None) == -1 and b"workspace" in lib.mxdet_last_error()
    assert lib.mxdet_gc_fuse_fwd(C.byref(good), None, None, None, None, None, None) == -1 and b"null" in lib.mxdet_last_error()
    # a workspace that is present but too small, and a misaligned pointer (host addresses: nothing is launched)
    buf = (C.c_char * 64)()
    base = (C.addressof(buf) + 15) // 16 * 16
    assert lib.mxdet_gc_reduce_bwd(C.byref(good), None, C.c_void_p(base), 16, None) == -3 and b"need" in lib.mxdet_last_error()
    assert lib.mxdet_gc_reduce_bwd(C.byref(good), None, C.c_void_p(base + 4), need, None) == -1
    assert lib.mxdet_gc_fuse_fwd(C.byref(good), C.c_void_p(base + 2), C.c_void_p(base), C.c_void_p(base), C.c_void_p(base), None,
                                 None) == -1 and b"aligned" in lib.mxdet_last_error()
    with pytest.raises(ValueError, match="inner width 4"):
        context.check_shape(512, 4)
    with pytest.raises(ValueError, match="C = 4096"):
        context.check_shape(4096, 64)
