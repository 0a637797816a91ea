"""The non-local refine without a GPU: the fp64 reference of tests/_nonlocal_ref.py pinned against torch.autograd, its
softmax and L = 1 properties, the attention entries' host argument checks through the loaded library (no launch happens),
and the option validation of the model, the builder and the config files."""
import ctypes as C
import glob
import os

import pytest
import torch

import _nonlocal_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,d,scale", [(1, 64, 1.0), (37, 64, 0.125), (70, 128, 1.0)])
def test_reference_backward_is_autograd(L, d, scale):
    packed, d_out = ref.random_packed(2, L, d, 8, seed=L)
    q, k, v = [t.clone().requires_grad_() for t in ref.split_packed(packed, d, 0, d, 2 * d)]
    o = torch.softmax(scale * q @ k.transpose(1, 2), dim=2) @ v
    (o * d_out).sum().backward()
    want_o, lse = ref.attention_forward(q.detach(), k.detach(), v.detach(), scale)
    assert float((want_o - o.detach()).abs().max()) <= 1e-10
    assert float((lse - torch.logsumexp(scale * q.detach() @ k.detach().transpose(1, 2), dim=2)).abs().max()) <= 1e-10
    for got, t in zip(ref.attention_backward(q.detach(), k.detach(), v.detach(), d_out, scale), (q, k, v)):
        assert float((got - t.grad).abs().max()) <= 1e-10


def test_softmax_rows_sum_to_one_and_a_single_key_returns_v():
    packed, _ = ref.random_packed(2, 50, 64, 0, seed=3)
    q, k, v = ref.split_packed(packed, 64, 0, 64, 128)
    _, lse = ref.attention_forward(q, k, v, 1.0)
    p = torch.exp(q @ k.transpose(1, 2) - lse[..., None])
    assert float((p.sum(dim=2) - 1).abs().max()) <= 1e-12
    packed, d_out = ref.random_packed(2, 1, 128, 0, seed=4)
    q, k, v = ref.split_packed(packed, 128, 0, 128, 256)
    for emulate in (False, True):
        o, _ = ref.attention_forward(q, k, v, 1.0, emulate)
        assert torch.equal(o, v)
        dq, dk, dv = ref.attention_backward(q, k, v, d_out, 1.0, emulate=emulate)
        assert not dq.any() and not dk.any() and torch.equal(dv, d_out)


def test_emulated_reference_stays_near_the_exact_one():
    """The emulated roundings are those of bf16 operands and outputs: a few 2^-9 of the gradients' magnitude."""
    packed, d_out = ref.random_packed(2, 130, 64, 0, seed=5)
    q, k, v = ref.split_packed(packed, 64, 0, 64, 128)
    exact = ref.attention_backward(q, k, v, d_out, 0.125)
    emulated = ref.attention_backward(q, k, v, d_out, 0.125, emulate=True)
    for a, b in zip(emulated, exact):
        E = float((a - b).abs().max())
        assert 0 < E <= 8 * 2.0 ** -9 * float(b.abs().max())
        assert torch.equal(a, ref.round_bf16(a))


def test_refine_reference_is_autograd():
    g = torch.Generator().manual_seed(6)
    N, h, w, Cc, Ci = 2, 3, 5, 16, 8
    rnd = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)   # noqa: E731
    B, dRf = rnd(N, h, w, Cc), rnd(N, h, w, Cc)
    params = [rnd(3 * Ci, Cc) * 0.3, rnd(3 * Ci) * 0.1, rnd(Cc, Ci) * 0.3, rnd(Cc) * 0.1]
    leaves = [t.clone().requires_grad_() for t in [B] + params]
    Rf, _ = ref.refine_forward(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], 0.5)
    (Rf * dRf).sum().backward()
    Rf0, cache = ref.refine_forward(B, *params, 0.5)
    got = ref.refine_backward(B, dRf, params[0], params[2], 0.5, cache)
    assert float((Rf0 - Rf.detach()).abs().max()) <= 1e-12
    for name, leaf in zip(("dB", "dw_qkv", "db_qkv", "dw_out", "db_out"), leaves):
        assert float((got[name] - leaf.grad).abs().max()) <= 1e-10, name


# ---- host validation of the entries (no GPU: every case returns before a launch) --------------------------------------
def _desc(**kw):
    from mxdetection_amd import _lib
    d = _lib.AttnDescT()
    vals = dict(N=2, L=100, d=64, row_stride=192, q_off=0, k_off=64, v_off=128, scale=1.0)
    vals.update(kw)
    for k, v in vals.items():
        setattr(d, k, v)
    return d


def test_entries_validate_on_the_host():
    from mxdetection_amd import _lib
    lib = _lib.load()
    err = lambda: lib.mxdet_last_error().decode()   # noqa: E731
    p = C.c_void_p(0x10000)                          # never dereferenced: every call below is refused before a launch
    ok = _desc()
    need = lib.mxdet_attention_workspace_bytes(ok)
    assert need >= 2 * 100 * 4
    # null pointers
    assert lib.mxdet_attention_fwd(ok, None, p, p, None) == -1 and "null" in err()
    assert lib.mxdet_attention_fwd(ok, p, None, p, None) == -1 and "null" in err()
    assert lib.mxdet_attention_fwd(None, p, p, p, None) == -1 and "null" in err()
    assert lib.mxdet_attention_bwd(ok, p, p, p, p, None, p, need, None) == -1 and "null" in err()
    assert lib.mxdet_attention_bwd(ok, p, p, p, p, p, None, need, None) == -1 and "null" in err()
    assert lib.mxdet_attention_fwd(ok, C.c_void_p(0x10008), p, p, None) == -1 and "aligned" in err()
    # shapes
    bad = [(dict(d=96, row_stride=288, k_off=96, v_off=192), "d = 96"),
           (dict(d=256, row_stride=768, k_off=256, v_off=512), "d = 256"),
           (dict(L=0), "L = 0"), (dict(L=65537), "L = 65537"), (dict(N=0), "N = 0"),
           (dict(row_stride=196), "row_stride"), (dict(k_off=68), "k_off"),
           (dict(q_off=136), "q_off + d"), (dict(v_off=192), "v_off + d")]
    for kw, msg in bad:
        d = _desc(**kw)
        assert lib.mxdet_attention_workspace_bytes(d) == 0 and msg in err(), (kw, err())
        assert lib.mxdet_attention_fwd(d, p, p, p, None) == -2 and msg in err(), (kw, err())
        assert lib.mxdet_attention_bwd(d, p, p, p, p, p, p, 1 << 30, None) == -2 and msg in err(), (kw, err())
    assert lib.mxdet_attention_fwd(_desc(scale=0.0), p, p, p, None) == -1 and "scale" in err()
    # workspace
    assert lib.mxdet_attention_bwd(ok, p, p, p, p, p, p, need - 1, None) == -3 and "workspace" in err()
    assert lib.mxdet_attention_workspace_bytes(_desc(L=65536, d=128, row_stride=384, k_off=128, v_off=256)) >= 2 * 65536 * 4


# ---- options -----------------------------------------------------------------------------------------------------------
def test_option_validation_in_the_model():
    """The checks run before anything is allocated; the neck itself is built on a CPU arena (no kernel runs)."""
    from mxdetection_amd.models import FasterRCNN, RetinaNet
    from mxdetection_amd.models.necks import BFP, check_neck
    from mxdetection_amd.models.utils.layers import ParamArena, Workspace
    check_neck("bfp", "embedded_gaussian")
    check_neck("bfp", "embedded_gaussian", 4, True)
    for kw in (dict(bfp_nl_reduction=3), dict(bfp_nl_reduction=1), dict(bfp_nl_reduction=8), dict(bfp_nl_reduction=2.0),
               dict(bfp_nl_reduction=True), dict(bfp_nl_use_scale="yes")):
        with pytest.raises(ValueError, match="bfp_nl"):
            FasterRCNN("cpu", neck="bfp", bfp_refine="embedded_gaussian", **kw)
    for kw in (dict(bfp_nl_reduction=2), dict(bfp_nl_use_scale=True)):
        with pytest.raises(TypeError):
            RetinaNet("cpu", **kw)

    def neck(**kw):
        arena = ParamArena("cpu")
        b = BFP(256, arena, Workspace("cpu"), "cpu", torch.Generator().manual_seed(5), refine="embedded_gaussian", **kw)
        return b, arena

    b, arena = neck()
    assert [l.name for l in b.layers()] == ["bfp.nl.out", "bfp.nl.qkv"]      # backward completion order
    assert [e[0] for e in arena.entries] == ["bfp.nl.out.weight", "bfp.nl.out.bias", "bfp.nl.qkv.weight", "bfp.nl.qkv.bias"]
    assert (b.Ci, b.nl_scale, b.refine) == (128, 1.0, None)
    assert (b.nl_qkv.cin, b.nl_qkv.cout, b.nl_qkv.k, b.nl_out.cin, b.nl_out.cout, b.nl_out.k) == (256, 384, 1, 128, 256, 1)
    assert not b.nl_out._w0.any() and abs(float(b.nl_qkv._w0.std()) - 0.01) < 1e-3
    b4, _ = neck(nl_reduction=4, nl_use_scale=True)
    assert (b4.Ci, b4.nl_scale, b4.nl_qkv.cout) == (64, 0.125, 192)
    with pytest.raises(ValueError, match="bfp_nl_reduction"):
        neck(nl_reduction=3)


def test_option_validation_in_the_builder_and_config(monkeypatch):
    import mxdetection_amd.models as models
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils.config import default_config, load_config
    for key in ("network.bfp_nl_reduction=4", "network.bfp_nl_use_scale=true"):
        cfg = load_config(None, ["network.type=retinanet", key])
        with pytest.raises(ValueError, match=key.split("=")[0].split(".")[1]):
            build_detector(cfg, "cpu")
    with pytest.raises(ValueError, match="bfp_nl_reduction"):
        build_detector(load_config(None, ["network.neck=bfp", "network.bfp_refine=embedded_gaussian",
                                          "network.bfp_nl_reduction=3"]), "cpu")
    with pytest.raises(KeyError):
        load_config(None, ["network.bfp_nl_reductions=2"])
    cfg = load_config(os.path.join(ROOT, "configs", "libra_faster_rcnn_r50_fpn_nonlocal.yaml"))
    net = cfg.network
    assert (net.neck, net.bfp_refine, net.bfp_nl_reduction, net.bfp_nl_use_scale) == ("bfp", "embedded_gaussian", 2, False)
    assert (net.sampler, net.sampler_bins, net.reg_loss, net.reg_loss_weight) == ("iou_balanced", 3, "balanced_l1", 1.0)
    # the builder hands the keys to the model
    seen = {}
    monkeypatch.setattr(models, "FasterRCNN", lambda device, **kw: seen.update(kw) or "model")
    assert build_detector(cfg, "cpu") == "model"
    assert (seen["neck"], seen["bfp_refine"], seen["bfp_nl_reduction"], seen["bfp_nl_use_scale"]) == \
        ("bfp", "embedded_gaussian", 2, False)
    d = default_config().network
    assert (d.bfp_refine, d.bfp_nl_reduction, d.bfp_nl_use_scale) == ("conv", 2, False)
    others = [p for p in sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml"))) if "nonlocal" not in os.path.basename(p)]
    assert len(others) >= 20
    for p in others:
        net = load_config(p).network
        assert (net.bfp_nl_reduction, net.bfp_nl_use_scale) == (2, False) and net.bfp_refine in ("conv", "none"), p
