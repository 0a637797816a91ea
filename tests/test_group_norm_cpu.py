"""GroupNorm without a GPU: the fp64 reference the GPU tests compare against (checked here against torch's own
group_norm + ReLU under fp64 autograd), and everything the C-ABI entries decide on the host -- argument validation,
workspace sizes, the route a shape takes."""
import ctypes as C

import numpy as np
import pytest
import torch


def gn_ref(x, gamma, beta, groups, eps=1e-5, relu=False):
    """x [N, HW, C] float64 -> (y, mean [N,G], rstd [N,G]); biased variance about the mean."""
    N, HW, Cc = x.shape
    xg = x.reshape(N, HW, groups, Cc // groups)
    mean = xg.mean(axis=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    rstd = 1.0 / np.sqrt(var + eps)
    xh = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(N, HW, Cc)
    y = xh * gamma + beta
    if relu:
        y = np.maximum(y, 0.0)
    return y, mean, rstd


def gn_ref_backward(x, dy, gamma, beta, groups, eps=1e-5, relu=False, y_mask=None):
    """(dx, dgamma, dbeta) in float64. relu: dy counts where y > 0 (y_mask: the boolean mask to use instead of the
    reference's own y > 0, e.g. the one a bf16 forward output defines)."""
    N, HW, Cc = x.shape
    cpg = Cc // groups
    y, mean, rstd = gn_ref(x, gamma, beta, groups, eps, False)
    g = dy.copy()
    if relu:
        g = g * ((y > 0) if y_mask is None else y_mask)
    xh = (x.reshape(N, HW, groups, cpg) - mean[:, None, :, None]) * rstd[:, None, :, None]
    gg = (g * gamma).reshape(N, HW, groups, cpg)
    m = HW * cpg
    s1 = (gg * xh).sum(axis=(1, 3))
    s2 = gg.sum(axis=(1, 3))
    dx = rstd[:, None, :, None] * (gg - (s2[:, None, :, None] + xh * s1[:, None, :, None]) / m)
    xh = xh.reshape(N, HW, Cc)
    return dx.reshape(N, HW, Cc), (g * xh).sum(axis=(0, 1)), g.sum(axis=(0, 1))


@pytest.mark.parametrize("N,HW,Cc,G", [(3, 49, 256, 32), (2, 5, 64, 8), (2, 7, 64, 4), (4, 1, 128, 16), (1, 3, 512, 32),
                                       (2, 12, 256, 16)])
@pytest.mark.parametrize("relu", [False, True])
def test_reference_matches_torch_fp64(N, HW, Cc, G, relu):
    rng = np.random.default_rng(N * 1000 + HW + Cc + G)
    x = rng.standard_normal((N, HW, Cc)) + 3.0 * rng.standard_normal((N, 1, Cc))
    gamma, beta = rng.standard_normal(Cc), rng.standard_normal(Cc)
    dy = rng.standard_normal((N, HW, Cc))
    xt = torch.tensor(x.transpose(0, 2, 1).copy(), requires_grad=True)          # [N, C, HW]
    gt, bt = torch.tensor(gamma, requires_grad=True), torch.tensor(beta, requires_grad=True)
    yt = torch.nn.functional.group_norm(xt, G, gt, bt, 1e-5)
    if relu:
        yt = torch.relu(yt)
    yt.backward(torch.tensor(dy.transpose(0, 2, 1).copy()))
    y, mean, rstd = gn_ref(x, gamma, beta, G, 1e-5, relu)
    dx, dg, db = gn_ref_backward(x, dy, gamma, beta, G, 1e-5, relu)
    np.testing.assert_allclose(y, yt.detach().numpy().transpose(0, 2, 1), rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(dx, xt.grad.numpy().transpose(0, 2, 1), rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(dg, gt.grad.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(db, bt.grad.numpy(), rtol=1e-10, atol=1e-10)
    if HW * Cc // G > 1:
        assert np.all(rstd > 0) and mean.shape == (N, G)


# ---- host side of the C-ABI ----

def _lib_desc(N, HW, Cc, G, relu=0, acc=0, eps=1e-5):
    from mxdetection_amd import _lib
    d = _lib.GnDescT()
    d.N, d.HW, d.C, d.G, d.eps, d.relu, d.accumulate = N, HW, Cc, G, eps, relu, acc
    return _lib.load(), d


_P = C.c_void_p(4096)      # a non-null, 16-byte aligned dummy: validation fails before anything is dereferenced


def test_entries_reject_bad_arguments_on_the_host():
    lib, d = _lib_desc(4, 49, 256, 32)
    err = lambda: lib.mxdet_last_error()   # noqa: E731
    assert lib.mxdet_group_norm_fwd(None, _P, _P, _P, _P, _P, _P, None, 0, None) == -1 and b"null descriptor" in err()
    assert lib.mxdet_group_norm_fwd(C.byref(d), None, _P, _P, _P, _P, _P, None, 0, None) == -1 and b"null pointer" in err()
    assert lib.mxdet_group_norm_fwd(C.byref(d), _P, _P, _P, _P, None, _P, None, 0, None) == -1 and b"null pointer" in err()
    assert lib.mxdet_group_norm_bwd(C.byref(d), _P, None, _P, _P, _P, _P, _P, _P, _P, _P, _P, 1 << 30, None) == -1
    assert b"null pointer" in err()
    assert lib.mxdet_group_norm_bwd(C.byref(d), _P, _P, _P, _P, _P, _P, _P, _P, None, _P, _P, 1 << 30, None) == -1
    _, dr = _lib_desc(4, 49, 256, 32, relu=1)
    # relu without y needs beta to recompute the mask
    assert lib.mxdet_group_norm_bwd(C.byref(dr), _P, _P, None, _P, _P, _P, None, _P, _P, _P, _P, 1 << 30, None) == -1
    assert b"relu" in err()
    assert lib.mxdet_group_norm_fwd(C.byref(d), C.c_void_p(4098), _P, _P, _P, _P, _P, None, 0, None) == -1
    assert b"16-byte aligned" in err()
    for bad, word in (((4, 49, 256, 48), b"C % G"), ((4, 49, 96, 24), b"multiple of 8"), ((4, 49, 2048, 32), b"1024"),
                      ((4, 0, 256, 32), b"positive"), ((0, 49, 256, 32), b"positive"), ((4, 49, 256, 0), b"positive")):
        _, db_ = _lib_desc(*bad)
        assert lib.mxdet_group_norm_fwd(C.byref(db_), _P, _P, _P, _P, _P, _P, _P, 1 << 30, None) == -2, bad
        assert word in err(), (bad, err())
        assert lib.mxdet_group_norm_bwd(C.byref(db_), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, 1 << 30, None) == -2
        assert lib.mxdet_group_norm_workspace_bytes(C.byref(db_), 1) == 0
        assert lib.mxdet_debug_group_norm_route(C.byref(db_)) == -2


def test_workspace_too_small_is_reported():
    lib, d = _lib_desc(4, 49, 256, 32)
    need = lib.mxdet_group_norm_workspace_bytes(C.byref(d), 1)
    assert need >= 4 * 2 * 256 * 4
    rc = lib.mxdet_group_norm_bwd(C.byref(d), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, need - 1, None)
    assert rc == -3 and b"workspace" in lib.mxdet_last_error()
    rc = lib.mxdet_group_norm_bwd(C.byref(d), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, None, need, None)
    assert rc == -3
    _, dt = _lib_desc(2, 100 * 168, 256, 32)
    need = lib.mxdet_group_norm_workspace_bytes(C.byref(dt), 0)
    assert need > 0
    assert lib.mxdet_group_norm_fwd(C.byref(dt), _P, _P, _P, _P, _P, _P, _P, need - 1, None) == -3
    assert lib.mxdet_group_norm_fwd(C.byref(dt), _P, _P, _P, _P, _P, _P, None, 0, None) == -3


def test_workspace_and_route_of_the_three_shapes():
    from mxdetection_amd.ops import group_norm as GN
    box, mask, tiled = (1024, 7, 7, 256), (256, 14, 14, 256), (2, 100 * 168, 256)
    assert GN.route(box, 32) == GN.ROUTE_RESIDENT
    assert GN.route(mask, 32) == GN.ROUTE_RESIDENT
    assert GN.route(tiled, 32) == GN.ROUTE_TILED
    # resident forward: no workspace; backward: one fp32 row of (dgamma | dbeta) per sample
    assert GN.workspace_bytes(box, 32, False) == 0 and GN.workspace_bytes(mask, 32, False) == 0
    assert GN.workspace_bytes(box, 32, True) == 1024 * 2 * 256 * 4
    assert GN.workspace_bytes(mask, 32, True) == 256 * 2 * 256 * 4
    # tiled: chunks of 64 pixels at C = 256 -> 263 per sample; (mean, M2) per (sample, chunk, group)
    chunks = -(-100 * 168 // 64)
    assert GN.workspace_bytes(tiled, 32, False) == 2 * chunks * 32 * 2 * 4
    assert GN.workspace_bytes(tiled, 32, True) >= 2 * chunks * 2 * 256 * 4 + 2 * chunks * 32 * 2 * 4 + 2 * 32 * 2 * 4
    # the route boundary: 8 vectors per thread of a 1024-thread workgroup, i.e. 8 * (1024 // (C / 8)) pixels
    for Cc in (64, 256, 512):
        edge = 8 * (1024 // (Cc // 8))
        assert GN.route((1, edge, Cc), 8) == GN.ROUTE_RESIDENT
        assert GN.route((1, edge + 1, Cc), 8) == GN.ROUTE_TILED
    # the route is a function of the sample alone
    assert GN.route((1, 49, 256), 32) == GN.route((4096, 49, 256), 32)


# ---- configuration of the GN heads ----

def test_config_defaults_are_todays_model():
    from mxdetection_amd.utils.config import default_config, load_config
    net = default_config().network
    assert (net.bbox_head, net.head_norm, net.gn_groups) == ("2fc", "none", 32)
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for fn, typ in (("faster_rcnn_r50_fpn_gn_head.yaml", "faster_rcnn"), ("mask_rcnn_r50_fpn_gn_head.yaml", "mask_rcnn")):
        net = load_config(os.path.join(root, "configs", fn)).network
        assert (net.type, net.bbox_head, net.head_norm, net.gn_groups) == (typ, "4conv1fc", "gn", 32)
    net = load_config(None, ["network.bbox_head=4conv1fc", "network.gn_groups=16"]).network
    assert (net.bbox_head, net.gn_groups) == ("4conv1fc", 16)


@pytest.mark.parametrize("kw,word", [
    (dict(bbox_head="2conv"), "bbox_head"), (dict(head_norm="bn"), "head_norm"),
    (dict(head_norm="gn"), "nothing to normalise"),                       # 2fc box head, no mask head
    (dict(bbox_head="4conv1fc", head_norm="gn", gn_groups=48), "gn_groups"),        # 256 % 48 != 0
    (dict(bbox_head="4conv1fc", head_norm="gn", gn_groups=64), "gn_groups"),        # 256 / 64 = 4, not a multiple of 8
    (dict(bbox_head="4conv1fc", head_norm="gn", gn_groups=0), "gn_groups"),
])
def test_bad_head_options_raise_before_any_allocation(kw, word, monkeypatch):
    """ValueError on a machine without a GPU: nothing touches the device before the check."""
    from mxdetection_amd.models import FasterRCNN
    from mxdetection_amd.models.utils import layers
    monkeypatch.setattr(layers.ParamArena, "finalize", lambda self: (_ for _ in ()).throw(AssertionError("allocated")))
    with pytest.raises(ValueError, match=word):
        FasterRCNN("cuda", **kw)


def test_builder_plumbs_and_rejects_head_options():
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils.config import load_config
    with pytest.raises(ValueError, match="head_norm"):
        build_detector(load_config(None, ["network.head_norm=ln"]))
    with pytest.raises(ValueError, match="nothing to normalise"):
        build_detector(load_config(None, ["network.head_norm=gn"]))
    with pytest.raises(ValueError, match="gn_groups"):
        build_detector(load_config(None, ["network.type=mask_rcnn", "network.head_norm=gn", "network.gn_groups=7"]))
    for o in ("network.bbox_head=4conv1fc", "network.head_norm=gn"):
        with pytest.raises(ValueError, match="retinanet"):
            build_detector(load_config(None, ["network.type=retinanet", o]))


def test_group_norm_layer_registers_fp32_arena_entries_without_random_draws():
    from mxdetection_amd.models.utils.layers import GroupNormLayer, ParamArena
    a = ParamArena("cpu")
    state = torch.random.get_rng_state()
    l = GroupNormLayer("bbox.conv0_gn", 256, 32, a, "cpu")
    assert torch.equal(state, torch.random.get_rng_state())
    assert [e[:2] for e in a.entries] == [("bbox.conv0_gn.gamma", (256,)), ("bbox.conv0_gn.beta", (256,))]
    a.finalize()
    l.materialize()
    assert a.w.dtype == torch.float32 and torch.all(l.gamma == 1) and not l.beta.any()
    assert l.gamma.data_ptr() == a.view(l.gi, "w").data_ptr()          # the kernel reads the master copy
    with pytest.raises(ValueError, match="groups"):
        GroupNormLayer("x", 256, 64, a, "cpu")
