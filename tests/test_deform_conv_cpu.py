"""Deformable convolution without a GPU: the config keys and the DCN experiment file, the C-ABI's argument checks, and
the fp64 torch reference of tests/test_gpu_deform_conv.py against plain / shifted convolutions."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_deform_conv import deform_conv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_defaults_and_dcn_experiment_file(monkeypatch):
    from mxdetection_amd import models
    from mxdetection_amd.models import builder
    from mxdetection_amd.utils.config import default_config, load_config
    d = default_config()
    assert d.network.dcn_stages == [] and d.network.dcn_modulated is True and d.network.dcn_groups == 1
    cfg = load_config(os.path.join(ROOT, "configs", "faster_rcnn_r50_fpn_dcn.yaml"))
    assert cfg.network.type == "faster_rcnn" and sorted(cfg.network.dcn_stages) == [3, 4, 5]
    assert cfg.network.dcn_modulated is True and cfg.network.dcn_groups == 1
    seen = {}

    class Recorder:
        def __init__(self, device, **kw):
            seen.update(kw)

    monkeypatch.setattr(models, "FasterRCNN", Recorder)
    builder.build_detector(cfg, device="cpu")
    assert seen["dcn_stages"] == (3, 4, 5) and seen["dcn_modulated"] is True and seen["dcn_groups"] == 1
    seen.clear()
    builder.build_detector(load_config(None, ["network.dcn_modulated=false", "network.dcn_stages=[5]"]), device="cpu")
    assert seen["dcn_stages"] == (5,) and seen["dcn_modulated"] is False
    seen.clear()
    builder.build_detector(default_config(), device="cpu")
    assert seen["dcn_stages"] == ()


def test_resnet_refuses_dcn_outside_the_trainable_stages():
    from mxdetection_amd.models.backbones import ResNet
    for bad in ((2,), (6,)):
        with pytest.raises(ValueError, match="dcn_stages"):
            ResNet(50, None, None, "cpu", None, dcn_stages=bad)


def _lib():
    from mxdetection_amd import _lib as L, build
    if not os.path.exists(L.LIB_PATH):
        build.build_hip(verbose=False)
    return L, L.load()


def _desc(L, **kw):
    d = L.DeformDescT()
    vals = dict(N=2, H=9, W=11, C=64, Ho=9, Wo=11, KH=3, KW=3, stride=1, pad=1, groups=1, modulated=1, off_channels=32,
                accumulate=0)
    vals.update(kw)
    for k, v in vals.items():
        setattr(d, k, v)
    return d


def test_deform_entries_validate_arguments():
    """Bad shapes are MXDET_ESHAPE, null pointers MXDET_EINVAL, a short workspace MXDET_EWORKSPACE: all decided on the
    host before any launch."""
    L, lib = _lib()
    p = C.c_void_p(16)                      # never dereferenced: every call below fails its checks first
    ok = _desc(L)
    assert lib.mxdet_deform_col2im_workspace_bytes(C.byref(ok)) > 0
    for bad in (dict(KH=5, KW=5, Ho=7, Wo=9), dict(KH=1, KW=1), dict(C=60), dict(groups=3), dict(off_channels=24),
                dict(off_channels=36), dict(modulated=0, off_channels=12), dict(Ho=8), dict(stride=2),
                dict(N=0), dict(groups=0)):
        d = _desc(L, **bad)
        assert lib.mxdet_deform_im2col(C.byref(d), p, p, p, None) == -2, bad
        assert lib.mxdet_deform_col2im_coord(C.byref(d), p, p, p, p, None) == -2, bad
        assert lib.mxdet_deform_col2im(C.byref(d), p, p, p, p, 1 << 30, None) == -2, bad
        assert lib.mxdet_deform_col2im_workspace_bytes(C.byref(d)) == 0, bad
    assert b"3x3" in (lib.mxdet_deform_im2col(C.byref(_desc(L, KH=5, KW=5)), p, p, p, None) and lib.mxdet_last_error())
    v1 = _desc(L, modulated=0, off_channels=24)
    assert lib.mxdet_deform_col2im_workspace_bytes(C.byref(v1)) > 0
    assert lib.mxdet_deform_im2col(None, p, p, p, None) == -1
    assert lib.mxdet_deform_im2col(C.byref(ok), None, p, p, None) == -1
    assert lib.mxdet_deform_im2col(C.byref(ok), p, p, None, None) == -1
    assert lib.mxdet_deform_col2im_coord(C.byref(ok), p, p, None, p, None) == -1
    assert lib.mxdet_deform_col2im_coord(C.byref(ok), p, p, p, None, None) == -1
    assert lib.mxdet_deform_col2im(C.byref(ok), None, p, p, p, 1 << 30, None) == -1
    need = lib.mxdet_deform_col2im_workspace_bytes(C.byref(ok))
    assert lib.mxdet_deform_col2im(C.byref(ok), p, p, p, p, need - 1, None) == -3
    assert lib.mxdet_deform_col2im(C.byref(ok), p, p, p, None, need, None) == -3


def _nhwc_conv(x, w, stride, pad):
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("stride", [1, 2])
def test_reference_is_conv2d_at_zero_offsets(stride):
    g = torch.Generator().manual_seed(stride)
    N, H, W, Cc, Cout = 2, 9, 12, 16, 8
    x = torch.randn((N, H, W, Cc), generator=g, dtype=torch.float64)
    w = torch.randn((Cout, 3, 3, Cc), generator=g, dtype=torch.float64)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    for modulated in (False, True):
        off = torch.zeros((N, Ho, Wo, 32), dtype=torch.float64)
        if modulated:
            off[..., 18:27] = 30.0          # sigmoid(30) == 1 in fp64 up to 1e-13
        y, _ = deform_conv_ref(x, off, w, stride, 1, 1, modulated)
        assert torch.allclose(y, _nhwc_conv(x, w, stride, 1), rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("dy,dx,stride,groups", [(1, -2, 1, 1), (-3, 2, 2, 2), (0, 4, 1, 2)])
def test_reference_is_a_shifted_conv2d_at_integer_offsets(dy, dx, stride, groups):
    """Integer offsets (dy, dx) everywhere sample x[y*s - pad + i + dy, x*s - pad + j + dx] (zero outside the map): a
    plain convolution over the zero-padded map with its window origin moved by (dy, dx). With G groups, group g gets
    (dy + g, dx - g)."""
    g = torch.Generator().manual_seed(7)
    N, H, W, Cc, Cout = 2, 11, 10, 16, 8
    x = torch.randn((N, H, W, Cc), generator=g, dtype=torch.float64)
    w = torch.randn((Cout, 3, 3, Cc), generator=g, dtype=torch.float64)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    off = torch.zeros((N, Ho, Wo, 40), dtype=torch.float64)
    Cg = Cc // groups
    want = 0
    M = 16
    xp = F.pad(x.permute(0, 3, 1, 2), (M, M, M, M))
    for gi in range(groups):
        gy, gx = dy + gi, dx - gi
        off[..., gi * 18:(gi + 1) * 18:2] = gy
        off[..., gi * 18 + 1:(gi + 1) * 18:2] = gx
        sub = xp[:, gi * Cg:(gi + 1) * Cg, M - 1 + gy:, M - 1 + gx:]
        yg = F.conv2d(sub, w[..., gi * Cg:(gi + 1) * Cg].permute(0, 3, 1, 2), stride=stride)[:, :, :Ho, :Wo]
        want = want + yg.permute(0, 2, 3, 1)
    y, _ = deform_conv_ref(x, off, w, stride, 1, groups, False)
    assert torch.allclose(y, want, rtol=1e-10, atol=1e-10)
