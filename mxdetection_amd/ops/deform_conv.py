"""Deformable convolution (MXNet role: contrib.DeformableConvolution) over the HIP C-ABI: the bilinear gather into the
column tensor and its two adjoints. The contraction is dense.conv2d_* as a 1x1 convolution on the column tensor
(include/mxdet.h, mxdet_deform_desc_t)."""
import ctypes as C

import torch

from .. import _lib
from .._lib import DeformDescT, check, ptr, stream_ptr


def deform_desc(x_shape, stride, pad, groups, modulated, off_channels, accumulate=False, k=3):
    d = DeformDescT()
    N, H, W, Cc = x_shape
    d.N, d.H, d.W, d.C = N, H, W, Cc
    d.KH = d.KW = k
    d.Ho = (H + 2 * pad - k) // stride + 1
    d.Wo = (W + 2 * pad - k) // stride + 1
    d.stride, d.pad, d.groups, d.modulated = stride, pad, groups, int(modulated)
    d.off_channels, d.accumulate = off_channels, int(accumulate)
    return d


def im2col(x, off, stride, pad, groups, modulated, out=None):
    """x bf16 [N,H,W,C], off bf16 [N,Ho,Wo,Coff] -> col bf16 [N,Ho,Wo,9C]."""
    d = deform_desc(x.shape, stride, pad, groups, modulated, off.shape[3])
    if out is None:
        out = torch.empty((d.N, d.Ho, d.Wo, 9 * d.C), dtype=torch.bfloat16, device=x.device)
    check(_lib.load().mxdet_deform_im2col(C.byref(d), ptr(x), ptr(off), ptr(out), stream_ptr()), "deform_im2col")
    return out


def col2im_coord(x, off, dcol, stride, pad, groups, modulated, out=None):
    """Gradient w.r.t. the offsets (and v2 mask logits): bf16 [N,Ho,Wo,Coff], padding channels zero."""
    d = deform_desc(x.shape, stride, pad, groups, modulated, off.shape[3])
    if out is None:
        out = torch.empty(off.shape, dtype=torch.bfloat16, device=x.device)
    check(_lib.load().mxdet_deform_col2im_coord(C.byref(d), ptr(x), ptr(off), ptr(dcol), ptr(out), stream_ptr()),
          "deform_col2im_coord")
    return out


def col2im_workspace_bytes(x_shape, stride, pad, groups, modulated, off_channels):
    d = deform_desc(x_shape, stride, pad, groups, modulated, off_channels)
    return _lib.load().mxdet_deform_col2im_workspace_bytes(C.byref(d))


def col2im(off, dcol, x_shape, stride, pad, groups, modulated, out=None, accumulate=False, workspace=None):
    """Gradient w.r.t. the input (bit-reproducible gather, no float atomics): bf16 [N,H,W,C] (+= under accumulate)."""
    lib = _lib.load()
    d = deform_desc(x_shape, stride, pad, groups, modulated, off.shape[3], accumulate)
    need = lib.mxdet_deform_col2im_workspace_bytes(C.byref(d))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 256),), dtype=torch.uint8, device=dcol.device)
    if out is None:
        out = torch.empty(tuple(x_shape), dtype=torch.bfloat16, device=dcol.device)
    check(lib.mxdet_deform_col2im(C.byref(d), ptr(off), ptr(dcol), ptr(out), ptr(workspace), workspace.numel(),
                                  stream_ptr()), "deform_col2im")
    return out
