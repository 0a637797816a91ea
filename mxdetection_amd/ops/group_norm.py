"""GroupNorm (+ fused ReLU) over the HIP C-ABI (include/mxdet.h, mxdet_gn_desc_t): channels-last bf16 activations
[N, ..., C], fp32 gamma / beta, fp32 per-(sample, group) mean / rstd kept for the backward pass."""
import ctypes as C

import torch

from .. import _lib
from .._lib import GnDescT, check, ptr, stream_ptr

ROUTE_RESIDENT, ROUTE_TILED = 1, 2


def gn_desc(x_shape, groups, eps=1e-5, relu=False, accumulate=False):
    """Descriptor of a [N, ..., C] tensor: every axis between the first and the last is the sample's HW."""
    d = GnDescT()
    hw = 1
    for s in x_shape[1:-1]:
        hw *= s
    d.N, d.HW, d.C, d.G = x_shape[0], hw, x_shape[-1], groups
    d.eps, d.relu, d.accumulate = eps, int(bool(relu)), int(bool(accumulate))
    return d


def workspace_bytes(x_shape, groups, backward):
    return _lib.load().mxdet_group_norm_workspace_bytes(C.byref(gn_desc(x_shape, groups)), int(bool(backward)))


def route(x_shape, groups):
    """ROUTE_RESIDENT / ROUTE_TILED for this shape (a negative MXDET_E* code for an unsupported one)."""
    return _lib.load().mxdet_debug_group_norm_route(C.byref(gn_desc(x_shape, groups)))


def _nbytes(t):
    return 0 if t is None else t.numel() * t.element_size()


def _workspace(need, workspace, device):
    """The caller's workspace if it is large enough, else a fresh one (hot paths pre-plan theirs: GroupNormLayer.plan)."""
    if need and _nbytes(workspace) < need:
        workspace = torch.empty((max(need, 256),), dtype=torch.uint8, device=device)
    return workspace


def group_norm_forward(x, gamma, beta, groups, eps=1e-5, relu=False, out=None, mean=None, rstd=None, workspace=None):
    """y = act(gamma * (x - mean) * rstd + beta); returns (y, mean [N,G], rstd [N,G])."""
    lib = _lib.load()
    d = gn_desc(x.shape, groups, eps, relu)
    if out is None:
        out = torch.empty_like(x)
    if mean is None:
        mean = torch.empty((d.N, groups), dtype=torch.float32, device=x.device)
    if rstd is None:
        rstd = torch.empty((d.N, groups), dtype=torch.float32, device=x.device)
    workspace = _workspace(lib.mxdet_group_norm_workspace_bytes(C.byref(d), 0), workspace, x.device)
    check(lib.mxdet_group_norm_fwd(C.byref(d), ptr(x), ptr(gamma), ptr(beta), ptr(out), ptr(mean), ptr(rstd),
                                   ptr(workspace), _nbytes(workspace), stream_ptr()),
          "group_norm_fwd")
    return out, mean, rstd


def group_norm_backward(x, dy, mean, rstd, gamma, groups, dgamma, dbeta, y=None, beta=None, eps=1e-5, relu=False,
                        accumulate=False, out=None, workspace=None):
    """dx (returned), and dgamma / dbeta written (added to under accumulate). relu: dy counts where y > 0 (y the
    forward output; without it the mask is recomputed from x, gamma and beta)."""
    lib = _lib.load()
    d = gn_desc(x.shape, groups, eps, relu, accumulate)
    if out is None:
        out = torch.empty_like(x)
    workspace = _workspace(lib.mxdet_group_norm_workspace_bytes(C.byref(d), 1), workspace, x.device)
    check(lib.mxdet_group_norm_bwd(C.byref(d), ptr(x), ptr(dy), ptr(y), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
                                   ptr(out), ptr(dgamma), ptr(dbeta), ptr(workspace),
                                   _nbytes(workspace), stream_ptr()), "group_norm_bwd")
    return out
