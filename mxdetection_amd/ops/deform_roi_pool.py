"""ops: (modulated) deformable RoI pooling over the FPN pyramid (MXNet role: contrib.DeformablePSROIPooling with
group_size 1; mmdetection dpool / mdpool). Semantics and layouts: include/mxdet.h, mxdet_dpool_desc_t."""
import ctypes as C

import torch

from .. import _lib
from .._lib import DpoolDescT, check, ptr, stream_ptr
from .roi_align import _pyr


def dpool_desc(maps, scales, lvl_min=2, pooled=(7, 7), sample_per_part=4, trans_std=0.1, trans=None, mask=None,
               accumulate=False):
    """Descriptor of one call. maps[l]: bf16 [N,H,W,C] (features, or the gradient maps of bwd_feat); trans [R, >= 2*PH*PW]
    and mask [R, >= PH*PW] bf16 row-major with their own row strides (mask given: modulated)."""
    d = DpoolDescT()
    d.pyr = _pyr(maps, scales, lvl_min)
    d.N, d.C = maps[0].shape[0], maps[0].shape[3]
    d.PH, d.PW = pooled
    d.sample_per_part, d.trans_std = sample_per_part, trans_std
    d.modulated = int(mask is not None)
    d.trans_stride = trans.stride(0) if trans is not None else 0
    d.mask_stride = mask.stride(0) if mask is not None else 0
    d.accumulate = int(accumulate)
    return d


def _rows(t):
    assert t is None or (t.dtype == torch.bfloat16 and t.dim() == 2 and t.stride(1) == 1), "bf16 [R, stride] rows"
    return t


def dpool_forward(feats, scales, rois, levels, pooled=(7, 7), sample_per_part=4, trans_std=0.1, lvl_min=2, trans=None,
                  mask=None, out=None):
    """feats[l] bf16 [N,H,W,C]; rois [R,5] f32; levels [R] i32 -> bf16 [R,PH,PW,C]. trans None: the no-trans pass."""
    _rows(trans), _rows(mask)
    R = rois.shape[0]
    if out is None:
        out = torch.empty((R, pooled[0], pooled[1], feats[0].shape[3]), dtype=torch.bfloat16, device=rois.device)
    d = dpool_desc(feats, scales, lvl_min, pooled, sample_per_part, trans_std, trans, mask)
    check(_lib.load().mxdet_dpool_fwd(C.byref(d), ptr(rois), ptr(levels), R, ptr(trans), ptr(mask), ptr(out),
                                      stream_ptr()), "dpool_fwd")
    return out


def dpool_backward_trans(feats, scales, rois, levels, grad_out, trans, mask=None, sample_per_part=4, trans_std=0.1,
                         lvl_min=2, d_trans=None, d_mask=None):
    """-> (d_trans like trans, d_mask like mask or None), written in full (padding columns zero)."""
    _rows(trans), _rows(mask)
    d_trans = torch.empty_like(trans) if d_trans is None else d_trans
    if mask is not None and d_mask is None:
        d_mask = torch.empty_like(mask)
    assert d_trans.stride() == trans.stride() and (mask is None or d_mask.stride() == mask.stride())
    d = dpool_desc(feats, scales, lvl_min, tuple(grad_out.shape[1:3]), sample_per_part, trans_std, trans, mask)
    check(_lib.load().mxdet_dpool_bwd_trans(C.byref(d), ptr(rois), ptr(levels), rois.shape[0], ptr(trans), ptr(mask),
                                            ptr(grad_out), ptr(d_trans), ptr(d_mask), stream_ptr()), "dpool_bwd_trans")
    return d_trans, d_mask


def dpool_backward_feat_workspace(R, pooled=(7, 7), device="cuda"):
    d = DpoolDescT()
    d.PH, d.PW = pooled
    need = _lib.load().mxdet_dpool_bwd_feat_workspace_bytes(C.byref(d), R)
    return torch.empty((max(need, 256),), dtype=torch.uint8, device=device)


def dpool_backward_feat(dmaps, scales, rois, levels, grad_out, trans=None, mask=None, sample_per_part=4, trans_std=0.1,
                        lvl_min=2, accumulate=False, workspace=None):
    """Feature adjoint (deterministic gather, no float atomics): dmaps[l] bf16 [N,H,W,C] (=, or += under accumulate)."""
    _rows(trans), _rows(mask)
    R = rois.shape[0]
    pooled = tuple(grad_out.shape[1:3])
    if workspace is None:
        workspace = dpool_backward_feat_workspace(R, pooled, grad_out.device)
    d = dpool_desc(dmaps, scales, lvl_min, pooled, sample_per_part, trans_std, trans, mask, accumulate)
    check(_lib.load().mxdet_dpool_bwd_feat(C.byref(d), ptr(rois), ptr(levels), R, ptr(trans), ptr(mask), ptr(grad_out),
                                           ptr(workspace), workspace.numel(), stream_ptr()), "dpool_bwd_feat")
