"""core/bbox (/root/reference/README.md:17): box overlaps and proposal-target sampling on the GPU.

Names follow the py-faster-rcnn / mx-rcnn lineage the reference's declared layout comes from
(`bbox_overlaps`, `sample_rois`); every function launches hand-written HIP through the C-ABI.
"""
import ctypes as C

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr


def _f32c(t):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "expected contiguous cuda float32"
    return t


def bbox_overlaps(boxes, query_boxes):
    """IoU matrix [N,K] of boxes[N,4] vs query_boxes[K,4] (legacy +1 convention)."""
    lib = _lib.load()
    _f32c(boxes), _f32c(query_boxes)
    out = torch.empty((boxes.shape[0], query_boxes.shape[0]), dtype=torch.float32, device=boxes.device)
    check(lib.mxdet_box_iou(ptr(boxes), boxes.shape[0], ptr(query_boxes), query_boxes.shape[0], ptr(out),
                            stream_ptr()), "box_iou")
    return out


def sample_rois(rois, num_rois, gt_boxes, rois_per_image=512, fg_fraction=0.25, fg_thresh=0.5, bg_thresh_hi=0.5,
                bg_thresh_lo=0.0, num_classes=81, class_agnostic=False, bbox_means=(0.0, 0.0, 0.0, 0.0),
                bbox_stds=(0.1, 0.1, 0.2, 0.2), seed=0, step=0, image_offset=0, step_dev=None, num_bins=None):
    """proposal-target. rois [N,S,5], num_rois [N] int32, gt_boxes [N,G,5] (class < 0 = padding). num_bins: None = uniform
    background sampling; 1..SAMPLER_MAX_BINS = IoU-balanced background sampling over that many fixed IoU bins
    (mxdet_proposal_target_balanced; 1 bin gives the uniform sampler's bits).

    Returns (rois [N,R,5], labels [N,R] i32, bbox_targets [N,R,D], bbox_weights [N,R,D], matched_gt [N,R] i32,
    num_fg [N] i32); D = 4 (class agnostic) or 4*num_classes.
    """
    if num_bins is not None:
        check_sampler("iou_balanced", num_bins)
    lib = _lib.load()
    _f32c(rois), _f32c(gt_boxes)
    N, S = rois.shape[0], rois.shape[1]
    G = gt_boxes.shape[1]
    R = rois_per_image
    D = 4 if class_agnostic else 4 * num_classes
    dev = rois.device
    out_rois = torch.empty((N, R, 5), dtype=torch.float32, device=dev)
    labels = torch.empty((N, R), dtype=torch.int32, device=dev)
    tgt = torch.empty((N, R, D), dtype=torch.float32, device=dev)
    wgt = torch.empty((N, R, D), dtype=torch.float32, device=dev)
    matched = torch.empty((N, R), dtype=torch.int32, device=dev)
    num_fg = torch.empty((N,), dtype=torch.int32, device=dev)
    means = (C.c_float * 4)(*bbox_means)
    stds = (C.c_float * 4)(*bbox_stds)
    head = (ptr(rois), ptr(num_rois), S, ptr(gt_boxes), N, G, R, fg_fraction, fg_thresh, bg_thresh_hi, bg_thresh_lo, num_classes,
            int(class_agnostic), means, stds, seed, step, ptr(step_dev), image_offset)
    outs = (ptr(out_rois), ptr(labels), ptr(tgt), ptr(wgt), ptr(matched), ptr(num_fg), stream_ptr())
    if num_bins is None:
        check(lib.mxdet_proposal_target(*head, *outs), "proposal_target")
    else:
        check(lib.mxdet_proposal_target_balanced(*head, num_bins, *outs), "proposal_target_balanced")
    return out_rois, labels, tgt, wgt, matched, num_fg


# ---- IoU-balanced negative sampling (Libra R-CNN; include/mxdet.h) ----
SAMPLERS = ("random", "iou_balanced")
SAMPLER_MAX_BINS = _lib.SAMPLER_MAX_BINS


def check_sampler(sampler, sampler_bins=3, ohem=False):
    """The RoI sampler options of the box head, checked before anything is allocated."""
    if sampler not in SAMPLERS:
        raise ValueError("sampler must be one of %s (got %r)" % (", ".join(SAMPLERS), sampler))
    k = sampler_bins
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= SAMPLER_MAX_BINS:
        raise ValueError("sampler_bins must be an integer in 1..%d (got %r)" % (SAMPLER_MAX_BINS, k))
    if sampler == "iou_balanced" and ohem:
        raise ValueError("sampler = 'iou_balanced' cannot be combined with ohem: OHEM keeps no fg:bg quota for the IoU bins to "
                         "balance")


# ---- online hard example mining for the box head (include/mxdet.h) ----
OHEM_MAX_POOL = 16384 + 1024
OHEM_NMS_MAX_POOL = 4096


def check_ohem(ohem_nms):
    """The OHEM option of FasterRCNN, checked before anything is allocated: ohem_nms in (0, 1]; 1 = no dedup."""
    v = ohem_nms
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < float(v) <= 1.0:
        raise ValueError("ohem_nms must be a number in (0, 1] (got %r)" % (v,))


def ohem_pool_size(rois_stride, g_max):
    """Rows of an image's candidate pool: every proposal and every ground-truth box, rounded up to a multiple of 64 (the
    box head's fc1 then stays on its split-K route)."""
    return (rois_stride + g_max + 63) // 64 * 64


def ohem_select_workspace(N, P, device):
    lib = _lib.load()
    return torch.empty((max(lib.mxdet_ohem_select_workspace_bytes(N, P), 256),), dtype=torch.uint8, device=device)


def ohem_select(score, labels, rois, rois_per_image, nms_thresh=0.7, workspace=None, sel=None, num_sel=None, num_fg=None):
    """score / labels [N,P], rois [N,P,5] -> (sel [N,R] i32 pool slot or -1, num_sel [N] i32, num_fg [N] i32): the R
    highest-score candidates (label >= 0) that survive NMS at nms_thresh (>= 1: none), foreground first."""
    lib = _lib.load()
    _f32c(score), _f32c(rois)
    N, P = labels.shape
    R = rois_per_image
    dev = score.device
    if workspace is None:
        workspace = ohem_select_workspace(N, P, dev)
    if sel is None:
        sel = torch.empty((N, R), dtype=torch.int32, device=dev)
    if num_sel is None:
        num_sel = torch.empty((N,), dtype=torch.int32, device=dev)
    if num_fg is None:
        num_fg = torch.empty((N,), dtype=torch.int32, device=dev)
    check(lib.mxdet_ohem_select(ptr(score), ptr(labels), ptr(rois), N, P, R, nms_thresh, ptr(sel), ptr(num_sel), ptr(num_fg),
                                ptr(workspace), workspace.numel(), stream_ptr()), "ohem_select")
    return sel, num_sel, num_fg


def ohem_gather(sel, pool_rois, pool_labels, pool_matched, pool_tgt=None, pool_wgt=None, out=None):
    """Rows sel [N,R] of the pool (rois [N,P,5], labels / matched [N,P], targets / weights [N,P,D] or both None) in
    sample_rois' layout: (rois [N,R,5], labels [N,R], bbox_targets, bbox_weights [N,R,D] or None, matched_gt [N,R]);
    sel < 0 gives sample_rois' padding row. out: those five, preallocated."""
    lib = _lib.load()
    N, R = sel.shape
    P = pool_labels.shape[1]
    dev = sel.device
    D = 0 if pool_tgt is None else pool_tgt.shape[2]
    if out is None:
        out = (torch.empty((N, R, 5), dtype=torch.float32, device=dev), torch.empty((N, R), dtype=torch.int32, device=dev),
               None if pool_tgt is None else torch.empty((N, R, D), dtype=torch.float32, device=dev),
               None if pool_tgt is None else torch.empty((N, R, D), dtype=torch.float32, device=dev),
               torch.empty((N, R), dtype=torch.int32, device=dev))
    o_rois, o_lab, o_tgt, o_wgt, o_m = out
    check(lib.mxdet_ohem_gather(ptr(sel), ptr(pool_rois), ptr(pool_labels), ptr(pool_matched), ptr(pool_tgt), ptr(pool_wgt), N, P,
                                R, D, ptr(o_rois), ptr(o_lab), ptr(o_tgt), ptr(o_wgt), ptr(o_m), stream_ptr()), "ohem_gather")
    return out
