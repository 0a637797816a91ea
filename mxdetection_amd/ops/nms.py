"""ops: batched bitmask NMS (MXNet role: contrib.box_nms / cpu_nms / gpu_nms) and batched Soft-NMS."""
import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr


def nms_batched(boxes, counts, thresh, max_keep=None, invalid=None):
    """boxes [B,n,4] f32 sorted by descending score, counts [B] i32. Returns (keep_idx [B,n] i32, num_keep [B])."""
    lib = _lib.load()
    B, n = boxes.shape[0], boxes.shape[1]
    dev = boxes.device
    keep = torch.full((B, max(n, 1)), -1, dtype=torch.int32, device=dev)
    num = torch.zeros((B,), dtype=torch.int32, device=dev)
    ws_bytes = lib.mxdet_nms_batched_workspace_bytes(B, n)
    ws = torch.empty((max(ws_bytes, 8),), dtype=torch.uint8, device=dev)
    check(lib.mxdet_nms_batched(ptr(boxes), ptr(counts), ptr(invalid), B, n, thresh,
                                n if max_keep is None else max_keep, ptr(keep), ptr(num), ptr(ws), ws_bytes,
                                stream_ptr()), "nms_batched")
    return keep, num


SOFT_NMS_METHODS = {"hard": 0, "linear": 1, "gaussian": 2}


def soft_nms_method(name):
    """Method code of mxdet_soft_nms_batched for "hard" | "linear" | "gaussian"."""
    if name not in SOFT_NMS_METHODS:
        raise ValueError("nms_method %r: expected one of %s" % (name, sorted(SOFT_NMS_METHODS)))
    return SOFT_NMS_METHODS[name]


def soft_nms_batched(boxes, scores, counts, method="linear", nms_thresh=0.5, sigma=0.5, min_score=0.001, max_keep=None):
    """Soft-NMS (Bodla et al. 2017; semantics in include/mxdet.h) of B unsorted lists: boxes [B,n,4] f32, scores [B,n] f32,
    counts [B] i32. Returns (keep_idx [B,max_keep] i32 in selection order, padding -1; keep_scores [B,max_keep] f32, the
    scores at selection, padding 0; num_keep [B] i32)."""
    lib = _lib.load()
    B, n = boxes.shape[0], boxes.shape[1]
    dev = boxes.device
    mk = n if max_keep is None else max_keep
    keep = torch.empty((B, mk), dtype=torch.int32, device=dev)
    kept_scores = torch.empty((B, mk), dtype=torch.float32, device=dev)
    num = torch.empty((B,), dtype=torch.int32, device=dev)
    check(lib.mxdet_soft_nms_batched(ptr(boxes), ptr(scores), ptr(counts), B, n, soft_nms_method(method), nms_thresh, sigma,
                                     min_score, mk, ptr(keep), ptr(kept_scores), ptr(num), stream_ptr()), "soft_nms_batched")
    return keep, kept_scores, num
