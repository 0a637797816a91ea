"""Reference of the OHEM tests (tests/test_ohem_cpu.py, tests/test_gpu_ohem.py, tests/test_gpu_ohem_model.py); not collected.

It restates the selection semantics of include/mxdet.h (mxdet_ohem_select, mxdet_ohem_gather) literally in numpy float32 /
integers, one fp32 operation per step: the order by (score bits as uint32 descending, pool slot ascending), greedy NMS over
that order with mxdet_iou's "+1" convention and a strict `>`, the first R survivors, foreground first. It lives here because
oracle/ is frozen.
"""
import numpy as np

F = np.float32


def iou_one_to_many(a, b):
    """mxdet_iou (include/mxdet_math.h) of box a [4] against boxes b [k,4], float32, the same operations in the same order."""
    a = np.asarray(a, F)
    b = np.asarray(b, F).reshape(-1, 4)
    one = F(1.0)
    ix1, iy1 = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    ix2, iy2 = np.minimum(a[2], b[:, 2]), np.minimum(a[3], b[:, 3])
    iw = (ix2 - ix1).astype(F) + one
    ih = (iy2 - iy1).astype(F) + one
    inter = (iw * ih).astype(F)
    aa = ((a[2] - a[0] + one).astype(F) * (a[3] - a[1] + one).astype(F)).astype(F)
    ab = ((b[:, 2] - b[:, 0]).astype(F) + one) * ((b[:, 3] - b[:, 1]).astype(F) + one)
    ua = ((aa + ab.astype(F)).astype(F) - inter).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (inter / ua).astype(F)
    return np.where((iw <= 0) | (ih <= 0), F(0.0), v).astype(F)


def order_image(score, labels):
    """Pool slots of the candidates (label >= 0) of one image in the selection order."""
    score = np.ascontiguousarray(score, F)
    cand = np.flatnonzero(np.asarray(labels) >= 0)
    bits = score.view(np.uint32)[cand].astype(np.int64)
    return cand[np.lexsort((cand, -bits))]


def select_image(score, labels, boxes, R, nms_thresh):
    """One image: score / labels [P], boxes [P,4]. Returns (sel [R] int32 padded with -1, num_sel, num_fg, suppressed) where
    suppressed counts the candidates an earlier kept one removed before R were chosen or the list ended."""
    labels = np.asarray(labels)
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    order = order_image(score, labels)
    if nms_thresh >= 1.0:
        kept, suppressed = list(order[:R]), 0
    else:
        thr = F(nms_thresh)
        alive = np.ones(len(order), bool)
        kept, suppressed = [], 0
        for k, slot in enumerate(order):
            if not alive[k]:
                continue
            if len(kept) == R:
                break
            kept.append(slot)
            rest = np.flatnonzero(alive[k + 1:]) + k + 1
            if rest.size:
                hit = iou_one_to_many(boxes[slot], boxes[order[rest]]) > thr
                suppressed += int(hit.sum())
                alive[rest[hit]] = False
    kept = np.asarray(kept, np.int64)
    fg = np.sort(kept[labels[kept] > 0]) if kept.size else kept
    bg = np.sort(kept[labels[kept] == 0]) if kept.size else kept
    sel = -np.ones((R,), np.int32)
    sel[:len(fg)] = fg
    sel[len(fg):len(fg) + len(bg)] = bg
    return sel, len(fg) + len(bg), len(fg), suppressed


def select(score, labels, rois, R, nms_thresh):
    """score / labels [N,P], rois [N,P,5]. Returns (sel [N,R] int32, num_sel [N], num_fg [N], suppressed [N])."""
    N = labels.shape[0]
    sel = np.zeros((N, R), np.int32)
    num_sel, num_fg, sup = np.zeros((N,), np.int32), np.zeros((N,), np.int32), np.zeros((N,), np.int64)
    for n in range(N):
        sel[n], num_sel[n], num_fg[n], sup[n] = select_image(score[n], labels[n], np.asarray(rois)[n, :, 1:5], R, nms_thresh)
    return sel, num_sel, num_fg, sup


def gather(sel, rois, labels, matched, tgt=None, wgt=None):
    """The pool rows sel [N,R] in proposal-target's layout; sel < 0: its padding row. Returns (rois [N,R,5], labels [N,R],
    tgt, wgt [N,R,D] or None, matched [N,R])."""
    N, R = sel.shape
    idx = np.maximum(sel, 0).astype(np.int64)
    pad = sel < 0
    n_idx = np.arange(N)[:, None]
    o_rois = np.asarray(rois, F)[n_idx, idx].copy()
    o_rois[pad] = 0
    o_rois[..., 0] = np.arange(N, dtype=F)[:, None]
    o_lab = np.where(pad, -1, np.asarray(labels)[n_idx, idx]).astype(np.int32)
    o_m = np.where(pad, -1, np.asarray(matched)[n_idx, idx]).astype(np.int32)
    o_t = o_w = None
    if tgt is not None:
        o_t, o_w = np.asarray(tgt, F)[n_idx, idx].copy(), np.asarray(wgt, F)[n_idx, idx].copy()
        o_t[pad] = 0
        o_w[pad] = 0
    return o_rois, o_lab, o_t, o_w, o_m
