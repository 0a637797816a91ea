"""Reference and inputs of the Soft-NMS tests (tests/test_soft_nms_cpu.py, tests/test_gpu_soft_nms.py); not collected.

The reference restates the semantics of include/mxdet.h (mxdet_soft_nms_batched) literally in numpy float32: one fp32
operation per step, IoU and exp through the C oracle (`oracle.box_iou`, `oracle.expf`: the kernels' bits), selection by
np.lexsort((id, -score)). It lives here because oracle/ is frozen.

Inputs: the random boxes of tests/test_gpu_postprocess.py almost never overlap among the top scorers, so Soft-NMS would
change nothing there; `clustered_case` / `clustered_lists` draw most boxes as jitters of a few objects.
"""
import numpy as np

METHODS = {"hard": 0, "linear": 1, "gaussian": 2}


def weights(oracle, o, method, nms_thresh, sigma):
    """Soft-NMS weight of IoU values o [k] f32."""
    o = np.asarray(o, np.float32)
    thr, one = np.float32(nms_thresh), np.float32(1.0)
    if method == 0:
        return np.where(o > thr, np.float32(0.0), one).astype(np.float32)
    if method == 1:
        return np.where(o > thr, one - o, one).astype(np.float32)
    t = (o * o).astype(np.float32)
    t = (t / np.float32(sigma)).astype(np.float32)
    u, inv = np.unique(t, return_inverse=True)              # one oracle call per distinct value (most IoUs are 0)
    return oracle.expf(-u).astype(np.float32)[inv].reshape(t.shape)


def soft_nms_list(oracle, boxes, scores, ids, method, nms_thresh, sigma, min_score, max_keep):
    """One list. boxes [n,4], scores [n], ids [n] (unique). Returns (selected positions, their scores at selection), both in
    selection order."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
    s = np.array(scores, np.float32).reshape(-1)
    ids = np.asarray(ids, np.int64).reshape(-1)
    ms = np.float32(min_score)
    live = s > ms
    sel, out = [], []
    while len(sel) < max_keep and live.any():
        cand = np.flatnonzero(live)
        j = int(cand[np.lexsort((ids[cand], -s[cand]))[0]])     # largest score, then lower id
        sel.append(j)
        out.append(s[j])
        live[j] = False
        rest = np.flatnonzero(live)
        if rest.size:
            o = oracle.box_iou(boxes[j:j + 1], boxes[rest])[0]
            s[rest] = (s[rest] * weights(oracle, o, method, nms_thresh, sigma)).astype(np.float32)
            live[rest] = s[rest] > ms
    return np.asarray(sel, np.int32), np.asarray(out, np.float32)


def soft_nms_batched(oracle, boxes, scores, counts, method, nms_thresh, sigma, min_score, max_keep):
    """The standalone entry: id = position. Returns (keep_idx [B,max_keep] padded -1, keep_scores padded 0, num_keep [B])."""
    B = boxes.shape[0]
    keep = -np.ones((B, max_keep), np.int32)
    ksc = np.zeros((B, max_keep), np.float32)
    num = np.zeros((B,), np.int32)
    for b in range(B):
        n = int(counts[b])
        sel, sc = soft_nms_list(oracle, boxes[b, :n], scores[b, :n], np.arange(n), method, nms_thresh, sigma, min_score, max_keep)
        keep[b, :len(sel)], ksc[b, :len(sel)], num[b] = sel, sc, len(sel)
    return keep, ksc, num


def merge_image(rows, max_det):
    """rows: list of (score f32, id, class, box [4], score before Soft-NMS). The max_det best by (score desc, id asc, class
    asc) as (dets [max_det,6], their number, their scores before Soft-NMS [max_det])."""
    dets = np.zeros((max_det, 6), np.float32)
    dets[:, 5] = -1.0
    orig = np.zeros((max_det,), np.float32)
    if not rows:
        return dets, 0, orig
    sc = np.array([r[0] for r in rows], np.float32)
    order = np.lexsort((np.array([r[2] for r in rows]), np.array([r[1] for r in rows]), -sc))[:max_det]
    for k, i in enumerate(order):
        dets[k, :4], dets[k, 4], dets[k, 5], orig[k] = rows[i][3], rows[i][0], rows[i][2], rows[i][4]
    return dets, len(order), orig


def detection_postprocess(oracle, cls, reg, rois, num_rois, im_info, means, stds, score_thresh, nms_thresh, max_det, method,
                          sigma):
    """mxdet_detection_postprocess_soft: lists built from the `scores` / `boxes` outputs of oracle.detection_postprocess
    (softmax and decode are the hard entry's), Soft-NMS per (image, foreground class) with id = roi, then the merge.
    Returns (dets [N,max_det,6], num [N], the rows' scores before Soft-NMS [N,max_det])."""
    _, _, sc, bb = oracle.detection_postprocess(cls, reg, rois, num_rois, im_info, means, stds, score_thresh, nms_thresh, max_det)
    N, Cn = len(num_rois), sc.shape[1]
    R = sc.shape[0] // N
    dets = np.zeros((N, max_det, 6), np.float32)
    num = np.zeros((N,), np.int32)
    orig = np.zeros((N, max_det), np.float32)
    for n in range(N):
        rows = []
        nv = int(num_rois[n])
        for c in range(1, Cn):
            s, b = sc[n * R:n * R + nv, c], bb[n * R:n * R + nv, c]
            cand = np.flatnonzero(s > np.float32(score_thresh))
            sel, ssc = soft_nms_list(oracle, b[cand], s[cand], cand, method, nms_thresh, sigma, score_thresh, max_det)
            rows += [(ssc[k], int(cand[j]), c, b[cand[j]], s[cand[j]]) for k, j in enumerate(sel)]
        dets[n], num[n], orig[n] = merge_image(rows, max_det)
    return dets, num, orig


def retina_detect(oracle, cls_logits, deltas, base, H, W, strides, im_info, num_classes, pre_n, score_thresh, nms_thresh,
                  max_det, method, sigma, cap=4096):
    """mxdet_retina_detect_soft: the candidates exactly as oracle.retina_detect builds them (oracle.proposal with
    threshold 2.0, oracle_sigmoid), then Soft-NMS per class with id = candidate rank, then the merge.
    Returns (dets, num, the rows' scores before Soft-NMS [N,max_det])."""
    import ctypes as C
    Cn = num_classes
    exp_d = [np.repeat(np.ascontiguousarray(d, np.float32), Cn, axis=1) for d in deltas]
    exp_b = [np.repeat(np.ascontiguousarray(b, np.float32), Cn, axis=0) for b in base]
    post = min(len(cls_logits) * pre_n, cap)
    rois, logit, gidx, num = oracle.proposal(cls_logits, exp_d, exp_b, H, W, strides, im_info, pre_n, post, 2.0, 0.0)
    L = oracle.lib()
    L.oracle_sigmoid.restype = C.c_float
    L.oracle_sigmoid.argtypes = [C.c_float]
    prob = np.array([[L.oracle_sigmoid(float(z)) for z in row] for row in logit], np.float32)
    cls = (gidx % Cn + 1).astype(np.int32)
    N = rois.shape[0]
    dets = np.zeros((N, max_det, 6), np.float32)
    nd = np.zeros((N,), np.int32)
    orig = np.zeros((N, max_det), np.float32)
    for n in range(N):
        cls[n, num[n]:] = 0
        rows = []
        for c in range(1, Cn + 1):
            cand = np.flatnonzero((cls[n] == c) & (prob[n] > np.float32(score_thresh)))
            b = rois[n, :, 1:5]
            sel, ssc = soft_nms_list(oracle, b[cand], prob[n, cand], cand, method, nms_thresh, sigma, score_thresh, max_det)
            rows += [(ssc[k], int(cand[j]), c, b[cand[j]], prob[n, cand[j]]) for k, j in enumerate(sel)]
        dets[n], nd[n], orig[n] = merge_image(rows, max_det)
    return dets, nd, orig


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _clustered_boxes(rng, n, G):
    """n boxes (x1,y1,x2,y2): each a jitter of one of G objects with probability G/(G+1), else background clutter.
    Returns (boxes [n,4] f32, object index [n], -1 for clutter)."""
    octr = rng.uniform(120, 520, (G, 2))
    osz = np.exp(rng.uniform(np.log(48), np.log(220), (G, 2)))
    k = rng.integers(0, G + 1, n)
    obj = np.where(k < G, k, -1)
    kk = np.minimum(k, G - 1)
    sz = osz[kk] * np.exp(rng.uniform(-0.25, 0.25, (n, 2)))
    ctr = octr[kk] + rng.uniform(-0.2, 0.2, (n, 2)) * osz[kk]
    bctr = rng.uniform(40, 600, (n, 2))                                  # clutter as in test_gpu_postprocess._case
    bsz = np.exp(rng.uniform(np.log(16), np.log(300), (n, 2)))
    ctr = np.where(obj[:, None] >= 0, ctr, bctr)
    sz = np.where(obj[:, None] >= 0, sz, bsz)
    return np.concatenate([ctr - sz / 2, ctr + sz / 2], 1).astype(np.float32), obj


def clustered_case(rng, N, R, C, nvalid, G=6, ndup=6):
    """Two-stage head input (cls [N*R,C], reg [N*R,4C], rois [N*R,5], nvalid, im_info 640x704) whose top scorers overlap:
    G objects per image, each with a class whose logit gets +U(3,7) in its rois; logits N(0,1.5^2) rounded to 1/8, deltas
    N(0,0.3^2). The last `ndup` valid rows of every image are copies of its first object rows (same logits, deltas and roi):
    cross-roi ties in score and box."""
    cls = np.round(rng.standard_normal((N * R, C)) * 1.5 * 8) / 8
    reg = (rng.standard_normal((N * R, 4 * C)) * 0.3).astype(np.float32)
    rois = np.zeros((N * R, 5), np.float32)
    rois[:, 0] = np.repeat(np.arange(N), R)
    for n in range(N):
        boxes, obj = _clustered_boxes(rng, R, G)
        ocls = rng.integers(1, C, G)
        rois[n * R:(n + 1) * R, 1:] = boxes
        rows = np.flatnonzero(obj >= 0)
        cls[n * R + rows, ocls[obj[rows]]] += np.round(rng.uniform(3, 7, rows.size) * 8) / 8
        nv = int(nvalid[n])
        src = rows[rows < nv - ndup][:ndup]
        dst = np.arange(nv - len(src), nv)
        for a in (cls, reg, rois):
            a[n * R + dst] = a[n * R + src]
    info = np.array([[640.0, 704.0, 1.0]] * N, np.float32)
    return cls.astype(np.float32), reg, rois, np.asarray(nvalid, np.int32), info


def clustered_lists(rng, B, n_max, G=6, tie_list=None):
    """Standalone-entry input: boxes [B,n_max,4], scores [B,n_max] in [1/256, 1] rounded to 1/256 (many ties), object boxes
    scoring higher than clutter. List `tie_list` gets three groups of five identical (box, score) entries at shuffled
    positions."""
    boxes = np.zeros((B, n_max, 4), np.float32)
    scores = np.zeros((B, n_max), np.float32)
    for b in range(B):
        boxes[b], obj = _clustered_boxes(rng, n_max, G)
        s = np.where(obj >= 0, rng.uniform(0.3, 1.0, n_max), rng.uniform(0.0, 0.5, n_max))
        scores[b] = np.maximum(np.round(s * 256), 1) / 256
    if tie_list is not None:
        pos = rng.permutation(n_max)[:15].reshape(3, 5)
        for g in pos:
            boxes[tie_list, g] = boxes[tie_list, g[0]]
            scores[tie_list, g] = max(scores[tie_list, g[0]], 0.75)
    return boxes, scores


def retina_case(oracle, rng, N=2, A=3, Cn=5, shapes=((16, 20), (8, 10), (4, 5)), strides=(8, 16, 32), ld=64, nobj=6):
    """The 3-level, 3-anchor x 5-class geometry of test_retina_detect_bit_exact with bf16-valued logits; per image `nobj`
    objects (level, cell, class) raise the class logit of every anchor in the 3x3 cells around them, so clusters of
    neighbouring anchors of one class score high. Returns (cls [l][N,H,W,ld], reg [l][N,H,W,ld], base, info)."""
    base = [oracle.base_anchors(s) for s in strides]
    cls, reg = [], []
    for (H, W) in shapes:
        cls.append((rng.standard_normal((N, H, W, ld)) * 1.0 - 4.0).astype(np.float32))
        reg.append((rng.standard_normal((N, H, W, ld)) * 0.1).astype(np.float32))
    for n in range(N):
        for _ in range(nobj):
            l = int(rng.integers(0, len(shapes)))
            H, W = shapes[l]
            y, x, c = int(rng.integers(1, H - 1)), int(rng.integers(1, W - 1)), int(rng.integers(0, Cn))
            for a in range(A):
                cls[l][n, y - 1:y + 2, x - 1:x + 2, a * Cn + c] += rng.uniform(3.0, 6.0, (3, 3)).astype(np.float32)
    cls = [oracle.round_bf16(c) for c in cls]
    reg = [oracle.round_bf16(r) for r in reg]
    info = np.array([[128, 160, 1.0], [120, 150, 1.0]], np.float32)[:N]
    return cls, reg, base, info


def non_degenerate(dets, num, orig, hard_dets, hard_num):
    """Per image (rows whose score Soft-NMS changed, rows whose (box, class) the hard result does not have)."""
    out = []
    for n in range(dets.shape[0]):
        k = int(num[n])
        hard = {(tuple(r[:4]), r[5]) for r in hard_dets[n, :int(hard_num[n])].tolist()}
        decayed = int(np.sum(dets[n, :k, 4].view(np.uint32) != orig[n, :k].view(np.uint32)))
        absent = sum(1 for r in dets[n, :k].tolist() if (tuple(r[:4]), r[5]) not in hard)
        out.append((decayed, absent))
    return out
