"""Reference and inputs of the Keypoint R-CNN tests (tests/test_keypoint_cpu.py, tests/test_gpu_keypoint.py,
tests/test_gpu_keypoint_model.py); not collected.

A numpy restatement of the conventions of DESIGN.md 3 / 5p / include/mxdet.h (mxdet_keypoint_*). It lives here because
oracle/ is frozen.

Conventions
  gt_keypoints  fp32 [N,G,K,3] = (x, y, v) in the frame of the network input; v > 0 = labelled; padding instances all zero.
  logits        bf16 [R,S_in,S_in,Kpad], channels [K,Kpad) padding. S = 2*S_in.
  upsample      U [S,S] of one channel, half-pixel centres, edge replication, separable, horizontal first:
                h[i][2j+p] = 0.75f*in[i][j] + 0.25f*in[i][clamp(j-1+2p)], U[2i+q][X] = 0.75f*h[i][X] + 0.25f*h[clamp(i-1+2q)][X];
                each product and sum one unfused fp32 operation.
  target        int32 [R,K]: n = (int)rois[r,0], g = matched[r]; rows with label <= 0, g outside [0,G) or n outside [0,N)
                give -1. rw = max(x2-x1, 1), bx = S-1 if kx == x2 else (int)floor((kx-x1) * (S/rw)), by alike;
                by*S+bx when v > 0 and both bins are inside [0,S), else -1.
  loss          k = (loss_scale*weight) / max(n_valid, 1); loss = k * sum_valid CE(softmax over U, target);
                grad = ((softmax - onehot) * k) through the adjoint of the upsample, bf16, zeros elsewhere.
  decode        argmax of U (lowest index on ties) = (by,bx); x = x1 + (bx + 0.5f) * (rw / S), y alike; score = max U;
                rows of dets with class <= 0 give zeros.

float32 (bit-exact with the kernels) for the target, the upsample and the decode; float64 for the loss and its gradient.
`keypoint_loss_f32` is the float32 restatement of the kernel's formula (exp / log through the C oracle): the CPU test
measures it against the float64 reference to set the GPU test's gradient tolerance.
"""
import numpy as np

f32 = np.float32
SHAPES = [(28, 32, 17), (14, 32, 17), (7, 8, 5), (28, 24, 1)]      # (S_in, Kpad, K) of the GPU table
R_CASE = 37
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
COCO_FLIP_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))


def _nbr(n):
    """For output index X = 2j+p of an n -> 2n upsample: (j, clamp(j-1+2p))."""
    X = np.arange(2 * n)
    j = X >> 1
    return j, np.clip(j - 1 + 2 * (X & 1), 0, n - 1)


def upsample2(x):
    """float32 [..., S_in, S_in] -> [..., S, S], one fp32 operation per step in the order of the convention."""
    x = np.asarray(x, f32)
    n = x.shape[-1]
    j, jn = _nbr(n)
    h = (f32(0.75) * x[..., :, j]).astype(f32) + (f32(0.25) * x[..., :, jn]).astype(f32)
    h = h.astype(f32)
    i, inn = _nbr(x.shape[-2])
    return ((f32(0.75) * h[..., i, :]).astype(f32) + (f32(0.25) * h[..., inn, :]).astype(f32)).astype(f32)


def upsample_matrix(n):
    """A [2n, n] float64 with U = A @ x @ A.T."""
    A = np.zeros((2 * n, n))
    j, jn = _nbr(n)
    for X in range(2 * n):
        A[X, j[X]] += 0.75
        A[X, jn[X]] += 0.25
    return A


def keypoint_target(rois, matched, labels, gt_kp, S_in):
    N, G, K, _ = gt_kp.shape
    R = rois.shape[0]
    S = 2 * S_in
    out = -np.ones((R, K), np.int32)
    for r in range(R):
        n, g = int(rois[r, 0]), int(matched[r])
        if labels[r] <= 0 or g < 0 or g >= G or n < 0 or n >= N:
            continue
        x1, y1, x2, y2 = (f32(v) for v in rois[r, 1:5])
        rw, rh = np.maximum(f32(x2 - x1), f32(1.0)), np.maximum(f32(y2 - y1), f32(1.0))
        for j in range(K):
            kx, ky, v = (f32(t) for t in gt_kp[n, g, j])
            if not v > 0:
                continue
            bx = float(S - 1) if kx == x2 else float(np.floor(f32(f32(kx - x1) * f32(f32(S) / rw))))
            by = float(S - 1) if ky == y2 else float(np.floor(f32(f32(ky - y1) * f32(f32(S) / rh))))
            if 0 <= bx < S and 0 <= by < S:
                out[r, j] = int(by) * S + int(bx)
    return out


def _k(targets, SS, loss_scale, weight):
    nv = int(((targets >= 0) & (targets < SS)).sum())
    return nv, f32(f32(loss_scale) * f32(weight)) / f32(max(nv, 1))


def keypoint_loss(logits, targets, loss_scale=1.0, weight=1.0):
    """float64. logits: fp32 array of bf16-representable values [R,S_in,S_in,Kpad]; targets int32 [R,K].
    Returns (loss, grad float64 [R,S_in,S_in,Kpad] -- unrounded --, k float)."""
    R, S_in, _, Kpad = logits.shape
    K = targets.shape[1]
    S = 2 * S_in
    nv, k = _k(targets, S * S, loss_scale, weight)
    k = float(k)
    A = upsample_matrix(S_in)
    grad = np.zeros(logits.shape, np.float64)
    total = 0.0
    for r in range(R):
        for j in range(K):
            t = int(targets[r, j])
            if t < 0 or t >= S * S:
                continue
            U = upsample2(logits[r, :, :, j]).astype(np.float64)      # the fp32 map is the softmax's input by convention
            m = U.max()
            e = np.exp(U - m)
            s = e.sum()
            total += np.log(s) - (U.flat[t] - m)
            q = e / s
            q.flat[t] -= 1.0
            grad[r, :, :, j] = A.T @ (q * k) @ A
    return k * total, grad, k


def keypoint_loss_f32(oracle, logits, targets, loss_scale=1.0, weight=1.0):
    """The kernel's formula in float32 (mxdet_expf / mxdet_logf through the oracle; the adjoint's taps in the kernel's
    order). Returns (loss f32, grad f32 [R,S_in,S_in,Kpad] before the bf16 rounding)."""
    R, S_in, _, Kpad = logits.shape
    K = targets.shape[1]
    S = 2 * S_in
    nv, k = _k(targets, S * S, loss_scale, weight)
    grad = np.zeros(logits.shape, f32)
    w = (f32(0.25), f32(0.75), f32(0.75), f32(0.25))
    idx = [np.clip(2 * np.arange(S_in) - 1 + t, 0, S - 1) for t in range(4)]
    total = f32(0.0)
    for r in range(R):
        acc = f32(0.0)
        for j in range(K):
            t = int(targets[r, j])
            if t < 0 or t >= S * S:
                continue
            U = upsample2(logits[r, :, :, j])
            m = U.max()
            e = oracle.expf((U - m).astype(f32))
            s = e.sum(dtype=f32)          # fp32; the kernel's order differs (per thread, per wave, across waves)
            acc = f32(acc + f32(oracle.logf(s) - f32(U.flat[t] - m)))
            q = (e / s).astype(f32)
            q.flat[t] = f32(q.flat[t] - f32(1.0))
            q = (q * k).astype(f32)
            cols = []
            for tx in range(4):
                c = (w[0] * q[idx[0]][:, idx[tx]]).astype(f32)
                for sy in range(1, 4):
                    c = (c + (w[sy] * q[idx[sy]][:, idx[tx]]).astype(f32)).astype(f32)
                cols.append(c)
            g = (w[0] * cols[0]).astype(f32)
            for tx in range(1, 4):
                g = (g + (w[tx] * cols[tx]).astype(f32)).astype(f32)
            grad[r, :, :, j] = g
        total = f32(total + acc)
    return f32(k * total), grad


def keypoint_decode(logits, dets, K):
    """float32, bit-exact. logits fp32 array of bf16-representable values [R,S_in,S_in,Kpad], dets [R,6] -> [R,K,3]."""
    R, S_in = logits.shape[:2]
    S = 2 * S_in
    out = np.zeros((R, K, 3), f32)
    for r in range(R):
        if int(dets[r, 5]) <= 0:
            continue
        x1, y1, x2, y2 = (f32(v) for v in dets[r, :4])
        rw, rh = np.maximum(f32(x2 - x1), f32(1.0)), np.maximum(f32(y2 - y1), f32(1.0))
        U = upsample2(np.moveaxis(logits[r, :, :, :K], -1, 0))
        for j in range(K):
            b = int(np.argmax(U[j]))                     # the first occurrence: the lowest linear index
            by, bx = divmod(b, S)
            out[r, j, 0] = f32(x1 + f32(f32(f32(bx) + f32(0.5)) * f32(rw / f32(S))))
            out[r, j, 1] = f32(y1 + f32(f32(f32(by) + f32(0.5)) * f32(rh / f32(S))))
            out[r, j, 2] = U[j].flat[b]
    return out


def flip_keypoints(kp, width, pairs=COCO_FLIP_PAIRS):
    """The flip of process_data.transform.transform_keypoints in plain numpy: x' = w - 1 - x, pairs swapped, v = 0 rows zero."""
    out = np.array(kp, f32, copy=True)
    out[..., 0] = f32(width - 1) - out[..., 0]
    for a, b in pairs:
        if b < out.shape[-2]:
            out[..., [a, b], :] = out[..., [b, a], :]
    out[out[..., 2] <= 0] = 0
    return out


# ---- the GPU table's rows (shared by the CPU tolerance measurement and the GPU tests) -----------------------------------
def _place(roi, bx, by, S):
    """A keypoint in the middle of bin (by, bx) of the roi's S x S grid."""
    x1, y1, x2, y2 = roi
    rw, rh = max(x2 - x1, 1.0), max(y2 - y1, 1.0)
    return x1 + (bx + 0.5) * rw / S, y1 + (by + 0.5) * rh / S


def case(oracle, S_in, Kpad, K, seed=41):
    """R_CASE hand-placed rows, each with a ground-truth instance of its own (image r % 2, instance r // 2).
    Returns dict(rois, matched, labels, gt_kp, logits (fp32, bf16-representable), dets, targets (the reference's))."""
    rng = np.random.default_rng(seed + S_in + K)
    R, N, G, S = R_CASE, 2, (R_CASE + 1) // 2, 2 * S_in
    rois = np.zeros((R, 5), f32)
    matched = np.zeros((R,), np.int32)
    labels = np.ones((R,), np.int32)
    gt_kp = np.zeros((N, G, K, 3), f32)
    logits = (rng.standard_normal((R, S_in, S_in, Kpad)) * 3).astype(f32)
    corners = [(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)]
    for r in range(R):
        n, g = r % 2, r // 2
        x1, y1 = rng.uniform(0, 60), rng.uniform(0, 40)
        roi = (f32(x1), f32(y1), f32(x1 + rng.uniform(30, 120)), f32(y1 + rng.uniform(30, 100)))
        rois[r] = (n,) + roi
        matched[r] = g
        labels[r] = 1 + r % 3
        roi = tuple(float(v) for v in roi)
        for j in range(K):
            if r < 4:                                   # the four corners (clamped taps in both directions)
                by, bx = corners[(j + r) % 4]
            elif r < 8:                                 # the four edges
                mid = 1 + (3 * j + r) % (S - 2)
                by, bx = [(0, mid), (mid, 0), (S - 1, mid), (mid, S - 1)][(j + r) % 4]
            else:
                by, bx = int(rng.integers(0, S)), int(rng.integers(0, S))
            kx, ky = _place(roi, bx, by, S)
            gt_kp[n, g, j] = (kx, ky, 1 + (j + r) % 2)
    for j in range(K):
        gt_kp[0, 4, j, :2] = rois[8, 3:5]                                   # row 8: exactly on x2 / y2 -> bin S-1
        gt_kp[1, 4, j, 0] = rois[9, 3] + (1.0 if j % 2 == 0 else -1.0)      # row 9: one pixel outside / inside
    gt_kp[0, 5, :, 2] = 0                                                   # row 10: fg roi, nothing labelled
    rois[11, 3] = rois[11, 1]                                               # row 11: one pixel wide (rw = 1)
    gt_kp[1, 5, :, 0] = rois[11, 1] + (np.arange(K) % 2) * f32(0.25)        # on x2 (-> S-1) or a quarter pixel in
    matched[12] = -1                                                        # row 12: fg label, unmatched
    labels[13] = 0                                                          # row 13: background label
    for r in (14, 15, 16):                                                  # padding rows
        rois[r], matched[r], labels[r] = 0, -1, -1
    logits[17] = np.where((np.indices((S_in, S_in)).sum(0) % 2 == 0)[..., None], f32(60.0), f32(-60.0))   # row 17: +-60
    logits[18] = f32(0.5)                                                   # row 18: a constant map (argmax tie)
    rois[19, 0] = 5                                                         # row 19: image index past N
    matched[20] = G                                                         # row 20: instance index past G
    gt_kp[1, 11, :, 2] = np.arange(K) % 3 == 0                              # row 23: some labelled, some not
    gt_kp[0, 12, :, :2] += 400                                              # row 24: far outside its roi
    logits = oracle.round_bf16(logits)
    dets = np.zeros((R, 6), f32)
    dets[:, :4] = rois[:, 1:]
    dets[:, 4] = rng.uniform(0.1, 1.0, R)
    dets[:, 5] = labels
    targets = keypoint_target(rois, matched, labels, gt_kp, S_in)
    return dict(rois=rois, matched=matched, labels=labels, gt_kp=gt_kp, logits=logits, dets=dets, targets=targets)
