"""Reference and inputs of the Mask Scoring R-CNN tests (tests/test_mask_iou_cpu.py, tests/test_gpu_mask_iou.py,
tests/test_gpu_mask_iou_model.py); not collected.

A numpy-float32 restatement of the conventions of DESIGN.md 5n / include/mxdet.h (mxdet_maskiou_*): one fp32 operation per
step in the order written, exp through the C oracle (`oracle.expf`: the kernels' bits), bf16 rounding through
`oracle.f32_to_bf16_bits`. It lives here because oracle/ is frozen.
"""
import numpy as np

CIN = 320       # MaskIoU head input channels (mxdetection_amd.core.mask.MASKIOU_CIN)
f32 = np.float32


def ellipse_masks(gt, H, W):
    """[N,G,H,W] u8: a filled axis-aligned ellipse inside every valid GT box (as tests/test_gpu_mask.py)."""
    N, G = gt.shape[:2]
    m = np.zeros((N, G, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for n in range(N):
        for g in range(G):
            if gt[n, g, 4] < 0:
                continue
            x1, y1, x2, y2 = gt[n, g, :4]
            cx, cy, rx, ry = 0.5 * (x1 + x2), 0.5 * (y1 + y2), 0.5 * (x2 - x1) + 0.5, 0.5 * (y2 - y1) + 0.5
            m[n, g] = (((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0).astype(np.uint8)
    return m


def target_counts(rois, matched, cls, gt_boxes, gt_masks, logits, targets):
    """The five integer counts per roi, or None for rows that give 0 without reading a mask:
    list of (a_full, a_in, a_pred, a_tgt, a_ovr)."""
    N, G, H, W = gt_masks.shape
    R, S, _, Cpad = logits.shape
    out = []
    for r in range(R):
        c, g, n = int(cls[r]), int(matched[r]), int(rois[r, 0])
        if c <= 0 or c > Cpad or g < 0 or g >= G or n < 0 or n >= N:
            out.append(None)
            continue
        m = gt_masks[n, g] != 0
        a_full = int(m.sum()) if gt_boxes[n, g, 4] >= 0 else 0         # padding instances are never read
        x1, y1, x2, y2 = (float(v) for v in rois[r, 1:5])
        ix1, iy1 = max(0, int(np.floor(x1))), max(0, int(np.floor(y1)))
        ix2, iy2 = min(W - 1, int(np.ceil(x2))), min(H - 1, int(np.ceil(y2)))
        a_in = int(m[iy1:iy2 + 1, ix1:ix2 + 1].sum()) if (ix1 <= ix2 and iy1 <= iy2) else 0
        pred = logits[r, :, :, c - 1] > 0
        tg = targets[r] != 0
        out.append((a_full, a_in, int(pred.sum()), int(tg.sum()), int((pred & tg).sum())))
    return out


def maskiou_target(rois, matched, cls, gt_boxes, gt_masks, logits, targets):
    """Convention 1. logits: fp32 array of bf16-representable values [R,S,S,Cpad]. Returns f32 [R]."""
    t = np.zeros((len(cls),), f32)
    for r, cnt in enumerate(target_counts(rois, matched, cls, gt_boxes, gt_masks, logits, targets)):
        if cnt is None or cnt[1] == 0:
            continue
        a_full, a_in, a_pred, a_tgt, a_ovr = cnt
        gt_s = f32(f32(a_tgt) * f32(a_full)) / f32(a_in)
        uni = f32(f32(f32(a_pred) + gt_s) - f32(a_ovr))
        t[r] = f32(a_ovr) / np.maximum(uni, f32(1e-7))
    return t


def sigmoid(oracle, z):
    """The kernels' sigmoid: z >= 0 ? 1/(1+e^-z) : e^z/(1+e^z), fp32, unfused, exp = oracle.expf."""
    z = np.ascontiguousarray(z, f32)
    one = f32(1.0)
    en = oracle.expf((-np.abs(z)).astype(f32)).astype(f32)       # e^-|z|: e^-z for z >= 0, e^z for z < 0
    return np.where(z >= 0, one / (one + en), en / (one + en)).astype(f32)


def maskiou_input(oracle, mpooled, logits, cls, cin=CIN):
    """Convention 2. mpooled [R,h,h,C], logits [R,2h,2h,Cpad]: fp32 arrays of bf16-representable values.
    Returns the bf16 BITS (uint16) of the head input [R,h,h,cin]."""
    R, h, _, C = mpooled.shape
    Cpad = logits.shape[3]
    out = np.zeros((R, h, h, cin), np.uint16)
    out[..., :C] = oracle.f32_to_bf16_bits(mpooled)
    for r in range(R):
        c = int(cls[r])
        if c <= 0 or c > Cpad:
            continue
        ch = logits[r, :, :, c - 1]
        z = np.maximum(np.maximum(ch[0::2, 0::2], ch[0::2, 1::2]), np.maximum(ch[1::2, 0::2], ch[1::2, 1::2]))
        out[r, :, :, C] = oracle.f32_to_bf16_bits(sigmoid(oracle, z))
    return out


def maskiou_loss(oracle, pred, cls, t, loss_scale=1.0, weight=1.0):
    """Convention 4. pred: fp32 array of bf16-representable values [R,ld]. Returns (loss float64 -- the exact sum the fp32
    fixed-order kernel approximates --, grad bf16 bits [R,ld])."""
    R, ld = pred.shape
    pos = [r for r in range(R) if 0 < cls[r] <= ld and t[r] > 0]
    k = f32(f32(loss_scale) * f32(weight)) / f32(max(len(pos), 1))
    grad = np.zeros((R, ld), f32)
    acc = 0.0
    for r in pos:
        d = f32(f32(pred[r, cls[r] - 1]) - f32(t[r]))
        acc += 0.5 * (float(pred[r, cls[r] - 1]) - float(t[r])) ** 2
        grad[r, cls[r] - 1] = f32(d * k)
    return float(loss_scale) * float(weight) / max(len(pos), 1) * acc, oracle.f32_to_bf16_bits(grad)


def maskiou_score(dets, pred):
    """Convention 6. dets [R,6] f32, pred fp32 array of bf16-representable values [R,ld]. Returns f32 [R]."""
    R, ld = pred.shape
    s = np.zeros((R,), f32)
    for r in range(R):
        c = int(dets[r, 5])
        if 0 < c <= ld:
            s[r] = f32(dets[r, 4]) * f32(pred[r, c - 1])
    return s
