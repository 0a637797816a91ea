"""References of the quality-aware class losses (QFL / Varifocal; DESIGN.md 5j, include/mxdet.h). No tests here.

  * float64 torch autograd on the definition: the decode is that of tests/test_iou_loss_cases_cpu.py (_decode64, absolute
    coordinates, torch.exp), the quality q = inter / union is DETACHED (a constant of the class loss), QFL's modulating
    factor is abs().pow(beta), and torch.maximum / torch.minimum are the only selection functions (the y > 0 / y == 0 split
    of the Varifocal loss is a 0/1 mask that multiplies; nothing from include/mxdet_math.h).
  * numpy float32 restatements in the kernel's operation order (quality_fp32 = the inter / union of box_iou_loss_elem,
    cls_elem_fp32 = quality_cls_elem), oracle.expf / oracle.logf: CPU stand-ins that measure the float32 error, never
    references.
"""
import numpy as np

import test_iou_loss_cases_cpu as T

KINDS = ("qfl", "vfl")


def O():
    return T.O()


# ---------------------------------------------------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------------------------------------------------
def quality64(b, g, d, stds):
    """inter / union [n] (float64 numpy, no gradient) of boxes b decoded by raw deltas d against ground truth g."""
    import torch
    with torch.no_grad():
        b, g, d = T._t64(b), T._t64(g), T._t64(d)
        zero = torch.zeros((), dtype=torch.float64)
        ax = T._decode64(b, d, stds)
        il, gl = [], []
        for k, (pc, pl, p1, p2, _) in enumerate(ax):
            g1, g2 = g[:, k], g[:, 2 + k]
            il.append(torch.maximum(torch.minimum(p2, g2) - torch.maximum(p1, g1) + 1.0, zero))
            gl.append(g2 - g1 + 1.0)
        inter = il[0] * il[1]
        union = ax[0][1] * ax[1][1] + gl[0] * gl[1] - inter
        return (inter / union).numpy()


def cls_elems64(z, y, cls_loss, alpha, gamma):
    """Per-element loss (float64 tensor like z) of logits z against targets y (a float64 tensor WITHOUT gradient)."""
    import torch
    import torch.nn.functional as F
    assert not y.requires_grad
    lp, ln = F.logsigmoid(z), F.logsigmoid(-z)                     # log s, log(1 - s)
    s = torch.sigmoid(z)
    bce = -y * lp - (1.0 - y) * ln
    if cls_loss == "qfl":
        return (y - s).abs().pow(gamma) * bce
    assert cls_loss == "vfl"
    pos = (y > 0).to(z.dtype)
    return pos * (y * bce) + (1.0 - pos) * (-alpha * s.pow(gamma) * ln)


def ref_elems(x, y, cls_loss, alpha, gamma):
    """(L, dL/dx) float64 numpy, elementwise."""
    z = T._t64(x, True)
    L = cls_elems64(z, T._t64(y), cls_loss, alpha, gamma)
    L.sum().backward()
    return L.detach().numpy(), z.grad.numpy()


def targets64(lab, q, Cc):
    """y [..., Cc] float64: q in column lab - 1 of rows with lab > 0, else 0; valid [..., 1] = (lab >= 0)."""
    lab = np.asarray(lab, np.int64)
    onehot = lab[..., None] == np.arange(1, Cc + 1)
    return onehot * np.asarray(q, np.float64)[..., None], (lab >= 0)[..., None].astype(np.float64)


def ref_primitive(logits, labels, quality, cls_loss, alpha, gamma, grad_scale):
    """mxdet_quality_focal_loss: loss = sum / max(1, #labels > 0); grad = d loss / d logits * grad_scale."""
    n, Cc = np.shape(logits)
    y, valid = targets64(labels, quality, Cc)
    L, G = ref_elems(logits, y, cls_loss, alpha, gamma)
    inv = 1.0 / max(1, int((np.asarray(labels) > 0).sum()))
    return {"loss": float((L * valid).sum()) * inv, "grad": G * valid * inv * grad_scale, "unit": inv * grad_scale,
            "per_row": (L * valid).sum(axis=1)}


def level_quality(reg, A, cls_labels, anchors, matched, gt_boxes, level_offset, stds, fn):
    """q [N, n_lvl] of one level by fn (quality64 or quality_fp32): 0 for background, ignore and out-of-range matches."""
    N, H, W, _ = reg.shape
    n_lvl, G = H * W * A, np.shape(gt_boxes)[1]
    lab = np.asarray(cls_labels)[:, level_offset:level_offset + n_lvl]
    m = np.asarray(matched)[:, level_offset:level_offset + n_lvl]
    n_i, a_i = np.nonzero((lab > 0) & (m >= 0) & (m < G))
    q = np.zeros((N, n_lvl), np.float64 if fn is quality64 else np.float32)
    if len(n_i):
        d = np.asarray(reg)[..., :4 * A].reshape(N, n_lvl, 4)[n_i, a_i]
        q[n_i, a_i] = fn(np.asarray(anchors)[level_offset + a_i], np.asarray(gt_boxes)[n_i, m[n_i, a_i], :4], d, stds)
    return lab, q


def ref_retina_quality(cls, reg, A, Cc, cls_labels, anchors, matched, gt_boxes, level_offset, cls_loss, alpha, gamma, stds,
                       num_fg, loss_scale):
    """The class half of mxdet_retina_loss_level_quality in float64 (the box half is the IoU entry's, bit for bit):
    loss, grad_cls [N,H,W,ld] (zeros in the padding), per_anchor [N,n_lvl] class loss before normalisation, q, unit."""
    N, H, W, ld = cls.shape
    n_lvl = H * W * A
    lab, q = level_quality(reg, A, cls_labels, anchors, matched, gt_boxes, level_offset, stds, quality64)
    y, valid = targets64(lab, q, Cc)
    x = np.asarray(cls, np.float64)[..., :A * Cc].reshape(N, n_lvl, Cc)
    L, G = ref_elems(x, y, cls_loss, alpha, gamma)
    inv = 1.0 / max(1, int(num_fg))
    grad = np.zeros(cls.shape)
    grad[..., :A * Cc] = (G * valid * inv * loss_scale).reshape(N, H, W, A * Cc)
    per_anchor = (L * valid).sum(axis=2)
    return {"loss": float(per_anchor.sum()) * inv, "grad_cls": grad, "per_anchor": per_anchor, "q": q, "unit": inv * loss_scale,
            "n_valid": int((lab >= 0).sum())}


# ---------------------------------------------------------------------------------------------------------------------
# float32 restatements
# ---------------------------------------------------------------------------------------------------------------------
def quality_fp32(b, g, d, stds):
    """inter / uni [n] float32 in the operation order of box_iou_loss_elem (corner-relative, oracle.expf)."""
    f = np.float32
    b, g, d = np.asarray(b, f), np.asarray(g, f), np.asarray(d, f)
    one, half, clip = f(1.0), f(0.5), f(T.CLIP)
    pl, gl, il = [None, None], [None, None], [None, None]
    for k in (0, 1):
        g1, g2 = g[:, k] - b[:, k], g[:, 2 + k] - b[:, k]
        ln = b[:, 2 + k] - b[:, k] + one
        c0 = half * (ln - one)
        t = np.minimum(d[:, 2 + k] * f(stds[2 + k]), clip)
        pc = d[:, k] * f(stds[k]) * ln + c0
        pl[k] = T._expf32(t) * ln
        hl = half * (pl[k] - one)
        p1, p2 = pc - hl, pc + hl
        gl[k] = g2 - g1 + one
        il[k] = np.maximum(np.minimum(p2, g2) - np.maximum(p1, g1) + one, f(0.0))
    inter = il[0] * il[1]
    uni = pl[0] * pl[1] + gl[0] * gl[1] - inter
    out = inter / uni
    assert out.dtype == f
    return out


def _u(fn, x):
    u, inv = np.unique(np.asarray(x, np.float32), return_inverse=True)
    return fn(u)[inv].reshape(np.shape(x)).astype(np.float32)


def cls_elem_fp32(x, y, cls_loss, alpha, gamma):
    """(L, dL/dx) float32 per element, operation for operation what quality_cls_elem does."""
    o, f = O(), np.float32
    x, y = np.asarray(x, f), np.asarray(y, f)
    one = f(1.0)
    t = _u(o.expf, -np.abs(x))
    d = one + t
    dm1 = d - one
    sp = np.where(dm1 == 0, t, _u(o.logf, d) * (t / np.where(dm1 == 0, one, dm1))).astype(f)
    big, small = one / d, t / d
    p, q = np.where(x >= 0, big, small).astype(f), np.where(x >= 0, small, big).astype(f)
    logp = -(np.where(x < 0, -x, f(0.0)).astype(f) + sp)
    log1mp = -(np.where(x > 0, x, f(0.0)).astype(f) + sp)
    al, ga = f(alpha), f(gamma)
    bce = -y * logp - (one - y) * log1mp
    if cls_loss == "qfl":
        e = p - y
        if gamma == 2.0:
            mod, dmod = e * e, f(2.0) * e
        else:
            aec = np.maximum(np.abs(e), f(1e-30))
            mod = _u(o.expf, ga * _u(o.logf, aec))
            dmod = ga * (mod / aec)
            dmod = np.where(e < 0, -dmod, dmod).astype(f)
        L, G = mod * bce, dmod * (p * q) * bce + mod * e
    else:
        assert cls_loss == "vfl"
        mod = p * p if gamma == 2.0 else _u(o.expf, ga * _u(o.logf, np.maximum(p, f(1e-30))))
        L = np.where(y > 0, y * bce, -al * mod * log1mp)
        G = np.where(y > 0, y * (p - y), al * (ga * mod * q * (-log1mp) + mod * p))
    assert L.dtype == f and G.dtype == f
    return L, G


def retina_quality_fp32(cls, reg, A, Cc, cls_labels, anchors, matched, gt_boxes, level_offset, cls_loss, alpha, gamma, stds):
    """(per-anchor class loss [N,n_lvl], dL/dx [N,n_lvl,Cc]) float32, before normalisation; class columns summed in order."""
    N, H, W, ld = cls.shape
    n_lvl = H * W * A
    lab, q = level_quality(reg, A, cls_labels, anchors, matched, gt_boxes, level_offset, stds, quality_fp32)
    y, valid = targets64(lab, q, Cc)
    x = np.asarray(cls, np.float32)[..., :A * Cc].reshape(N, n_lvl, Cc)
    L, G = cls_elem_fp32(x, y.astype(np.float32), cls_loss, alpha, gamma)
    L, G = L * valid.astype(np.float32), G * valid.astype(np.float32)
    acc = np.zeros((N, n_lvl), np.float32)
    for c in range(Cc):
        acc = acc + L[..., c]
    return acc, G
