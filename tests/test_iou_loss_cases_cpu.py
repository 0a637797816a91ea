"""Case tables, float64 references and CPU proofs of the IoU / GIoU / DIoU box losses (mxdet_box_iou_loss, mxdet_rcnn_loss_iou,
mxdet_retina_loss_level_iou in csrc/losses.hip / retina_loss.hip). tests/test_gpu_iou_loss.py runs the same tables on the GPU.

References: float64 torch autograd on the definition of DESIGN.md 5f written in ABSOLUTE image coordinates with torch.exp,
torch.maximum and torch.minimum (whose gradient at an exact tie is 1/2 to each side: test_torch_maximum_splits_a_tie);
nothing from include/mxdet_math.h. Layout as in tests/test_loss_cases_cpu.py:
  loss  float64, as the entry reports it          grads  d(loss)/d(input) * loss_scale, zeros where the entry writes zeros
  unit  norm * loss_scale (the class half) and unit_reg = reg_weight * unit (the box half): gradients are compared after
        division by it, i.e. on the scale of dL / d(raw delta) of one box.

Every row of every table that is not a named tie case lies at least MARGIN = 2^-10 px from every max / min branch, from
rw = 0 and rh = 0, and 2^-10 from the dw / dh clamp, measured on the float64 reference (the generator redraws the deltas
until it does; test_every_row_keeps_the_branch_margin asserts it), so no row is skipped at comparison time. The tie cases
use integer-valued boxes and zero deltas: the tie is exact in fp32 and in fp64.

Tolerances (test_fp32_error_budget measures and bounds them): iou_loss_fp32 -- numpy float32, the corner-relative
operation order of box_iou_loss_elem, oracle.expf -- against the float64 reference over every table row plus 100 000
seeded random rows (boxes 2..800 px at coordinates <= 1333, bf16-exact deltas, the branch margin), all three kinds; the
bound is the largest difference times 4, rounded up to a power of two.
                                     measured       bound
  gradient, stds (0.1,0.1,0.2,0.2)   1.03e-7       ATOL_GRAD["head"] = 2^-21
  gradient, stds (1,1,1,1)           1.03e-6       ATOL_GRAD["unit"] = 2^-17
  per-box loss                       3.85e-7       ATOL_LOSS         = 2^-19
bf16 outputs add 2^-8 * |ref|. Summed losses: LOSS_RTOL = 3e-5 of the float64 sum on top of ATOL_LOSS per summed box.
The textbook form (the same formulas in absolute coordinates, float32) misses the gradient bound on the tiny_far case by
orders of magnitude: test_textbook_form_misses_the_bound_on_tiny_far keeps anybody from simplifying the kernel back.
"""
import ctypes as C
import functools
import math
import os
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("iou", "giou", "diou")
STDS = {"head": (0.1, 0.1, 0.2, 0.2), "unit": (1.0, 1.0, 1.0, 1.0)}
CLIP = math.log(1000.0 / 16.0)
MARGIN = 2.0 ** -10
MEASURED = {"head": 1.0333e-07, "unit": 1.0273e-06, "loss": 3.8498e-07}       # the figures of the docstring, in full
ATOL_GRAD = {"head": 2.0 ** -21, "unit": 2.0 ** -17}
ATOL_LOSS = 2.0 ** -19
BF16_STEP = 2.0 ** -8
LOSS_RTOL = 3e-5
N_RANDOM = 100000


def O():
    from oracle import oracle as o
    o.lib()
    return o


def bf16r(x):
    return O().round_bf16(np.asarray(x, np.float32))


def _t64(a, grad=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    return t.requires_grad_(True) if grad else t


def ids(cases):
    return [c["id"] for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference (torch autograd, absolute coordinates)
# ---------------------------------------------------------------------------------------------------------------------
def _decode64(b, d, stds):
    import torch
    clip = torch.tensor(CLIP, dtype=torch.float64)
    out = []
    for k in (0, 1):
        ln = b[:, 2 + k] - b[:, k] + 1.0
        c = b[:, k] + 0.5 * (ln - 1.0)
        t = d[:, 2 + k] * stds[2 + k]
        pc = d[:, k] * stds[k] * ln + c
        pl = torch.exp(torch.minimum(t, clip)) * ln
        out.append((pc, pl, pc - 0.5 * (pl - 1.0), pc + 0.5 * (pl - 1.0), t))
    return out


def iou_loss64(b, g, d, stds, kind):
    """L [n] float64 tensor of boxes b, ground truth g, raw deltas d (float64 tensors [n,4])."""
    import torch
    zero = torch.zeros((), dtype=torch.float64)
    ax = _decode64(b, d, stds)
    il, cl, gl, e2 = [], [], [], 0.0
    for k, (pc, pl, p1, p2, _) in enumerate(ax):
        g1, g2 = g[:, k], g[:, 2 + k]
        r = torch.minimum(p2, g2) - torch.maximum(p1, g1) + 1.0
        il.append(torch.maximum(r, zero))
        cl.append(torch.maximum(p2, g2) - torch.minimum(p1, g1) + 1.0)
        gl.append(g2 - g1 + 1.0)
        e2 = e2 + (pc - (g1 + 0.5 * (gl[k] - 1.0))) ** 2
    inter = il[0] * il[1]
    union = ax[0][1] * ax[1][1] + gl[0] * gl[1] - inter
    L = 1.0 - inter / union
    if kind == "giou":
        L = L + (cl[0] * cl[1] - union) / (cl[0] * cl[1])
    elif kind == "diou":
        L = L + e2 / (cl[0] ** 2 + cl[1] ** 2)
    else:
        assert kind == "iou"
    return L


def branch_margin(b, g, d, stds):
    """Smallest distance [n] of a row from a max / min tie, from rw = 0 / rh = 0 (px) and from the clamp, in float64."""
    import torch
    with torch.no_grad():
        b, g, d = _t64(b), _t64(g), _t64(d)
        m = torch.full((b.shape[0],), np.inf, dtype=torch.float64)
        for k, (pc, pl, p1, p2, t) in enumerate(_decode64(b, d, stds)):
            g1, g2 = g[:, k], g[:, 2 + k]
            r = torch.minimum(p2, g2) - torch.maximum(p1, g1) + 1.0
            for v in (p1 - g1, p2 - g2, r, t - CLIP):
                m = torch.minimum(m, v.abs())
    return m.numpy()


def ref_rows(b, g, d, stds, kind):
    """(L [n], dL/dd [n,4]) in float64."""
    dd = _t64(d, True)
    L = iou_loss64(_t64(b), _t64(g), dd, stds, kind)
    L.sum().backward()
    return L.detach().numpy(), dd.grad.numpy()


def ref_box_iou_loss(b, g, d, w, stds, kind, grad_scale):
    L, G = ref_rows(b, g, d, stds, kind)
    ww = np.ones(len(L)) if w is None else np.asarray(w, np.float64)
    return {"loss": L * ww, "grad": G * ww[:, None] * grad_scale, "unit": grad_scale}


def _ref_cls_rcnn(cls, labels, nc, norm, loss_scale):
    import torch
    import torch.nn.functional as F
    z = _t64(np.asarray(cls)[:, :nc], True)
    lab = torch.from_numpy(np.asarray(labels, np.int64))
    valid = lab >= 0
    lc = F.cross_entropy(z[valid], lab[valid], reduction="sum") * norm
    (lc + 0.0 * z.sum()).backward()
    return lc.item(), z.grad.numpy() * loss_scale


def ref_rcnn_iou(cls, reg, labels, rois, matched, gt_boxes, nc, kind, stds, reg_weight, norm, loss_scale):
    """cls [R,nc], reg [R,4nc]; returns loss (cls, reg), grad_cls [R,nc], grad_reg [R,4nc], unit, unit_reg, nfg."""
    R = len(labels)
    lc, gcls = _ref_cls_rcnn(cls, labels, nc, norm, loss_scale)
    fg = np.nonzero(np.asarray(labels) > 0)[0]
    greg, lr = np.zeros((R, 4 * nc)), 0.0
    if len(fg):
        lab = np.asarray(labels)[fg]
        cols = 4 * lab[:, None] + np.arange(4)[None]
        g = np.asarray(gt_boxes)[np.asarray(rois)[fg, 0].astype(np.int64), np.asarray(matched)[fg], :4]
        L, G = ref_rows(np.asarray(rois)[fg, 1:], g, np.asarray(reg)[fg[:, None], cols], stds, kind)
        lr = float(L.sum()) * reg_weight * norm
        greg[fg[:, None], cols] = G * reg_weight * norm * loss_scale
    return {"loss": np.array([lc, lr]), "grad_cls": gcls, "grad_reg": greg, "unit": norm * loss_scale,
            "unit_reg": reg_weight * norm * loss_scale, "nfg": len(fg)}


def ref_retina_iou(cls, reg, A, Cc, cls_labels, anchors, matched, gt_boxes, level_offset, alpha, gamma, kind, stds, reg_weight,
                   num_fg, loss_scale):
    import torch
    from test_loss_cases_cpu import _focal_terms
    N, H, W, _ = cls.shape
    n_lvl = H * W * A
    z = _t64(cls, True)
    lab = torch.from_numpy(np.asarray(cls_labels, np.int64))[:, level_offset:level_offset + n_lvl]
    inv = 1.0 / max(1, int(num_fg))
    lc = _focal_terms(z[..., :A * Cc].reshape(N, n_lvl, Cc), lab, Cc, alpha, gamma) * inv
    lc.backward()
    greg = np.zeros(reg.shape)
    n_i, a_i = np.nonzero(lab.numpy() > 0)
    lr = 0.0
    if len(n_i):
        d = np.asarray(reg)[..., :4 * A].reshape(N, n_lvl, 4)[n_i, a_i]
        m = np.asarray(matched)[n_i, level_offset + a_i]
        L, G = ref_rows(np.asarray(anchors)[level_offset + a_i], np.asarray(gt_boxes)[n_i, m, :4], d, stds, kind)
        lr = float(L.sum()) * reg_weight * inv
        greg.reshape(N, H * W, -1)[n_i[:, None], (a_i // A)[:, None], 4 * (a_i % A)[:, None] + np.arange(4)] = G * reg_weight * inv * loss_scale
    return {"loss": np.array([lc.item(), lr]), "grad_cls": z.grad.numpy() * loss_scale, "grad_reg": greg,
            "unit": inv * loss_scale, "unit_reg": reg_weight * inv * loss_scale, "nfg": len(n_i)}


# ---------------------------------------------------------------------------------------------------------------------
# float32 restatements (CPU stand-ins; never references)
# ---------------------------------------------------------------------------------------------------------------------
def _expf32(x):
    u, inv = np.unique(np.asarray(x, np.float32), return_inverse=True)
    return O().expf(u)[inv].reshape(np.shape(x)).astype(np.float32)


def _step(a, b):
    return np.where(a > b, np.float32(1.0), np.where(a == b, np.float32(0.5), np.float32(0.0))).astype(np.float32)


def iou_loss_fp32(b, g, d, stds, kind):
    """(L [n], dL/dd [n,4]) float32, operation for operation what box_iou_loss_elem does: everything relative to the box's
    own corner (x1, y1), oracle.expf."""
    f = np.float32
    b, g, d = np.asarray(b, f), np.asarray(g, f), np.asarray(d, f)
    one, half, clip = f(1.0), f(0.5), f(CLIP)
    ln, pc, pl, g1, g2, gl, il, cl, a1, a2, st, ck = ([None, None] for _ in range(12))
    for k in (0, 1):
        g1[k], g2[k] = g[:, k] - b[:, k], g[:, 2 + k] - b[:, k]
        ln[k] = b[:, 2 + k] - b[:, k] + one
        c0 = half * (ln[k] - one)
        t = d[:, 2 + k] * f(stds[2 + k])
        ck[k] = _step(clip, t)
        t = np.minimum(t, clip)
        pc[k] = d[:, k] * f(stds[k]) * ln[k] + c0
        pl[k] = _expf32(t) * ln[k]
        hl = half * (pl[k] - one)
        p1, p2 = pc[k] - hl, pc[k] + hl
        gl[k] = g2[k] - g1[k] + one
        a1[k], a2[k] = _step(p1, g1[k]), _step(g2[k], p2)
        r = np.minimum(p2, g2[k]) - np.maximum(p1, g1[k]) + one
        st[k] = _step(r, f(0.0))
        il[k] = np.maximum(r, f(0.0))
        cl[k] = np.maximum(p2, g2[k]) - np.minimum(p1, g1[k]) + one
    inter = il[0] * il[1]
    uni = pl[0] * pl[1] + gl[0] * gl[1] - inter
    L = one - inter / uni
    iu2 = one / (uni * uni)
    dI, dA = -(uni + inter) * iu2, inter * iu2
    gc, gp = [np.zeros_like(L), np.zeros_like(L)], [np.zeros_like(L), np.zeros_like(L)]
    if kind == "giou":
        Cc = cl[0] * cl[1]
        ic = one / Cc
        L = L + (Cc - uni) * ic
        dI, dA = dI + ic, dA - ic
        dC = uni * ic * ic
        gc = [dC * cl[1], dC * cl[0]]
    elif kind == "diou":
        e = [pc[k] - half * (g1[k] + g2[k]) for k in (0, 1)]
        rho, iD = e[0] * e[0] + e[1] * e[1], one / (cl[0] * cl[0] + cl[1] * cl[1])
        L = L + rho * iD
        q = f(-2.0) * rho * iD * iD
        gc = [q * cl[0], q * cl[1]]
        gp = [f(2.0) * e[0] * iD, f(2.0) * e[1] * iD]
    G = np.zeros((len(L), 4), f)
    for k in (0, 1):
        gi = dI * il[1 - k] * st[k]
        d2 = gi * a2[k] + gc[k] * (one - a2[k])
        d1 = -(gi * a1[k] + gc[k] * (one - a1[k]))
        dpl = dA * pl[1 - k] + half * (d2 - d1)
        G[:, k] = (d1 + d2 + gp[k]) * (f(stds[k]) * ln[k])
        G[:, 2 + k] = dpl * (pl[k] * f(stds[2 + k])) * ck[k]
    assert L.dtype == f and G.dtype == f
    return L, G


def iou_loss_textbook_fp32(b, g, d, stds, kind):
    """The same formulas in float32 torch in ABSOLUTE coordinates (centre, then corners, then differences), gradient by
    autograd: what the kernel must NOT be."""
    import torch
    f = torch.float32
    bb, gg = torch.from_numpy(np.asarray(b, np.float32)), torch.from_numpy(np.asarray(g, np.float32))
    dd = torch.from_numpy(np.asarray(d, np.float32)).requires_grad_(True)
    zero, clip = torch.zeros((), dtype=f), torch.tensor(CLIP, dtype=f)
    il, cl, gl, pl, e2 = [], [], [], [], 0.0
    for k in (0, 1):
        ln = bb[:, 2 + k] - bb[:, k] + 1.0
        pc = dd[:, k] * stds[k] * ln + (bb[:, k] + 0.5 * (ln - 1.0))
        p = torch.exp(torch.minimum(dd[:, 2 + k] * stds[2 + k], clip)) * ln
        p1, p2 = pc - 0.5 * (p - 1.0), pc + 0.5 * (p - 1.0)
        g1, g2 = gg[:, k], gg[:, 2 + k]
        il.append(torch.maximum(torch.minimum(p2, g2) - torch.maximum(p1, g1) + 1.0, zero))
        cl.append(torch.maximum(p2, g2) - torch.minimum(p1, g1) + 1.0)
        gl.append(g2 - g1 + 1.0)
        pl.append(p2 - p1 + 1.0)
        e2 = e2 + (pc - (g1 + 0.5 * (gl[k] - 1.0))) ** 2
    inter = il[0] * il[1]
    union = pl[0] * pl[1] + gl[0] * gl[1] - inter
    L = 1.0 - inter / union
    if kind == "giou":
        L = L + (cl[0] * cl[1] - union) / (cl[0] * cl[1])
    elif kind == "diou":
        L = L + e2 / (cl[0] ** 2 + cl[1] ** 2)
    L.sum().backward()
    return L.detach().numpy(), dd.grad.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------
def draw_boxes(rng, n):
    """n boxes [n,4] float32 with sides 2..800 px (log-uniform) inside [0, 1333]."""
    wh = np.exp(rng.uniform(np.log(2.0), np.log(800.0), (n, 2)))
    xy = rng.uniform(0.0, 1333.0 - wh)
    return np.concatenate([xy, xy + wh - 1.0], axis=1).astype(np.float32)


def jitter(rng, box):
    """A box near each given one (centre moved by ~0.2 sides, sides scaled by ~exp(0.25)), clipped as draw_boxes' are."""
    box = np.asarray(box, np.float64)
    wh = box[:, 2:] - box[:, :2] + 1.0
    c = box[:, :2] + 0.5 * (wh - 1.0) + rng.standard_normal(wh.shape) * 0.2 * wh
    wh = np.clip(wh * np.exp(rng.standard_normal(wh.shape) * 0.25), 2.0, 800.0)
    xy = np.clip(c - 0.5 * (wh - 1.0), 0.0, 1333.0 - wh)
    return np.concatenate([xy, xy + wh - 1.0], axis=1).astype(np.float32)


def draw_deltas(rng, box, gt, stds):
    """bf16-exact raw deltas [n,4] (decoded offsets ~0.15 sides, log-sizes ~0.25) such that every row keeps MARGIN from
    every branch; rows that do not are redrawn."""
    n = len(box)
    d = np.zeros((n, 4), np.float32)
    todo = np.arange(n)
    for _ in range(64):
        if not len(todo):
            return d
        t = rng.standard_normal((len(todo), 4)) * np.array([0.15, 0.15, 0.25, 0.25])
        d[todo] = bf16r(t / np.asarray(stds))
        todo = todo[branch_margin(box[todo], gt[todo], d[todo], stds) < MARGIN]
    raise AssertionError("rows within the branch margin after 64 redraws")


@functools.lru_cache(maxsize=None)
def random_rows(stds_name, n=N_RANDOM, seed=11):
    rng = np.random.default_rng(seed + zlib.crc32(stds_name.encode()))
    gt = draw_boxes(rng, n)
    box = jitter(rng, gt)
    return box, gt, draw_deltas(rng, box, gt, STDS[stds_name])


# ---- primitive: random tables and named cases -----------------------------------------------------------------------
NAMED = ("disjoint", "touching", "identical", "shared_edge", "pred_inside_gt", "gt_inside_pred", "clamped_dw", "gt_1x1",
         "tiny_far", "huge", "weights", "no_foreground")
TIE_CASES = ("touching", "identical", "shared_edge")
PRIM_N = (1, 3, 64, 65, 257)


def _prim_cases():
    out = []
    for i, n in enumerate(PRIM_N):
        for j, sn in enumerate(("head", "unit")):
            out.append({"id": "n%d-%s-gs%d" % (n, sn, (1, 512)[(i + j) % 2]), "name": "random", "n": n, "stds": sn,
                        "gs": (1, 512)[(i + j) % 2]})
    for i, name in enumerate(NAMED):
        for j, sn in enumerate(("head", "unit")):
            out.append({"id": "%s-%s-gs%d" % (name, sn, (1, 512)[(i + j) % 2]), "name": name, "stds": sn,
                        "n": {"weights": 65, "no_foreground": 3, "tiny_far": 32}.get(name, 1), "gs": (1, 512)[(i + j) % 2]})
    return out


PRIM_CASES = _prim_cases()


def _a(*rows):
    return np.array(rows, np.float32)


@functools.lru_cache(maxsize=None)
def _prim_data(cid):
    c = next(x for x in PRIM_CASES if x["id"] == cid)
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    stds, name, n = STDS[c["stds"]], c["name"], c["n"]
    w, zero = None, np.zeros((1, 4), np.float32)
    if name in ("random", "weights", "no_foreground"):
        gt = draw_boxes(rng, n)
        box = jitter(rng, gt)
        d = draw_deltas(rng, box, gt, stds)
        if name == "weights":
            w = rng.choice([0.0, 0.5, 1.0, 2.0], size=n).astype(np.float32)
            w[:4] = (0.0, 0.5, 1.0, 2.0)
        elif name == "no_foreground":
            w = np.zeros(n, np.float32)
    elif name == "disjoint":
        box, gt, d = _a((10, 10, 29, 29)), _a((100, 50, 139, 99)), zero
    elif name == "touching":                                          # min(px2, gx2) - max(px1, gx1) + 1 = 29 - 30 + 1 = 0
        box, gt, d = _a((10, 10, 29, 29)), _a((30, 15, 49, 40)), zero
    elif name == "identical":
        box, gt, d = _a((640, 480, 703, 511)), _a((640, 480, 703, 511)), zero
    elif name == "shared_edge":                                       # the left edges coincide, nothing else does
        box, gt, d = _a((10, 10, 29, 29)), _a((10, 15, 39, 40)), zero
    elif name == "pred_inside_gt":
        box, gt = _a((100, 100, 119, 129)), _a((90, 80, 150, 160))
        d = draw_deltas(rng, box, gt, np.asarray(stds) * 4.0)         # small deltas: the prediction stays inside
    elif name == "gt_inside_pred":
        box, gt = _a((90, 80, 150, 160)), _a((100, 100, 119, 129))
        d = draw_deltas(rng, box, gt, np.asarray(stds) * 4.0)
    elif name == "clamped_dw":                                        # dw * std_w = 5 > CLIP = 4.135; dh is not clamped
        box, gt = _a((200, 100, 203, 139)), _a((150, 90, 320, 150))
        d = draw_deltas(rng, box, gt, stds)
        d[0, 2] = bf16r([5.0 / stds[2]])[0]
        assert branch_margin(box, gt, d, stds)[0] >= MARGIN
    elif name == "gt_1x1":
        box, gt = _a((300, 200, 305, 207)), _a((303, 204, 303, 204))
        d = draw_deltas(rng, box, gt, stds)
    elif name == "tiny_far":                                          # 2-px boxes at ~1300, where ulp = 1.2e-4 px; no dyadic corners
        xy = rng.uniform(1290.0, 1330.0, (n, 2)).astype(np.float32)
        box = np.concatenate([xy, xy + np.float32(1.0)], axis=1)
        wh, c = rng.uniform(1.0, 3.0, (n, 2)), xy + 0.5 + rng.uniform(-1.0, 1.0, (n, 2))
        gt = np.concatenate([c - 0.5 * (wh - 1.0), c + 0.5 * (wh - 1.0)], axis=1).astype(np.float32)
        d = draw_deltas(rng, box, gt, stds)
    elif name == "huge":
        box, gt = _a((3, 5, 1302, 804)), _a((20.5, 1.25, 1330.75, 790.5))
        d = draw_deltas(rng, box, gt, stds)
    return {"box": box, "gt": gt, "d": d, "w": w, "stds": stds}


def prim_data(c):
    return _prim_data(c["id"])


@functools.lru_cache(maxsize=None)
def _prim_ref(cid, kind):
    c = next(x for x in PRIM_CASES if x["id"] == cid)
    d = _prim_data(cid)
    return ref_box_iou_loss(d["box"], d["gt"], d["d"], d["w"], d["stds"], kind, float(c["gs"]))


def prim_ref(c, kind):
    return _prim_ref(c["id"], kind)


# ---- box-head entry ---------------------------------------------------------------------------------------------------
RCNN_R, RCNN_NC, RCNN_LD = (1, 3, 64, 65, 257), (2, 81), 448
RCNN_IMAGES, RCNN_G = 2, 5
RCNN_STDS, RCNN_WEIGHT = "head", 10.0


def _rcnn_cases():
    out, i = [], 0
    for nc in RCNN_NC:
        for R in RCNN_R:
            for bf in (0, 1):
                mix = "all_bg" if (R == 3 and bf == 0) or (R == 64 and bf == 1) else "mixed"
                ls = (1, 256)[i % 2]
                out.append({"id": "nc%d-R%d-%s-%s-ls%d" % (nc, R, "bf16" if bf else "f32", mix, ls), "nc": nc, "R": R, "bf": bf,
                            "mix": mix, "ls": ls, "data_id": "nc%d-R%d-%s" % (nc, R, mix)})
                i += 1
    return out


RCNN_CASES = _rcnn_cases()


@functools.lru_cache(maxsize=None)
def _rcnn_data(data_id):
    c = next(x for x in RCNN_CASES if x["data_id"] == data_id)
    rng = np.random.default_rng(zlib.crc32(data_id.encode()))
    nc, R, stds = c["nc"], c["R"], STDS[RCNN_STDS]
    gt = np.zeros((RCNN_IMAGES, RCNN_G, 5), np.float32)
    gt[..., :4] = draw_boxes(rng, RCNN_IMAGES * RCNN_G).reshape(RCNN_IMAGES, RCNN_G, 4)
    gt[..., 4] = rng.integers(1, nc, (RCNN_IMAGES, RCNN_G))
    img, m = rng.integers(0, RCNN_IMAGES, R), rng.integers(0, RCNN_G, R).astype(np.int32)
    if c["mix"] == "all_bg":
        labels = rng.choice([-1, 0, 0], size=R).astype(np.int32)
    else:
        labels = rng.choice(np.arange(-1, nc), size=R, p=[0.15, 0.25] + [0.6 / (nc - 1)] * (nc - 1)).astype(np.int32)
        labels[0] = nc - 1                                            # the last class: the row's last four columns
        if R >= 3:
            labels[1], labels[2] = -1, 0
        if R >= 64:
            labels[R - 1] = 1
    rois = np.zeros((R, 5), np.float32)
    rois[:, 0] = img
    rois[:, 1:] = jitter(rng, gt[img, m, :4])
    cls = bf16r(rng.standard_normal((R, nc)) * 2)
    reg = bf16r(rng.standard_normal((R, 4 * nc)) * 2)
    fg = np.nonzero(labels > 0)[0]
    if len(fg):
        reg[fg[:, None], 4 * labels[fg][:, None] + np.arange(4)[None]] = draw_deltas(rng, rois[fg, 1:], gt[img[fg], m[fg], :4], stds)
    return {"cls": cls, "reg": reg, "labels": labels, "rois": rois, "matched": m, "gt": gt, "norm": 1.0 / R}


def rcnn_data(c):
    return _rcnn_data(c["data_id"])


@functools.lru_cache(maxsize=None)
def _rcnn_ref(cid, kind):
    c = next(x for x in RCNN_CASES if x["id"] == cid)
    d = _rcnn_data(c["data_id"])
    return ref_rcnn_iou(d["cls"], d["reg"], d["labels"], d["rois"], d["matched"], d["gt"], c["nc"], kind, STDS[RCNN_STDS], RCNN_WEIGHT,
                        d["norm"], float(c["ls"]))


def rcnn_ref(c, kind):
    return _rcnn_ref(c["id"], kind)


# ---- RetinaNet entry --------------------------------------------------------------------------------------------------
RETINA_SHAPES = (("one", (1, 1, 1, 1, 8), "vec", 0), ("coco", (2, 3, 5, 9, 80), "vec", 0), ("c3", (1, 2, 2, 9, 3), "scalar", 0),
                 ("offset", (2, 7, 9, 9, 80), "vec", 37))
RETINA_G, RETINA_ALPHA, RETINA_GAMMA, RETINA_STDS = 6, 0.25, 2.0, "unit"


def _retina_cases():
    out, i = [], 0
    for name, shape, form, off in RETINA_SHAPES:
        for nfg in ("true", "zero"):
            ls, rw = (1, 512)[i % 2], (1.0, 2.5)[(i // 2) % 2]
            out.append({"id": "%s-%s-nfg%s-ls%d-w%g" % (name, form, nfg, ls, rw), "name": name, "shape": shape, "form": form, "off": off,
                        "nfg": nfg, "ls": ls, "rw": rw})
            i += 1
    return out


RETINA_CASES = _retina_cases()


def retina_ld(c):
    N, H, W, A, Cc = c["shape"]
    return (A * Cc + 63) // 64 * 64, (4 * A + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def _retina_data(name):
    c = next(x for x in RETINA_CASES if x["name"] == name)
    rng = np.random.default_rng(zlib.crc32(("retina-" + name).encode()))
    N, H, W, A, Cc = c["shape"]
    ldc, ldr = retina_ld(c)
    off, n_lvl, stds = c["off"], H * W * A, STDS[RETINA_STDS]
    At = off + n_lvl + (11 if off else 0)
    gt = np.zeros((N, RETINA_G, 5), np.float32)
    gt[0, :, :4] = draw_boxes(rng, RETINA_G)
    for n in range(1, N):
        gt[n, :, :4] = jitter(rng, gt[0, :, :4])
    gt[..., 4] = rng.integers(1, Cc + 1, (N, RETINA_G))
    near = np.arange(At) % RETINA_G
    anchors = jitter(rng, gt[0, near, :4])
    matched = np.tile(near.astype(np.int32), (N, 1))
    labels = rng.choice([-1, 0, 1], size=(N, At), p=[0.15, 0.45, 0.4]).astype(np.int32)
    labels[0, off], labels[-1, off + n_lvl - 1] = 1, 1                  # the level's first and last anchor are foreground
    if n_lvl > 2:
        labels[0, off + 1], labels[0, off + 2] = -1, 0
    labels[:, :off], labels[:, off + n_lvl:] = 1, 1                     # foreground of other levels: counted, not visited
    cls_labels = np.where(labels == 1, gt[np.arange(N)[:, None], matched, 4].astype(np.int32), labels).astype(np.int32)
    reg = bf16r(rng.standard_normal((N, H, W, ldr)) * 0.5)
    n_i, a_i = np.nonzero(labels[:, off:off + n_lvl] > 0)
    reg.reshape(N, H * W, ldr)[n_i[:, None], (a_i // A)[:, None], 4 * (a_i % A)[:, None] + np.arange(4)] = draw_deltas(rng, anchors[off + a_i], gt[n_i, matched[n_i, off + a_i], :4], stds)
    return {"cls": bf16r(rng.standard_normal((N, H, W, ldc)) * 2 - 2), "reg": reg, "anchors": anchors, "matched": matched, "gt": gt,
            "cls_labels": cls_labels, "A_total": At, "num_fg_true": int((cls_labels > 0).sum())}


def retina_data(c):
    return _retina_data(c["name"])


def retina_num_fg(c):
    return retina_data(c)["num_fg_true"] if c["nfg"] == "true" else 0


@functools.lru_cache(maxsize=None)
def _retina_ref(cid, kind):
    c = next(x for x in RETINA_CASES if x["id"] == cid)
    d = retina_data(c)
    N, H, W, A, Cc = c["shape"]
    return ref_retina_iou(d["cls"], d["reg"], A, Cc, d["cls_labels"], d["anchors"], d["matched"], d["gt"], c["off"], RETINA_ALPHA,
                          RETINA_GAMMA, kind, STDS[RETINA_STDS], c["rw"], retina_num_fg(c), float(c["ls"]))


def retina_ref(c, kind):
    return _retina_ref(c["id"], kind)


def all_table_rows(stds_name):
    """(box, gt, deltas) of every regressed row of every table that uses this stds setting."""
    rows = []
    for c in PRIM_CASES:
        if c["stds"] == stds_name:
            d = prim_data(c)
            rows.append((d["box"], d["gt"], d["d"], c["name"]))
    if stds_name == RCNN_STDS:
        for c in RCNN_CASES:
            d = rcnn_data(c)
            fg = np.nonzero(d["labels"] > 0)[0]
            cols = 4 * d["labels"][fg][:, None] + np.arange(4)[None]
            rows.append((d["rois"][fg, 1:], d["gt"][d["rois"][fg, 0].astype(int), d["matched"][fg], :4], d["reg"][fg[:, None], cols], "rcnn"))
    if stds_name == RETINA_STDS:
        for c in RETINA_CASES:
            d = retina_data(c)
            N, H, W, A, Cc = c["shape"]
            n_lvl, off = H * W * A, c["off"]
            n_i, a_i = np.nonzero(d["cls_labels"][:, off:off + n_lvl] > 0)
            rows.append((d["anchors"][off + a_i], d["gt"][n_i, d["matched"][n_i, off + a_i], :4],
                         d["reg"][..., :4 * A].reshape(N, n_lvl, 4)[n_i, a_i], "retina"))
    return rows


# ---------------------------------------------------------------------------------------------------------------------
# proofs
# ---------------------------------------------------------------------------------------------------------------------
def test_torch_maximum_splits_a_tie():
    import torch
    x = torch.tensor([2.0, 3.0], dtype=torch.float64, requires_grad=True)
    y = torch.tensor([2.0, 1.0], dtype=torch.float64, requires_grad=True)
    (torch.maximum(x, y).sum() + 10.0 * torch.minimum(x, y).sum()).backward()
    assert x.grad.tolist() == [0.5 + 5.0, 1.0] and y.grad.tolist() == [0.5 + 5.0, 10.0]
    z = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    torch.maximum(z, torch.zeros((), dtype=torch.float64)).sum().backward()
    assert z.grad.item() == 0.5


def test_tables_cover_the_listed_values():
    assert {c["n"] for c in PRIM_CASES if c["name"] == "random"} == set(PRIM_N)
    assert {c["name"] for c in PRIM_CASES} == set(NAMED) | {"random"}
    for name in NAMED + ("random",):
        sub = [c for c in PRIM_CASES if c["name"] == name]
        assert {c["stds"] for c in sub} == {"head", "unit"} and {c["gs"] for c in sub} == {1, 512}
    assert {(c["nc"], c["R"], c["bf"]) for c in RCNN_CASES} == {(a, b, d) for a in RCNN_NC for b in RCNN_R for d in (0, 1)}
    for nc in RCNN_NC:
        sub = [c for c in RCNN_CASES if c["nc"] == nc]
        assert {c["mix"] for c in sub} == {"mixed", "all_bg"} and {c["ls"] for c in sub} == {1, 256}
        assert {c["bf"] for c in sub if c["mix"] == "all_bg"} == {0, 1}
    assert [s[1] for s in RETINA_SHAPES] == [(1, 1, 1, 1, 8), (2, 3, 5, 9, 80), (1, 2, 2, 9, 3), (2, 7, 9, 9, 80)]
    for name, *_ in RETINA_SHAPES:
        sub = [c for c in RETINA_CASES if c["name"] == name]
        assert {c["nfg"] for c in sub} == {"true", "zero"}
    assert {c["ls"] for c in RETINA_CASES} == {1, 512} and {c["rw"] for c in RETINA_CASES} == {1.0, 2.5}
    for table in (PRIM_CASES, RCNN_CASES, RETINA_CASES):
        assert len(set(ids(table))) == len(table)


def test_every_row_keeps_the_branch_margin():
    n = 0
    for sn in STDS:
        for box, gt, d, name in all_table_rows(sn):
            assert np.array_equal(bf16r(d), d), name
            if name in TIE_CASES or not len(box):
                continue
            assert branch_margin(box, gt, d, STDS[sn]).min() >= MARGIN, name
            n += len(box)
        box, gt, d = random_rows(sn)
        assert np.array_equal(bf16r(d), d) and branch_margin(box, gt, d, STDS[sn]).min() >= MARGIN
        wh = np.concatenate([box[:, 2:] - box[:, :2], gt[:, 2:] - gt[:, :2]]) + 1.0
        assert wh.min() >= 2.0 - 1e-3 and wh.max() <= 800.0 + 1e-3 and box.min() >= 0.0 and max(box.max(), gt.max()) <= 1333.0
    assert n > 500


@pytest.mark.parametrize("c", [c for c in PRIM_CASES if c["name"] != "random"], ids=ids([c for c in PRIM_CASES if c["name"] != "random"]))
def test_named_case_is_what_it_is_named(c):
    d, name, stds = prim_data(c), c["name"], STDS[c["stds"]]
    refs = {k: prim_ref(c, k) for k in KINDS}
    gs = c["gs"]
    b, g, dd = _t64(d["box"]), _t64(d["gt"]), _t64(d["d"])
    (xc, xl, x1, x2, tx), (yc, yl, y1, y2, ty) = [[v.numpy() for v in ax] for ax in _decode64(b, dd, stds)]
    gx1, gy1, gx2, gy2 = d["gt"].astype(np.float64).T
    rw, rh = np.minimum(x2, gx2) - np.maximum(x1, gx1) + 1, np.minimum(y2, gy2) - np.maximum(y1, gy1) + 1
    if name in TIE_CASES + ("disjoint",):
        assert not d["d"].any() and np.array_equal(d["box"], np.round(d["box"])) and np.array_equal(d["gt"], np.round(d["gt"]))
        assert np.array_equal([x1, y1, x2, y2], d["box"].astype(np.float64).T)          # the prediction IS the box, exactly
    if name == "disjoint":
        assert rw[0] < -MARGIN or rh[0] < -MARGIN
        assert refs["iou"]["loss"][0] == 1.0 and not refs["iou"]["grad"].any()
        assert np.abs(refs["giou"]["grad"]).max() > 1e-3 * gs and np.abs(refs["diou"]["grad"]).max() > 1e-3 * gs
    elif name == "touching":
        assert rw[0] == 0.0 and rh[0] > MARGIN
        # half the one-sided derivative: the gradient is neither that of the overlapping nor that of the disjoint side
        assert refs["iou"]["loss"][0] == 1.0 and refs["iou"]["grad"].any()
        eps = np.array([[2.0 ** -6 / stds[0] / 20.0, 0, 0, 0]])                           # the box moves 2^-6 px to either side
        for k in KINDS:
            gp = ref_rows(d["box"], d["gt"], d["d"] + eps, stds, k)[1]
            gm = ref_rows(d["box"], d["gt"], d["d"] - eps, stds, k)[1]
            assert np.allclose(refs[k]["grad"] / gs, 0.5 * (gp + gm), rtol=0, atol=1e-3), k
    elif name == "identical":
        assert np.array_equal(d["box"], d["gt"])
        for k in KINDS:
            assert refs[k]["loss"][0] == 0.0
            assert iou_loss_fp32(d["box"], d["gt"], d["d"], stds, k)[0][0] == 0.0
    elif name == "shared_edge":
        ties = [x1[0] == gx1[0], x2[0] == gx2[0], y1[0] == gy1[0], y2[0] == gy2[0]]
        assert ties == [True, False, False, False] and rw[0] > 0 and rh[0] > 0
    elif name == "pred_inside_gt":
        assert gx1[0] < x1[0] and x2[0] < gx2[0] and gy1[0] < y1[0] and y2[0] < gy2[0]
    elif name == "gt_inside_pred":
        assert x1[0] < gx1[0] and gx2[0] < x2[0] and y1[0] < gy1[0] and gy2[0] < y2[0]
    elif name == "clamped_dw":
        assert tx[0] > CLIP + MARGIN and ty[0] < CLIP - MARGIN
        for k in KINDS:
            assert refs[k]["grad"][0, 2] == 0.0 and refs[k]["grad"][0, 3] != 0.0
            assert iou_loss_fp32(d["box"], d["gt"], d["d"], stds, k)[1][0, 2] == 0.0
    elif name == "gt_1x1":
        assert gx1[0] == gx2[0] and gy1[0] == gy2[0] and rw[0] == 1.0 and rh[0] == 1.0
    elif name == "tiny_far":
        assert d["box"].min() >= 1290.0 and (d["box"][:, 2:] - d["box"][:, :2] + 1 == 2).all() and np.any((rw > 0) & (rh > 0))
        assert np.mean(d["box"] * 8 == np.round(d["box"] * 8)) < 0.1                      # corners that use the low mantissa bits
    elif name == "huge":
        assert d["box"][0, 2] - d["box"][0, 0] + 1 == 1300 and d["box"][0, 3] - d["box"][0, 1] + 1 == 800
    elif name == "weights":
        assert set(np.unique(d["w"])) == {0.0, 0.5, 1.0, 2.0}
        r = refs["giou"]
        assert not r["loss"][d["w"] == 0].any() and not r["grad"][d["w"] == 0].any() and r["grad"][d["w"] == 2].any(axis=1).all()
    elif name == "no_foreground":
        assert not d["w"].any() and all(not refs[k]["loss"].any() and not refs[k]["grad"].any() for k in KINDS)
    if name in TIE_CASES:                                                 # exact in fp32 too: the restatement agrees
        for k in KINDS:
            L32, G32 = iou_loss_fp32(d["box"], d["gt"], d["d"], stds, k)
            assert np.allclose(G32 * gs, refs[k]["grad"], rtol=0, atol=ATOL_GRAD[c["stds"]] * gs), k


@pytest.mark.parametrize("c", RCNN_CASES, ids=ids(RCNN_CASES))
def test_rcnn_case_is_what_it_is_named(c):
    d, r = rcnn_data(c), rcnn_ref(c, "giou")
    nc, R, lab = c["nc"], c["R"], rcnn_data(c)["labels"]
    assert {1: R < 4, 3: R < 4, 64: R % 4 == 0, 65: R % 4 == 1, 257: R % 4 == 1 and R > 256}[R]
    assert nc + 4 * nc <= RCNN_LD and set(np.unique(d["rois"][:, 0])) <= {0.0, 1.0} and d["matched"].max() < RCNN_G
    if c["mix"] == "all_bg":
        assert lab.max() <= 0 and r["loss"][1] == 0.0 and not r["grad_reg"].any() and r["nfg"] == 0
    else:
        assert lab[0] == nc - 1 and r["grad_reg"][0, 4 * nc - 4:].any() and r["loss"][1] > 0
        if R >= 3:
            assert lab[1] == -1 and lab[2] == 0 and not r["grad_reg"][1:3].any() and not r["grad_cls"][1].any() and r["grad_cls"][2].any()
        own = np.zeros(r["grad_reg"].shape, bool)                          # the four columns of the row's own class, no others
        own[np.nonzero(lab > 0)[0][:, None], 4 * lab[lab > 0][:, None] + np.arange(4)] = True
        assert not r["grad_reg"][~own].any() and np.array_equal((r["grad_reg"] != 0).any(axis=1), lab > 0)
    assert np.array_equal(bf16r(d["cls"]), d["cls"]) and np.array_equal(bf16r(d["reg"]), d["reg"])


def retina_iou_route(c, off_reg=0, L=None):
    """(kind word, vec, grid) of mxdet_retina_loss_level_iou as the library's selector reports it (route probe, no device)."""
    from mxdetection_amd import _lib
    L = L or _lib.load()
    N, H, W, A, Cc = c["shape"]
    ldc, ldr = retina_ld(c)
    base = 1 << 20
    p, pr = C.c_void_p(base), C.c_void_p(base + off_reg)
    L.mxdet_debug_route_probe(1)
    try:
        rc = L.mxdet_retina_loss_level_iou(p, pr, N, H, W, A, Cc, ldc, ldr, p, p, p, p, RETINA_G, c["off"] + H * W * A + 11, c["off"],
                                           RETINA_ALPHA, RETINA_GAMMA, 1, 1.0, 1.0, 1.0, 1.0, c["rw"], p, float(c["ls"]), p, pr, p, None)
        assert rc == 0, L.mxdet_last_error()
        buf = (C.c_int32 * 64)()
        assert L.mxdet_debug_route_read(buf, 4) == 1
    finally:
        L.mxdet_debug_route_probe(0)
    assert not any(buf[3:16])
    return buf[0], bool(buf[1]), buf[2]


@pytest.mark.parametrize("c", RETINA_CASES, ids=ids(RETINA_CASES))
def test_retina_case_is_what_it_is_named(c):
    from mxdetection_amd import _lib
    d, r = retina_data(c), retina_ref(c, "giou")
    N, H, W, A, Cc = c["shape"]
    n_lvl = H * W * A
    kind, vec, grid = retina_iou_route(c)
    assert kind == _lib.ROUTE_KINDS["RETINA_LOSS_IOU"] and vec == (c["form"] == "vec") == (Cc % 8 == 0)
    assert grid == _lib.load().mxdet_retina_loss_num_partials(N, H, W, A) == (N * n_lvl + 255) // 256
    assert {"one": N * n_lvl == 1, "coco": N * n_lvl > 256, "c3": Cc == 3, "offset": c["off"] > 0 and N * n_lvl > 1024}[c["name"]]
    lv = d["cls_labels"][:, c["off"]:c["off"] + n_lvl]
    assert lv[0, 0] > 0 and lv[-1, -1] > 0 and r["nfg"] == int((lv > 0).sum())
    if n_lvl > 2:
        assert np.any(lv == 0) and np.any(lv == -1)
    assert r["unit"] == (1.0 if c["nfg"] == "zero" else 1.0 / d["num_fg_true"]) * c["ls"]
    if c["name"] == "offset":
        assert d["num_fg_true"] > r["nfg"] and d["A_total"] > c["off"] + n_lvl
    nz = (r["grad_reg"][..., :4 * A].reshape(N, n_lvl, 4) != 0).any(axis=2)
    assert np.array_equal(nz, lv > 0) and not r["grad_reg"][..., 4 * A:].any()


def test_retina_iou_route_follows_the_smooth_l1_entry():
    """C = 80 gives the vector form and C = 3 the scalar one; a reg view 4 bytes off drops to the scalar form, as there."""
    from mxdetection_amd import _lib
    coco = next(c for c in RETINA_CASES if c["name"] == "coco")
    c3 = next(c for c in RETINA_CASES if c["name"] == "c3")
    assert retina_iou_route(coco)[:2] == (_lib.ROUTE_KINDS["RETINA_LOSS_IOU"], True)
    assert retina_iou_route(c3)[:2] == (_lib.ROUTE_KINDS["RETINA_LOSS_IOU"], False)
    assert retina_iou_route(coco, off_reg=4)[1] is False


# ---- host-side validation (no GPU: every check happens before a launch) ------------------------------------------------
def test_entries_validate_their_arguments():
    from mxdetection_amd import _lib
    L = _lib.load()
    p, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 4)

    def err():
        return L.mxdet_last_error()

    def prim(boxes=p, gt=p, deltas=p, dtype=0, ld=4, n=5, kind=1, stds=(1.0,) * 4, loss=p, grad=p):
        return L.mxdet_box_iou_loss(boxes, gt, deltas, dtype, ld, None, n, kind, *stds, 1.0, loss, grad, None)
    assert prim(n=0, boxes=None, gt=None, deltas=None, loss=None, grad=None) == 0 and err() == b""
    assert prim(n=-1) == -2 and prim(ld=3) == -2 and b"ld must be >= 4" in err()
    assert prim(dtype=2) == -1 and b"dtype" in err()
    assert prim(kind=3) == -1 and b"kind" in err()
    assert prim(stds=(1.0, 1.0, 0.0, 1.0)) == -1 and b"stds" in err()
    for k in ("boxes", "gt", "deltas", "loss", "grad"):
        assert prim(**{k: None}) == -1 and b"null pointer" in err(), k
    assert prim(boxes=odd) == -1 and b"16-byte aligned" in err()
    assert prim(gt=odd) == -1 and b"16-byte aligned" in err()

    def rcnn(cls=p, reg=p, dtype=1, ldc=448, ldr=448, labels=p, rois=p, m=p, gt=p, N=2, G=5, R=8, nc=81, rd=324, kind=1, stds=(0.1, 0.1, 0.2, 0.2),
             w=10.0, loss=p, gc=p, gr=p, ws=p, wsb=1 << 20):
        return L.mxdet_rcnn_loss_iou(cls, reg, dtype, ldc, ldr, labels, rois, m, gt, N, G, R, nc, rd, kind, *stds, w, 0.125, 1.0, loss, gc, gr,
                                     ws, wsb, None)
    assert rcnn(R=0) == -2 and rcnn(rd=4) == -2 and b"reg_dim must be 4 * num_classes" in err()
    assert rcnn(ldr=320) == -2 and rcnn(G=0) == -2 and rcnn(N=0) == -2
    assert rcnn(dtype=3) == -1 and b"dtype" in err()
    assert rcnn(kind=-1) == -1 and b"kind" in err()
    assert rcnn(w=0.0) == -1 and b"reg_weight" in err()
    assert rcnn(stds=(0.1, -0.1, 0.2, 0.2)) == -1
    for k in ("cls", "reg", "labels", "rois", "m", "gt", "loss", "gc", "gr"):
        assert rcnn(**{k: None}) == -1 and b"null pointer" in err(), k
    assert rcnn(ws=None) == -3 and rcnn(wsb=16) == -3 and b"workspace too small" in err()

    def retina(cls=p, reg=p, shape=(1, 3, 5, 3, 8), ldc=24, ldr=12, lab=p, anchors=p, m=p, gt=p, G=4, At=100, off=0, kind=2, stds=(1.0,) * 4,
               w=1.0, nfg=p, gc=p, gr=p, part=p):
        return L.mxdet_retina_loss_level_iou(cls, reg, *shape, ldc, ldr, lab, anchors, m, gt, G, At, off, 0.25, 2.0, kind, *stds, w, nfg, 1.0,
                                             gc, gr, part, None)
    assert retina(ldc=16) == -2 and b"bad shape" in err()
    assert retina(ldr=8) == -2 and retina(G=0) == -2
    assert retina(At=44) == -2 and b"level outside the anchor range" in err()
    assert retina(off=-1) == -2
    assert retina(kind=7) == -1 and b"kind" in err()
    assert retina(w=-1.0) == -1 and retina(stds=(0.0, 1.0, 1.0, 1.0)) == -1 and b"positive" in err()
    for k in ("cls", "reg", "lab", "anchors", "m", "gt", "nfg", "gc", "gr", "part"):
        assert retina(**{k: None}) == -1 and b"null pointer" in err(), k
    assert retina(anchors=odd) == -1 and b"anchors must be 16-byte aligned" in err()
    # while the probe is on the arguments are validated as usual, and a rejected call leaves no record
    L.mxdet_debug_route_probe(1)
    try:
        assert retina(ldc=16) == -2 and retina(cls=None) == -1
        assert L.mxdet_debug_route_read((C.c_int32 * 64)(), 4) == 0
    finally:
        L.mxdet_debug_route_probe(0)


# ---- options: defaults, bad values, config, experiment files ----------------------------------------------------------
BAD_OPTIONS = [(dict(reg_loss="ciou"), "reg_loss"), (dict(reg_loss="giou", reg_loss_weight=0.0), "reg_loss_weight"),
               (dict(reg_loss="giou", reg_loss_weight=-2.0), "reg_loss_weight"), (dict(reg_loss_weight=2.0), "smooth_l1 takes no weight"),
               (dict(reg_loss="diou", reg_loss_weight="10"), "reg_loss_weight")]


@pytest.mark.parametrize("model", ["FasterRCNN", "MaskRCNN", "RetinaNet"])
@pytest.mark.parametrize("kw,word", BAD_OPTIONS, ids=[w + "-%d" % i for i, (_, w) in enumerate(BAD_OPTIONS)])
def test_bad_reg_loss_options_raise_before_any_allocation(model, kw, word, monkeypatch):
    """ValueError on a machine without a GPU: nothing touches the device before the check."""
    from mxdetection_amd import models
    from mxdetection_amd.models.utils import layers
    monkeypatch.setattr(layers.ParamArena, "finalize", lambda self: (_ for _ in ()).throw(AssertionError("allocated")))
    monkeypatch.setattr(layers.ParamArena, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("allocated")))
    with pytest.raises(ValueError, match=word):
        if model == "RetinaNet":
            models.RetinaNet("cuda", **kw)
        else:
            models.FasterRCNN("cuda", with_mask=(model == "MaskRCNN"), **kw)


def test_heads_check_their_own_options():
    from mxdetection_amd.models.bbox_heads import BBoxHead, ConvFCBBoxHead
    from mxdetection_amd.models.rpn_heads.retina_head import RetinaHead
    for kw, word in BAD_OPTIONS:
        with pytest.raises(ValueError, match=word):
            BBoxHead(7 * 7 * 256, None, None, "cuda", None, **kw)
        with pytest.raises(ValueError, match=word):
            ConvFCBBoxHead(7 * 7 * 256, None, None, "cuda", None, **kw)
        with pytest.raises(ValueError, match=word):
            RetinaHead(256, [8, 16, 32, 64, 128], None, None, "cuda", None, **kw)


def test_config_defaults_are_todays_model_and_the_builder_plumbs_the_keys(monkeypatch):
    from mxdetection_amd import models
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils.config import DEFAULTS, load_config
    assert DEFAULTS["network"]["reg_loss"] == "smooth_l1" and DEFAULTS["network"]["reg_loss_weight"] == 1.0
    seen = []
    monkeypatch.setattr(models, "FasterRCNN", lambda device, **kw: seen.append(("frcnn", kw)) or "m")
    monkeypatch.setattr(models, "RetinaNet", lambda device, **kw: seen.append(("retina", kw)) or "m")
    for typ in ("faster_rcnn", "mask_rcnn", "retinanet"):
        build_detector(load_config(None, ["network.type=" + typ]))
        assert seen[-1][1]["reg_loss"] == "smooth_l1" and seen[-1][1]["reg_loss_weight"] == 1.0
        build_detector(load_config(None, ["network.type=" + typ, "network.reg_loss=diou", "network.reg_loss_weight=2.5"]))
        assert seen[-1][1]["reg_loss"] == "diou" and seen[-1][1]["reg_loss_weight"] == 2.5
    monkeypatch.undo()
    for typ in ("faster_rcnn", "mask_rcnn", "retinanet"):
        with pytest.raises(ValueError, match="reg_loss"):
            build_detector(load_config(None, ["network.type=" + typ, "network.reg_loss=ciou"]))
        with pytest.raises(ValueError, match="smooth_l1 takes no weight"):
            build_detector(load_config(None, ["network.type=" + typ, "network.reg_loss_weight=10"]))
    import inspect
    for cls in (models.FasterRCNN, models.RetinaNet):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["reg_loss"].default == "smooth_l1" and sig["reg_loss_weight"].default == 1.0


def test_the_giou_experiment_files_load():
    from mxdetection_amd.utils.config import load_config
    f = load_config(os.path.join(ROOT, "configs", "faster_rcnn_r50_fpn_giou.yaml"))
    assert (f.network.type, f.network.reg_loss, f.network.reg_loss_weight) == ("faster_rcnn", "giou", 10.0)
    r = load_config(os.path.join(ROOT, "configs", "retinanet_r101_fpn_giou.yaml"))
    assert (r.network.type, r.network.backbone_depth, r.network.reg_loss, r.network.reg_loss_weight) == ("retinanet", 101, "giou", 1.0)
    base = load_config(os.path.join(ROOT, "configs", "retinanet_r101_fpn.yaml"))
    assert base.network.reg_loss == "smooth_l1" and {k: v for k, v in r.TRAIN.items()} == {k: v for k, v in base.TRAIN.items()}


# ---- tolerances ---------------------------------------------------------------------------------------------------------
def _pow2_ceil(x):
    return 2.0 ** math.ceil(math.log2(x))


@functools.lru_cache(maxsize=None)
def measure_fp32_error():
    """Largest |iou_loss_fp32 - float64 reference| over every table row and the random rows: gradient per stds setting, loss."""
    worst = {"head": 0.0, "unit": 0.0, "loss": 0.0}
    for sn, stds in STDS.items():
        parts = [r[:3] for r in all_table_rows(sn) if len(r[0])] + [random_rows(sn)]
        box, gt, d = (np.concatenate([p[i] for p in parts]) for i in range(3))
        for kind in KINDS:
            L64, G64 = ref_rows(box, gt, d, stds, kind)
            L32, G32 = iou_loss_fp32(box, gt, d, stds, kind)
            worst[sn] = max(worst[sn], float(np.abs(G32 - G64).max()))
            worst["loss"] = max(worst["loss"], float(np.abs(L32 - L64).max()))
    return worst


def test_fp32_error_budget():
    w = measure_fp32_error()
    print("iou_loss_fp32 vs float64 autograd, max error: gradient head %.3e unit %.3e, per-box loss %.3e" % (w["head"], w["unit"], w["loss"]))
    print("bounds by the x4 / power-of-two rule: 2^%d 2^%d 2^%d" % tuple(math.log2(_pow2_ceil(4 * w[k])) for k in ("head", "unit", "loss")))
    assert ATOL_GRAD["head"] == _pow2_ceil(4 * w["head"]) and ATOL_GRAD["unit"] == _pow2_ceil(4 * w["unit"])
    assert ATOL_LOSS == _pow2_ceil(4 * w["loss"])
    for k in ("head", "unit", "loss"):
        assert abs(w[k] - MEASURED[k]) <= 0.02 * MEASURED[k], (k, w[k])        # the docstring's figures are these


def test_textbook_form_misses_the_bound_on_tiny_far():
    for c in [c for c in PRIM_CASES if c["name"] == "tiny_far"]:
        d, stds = prim_data(c), STDS[c["stds"]]
        for kind in KINDS:
            L64, G64 = ref_rows(d["box"], d["gt"], d["d"], stds, kind)
            Lt, Gt = iou_loss_textbook_fp32(d["box"], d["gt"], d["d"], stds, kind)
            L32, G32 = iou_loss_fp32(d["box"], d["gt"], d["d"], stds, kind)
            print(c["id"], kind, "textbook grad err %.3e, corner-relative %.3e" % (np.abs(Gt - G64).max(), np.abs(G32 - G64).max()))
            assert np.abs(G32 - G64).max() <= ATOL_GRAD[c["stds"]] / 4 and np.abs(L32 - L64).max() <= ATOL_LOSS / 4
            assert np.abs(Gt - G64).max() > 4 * ATOL_GRAD[c["stds"]], (c["id"], kind)
            assert np.abs(Lt - L64).max() > 4 * ATOL_LOSS, (c["id"], kind)


def test_references_are_sensitive_to_the_listed_mistakes():
    box, gt, d = (x[:2000] for x in random_rows("head"))
    stds = STDS["head"]
    L, G = ref_rows(box, gt, d, stds, "giou")
    # stds forgotten on the size deltas; the image clip of the inference decode; the un-clamped exponent
    assert np.abs(ref_rows(box, gt, d, (0.1, 0.1, 1.0, 1.0), "giou")[1] - G).max() > 1000 * ATOL_GRAD["head"]
    assert np.abs(ref_rows(box, gt, d, stds, "iou")[1] - G).max() > 1000 * ATOL_GRAD["head"]
    assert np.abs(ref_rows(box, gt, d, stds, "diou")[1] - G).max() > 1000 * ATOL_GRAD["head"]
    # the "+1" of the pixel convention dropped from the ground-truth sides
    assert np.abs(ref_rows(box, gt - np.array([0, 0, 1, 1], np.float32), d, stds, "giou")[0] - L).max() > 1000 * ATOL_LOSS
