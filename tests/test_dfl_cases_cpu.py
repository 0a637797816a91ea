"""Case tables, tolerances and host-side checks of the distribution box head: mxdet_box_dist_loss,
mxdet_retina_loss_level_dfl, mxdet_retina_detect_dfl. No GPU here; tests/test_gpu_dfl.py runs the kernels on these tables.

Tolerances, by the rule of 5f / 5j: the largest difference between the float32 restatement (_dfl_ref.rows_fp32, the kernel's
operation order) and the float64 autograd reference over every table row plus N_RANDOM seeded random rows, every box kind
and both weight settings of WEIGHTS, times 4, rounded up to a power of two. Measured (MEASURED below, asserted by
test_fp32_error_budget):
    logit gradient  5.3935e-07 -> 2^-18      per-row box loss 1.1794e-06 -> 2^-17
    per-row DFL     6.2125e-06 -> 2^-15      quality          5.8748e-07 -> 2^-18
    decoded corner  1.4623e-04 px -> 2^-10 (absolute coordinates up to ~3000, where one ulp is 2.4e-4)
(the DFL of a row with logits of +-30 is itself 10..30: 6e-6 is 2e-7 of it)
The loss figures are those of the WEIGHTED terms (reg_weight * L, dfl_weight * DFL / 4) at both settings of WEIGHTS, the only
ones the tests use: the bounds apply as they stand, without a weight factor. bf16 outputs add one bf16 step 2^-8 |ref|. Every row keeps the 2^-10 branch margin of the IoU tables (a predicted corner from
its ground-truth corner, the intersection length from 0): asserted here, nothing is excluded at comparison time. The DFL has
no branch to keep away from: it is continuous in its target, at integers and at both clamps.
"""
import ctypes as C
import functools
import math
import os
import zlib

import numpy as np
import pytest

import _dfl_ref as D
import test_iou_loss_cases_cpu as T

ROOT = T.ROOT
MARGIN = T.MARGIN
BF16_STEP, LOSS_RTOL, N_RANDOM = T.BF16_STEP, T.LOSS_RTOL, T.N_RANDOM
KINDS, CLS_KINDS = D.KINDS, D.CLS_KINDS
REG_MAXES = (1, 7, 16)
WEIGHTS = ((2.0, 0.25), (1.0, 1.0))                       # (reg_weight, dfl_weight): as published, and unit
MEASURED = {"grad": 5.3935e-07, "box": 1.1794e-06, "dfl": 6.2125e-06, "q": 5.8748e-07, "decode": 1.4623e-04}      # the docstring's figures
ATOL_GRAD, ATOL_BOX, ATOL_DFL, ATOL_Q = 2.0 ** -18, 2.0 ** -17, 2.0 ** -15, 2.0 ** -18
ATOL_DECODE = 2.0 ** -10                                  # px, a decoded corner at coordinates up to ~3000 (ulp 2.4e-4)
CLS_PARAMS = {"focal": (0.25, 2.0), "qfl": (0.0, 2.0), "vfl": (0.75, 2.0)}


def bf16r(x):
    return T.bf16r(x)


def ids(cases):
    return [c["id"] for c in cases]


# ---- rows: anchor, ground truth, 4 (R + 1) logits ----------------------------------------------------------------------
def anchor_at(cx, cy, s, scale=8.0):
    h = 0.5 * (scale * s - 1.0)
    return np.array([cx - h, cy - h, cx + h, cy + h], np.float32)


def gt_at(cx, cy, dist):
    l, t, r, b = dist
    return np.array([cx - l, cy - t, cx + r, cy + b], np.float32)


def peaked(R, at, sharp=4.0):
    """Logits whose softmax peaks at `at` (strides), bf16-exact."""
    return bf16r(-sharp * np.abs(np.arange(R + 1, dtype=np.float64)[None] - np.asarray(at, np.float64)[:, None]))


def branch_margin(b, g, x, R, s):
    """Smallest distance [n] (px, float64) of a row from a max / min tie and from an empty intersection."""
    import torch
    with torch.no_grad():
        n = np.shape(x)[0]
        p, _ = D.decode64(T._t64(b), T._t64(np.asarray(x, np.float64).reshape(n, 4, R + 1)), R, float(s))
        g = T._t64(g)
        m = torch.full((n,), np.inf, dtype=torch.float64)
        for k in (0, 1):
            r = torch.minimum(p[:, 2 + k], g[:, 2 + k]) - torch.maximum(p[:, k], g[:, k]) + 1.0
            for v in (p[:, k] - g[:, k], p[:, 2 + k] - g[:, 2 + k], r):
                m = torch.minimum(m, v.abs())
    return m.numpy()


NAMED = ("clamp0", "clampR", "integer", "peaked", "flat", "pm30", "disjoint")


@functools.lru_cache(maxsize=None)
def named_rows(R, s=8.0):
    """name -> (box [1,4], gt [1,4], x [1,4(R+1)]) for one reg_max; the anchor centre is (200.5, 120.5)."""
    cx, cy = 200.5, 120.5
    b = anchor_at(cx, cy, s)[None]
    mid = 0.45 * R
    out = {}

    def put(name, dist, x):
        out[name] = (b, gt_at(cx, cy, dist)[None], np.asarray(x, np.float32).reshape(1, 4 * (R + 1)))
    # the anchor centre left of / above its ground truth: two targets clamp at 0
    put("clamp0", (-0.75 * s, -0.25 * s, (mid + 1.3) * s, (mid + 1.6) * s), peaked(R, [0.2, 0.1, mid + 0.2, mid + 0.4]))
    # ground truth out of reach: dist / s > R - 0.1 on two sides
    put("clampR", ((R + 2.3) * s, 0.4 * R * s, (R + 0.05) * s, 0.3 * R * s), peaked(R, [R - 0.2, 0.3 * R, R - 0.3, 0.4 * R]))
    # targets exactly integer (R = 1: 0 on every side)
    ti = (float(min(1, R - 1)), 0.0, float(R - 1), float(min(2, R - 1)))
    put("integer", tuple(v * s for v in ti), peaked(R, [0.7, 0.4, 0.6 * R, 0.3 * R], 1.5))
    put("peaked", (0.3 * R * s + 1.25, 0.5 * R * s + 0.5, 0.6 * R * s + 2.0, 0.2 * R * s + 0.75),
        peaked(R, [round(0.35 * R), round(0.45 * R + 0.1), round(0.55 * R + 0.1), round(0.25 * R)], 16.0))
    put("flat", (0.4 * R * s + 1.5, 0.7 * R * s, 0.3 * R * s + 0.25, 0.6 * R * s + 3.0), np.zeros((4, R + 1)))
    pm = np.full((4, R + 1), -30.0)
    pm[np.arange(4), [0, R, R // 2, (R + 1) // 2]] = 30.0
    put("pm30", (0.2 * s + 0.5, (R - 0.4) * s, 0.5 * R * s + 1.0, 0.5 * R * s + 2.0), pm)
    # the prediction lies left of its ground truth: no overlap, q == 0
    far = 3.0 * R * s + 40.0
    out["disjoint"] = (b, np.array([[cx + far, cy - 3.0, cx + far + 2.0 * s, cy + 9.0]], np.float32),
                       peaked(R, [0.3 * R, 0.2, 0.3 * R, 0.4], 3.0).reshape(1, -1))
    return out


def draw_rows(rng, n, R, s):
    """n seeded random rows (box, gt, x) that keep the branch margin: drawn in excess, the close ones dropped HERE."""
    m = n + n // 8 + 16
    cx, cy = np.round(rng.uniform(0, 1000, m) * 2) / 2, np.round(rng.uniform(0, 1000, m) * 2) / 2
    u = rng.uniform(0.2, R + 1.5, (m, 4))
    neg = rng.random((m, 4)) < 0.06
    u = np.where(neg, rng.uniform(-1.0, 0.0, (m, 4)), u)
    for k in (0, 1):                                        # keep the ground truth at least one stride long
        short = u[:, k] + u[:, 2 + k] < 1.0
        u[short, 2 + k] = 1.0 - u[short, k]
    dist = np.round(u * s * 8) / 8
    h = 0.5 * (8.0 * s - 1.0)                              # anchor_at, for all rows at once
    b = np.stack([cx - h, cy - h, cx + h, cy + h], axis=1).astype(np.float32)
    g = np.stack([cx - dist[:, 0], cy - dist[:, 1], cx + dist[:, 2], cy + dist[:, 3]], axis=1).astype(np.float32)
    at = np.clip(u + rng.standard_normal((m, 4)), -1.0, R + 1.0)
    sharp = rng.uniform(0.3, 3.0, (m, 4, 1))
    x = -sharp * np.abs(np.arange(R + 1)[None, None] - at[..., None]) + 0.5 * rng.standard_normal((m, 4, R + 1))
    big = rng.random((m, 4, R + 1)) < 0.01
    x = np.where(big, rng.choice([-30.0, 30.0], (m, 4, R + 1)), x)
    x = bf16r(x).reshape(m, 4 * (R + 1))
    keep = np.nonzero(branch_margin(b, g, x, R, s) >= 2 * MARGIN)[0][:n]
    assert len(keep) == n
    return b[keep], g[keep], x[keep]


@functools.lru_cache(maxsize=None)
def random_rows(R, n=N_RANDOM, seed=23):
    s = {1: 8.0, 7: 32.0, 16: 16.0}[R]
    return draw_rows(np.random.default_rng(seed + R), n, R, s) + (s,)


# ---- primitive cases ---------------------------------------------------------------------------------------------------
PRIM_N = (1, 3, 64, 65, 257)
PRIM_STRIDE = {1: 8.0, 7: 32.0, 16: 16.0}


def _prim_cases():
    out = []
    for i, n in enumerate(PRIM_N):
        for j, R in enumerate(REG_MAXES):
            pad = (i + j) % 2                                # rows of 4 (R + 1) + 12 elements, or tight
            kind = KINDS[(i + j) % 3]
            rw, dw = WEIGHTS[(i + j) % 2]
            out.append({"id": "n%d-R%d-%s-%s-w%g" % (n, R, "pad" if pad else "tight", kind, rw), "n": n, "R": R, "pad": 12 * pad,
                        "kind": kind, "rw": rw, "dw": dw, "gs": (1.0, 512.0)[i % 2], "s": PRIM_STRIDE[R]})
    return out


PRIM_CASES = _prim_cases()


@functools.lru_cache(maxsize=None)
def _prim_data(n, R):
    """The named rows first (as many as fit), then random ones."""
    s = PRIM_STRIDE[R]
    named = named_rows(R, s)
    parts = [named[k] for k in NAMED][:n]
    if n > len(parts):
        parts.append(draw_rows(np.random.default_rng(zlib.crc32(b"prim-%d-%d" % (n, R))), n - len(parts), R, s))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def prim_data(c):
    return _prim_data(c["n"], c["R"])


@functools.lru_cache(maxsize=None)
def _prim_ref(cid):
    c = next(x for x in PRIM_CASES if x["id"] == cid)
    b, g, x = prim_data(c)
    lb, ld, q, G = D.ref_rows(b, g, x, c["R"], c["s"], c["kind"], c["rw"], c["dw"])
    return {"box": lb, "dfl": ld, "q": q, "grad": G * c["gs"], "unit": c["gs"]}


def prim_ref(c):
    return _prim_ref(c["id"])


# ---- level cases -------------------------------------------------------------------------------------------------------
# (N, H, W, A, C, reg_max): one anchor; the vector class walk; the scalar walk with two anchors per cell and 8-bin sides;
# more than one workgroup with a tail (270 anchors). "offset": a level behind another one. "bg": no foreground at all.
LEVEL_SHAPES = (("one", (1, 1, 1, 1, 8, 16), "vec", 0, 8), ("coco", (2, 3, 5, 1, 80, 16), "vec", 0, 16),
                ("c3", (1, 2, 2, 2, 3, 7), "scalar", 0, 32), ("tail", (2, 9, 15, 1, 8, 1), "vec", 0, 8),
                ("offset", (2, 3, 5, 1, 80, 16), "vec", 37, 64), ("bg", (2, 3, 5, 1, 80, 16), "vec", 0, 16))
LEVEL_G = 6
SPECIAL = {"ignored": 1, "bg": 2, "out_of_range": 3}       # anchors of image 0 (levels with more than 4 anchors)


def _level_cases():
    out, i = [], 0
    for name, shape, form, off, s in LEVEL_SHAPES:
        for ck in CLS_KINDS:
            for kind in KINDS:
                if name in ("offset", "bg", "one") and (ck, kind) not in (("qfl", "giou"), ("focal", "diou"), ("vfl", "iou")):
                    continue
                rw, dw = WEIGHTS[i % 2]
                ls = (1, 512)[(i // 2) % 2]
                out.append({"id": "%s-%s-%s-%s-ls%d-w%g" % (name, form, ck, kind, ls, rw), "name": name, "shape": shape, "form": form,
                            "off": off, "s": float(s), "cls_loss": ck, "kind": kind, "rw": rw, "dw": dw, "ls": ls,
                            "alpha": CLS_PARAMS[ck][0], "gamma": CLS_PARAMS[ck][1]})
                i += 1
    return out


LEVEL_CASES = _level_cases()


def level_ld(c):
    N, H, W, A, Cc, R = c["shape"]
    return (A * Cc + 63) // 64 * 64, (A * 4 * (R + 1) + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def _level_data(name):
    c = next(x for x in LEVEL_CASES if x["name"] == name)
    rng = np.random.default_rng(zlib.crc32(("dfl-level-" + name).encode()))
    N, H, W, A, Cc, R = c["shape"]
    ldc, ldr = level_ld(c)
    off, s, n_lvl, nb = c["off"], c["s"], H * W * A, R + 1
    At = off + n_lvl + (11 if off else 0)
    anchors = np.zeros((At, 4), np.float32)
    anchors[:, 2:] = 15.0
    for i in range(n_lvl):
        cell, a = divmod(i, A)
        anchors[off + i] = anchor_at((cell % W) * s + 0.5 * (s - 1), (cell // W) * s + 0.5 * (s - 1), s, 8.0 if a == 0 else 5.0)
    labels = rng.choice([-1, 0, 1], size=(N, At), p=[0.15, 0.45, 0.4]).astype(np.int32)
    labels[0, off], labels[-1, off + n_lvl - 1] = 1, 1      # the level's first and last anchor are foreground
    matched = rng.integers(0, LEVEL_G, (N, At)).astype(np.int32)
    if n_lvl > 4:
        labels[0, off + SPECIAL["ignored"]], labels[0, off + SPECIAL["bg"]], labels[0, off + SPECIAL["out_of_range"]] = -1, 0, 1
        matched[0, off + SPECIAL["out_of_range"]] = LEVEL_G
        labels[-1, off + 4], matched[-1, off + 4] = 1, -1
    labels[:, :off], labels[:, off + n_lvl:] = 1, 1         # foreground of other levels: counted, not visited
    if name == "bg":
        labels[:, off:off + n_lvl] = np.minimum(labels[:, off:off + n_lvl], 0)
    # ground truth: each image's G boxes are built around anchors of the level; a positive is matched to one of them
    gt = np.zeros((N, LEVEL_G, 5), np.float32)
    reg = bf16r(rng.standard_normal((N, H, W, ldr)) * 1.5)
    for n in range(N):
        home = rng.integers(0, n_lvl, LEVEL_G)
        for j in range(LEVEL_G):
            a = anchors[off + home[j]]
            u = rng.uniform(0.3, R + 0.8, 4)
            gt[n, j, :4] = gt_at(0.5 * (a[0] + a[2]), 0.5 * (a[1] + a[3]), np.round(u * s * 8) / 8)
        gt[n, :, 4] = rng.integers(1, Cc + 1, LEVEL_G)
        for i in range(n_lvl):
            m = matched[n, off + i]
            if labels[n, off + i] > 0 and 0 <= m < LEVEL_G:
                cxy = 0.5 * (anchors[off + i, :2] + anchors[off + i, 2:])
                if rng.random() < 0.7:                      # most positives take the nearest box: they overlap it
                    gc = 0.5 * (gt[n, :, :2] + gt[n, :, 2:4])
                    matched[n, off + i] = m = int(np.argmin(((gc - cxy[None]) ** 2).sum(1)))
                g = gt[n, m, :4]
                u = np.array([cxy[0] - g[0], cxy[1] - g[1], g[2] - cxy[0], g[3] - cxy[1]]) / s
                x = -rng.uniform(0.5, 3.0, (4, 1)) * np.abs(np.arange(nb)[None] - np.clip(u + 0.6 * rng.standard_normal(4), -1, R + 1)[:, None])
                cell, a_ = divmod(i, A)
                reg[n].reshape(H * W, ldr)[cell, a_ * 4 * nb:(a_ + 1) * 4 * nb] = bf16r(x + 0.3 * rng.standard_normal((4, nb))).reshape(-1)
    cls_labels = np.where(labels == 1, gt[np.arange(N)[:, None], np.clip(matched, 0, LEVEL_G - 1), 4].astype(np.int32), labels).astype(np.int32)
    return {"cls": bf16r(rng.standard_normal((N, H, W, ldc)) * 2 - 2), "reg": reg, "anchors": anchors, "matched": matched, "gt": gt,
            "cls_labels": cls_labels, "A_total": At, "num_fg": int((cls_labels > 0).sum())}


def level_data(c):
    return _level_data(c["name"])


def level_rows(c):
    """The level's regressing anchors as rows (box, gt, x)."""
    d = level_data(c)
    N, H, W, A, Cc, R = c["shape"]
    n_lvl, nb = H * W * A, R + 1
    lab, m, n_i, a_i = D.level_positives(A, d["cls_labels"], d["matched"], LEVEL_G, c["off"], n_lvl)
    x = d["reg"][..., :4 * nb * A].reshape(N, n_lvl, 4 * nb)[n_i, a_i]
    return d["anchors"][c["off"] + a_i], d["gt"][n_i, m[n_i, a_i], :4], x


@functools.lru_cache(maxsize=None)
def _level_ref(cid):
    c = next(x for x in LEVEL_CASES if x["id"] == cid)
    d = level_data(c)
    N, H, W, A, Cc, R = c["shape"]
    return D.ref_level(d["cls"], d["reg"], A, Cc, d["cls_labels"], d["anchors"], d["matched"], d["gt"], c["off"], c["cls_loss"],
                       c["alpha"], c["gamma"], c["kind"], R, c["s"], c["rw"], c["dw"], d["num_fg"], float(c["ls"]))


def level_ref(c):
    return _level_ref(c["id"])


def level_route(c, off_reg=0, off_cls=0):
    from mxdetection_amd import _lib
    L = _lib.load()
    N, H, W, A, Cc, R = c["shape"]
    ldc, ldr = level_ld(c)
    p = 1 << 20
    L.mxdet_debug_route_probe(1)
    try:
        rc = L.mxdet_retina_loss_level_dfl(C.c_void_p(p + off_cls), C.c_void_p(p + off_reg), N, H, W, A, Cc, ldc, ldr, C.c_void_p(p),
                                           C.c_void_p(p), C.c_void_p(p), C.c_void_p(p), LEVEL_G, c["off"] + H * W * A, c["off"],
                                           D.CLS_KINDS.index(c["cls_loss"]), 0.25, 2.0, KINDS.index(c["kind"]), R, c["s"], 1.0, 0.25,
                                           C.c_void_p(p), 1.0, C.c_void_p(p + off_cls), C.c_void_p(p + off_reg), C.c_void_p(p), None)
        assert rc == 0, L.mxdet_last_error()
        buf = (C.c_int32 * 64)()
        assert L.mxdet_debug_route_read(buf, 4) == 1
    finally:
        L.mxdet_debug_route_probe(0)
    return buf[0], bool(buf[1]), buf[2]


def all_table_rows():
    """(box, gt, x, R, s) of every named row and every level's regressing anchors."""
    out = []
    for R in REG_MAXES:
        for k in NAMED:
            out.append(named_rows(R, PRIM_STRIDE[R])[k] + (R, PRIM_STRIDE[R]))
    for c in PRIM_CASES:
        out.append(prim_data(c) + (c["R"], c["s"]))
    for name in dict.fromkeys(c["name"] for c in LEVEL_CASES):
        c = next(x for x in LEVEL_CASES if x["name"] == name)
        r = level_rows(c)
        if len(r[0]):
            out.append(r + (c["shape"][5], c["s"]))
    return out


# ---- the tables are what they say ----------------------------------------------------------------------------------------
def test_every_row_keeps_the_branch_margin():
    for b, g, x, R, s in all_table_rows() + [random_rows(R)[:3] + (R, random_rows(R)[3]) for R in REG_MAXES]:
        m = branch_margin(b, g, x, R, s)
        assert m.min() >= MARGIN, (R, s, int(m.argmin()), float(m.min()))


@pytest.mark.parametrize("R", REG_MAXES)
def test_named_case_is_what_it_is_named(R):
    import torch
    s = PRIM_STRIDE[R]
    rows = named_rows(R, s)
    assert tuple(rows) == NAMED

    def parts(name):
        b, g, x = rows[name]
        xx = T._t64(np.asarray(x, np.float64).reshape(1, 4, R + 1))
        y = D.targets64(T._t64(b), T._t64(g), R, s).numpy()[0]
        raw = np.array([0.5 * (b[0, 0] + b[0, 2]) - g[0, 0], 0.5 * (b[0, 1] + b[0, 3]) - g[0, 1], g[0, 2] - 0.5 * (b[0, 0] + b[0, 2]),
                        g[0, 3] - 0.5 * (b[0, 1] + b[0, 3])], np.float64) / s
        _, _, q = D.rows64(T._t64(b), T._t64(g), xx, R, s, "giou")
        return y, raw, torch.softmax(xx, -1).numpy()[0], float(q[0]), x
    y, raw, p, q, x = parts("clamp0")
    assert (raw[:2] < 0).all() and (y[:2] == 0).all() and (raw[2:] > 0).all()
    y, raw, p, q, x = parts("clampR")
    assert (raw[[0, 2]] > R - 0.1).all() and np.allclose(y[[0, 2]], R - 0.1, rtol=0, atol=1e-12) and (y[[1, 3]] < R - 0.1).all()
    y, raw, p, q, x = parts("integer")
    assert (y == np.round(y)).all() and (y == raw).all()
    assert parts("peaked")[2].max(axis=1).min() > 0.99 and q >= 0
    assert np.allclose(parts("flat")[2], 1.0 / (R + 1), rtol=0, atol=1e-15)
    assert set(np.unique(parts("pm30")[4])) == {-30.0, 30.0}
    assert parts("disjoint")[3] == 0.0
    assert all(parts(k)[3] > 0.0 for k in NAMED if k != "disjoint")


@pytest.mark.parametrize("name", [s[0] for s in LEVEL_SHAPES])
def test_level_case_is_what_it_is_named(name):
    c = next(x for x in LEVEL_CASES if x["name"] == name)
    d = level_data(c)
    N, H, W, A, Cc, R = c["shape"]
    n_lvl, off = H * W * A, c["off"]
    ldc, ldr = level_ld(c)
    lab, m, n_i, a_i = D.level_positives(A, d["cls_labels"], d["matched"], LEVEL_G, off, n_lvl)
    route = level_route(c)
    from mxdetection_amd import _lib
    assert route[0] == _lib.ROUTE_KINDS["RETINA_LOSS_DFL"] and route[1] == (c["form"] == "vec")
    assert route[2] == (N * n_lvl + 255) // 256
    assert level_route(c, off_reg=4)[1] is False and level_route(c, off_cls=8)[1] is False       # unaligned views: scalar
    if name == "bg":
        assert len(n_i) == 0 and d["num_fg"] == 0
    else:
        assert len(n_i) >= 1 and d["num_fg"] >= len(n_i)
    if name == "tail":
        assert route[2] == 2 and (N * n_lvl) % 256 != 0 and R == 1
    if name == "c3":
        assert A == 2 and Cc % 8 and R + 1 == 8 and ldr == A * 4 * (R + 1)                         # no padding channel at all
    if name in ("coco", "offset", "one"):
        assert ldr == 128 and 4 * (R + 1) == 68
    if name == "offset":
        assert off > 0 and d["A_total"] > off + n_lvl
    if n_lvl > 4 and name != "bg":
        cl, mt = d["cls_labels"][0, off:], d["matched"][0, off:]
        assert cl[SPECIAL["ignored"]] < 0 and cl[SPECIAL["bg"]] == 0
        assert cl[SPECIAL["out_of_range"]] > 0 and mt[SPECIAL["out_of_range"]] == LEVEL_G
        assert d["cls_labels"][-1, off + 4] > 0 and d["matched"][-1, off + 4] == -1
        ref = level_ref(c)
        nb4 = 4 * (R + 1)
        for n, i in ((0, SPECIAL["out_of_range"]), (N - 1, 4), (0, SPECIAL["ignored"]), (0, SPECIAL["bg"])):
            assert ref["q"][n, i] == 0 and not ref["grad_reg"].reshape(N, H * W, ldr)[n, i // A, (i % A) * nb4:(i % A + 1) * nb4].any()
        assert (ref["q"][n_i, a_i] > 0).any()


# ---- tolerances ----------------------------------------------------------------------------------------------------------
def _pow2_ceil(x):
    return 2.0 ** math.ceil(math.log2(x))


@functools.lru_cache(maxsize=None)
def measure_fp32_error():
    import torch
    worst = {"grad": 0.0, "box": 0.0, "dfl": 0.0, "q": 0.0, "decode": 0.0}
    groups = all_table_rows() + [random_rows(R)[:3] + (R, random_rows(R)[3]) for R in REG_MAXES]
    for b, g, x, R, s in groups:
        n = len(b)
        with torch.no_grad():
            p64 = D.decode64(T._t64(b), T._t64(np.asarray(x, np.float64).reshape(n, 4, R + 1)), R, float(s))[0].numpy()
        worst["decode"] = max(worst["decode"], float(np.abs(D.decode_fp32(b, x.reshape(n, 4, R + 1), s) - p64).max()))
        for kind in KINDS:
            for rw, dw in WEIGHTS:
                r64 = D.ref_rows(b, g, x, R, s, kind, rw, dw)
                r32 = D.rows_fp32(b, g, x, R, s, kind, rw, dw)
                for k, a, e in zip(("box", "dfl", "q", "grad"), r32, r64):
                    worst[k] = max(worst[k], float(np.abs(a.astype(np.float64) - e).max()))
    return worst


def test_fp32_error_budget():
    w = measure_fp32_error()
    print("rows_fp32 vs float64 autograd, max error: grad %.4e box %.4e dfl %.4e q %.4e; decoded corner (px) %.4e"
          % (w["grad"], w["box"], w["dfl"], w["q"], w["decode"]))
    print("bounds by the x4 / power-of-two rule: " + " ".join("%s 2^%d" % (k, math.log2(_pow2_ceil(4 * w[k]))) for k in w))
    assert ATOL_GRAD == _pow2_ceil(4 * w["grad"]) and ATOL_BOX == _pow2_ceil(4 * w["box"])
    assert ATOL_DFL == _pow2_ceil(4 * w["dfl"]) and ATOL_Q == _pow2_ceil(4 * w["q"]) and ATOL_DECODE == _pow2_ceil(4 * w["decode"])
    for k in w:
        assert abs(w[k] - MEASURED[k]) <= 0.02 * MEASURED[k], (k, w[k])        # the docstring's figures are these


def test_references_are_sensitive_to_the_listed_mistakes():
    """Each mistake moves a result of the reference (and of the restatement, where it has the switch) past its bound."""
    for R in REG_MAXES:
        s = PRIM_STRIDE[R]
        rows = named_rows(R, s)
        b, g, x = (np.concatenate([rows[k][i] for k in NAMED]) for i in range(3))
        rw, dw = WEIGHTS[0]
        good64, good32 = D.ref_rows(b, g, x, R, s, "giou", rw, dw), D.rows_fp32(b, g, x, R, s, "giou", rw, dw)
        for mistake in ("quarter", "eps", "stride"):
            for good, fn in ((good64, D.ref_rows), (good32, D.rows_fp32)):
                bad = fn(b, g, x, R, s, "giou", rw, dw, mistake=mistake)
                d_dfl, d_grad = np.abs(bad[1] - good[1]).max(), np.abs(bad[3] - good[3]).max()
                print("R=%d %s %s: DFL moves %.3e, gradient %.3e" % (R, mistake, fn.__name__, d_dfl, d_grad))
                assert d_dfl > ATOL_DFL and d_grad > ATOL_GRAD
        bad = D.rows_fp32(b, g, x, R, s, "giou", rw, dw, mistake="k_not_k_minus_E")
        assert np.abs(bad[3] - good64[3]).max() > ATOL_GRAD and np.abs(good32[3] - good64[3]).max() <= ATOL_GRAD
    c = next(x for x in LEVEL_CASES if x["id"].startswith("coco-vec-qfl-giou"))
    d = level_data(c)
    N, H, W, A, Cc, R = c["shape"]
    bad = D.ref_level(d["cls"], d["reg"], A, Cc, d["cls_labels"], d["anchors"], d["matched"], d["gt"], c["off"], "qfl", c["alpha"],
                      c["gamma"], c["kind"], R, c["s"], c["rw"], c["dw"], d["num_fg"], float(c["ls"]), mistake="q_attached")
    good = level_ref(c)
    moved = np.abs(bad["grad_reg"] - good["grad_reg"]).max() / good["unit"]
    print("q not detached: grad_reg moves %.3e units" % moved)
    assert moved > ATOL_GRAD and np.array_equal(bad["loss"], good["loss"])


# ---- host-side validation (no GPU: every check happens before a launch) --------------------------------------------------
def test_entries_validate_their_arguments():
    from mxdetection_amd import _lib
    L = _lib.load()
    p, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 4)

    def err():
        return L.mxdet_last_error()

    def prim(boxes=p, gt=p, x=p, dtype=0, ld=68, n=5, R=16, s=8.0, kind=1, rw=2.0, dw=0.25, lb=p, ld_=p, q=p, grad=p):
        return L.mxdet_box_dist_loss(boxes, gt, x, dtype, ld, n, R, s, kind, rw, dw, 1.0, lb, ld_, q, grad, None)
    assert prim(n=0, boxes=None, gt=None, x=None, lb=None, ld_=None, q=None, grad=None) == 0 and err() == b""
    assert prim(n=-1) == -2 and prim(ld=67) == -2 and b"ld must be >= 4 * (reg_max + 1)" in err()
    assert prim(R=0) == -1 and prim(R=32) == -1 and b"reg_max" in err()
    assert prim(dtype=2) == -1 and b"dtype" in err()
    assert prim(kind=3) == -1 and b"kind" in err()
    assert prim(s=0.0) == -1 and prim(rw=0.0) == -1 and prim(dw=-1.0) == -1 and b"positive" in err()
    for k in ("boxes", "gt", "x", "lb", "ld_", "grad"):
        assert prim(**{k: None}) == -1 and b"null pointer" in err(), k
    assert prim(boxes=odd) == -1 and prim(gt=odd) == -1 and b"16-byte aligned" in err()

    def level(cls=p, reg=p, shape=(1, 3, 5, 2, 8), ldc=16, ldr=136, lab=p, anchors=p, m=p, gt=p, G=4, At=100, off=0, ck=1, gamma=2.0, kind=1,
              R=16, s=8.0, rw=2.0, dw=0.25, nfg=p, gc=p, gr=p, part=p):
        return L.mxdet_retina_loss_level_dfl(cls, reg, *shape, ldc, ldr, lab, anchors, m, gt, G, At, off, ck, 0.25, gamma, kind, R, s, rw, dw,
                                             nfg, 1.0, gc, gr, part, None)
    L.mxdet_debug_route_probe(1)
    try:
        assert level() == 0 and level(ck=0) == 0 and level(ck=2) == 0
        assert L.mxdet_debug_route_read((C.c_int32 * 64)(), 4) == 3
        L.mxdet_debug_route_probe(1)
        assert level(ldc=8) == -2 and b"bad shape" in err()
        assert level(ldr=135) == -2 and level(G=0) == -2
        assert level(At=29) == -2 and b"level outside the anchor range" in err()
        assert level(off=-1) == -2
        assert level(ck=3) == -1 and level(ck=-1) == -1 and b"cls_kind" in err()
        assert level(gamma=0.0) == -1 and b"gamma" in err()
        assert level(kind=7) == -1 and b"kind" in err()
        assert level(R=0) == -1 and level(R=32, ldr=1024) == -1 and b"reg_max" in err()
        assert level(s=-8.0) == -1 and level(rw=0.0) == -1 and level(dw=0.0) == -1 and b"positive" in err()
        for k in ("cls", "reg", "lab", "anchors", "m", "gt", "nfg", "gc", "gr", "part"):
            assert level(**{k: None}) == -1 and b"null pointer" in err(), k
        assert level(anchors=odd) == -1 and b"anchors must be 16-byte aligned" in err()
        assert L.mxdet_debug_route_read((C.c_int32 * 64)(), 4) == 0                 # a rejected call leaves no record
    finally:
        L.mxdet_debug_route_probe(0)

    d = _lib.PyramidT()
    d.num_levels, d.A, d.classes, d.dtype = 1, 8, 8, 1
    d.H[0], d.W[0], d.stride[0] = 2, 2, 8

    def det(pyr=C.byref(d), method=-1, sigma=0.5, R=16, ws=p, wsb=1 << 30, dets=p):
        return L.mxdet_retina_detect_dfl(pyr, 1, p, 100, 0.05, 0.5, 10, dets, p, ws, wsb, method, sigma, R, None)
    assert det(method=-2) == -1 and det(method=3) == -1 and b"method" in err()
    assert det(method=2, sigma=0.0) == -1 and b"sigma" in err()
    assert det(R=0) == -1 and det(R=32) == -1 and b"reg_max" in err()
    assert det(pyr=None) == -1 and det(dets=None) == -1 and b"null pointer" in err()
    assert det(wsb=16) == -3
    d.A = 9
    assert det() == -2 and b"multiple of classes" in err()


# ---- options: defaults, bad values, config, experiment file ---------------------------------------------------------------
BAD_OPTIONS = [(dict(reg_loss="giou", reg_max=-1), "reg_max"), (dict(reg_loss="giou", reg_max=32), "reg_max"),
               (dict(reg_loss="giou", reg_max=16.0), "reg_max"), (dict(reg_loss="giou", reg_max=True), "reg_max"),
               (dict(reg_max=16), "needs an IoU-family reg_loss"), (dict(reg_loss="giou", reg_max=16, dfl_weight=0.0), "dfl_weight"),
               (dict(reg_loss="giou", dfl_weight="0.25"), "dfl_weight")]


@pytest.mark.parametrize("kw,word", BAD_OPTIONS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(BAD_OPTIONS)])
def test_bad_reg_max_options_raise_before_any_allocation(kw, word, monkeypatch):
    from mxdetection_amd import models
    from mxdetection_amd.core.loss import check_reg_max
    from mxdetection_amd.models.rpn_heads.retina_head import RetinaHead
    from mxdetection_amd.models.utils import layers
    monkeypatch.setattr(layers.ParamArena, "finalize", lambda self: (_ for _ in ()).throw(AssertionError("allocated")))
    monkeypatch.setattr(layers.ParamArena, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("allocated")))
    with pytest.raises(ValueError, match=word):
        models.RetinaNet("cuda", **kw)
    with pytest.raises(ValueError, match=word):
        RetinaHead(256, [8, 16, 32, 64, 128], None, None, "cuda", None, **kw)
    with pytest.raises(ValueError, match=word):
        check_reg_max(kw.get("reg_max", 0), kw.get("reg_loss", "smooth_l1"), kw.get("dfl_weight", 0.25))


def test_check_reg_max_accepts_the_range_and_detect_checks_its_own():
    from mxdetection_amd.core.evaluation import RetinaDetect
    from mxdetection_amd.core.loss import REG_MAX_LIMIT, check_reg_max
    assert REG_MAX_LIMIT == 31
    check_reg_max(0, "smooth_l1", 0.25)
    for kind in KINDS:
        check_reg_max(1, kind, 0.25)
        check_reg_max(31, kind, 1)
    for bad in (-1, 32, 1.0, True):
        with pytest.raises(ValueError, match="reg_max"):
            RetinaDetect(80, [8], [None], reg_max=bad)
    assert RetinaDetect(80, [8], [None]).reg_max == 0 and RetinaDetect(80, [8], [None], reg_max=16).reg_max == 16


def test_box_dist_loss_checks_the_row_strides():
    """grad_logits shares the leading dimension of logits: another row stride, dtype or a strided row is a ValueError (raised
    before the launch, so on a machine without a GPU too)."""
    import torch
    from mxdetection_amd.core.loss import box_dist_loss
    b = torch.zeros((3, 4))
    x = torch.zeros((3, 80))[:, :68]
    for bad in (torch.zeros((3, 68)), torch.zeros((3, 80), dtype=torch.bfloat16)[:, :68], torch.zeros((3, 160))[:, :136:2],
                torch.zeros((3, 80))[:, :64]):
        with pytest.raises(ValueError, match="grad_logits must hold rows"):
            box_dist_loss(b, b, x, 16, 8.0, grad_logits=bad)
    with pytest.raises(ValueError, match="logits must hold rows"):
        box_dist_loss(b, b, torch.zeros((3, 136))[:, ::2], 16, 8.0)


def test_config_defaults_are_todays_model_and_the_builder_plumbs_the_keys(monkeypatch):
    import inspect
    from mxdetection_amd import models
    from mxdetection_amd.core.evaluation import RetinaDetect
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.models.rpn_heads.retina_head import RetinaHead
    from mxdetection_amd.utils.config import DEFAULTS, load_config
    assert DEFAULTS["network"]["reg_max"] == 0 and DEFAULTS["network"]["dfl_weight"] == 0.25
    seen = []
    monkeypatch.setattr(models, "FasterRCNN", lambda device, **kw: seen.append(("frcnn", kw)) or "m")
    monkeypatch.setattr(models, "RetinaNet", lambda device, **kw: seen.append(("retina", kw)) or "m")
    build_detector(load_config(None, ["network.type=retinanet"]))
    assert seen[-1][1]["reg_max"] == 0 and seen[-1][1]["dfl_weight"] == 0.25
    build_detector(load_config(None, ["network.type=retinanet", "network.reg_loss=giou", "network.reg_max=16", "network.dfl_weight=0.5"]))
    assert seen[-1][1]["reg_max"] == 16 and seen[-1][1]["dfl_weight"] == 0.5
    for typ in ("faster_rcnn", "mask_rcnn"):
        build_detector(load_config(None, ["network.type=" + typ]))
        assert "reg_max" not in seen[-1][1]
        with pytest.raises(ValueError, match="reg_max"):
            build_detector(load_config(None, ["network.type=" + typ, "network.reg_loss=giou", "network.reg_max=16"]))
    monkeypatch.undo()
    for cls in (models.RetinaNet, RetinaHead):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["reg_max"].default == 0 and sig["dfl_weight"].default == 0.25
    assert inspect.signature(RetinaDetect.__init__).parameters["reg_max"].default == 0


def test_the_gfl_experiment_file_loads():
    from mxdetection_amd.utils.config import load_config
    f = load_config(os.path.join(ROOT, "configs", "retinanet_r101_fpn_gfl.yaml"))
    q = load_config(os.path.join(ROOT, "configs", "retinanet_r101_fpn_atss_qfl.yaml"))
    assert (f.network.reg_max, f.network.dfl_weight, f.network.reg_loss, f.network.reg_loss_weight) == (16, 0.25, "giou", 2.0)
    assert (f.network.cls_loss, f.network.assigner, list(f.network.anchor_ratios), f.network.anchor_scale) == ("qfl", "atss", [1.0], 8.0)
    assert q.network.reg_max == 0
    same = {k: v for k, v in f.network.items() if k not in ("reg_max", "dfl_weight")}
    assert same == {k: v for k, v in q.network.items() if k not in ("reg_max", "dfl_weight")}
    assert {k: v for k, v in f.TRAIN.items()} == {k: v for k, v in q.TRAIN.items()}
