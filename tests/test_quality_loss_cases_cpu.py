"""Case tables and CPU proofs of the quality-aware class losses (mxdet_quality_focal_loss, mxdet_retina_loss_level_quality in
csrc/losses.hip / retina_loss.hip). tests/test_gpu_quality_loss.py runs the same tables on the GPU; the references are in
tests/_quality_loss_ref.py.

Level tables: the four RETINA_SHAPES of tests/test_iou_loss_cases_cpu.py on THEIR data (boxes, deltas, labels, logits) plus
(2,5,7,1,80), the one-anchor ATSS layout, drawn the same way, crossed with {qfl beta=2, qfl beta=1.5, vfl} x {giou, iou} x
loss_scale {1, 512} x num_fg {true, 0}; and "coco_bg", the coco shape with every label <= 0 (a level with no foreground).
Two things are laid over that data (level_data):
  * the logits are clipped to [-6.5, 6.5] (sigmoid >= 1.5e-3), so that with beta != 2 no element of any table lies within
    MARGIN_E = 2^-10 of sigmoid == y, where |e|^beta is not smooth (test_no_element_sits_on_sigma_equals_y; nothing is
    excluded at comparison time). Logits beyond that are in the primitive's hand table (beta = 2 and vfl only);
  * levels of more than 8 anchors get four constructed rows in image 0: anchor 3 matched with a prediction that misses
    its ground truth (q == 0: a negative in its own column), anchor 4 nearly on it (q > 0.9), anchors 5 and 6 foreground with
    matches G_max and -1 (outside gt_boxes: q = 0, nothing regressed); anchors 1, 2 are ignore / background as before.

Tolerances, by the rule of DESIGN.md 5f (test_fp32_error_budget measures and bounds them): the numpy float32 restatement
(quality_fp32 + cls_elem_fp32 of tests/_quality_loss_ref.py, oracle.expf / oracle.logf) against the float64 reference over
every row of the level tables and of the primitive's tables (its logits reach +-90: the loss figure is theirs) plus
N_RANDOM = 100 000 seeded random anchors (the random rows of the IoU-loss module at stds 1, C = 8 logits
each, 70 % foreground), all three class settings; bound = largest difference x 4, rounded up to a power of two.
                                                        measured       bound
  class gradient / (inv * loss_scale)                   8.24e-7      ATOL_CLS_GRAD = 2^-18
  per-anchor class loss (sum over the C columns)        2.32e-5      ATOL_CLS_LOSS = 2^-13
bf16 outputs add 2^-8 * |ref|. Summed losses: LOSS_RTOL of the float64 sum on top of ATOL_CLS_LOSS per summed anchor.
"""
import ctypes as C
import functools
import math
import os
import zlib

import numpy as np
import pytest

import _quality_loss_ref as Q
import test_iou_loss_cases_cpu as T

ROOT = T.ROOT
MARGIN_E = 2.0 ** -10
LOGIT_CLIP = 6.5
MEASURED = {"grad": 8.2383e-07, "loss": 2.3230e-05}                     # the figures of the docstring, in full
ATOL_CLS_GRAD = 2.0 ** -18
ATOL_CLS_LOSS = 2.0 ** -13
BF16_STEP, LOSS_RTOL, N_RANDOM = T.BF16_STEP, T.LOSS_RTOL, T.N_RANDOM
STDS = T.STDS[T.RETINA_STDS]

CLS_SETTINGS = (("qfl2", "qfl", 0.0, 2.0), ("qfl1.5", "qfl", 0.0, 1.5), ("vfl", "vfl", 0.75, 2.0))
REG_KINDS = ("giou", "iou")
SHAPES = tuple(T.RETINA_SHAPES) + (("atss1", (2, 5, 7, 1, 80), "vec", 0),)
SPECIAL = {"miss": 3, "hit": 4, "m_high": 5, "m_neg": 6}


def _cases():
    out = []
    for name, shape, form, off in SHAPES:
        for cid, cls_loss, alpha, gamma in CLS_SETTINGS:
            for kind in REG_KINDS:
                for ls in (1, 512):
                    for nfg in ("true", "zero"):
                        out.append({"id": "%s-%s-%s-%s-ls%d-nfg%s" % (name, form, cid, kind, ls, nfg), "name": name, "shape": shape,
                                    "form": form, "off": off, "cls_id": cid, "cls_loss": cls_loss, "alpha": alpha, "gamma": gamma,
                                    "kind": kind, "ls": ls, "nfg": nfg, "rw": 2.0 if kind == "giou" else 1.0})
    for i, (cid, cls_loss, alpha, gamma) in enumerate(CLS_SETTINGS):         # a level with no foreground
        out.append({"id": "coco_bg-vec-%s-giou-ls%d-nfgzero" % (cid, (1, 512)[i % 2]), "name": "coco_bg", "shape": (2, 3, 5, 9, 80),
                    "form": "vec", "off": 0, "cls_id": cid, "cls_loss": cls_loss, "alpha": alpha, "gamma": gamma, "kind": "giou",
                    "ls": (1, 512)[i % 2], "nfg": "zero", "rw": 2.0})
    return out


CASES = _cases()
DATA_NAMES = tuple(s[0] for s in SHAPES) + ("coco_bg",)
ids = T.ids
retina_ld = T.retina_ld


def _shape_of(name):
    return next(c for c in CASES if c["name"] == name)


def _draw_level(name, shape, off):
    """A level drawn as tests/test_iou_loss_cases_cpu.py draws its RETINA_SHAPES (for the shape it does not have)."""
    rng = np.random.default_rng(zlib.crc32(("retina-" + name).encode()))
    N, H, W, A, Cc = shape
    ldc, ldr = retina_ld({"shape": shape})
    n_lvl, G = H * W * A, T.RETINA_G
    At = off + n_lvl + (11 if off else 0)
    gt = np.zeros((N, G, 5), np.float32)
    gt[0, :, :4] = T.draw_boxes(rng, G)
    for n in range(1, N):
        gt[n, :, :4] = T.jitter(rng, gt[0, :, :4])
    gt[..., 4] = rng.integers(1, Cc + 1, (N, G))
    near = np.arange(At) % G
    anchors = T.jitter(rng, gt[0, near, :4])
    matched = np.tile(near.astype(np.int32), (N, 1))
    labels = rng.choice([-1, 0, 1], size=(N, At), p=[0.15, 0.45, 0.4]).astype(np.int32)
    labels[0, off], labels[-1, off + n_lvl - 1] = 1, 1
    labels[0, off + 1], labels[0, off + 2] = -1, 0
    cls_labels = np.where(labels == 1, gt[np.arange(N)[:, None], matched, 4].astype(np.int32), labels).astype(np.int32)
    reg = T.bf16r(rng.standard_normal((N, H, W, ldr)) * 0.5)
    n_i, a_i = np.nonzero(labels[:, off:off + n_lvl] > 0)
    reg.reshape(N, H * W, ldr)[n_i[:, None], (a_i // A)[:, None], 4 * (a_i % A)[:, None] + np.arange(4)] = T.draw_deltas(
        rng, anchors[off + a_i], gt[n_i, matched[n_i, off + a_i], :4], STDS)
    return {"cls": T.bf16r(rng.standard_normal((N, H, W, ldc)) * 2 - 2), "reg": reg, "anchors": anchors, "matched": matched, "gt": gt,
            "cls_labels": cls_labels, "A_total": At}


@functools.lru_cache(maxsize=None)
def _level_data(name):
    c = _shape_of(name)
    N, H, W, A, Cc = c["shape"]
    off, n_lvl = c["off"], H * W * A
    if name == "atss1":
        src = _draw_level(name, c["shape"], off)
    else:
        src = T._retina_data("coco" if name == "coco_bg" else name)
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in src.items()}
    d["cls"] = np.clip(d["cls"], -LOGIT_CLIP, LOGIT_CLIP).astype(np.float32)
    assert np.array_equal(T.bf16r(d["cls"]), d["cls"])
    if name == "coco_bg":
        lv = d["cls_labels"][:, off:off + n_lvl]
        d["cls_labels"][:, off:off + n_lvl] = np.minimum(lv, 0)
    elif n_lvl > 8:
        regv = d["reg"].reshape(N, H * W, -1)
        for key, al in SPECIAL.items():
            gi = off + al
            m = d["matched"][0, gi]
            d["cls_labels"][0, gi] = int(d["gt"][0, m, 4])
            if key == "miss":       # the centre moves 8 widths: no overlap
                regv[0, al // A, 4 * (al % A):4 * (al % A) + 4] = (8.0, 0.0, 0.0, 0.0)
            elif key == "hit":      # the anchor IS image 0's box, the prediction 1/64 of its width beside it
                d["anchors"][gi] = d["gt"][0, m, :4]
                regv[0, al // A, 4 * (al % A):4 * (al % A) + 4] = (2.0 ** -6, 0.0, 0.0, 0.0)
                for n in range(1, N):                                    # other images: keep this anchor out of the box term
                    d["cls_labels"][n, gi] = min(d["cls_labels"][n, gi], 0)
            elif key == "m_high":
                d["matched"][0, gi] = T.RETINA_G
            else:
                d["matched"][0, gi] = -1
    d["num_fg_true"] = int((d["cls_labels"] > 0).sum())
    return d


def level_data(c):
    return _level_data(c["name"])


def num_fg(c):
    return level_data(c)["num_fg_true"] if c["nfg"] == "true" else 0


@functools.lru_cache(maxsize=None)
def _level_ref(name, cls_id):
    """The float64 reference at inv = 1, loss_scale = 1 (both are plain factors)."""
    c = next(x for x in CASES if x["name"] == name and x["cls_id"] == cls_id)
    d = _level_data(name)
    N, H, W, A, Cc = c["shape"]
    return Q.ref_retina_quality(d["cls"], d["reg"], A, Cc, d["cls_labels"], d["anchors"], d["matched"], d["gt"], c["off"], c["cls_loss"],
                                c["alpha"], c["gamma"], STDS, 0, 1.0)


def level_ref(c):
    """loss, grad_cls, unit of the case (its num_fg and loss_scale applied to the cached unit-scale reference)."""
    r = _level_ref(c["name"], c["cls_id"])
    inv = 1.0 / max(1, num_fg(c))
    return {"loss": r["loss"] * inv, "grad_cls": r["grad_cls"] * (inv * c["ls"]), "unit": inv * c["ls"], "inv": inv,
            "n_valid": r["n_valid"], "q": r["q"], "per_anchor": r["per_anchor"]}


# ---- the primitive's tables -------------------------------------------------------------------------------------------
PRIM_N = (1, 3, 65, 257)
PRIM_C = (1, 8, 80)


def _prim_cases():
    out, i = [], 0
    for n in PRIM_N:
        for Cc in PRIM_C:
            for cid, cls_loss, alpha, gamma in CLS_SETTINGS:
                out.append({"id": "n%d-C%d-%s-gs%d" % (n, Cc, cid, (1, 512)[i % 2]), "n": n, "C": Cc, "cls_id": cid, "cls_loss": cls_loss,
                            "alpha": alpha, "gamma": gamma, "gs": (1, 512)[i % 2], "name": "random"})
                i += 1
    for cid, cls_loss, alpha, gamma in CLS_SETTINGS:
        if gamma == 2.0:
            out.append({"id": "extreme-%s" % cid, "n": 26, "C": 2, "cls_id": cid, "cls_loss": cls_loss, "alpha": alpha, "gamma": gamma,
                        "gs": 1, "name": "extreme"})
        out.append({"id": "all_bg-%s" % cid, "n": 65, "C": 8, "cls_id": cid, "cls_loss": cls_loss, "alpha": alpha, "gamma": gamma,
                    "gs": 512, "name": "all_bg"})
    return out


PRIM_CASES = _prim_cases()


def _nudge(x, y, rng=None):
    """Logits moved by +1 (at most four times) where sigmoid(x) is within 2 * MARGIN_E of y; bf16-exact, inside the clip."""
    x = np.array(x, np.float32)
    for _ in range(4):
        s = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
        bad = np.abs(s - y) < 2 * MARGIN_E
        if not bad.any():
            return x
        x = np.where(bad, np.where(x > 0, x - 1.0, x + 1.0), x).astype(np.float32)
    raise AssertionError("elements on sigma == y after four nudges")


@functools.lru_cache(maxsize=None)
def _prim_data(n, Cc, name):
    rng = np.random.default_rng(zlib.crc32(("qprim-%d-%d-%s" % (n, Cc, name)).encode()))
    if name == "extreme":       # logits out to +-90 against y in {0, 0.5, 1}, both columns (beta = 2 / vfl only)
        xs = np.array([-90.0, -40.0, -17.0, -9.0, -1.0, 0.0, 1.0, 9.0, 17.0, 40.0, 90.0, 3.0, -3.0], np.float32)
        x = np.stack([np.concatenate([xs, xs]), np.concatenate([xs[::-1], xs])], axis=1)
        labels = np.array([1] * 13 + [2] * 6 + [0] * 5 + [-1] * 2, np.int32)
        quality = np.tile(np.array([0.5, 1.0, 0.0], np.float32), 9)[:26]
        return {"x": x, "labels": labels, "q": quality}
    labels = rng.choice(np.arange(-1, Cc + 1), size=n, p=[0.1, 0.3] + [0.6 / Cc] * Cc).astype(np.int32)
    if name == "all_bg":
        labels = rng.choice([-1, 0, 0], size=n).astype(np.int32)
    else:
        labels[0] = Cc
        if n >= 3:
            labels[1], labels[2] = -1, 0
    quality = rng.uniform(0.0, 1.0, n).astype(np.float32)
    if n >= 65 and name == "random":
        quality[3], labels[3] = 0.0, 1                                   # foreground with q == 0
    x = T.bf16r(np.clip(rng.standard_normal((n, Cc)) * 2.5 - 1.0, -LOGIT_CLIP, LOGIT_CLIP))
    y, _ = Q.targets64(labels, quality, Cc)
    return {"x": T.bf16r(_nudge(x, y)), "labels": labels, "q": quality}


def prim_data(c):
    return _prim_data(c["n"], c["C"], c["name"])


@functools.lru_cache(maxsize=None)
def _prim_ref(cid):
    c = next(x for x in PRIM_CASES if x["id"] == cid)
    d = prim_data(c)
    return Q.ref_primitive(d["x"], d["labels"], d["q"], c["cls_loss"], c["alpha"], c["gamma"], float(c["gs"]))


def prim_ref(c):
    return _prim_ref(c["id"])


# ---------------------------------------------------------------------------------------------------------------------
# proofs
# ---------------------------------------------------------------------------------------------------------------------
def test_tables_cover_the_listed_values():
    assert [s[1] for s in SHAPES] == [(1, 1, 1, 1, 8), (2, 3, 5, 9, 80), (1, 2, 2, 9, 3), (2, 7, 9, 9, 80), (2, 5, 7, 1, 80)]
    for name, *_ in SHAPES:
        sub = [c for c in CASES if c["name"] == name]
        assert len(sub) == 3 * 2 * 2 * 2
        assert {(c["cls_id"], c["kind"], c["ls"], c["nfg"]) for c in sub} == {(a[0], k, ls, nf) for a in CLS_SETTINGS for k in REG_KINDS
                                                                              for ls in (1, 512) for nf in ("true", "zero")}
    assert {(c["cls_loss"], c["gamma"]) for c in CASES} == {("qfl", 2.0), ("qfl", 1.5), ("vfl", 2.0)}
    assert len(set(ids(CASES))) == len(CASES) and len(set(ids(PRIM_CASES))) == len(PRIM_CASES)
    for name, *_ in T.RETINA_SHAPES:                                      # the IoU module's data, not a redraw
        a, b = _level_data(name), T._retina_data(name)
        assert np.array_equal(a["gt"], b["gt"]) and np.array_equal(a["cls"], np.clip(b["cls"], -LOGIT_CLIP, LOGIT_CLIP))
        assert np.mean(a["reg"] == b["reg"]) > 0.9 or a["reg"].size < 100


@pytest.mark.parametrize("name", DATA_NAMES)
def test_fixture_reaches_its_branches(name):
    c = _shape_of(name)
    d, r = _level_data(name), _level_ref(name, "vfl")
    N, H, W, A, Cc = c["shape"]
    n_lvl, off = H * W * A, c["off"]
    lv = d["cls_labels"][:, off:off + n_lvl]
    q = r["q"]
    assert {"one": N * n_lvl == 1, "coco": N * n_lvl > 256, "c3": Cc % 8 != 0, "offset": off > 0 and N * n_lvl > 1024,
            "atss1": A == 1 and Cc % 8 == 0, "coco_bg": lv.max() <= 0}[name]
    assert np.all(q[lv <= 0] == 0) and q.min() >= 0.0 and q.max() <= 1.0
    if name == "coco_bg":
        assert not q.any() and np.any(lv == 0) and np.any(lv == -1)
        return
    if n_lvl <= 8:
        assert lv[0, 0] > 0 and 0.0 < q[0, 0] < 1.0
        return
    m = d["matched"][0, off:off + n_lvl]
    assert lv[0, 1] == -1 and lv[0, 2] == 0 and not r["grad_cls"][..., :A * Cc].reshape(N, n_lvl, Cc)[0, 1].any()
    assert lv[0, SPECIAL["miss"]] > 0 and 0 <= m[SPECIAL["miss"]] < T.RETINA_G and q[0, SPECIAL["miss"]] == 0.0
    assert lv[0, SPECIAL["hit"]] > 0 and 0.9 < q[0, SPECIAL["hit"]] < 1.0
    assert lv[0, SPECIAL["m_high"]] > 0 and m[SPECIAL["m_high"]] == T.RETINA_G and q[0, SPECIAL["m_high"]] == 0.0
    assert lv[0, SPECIAL["m_neg"]] > 0 and m[SPECIAL["m_neg"]] == -1 and q[0, SPECIAL["m_neg"]] == 0.0
    # a matched anchor with q == 0 is a negative in its own column: the Varifocal gradient there is the negatives' (> 0)
    col = lv[0, SPECIAL["miss"]] - 1
    assert r["grad_cls"][..., :A * Cc].reshape(N, n_lvl, Cc)[0, SPECIAL["miss"], col] > 0
    assert np.count_nonzero((lv > 0) & (q > 0)) >= 2
    if name == "offset":                                                  # positives in at least two workgroups, a part-empty last one
        wg = np.nonzero((lv > 0).reshape(-1))[0] // 256
        assert len(set(wg.tolist())) >= 2 and (N * n_lvl) % 256 != 0 and (N * n_lvl + 255) // 256 == 5
        assert d["num_fg_true"] > int((lv > 0).sum())


def _sigma_margin(x, y, valid):
    s = 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))
    return float(np.min(np.where(valid > 0, np.abs(s - y), np.inf)))


def test_no_element_sits_on_sigma_equals_y():
    """beta != 2: |e|^beta is not smooth at e = 0; every element of every table keeps MARGIN_E from it (nothing is excluded)."""
    for name in DATA_NAMES:
        c = _shape_of(name)
        d, r = _level_data(name), _level_ref(name, "qfl1.5")
        N, H, W, A, Cc = c["shape"]
        lv = d["cls_labels"][:, c["off"]:c["off"] + H * W * A]
        y, valid = Q.targets64(lv, r["q"], Cc)
        x = d["cls"][..., :A * Cc].reshape(N, H * W * A, Cc)
        assert _sigma_margin(x, y, valid * np.ones_like(y)) >= MARGIN_E, name
    for c in PRIM_CASES:
        if c["gamma"] != 2.0:
            d = prim_data(c)
            y, valid = Q.targets64(d["labels"], d["q"], c["C"])
            assert _sigma_margin(d["x"], y, valid * np.ones_like(y)) >= MARGIN_E, c["id"]
    x, y, valid = random_rows()[:3]
    assert _sigma_margin(x, y, valid * np.ones_like(y)) >= MARGIN_E


def test_hand_computed_elements():
    """x = 0: sigma = 1/2 and both logs are -ln 2, so BCE(1/2, y) = ln 2 for every y."""
    ln2 = math.log(2.0)
    want = {("qfl", 0.75): (0.0625 * ln2, 2 * -0.25 * 0.25 * ln2 + 0.0625 * -0.25),       # e = -1/4
            ("qfl", 0.0): (0.25 * ln2, 2 * 0.5 * 0.25 * ln2 + 0.125),                     # e = 1/2
            ("vfl", 0.75): (0.75 * ln2, 0.75 * -0.25),
            ("vfl", 0.0): (0.75 * 0.25 * ln2, 0.75 * (2 * 0.25 * 0.5 * ln2 + 0.25 * 0.5))}
    for (kind, y), (L, G) in want.items():
        l64, g64 = Q.ref_elems(np.zeros(1), np.array([y]), kind, 0.75, 2.0)
        assert abs(l64[0] - L) < 1e-15 and abs(g64[0] - G) < 1e-15, (kind, y)
        l32, g32 = Q.cls_elem_fp32(np.zeros(1), np.array([y]), kind, 0.75, 2.0)
        assert abs(l32[0] - L) < 1e-7 and abs(g32[0] - G) < 1e-7, (kind, y)
    # beta = 1.5 at e = 1/4 (x = 0, y = 1/4): |e|^1.5 = 1/8
    l64, g64 = Q.ref_elems(np.zeros(1), np.array([0.25]), "qfl", 0.0, 1.5)
    assert abs(l64[0] - 0.125 * ln2) < 1e-15 and abs(g64[0] - (1.5 * 0.5 * 0.25 * ln2 + 0.125 * 0.25)) < 1e-15
    l32, g32 = Q.cls_elem_fp32(np.zeros(1), np.array([0.25]), "qfl", 0.0, 1.5)
    assert abs(l32[0] - l64[0]) < 1e-7 and abs(g32[0] - g64[0]) < 1e-7
    # y = sigma exactly (x = 0, y = 1/2): QFL is 0 with gradient 0; beta != 2 goes through max(|e|, 1e-30) and the smallest
    # normal float of expf, which leaves 1.5 * 1.2e-38 / 1e-30 * s (1 - s) BCE = 4e-9
    for beta, tiny in ((2.0, 0.0), (1.5, 1e-8)):
        l32, g32 = Q.cls_elem_fp32(np.zeros(1), np.array([0.5]), "qfl", 0.0, beta)
        assert abs(l32[0]) < 1e-30 and abs(g32[0]) <= tiny
    # the quality is a constant: the class loss has no gradient with respect to it in the reference
    import torch
    z, y = T._t64(np.zeros(1), True), T._t64(np.array([0.75]), True)
    with pytest.raises(AssertionError):
        Q.cls_elems64(z, y, "qfl", 0.0, 2.0)


def test_qfl_beta2_negatives_are_the_focal_negatives():
    """y == 0: QFL(beta = 2) = sigma^2 * (-log(1 - sigma)) = the focal negative term divided by (1 - alpha)."""
    from test_loss_cases_cpu import focal_fp32
    x = T.bf16r(np.linspace(-20, 20, 321))
    lq, gq = Q.cls_elem_fp32(x, np.zeros_like(x), "qfl", 0.0, 2.0)
    lf, gf = focal_fp32(x, False, 0.25, 2.0)
    assert np.allclose(lq, lf / 0.75, rtol=2e-6, atol=0) and np.allclose(gq, gf / 0.75, rtol=2e-6, atol=1e-30)


# ---- route probe --------------------------------------------------------------------------------------------------------
def quality_route(c, off_reg=0):
    """(kind word, vec, grid) of mxdet_retina_loss_level_quality as the library's selector reports it (no device)."""
    from mxdetection_amd import _lib
    L = _lib.load()
    N, H, W, A, Cc = c["shape"]
    ldc, ldr = retina_ld(c)
    base = 1 << 20
    p, pr = C.c_void_p(base), C.c_void_p(base + off_reg)
    L.mxdet_debug_route_probe(1)
    try:
        rc = L.mxdet_retina_loss_level_quality(p, pr, N, H, W, A, Cc, ldc, ldr, p, p, p, p, T.RETINA_G, c["off"] + H * W * A + 11, c["off"],
                                               _lib.CLS_LOSS_KINDS[c["cls_loss"]], c["alpha"], c["gamma"], 1, 1.0, 1.0, 1.0, 1.0, c["rw"], p,
                                               float(c["ls"]), p, pr, p, None)
        assert rc == 0, L.mxdet_last_error()
        buf = (C.c_int32 * 64)()
        assert L.mxdet_debug_route_read(buf, 4) == 1
    finally:
        L.mxdet_debug_route_probe(0)
    assert not any(buf[3:16])
    return buf[0], bool(buf[1]), buf[2]


@pytest.mark.parametrize("name", DATA_NAMES)
def test_route_is_the_iou_entrys(name):
    from mxdetection_amd import _lib
    c = _shape_of(name)
    N, H, W, A, Cc = c["shape"]
    kind, vec, grid = quality_route(c)
    ikind, ivec, igrid = T.retina_iou_route(c)
    assert kind == _lib.ROUTE_KINDS["RETINA_LOSS_QUALITY"] == 7 and ikind == _lib.ROUTE_KINDS["RETINA_LOSS_IOU"]
    assert (vec, grid) == (ivec, igrid) and vec == (c["form"] == "vec")
    assert grid == _lib.load().mxdet_retina_loss_num_partials(N, H, W, A) == (N * H * W * A + 255) // 256
    assert quality_route(c, off_reg=4)[1] is False and T.retina_iou_route(c, off_reg=4)[1] is False


# ---- host-side validation (no GPU: every check happens before a launch) ------------------------------------------------
def test_entries_validate_their_arguments():
    from mxdetection_amd import _lib
    L = _lib.load()
    p, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 4)

    def err():
        return L.mxdet_last_error()

    def prim(logits=p, dtype=1, labels=p, quality=p, n=5, Cc=8, ck=1, alpha=0.75, gamma=2.0, loss=p, grad=p, ws=p, wsb=1 << 20):
        return L.mxdet_quality_focal_loss(logits, dtype, labels, quality, n, Cc, ck, alpha, gamma, 1.0, loss, grad, ws, wsb, None)
    assert prim(n=-1) == -2 and prim(Cc=0) == -2 and b"bad shape" in err()
    assert prim(dtype=2) == -1 and b"dtype" in err()
    assert prim(ck=0) == -1 and b"cls_kind" in err() and prim(ck=3) == -1 and b"cls_kind" in err()
    assert prim(gamma=0.0) == -1 and b"gamma" in err() and prim(gamma=-1.0) == -1
    for k in ("logits", "labels", "quality", "loss", "grad"):
        assert prim(**{k: None}) == -1 and b"null pointer" in err(), k
    assert prim(n=0, loss=None) == -1
    assert prim(ws=None) == -3 and prim(wsb=16) == -3 and b"workspace too small" in err()

    def retina(cls=p, reg=p, shape=(1, 3, 5, 3, 8), ldc=24, ldr=12, lab=p, anchors=p, m=p, gt=p, G=4, At=100, off=0, ck=2, gamma=2.0, kind=1,
               stds=(1.0,) * 4, w=1.0, nfg=p, gc=p, gr=p, part=p):
        return L.mxdet_retina_loss_level_quality(cls, reg, *shape, ldc, ldr, lab, anchors, m, gt, G, At, off, ck, 0.75, gamma, kind, *stds, w,
                                                 nfg, 1.0, gc, gr, part, None)
    # the checks and messages of mxdet_retina_loss_level_iou ...
    assert retina(ldc=16) == -2 and b"bad shape" in err()
    assert retina(ldr=8) == -2 and retina(G=0) == -2
    assert retina(At=44) == -2 and b"level outside the anchor range" in err()
    assert retina(off=-1) == -2
    assert retina(kind=7) == -1 and b"kind must be MXDET_IOU_LOSS_IOU, _GIOU or _DIOU" in err()
    assert retina(w=-1.0) == -1 and retina(stds=(0.0, 1.0, 1.0, 1.0)) == -1 and b"positive" in err()
    for k in ("cls", "reg", "lab", "anchors", "m", "gt", "nfg", "gc", "gr", "part"):
        assert retina(**{k: None}) == -1 and b"null pointer" in err(), k
    assert retina(anchors=odd) == -1 and b"anchors must be 16-byte aligned" in err()
    # ... and its own two
    assert retina(ck=0) == -1 and b"cls_kind" in err() and retina(ck=3) == -1 and b"cls_kind" in err()
    assert retina(gamma=0.0) == -1 and b"gamma" in err() and retina(gamma=-2.0) == -1 and b"gamma" in err()
    L.mxdet_debug_route_probe(1)
    try:
        assert retina(ldc=16) == -2 and retina(cls=None) == -1 and retina(ck=9) == -1
        assert L.mxdet_debug_route_read((C.c_int32 * 64)(), 4) == 0
    finally:
        L.mxdet_debug_route_probe(0)


# ---- options: defaults, bad values, config, experiment files ----------------------------------------------------------
BAD_OPTIONS = [(dict(cls_loss="gfl", reg_loss="giou"), "cls_loss must be one of"),
               (dict(cls_loss="qfl"), "needs an IoU-family reg_loss"),
               (dict(cls_loss="vfl", reg_loss="smooth_l1"), "needs an IoU-family reg_loss"),
               (dict(cls_loss="qfl", reg_loss="giou", cls_loss_gamma=0.0), "cls_loss_gamma"),
               (dict(cls_loss="vfl", reg_loss="giou", cls_loss_gamma="2"), "cls_loss_gamma"),
               (dict(cls_loss="vfl", reg_loss="giou", cls_loss_alpha=1.5), "cls_loss_alpha"),
               (dict(cls_loss="focal", cls_loss_gamma=-1.0), "cls_loss_gamma")]


@pytest.mark.parametrize("kw,word", BAD_OPTIONS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(BAD_OPTIONS)])
def test_bad_cls_loss_options_raise_before_any_allocation(kw, word, monkeypatch):
    from mxdetection_amd import models
    from mxdetection_amd.core import loss as L
    from mxdetection_amd.models.rpn_heads.retina_head import RetinaHead
    from mxdetection_amd.models.utils import layers
    monkeypatch.setattr(layers.ParamArena, "finalize", lambda self: (_ for _ in ()).throw(AssertionError("allocated")))
    monkeypatch.setattr(layers.ParamArena, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("allocated")))
    with pytest.raises(ValueError, match=word):
        models.RetinaNet("cuda", **kw)
    with pytest.raises(ValueError, match=word):
        RetinaHead(256, [8, 16, 32, 64, 128], None, None, "cuda", None, **kw)
    with pytest.raises(ValueError, match=word):
        L.check_cls_loss(kw["cls_loss"], kw.get("reg_loss", "smooth_l1"), kw.get("cls_loss_alpha"), kw.get("cls_loss_gamma"))


def test_check_cls_loss_gives_the_published_defaults():
    from mxdetection_amd.core import loss as L
    assert L.check_cls_loss("focal", "smooth_l1") is None and L.check_cls_loss("focal", "giou", 0.3, 1.5) is None
    assert L.check_cls_loss("qfl", "giou") == (0.0, 2.0) and L.check_cls_loss("vfl", "iou") == (0.75, 2.0)
    assert L.check_cls_loss("qfl", "diou", None, 1.5) == (0.0, 1.5) and L.check_cls_loss("vfl", "giou", 0.5, 1.0) == (0.5, 1.0)
    assert L.CLS_LOSSES == ("focal", "qfl", "vfl")
    from mxdetection_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mxdet.h")).read()
    for k, v in _lib.CLS_LOSS_KINDS.items():
        assert "#define MXDET_CLS_LOSS_%s %d\n" % (k.upper(), v) in hdr
    assert "#define MXDET_ROUTE_RETINA_LOSS_QUALITY %d\n" % _lib.ROUTE_KINDS["RETINA_LOSS_QUALITY"] in open(
        os.path.join(ROOT, "include", "mxdet_debug.h")).read()
    # the wrappers refuse what the C entries would not see
    with pytest.raises(ValueError, match="IoU-family"):
        L.retina_loss_level_quality(None, None, 1, 8, None, None, None, None, 0, "qfl", 0.0, 2.0, "smooth_l1", (1.0,) * 4, 1.0, None, 1.0,
                                    None, None, None)
    with pytest.raises(ValueError, match="cls_loss"):
        L.quality_focal_loss(None, None, None, "focal")


def test_config_defaults_are_todays_model_and_the_builder_plumbs_the_keys(monkeypatch):
    import inspect
    from mxdetection_amd import models
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.models.rpn_heads.retina_head import RetinaHead
    from mxdetection_amd.utils.config import DEFAULTS, load_config
    net = DEFAULTS["network"]
    assert net["cls_loss"] == "focal" and net["cls_loss_alpha"] is None and net["cls_loss_gamma"] is None
    seen = []
    monkeypatch.setattr(models, "FasterRCNN", lambda device, **kw: seen.append(("frcnn", kw)) or "m")
    monkeypatch.setattr(models, "RetinaNet", lambda device, **kw: seen.append(("retina", kw)) or "m")
    build_detector(load_config(None, ["network.type=retinanet"]))
    assert (seen[-1][1]["cls_loss"], seen[-1][1]["cls_loss_alpha"], seen[-1][1]["cls_loss_gamma"]) == ("focal", None, None)
    build_detector(load_config(None, ["network.type=retinanet", "network.reg_loss=giou", "network.cls_loss=vfl", "network.cls_loss_alpha=0.5",
                                      "network.cls_loss_gamma=1.5"]))
    assert (seen[-1][1]["cls_loss"], seen[-1][1]["cls_loss_alpha"], seen[-1][1]["cls_loss_gamma"]) == ("vfl", 0.5, 1.5)
    for typ in ("faster_rcnn", "mask_rcnn"):
        build_detector(load_config(None, ["network.type=" + typ]))
        assert "cls_loss" not in seen[-1][1]
        with pytest.raises(ValueError, match="cls_loss"):
            build_detector(load_config(None, ["network.type=" + typ, "network.reg_loss=giou", "network.cls_loss=qfl"]))
    monkeypatch.undo()
    with pytest.raises(ValueError, match="needs an IoU-family reg_loss"):
        build_detector(load_config(None, ["network.type=retinanet", "network.cls_loss=qfl"]))
    with pytest.raises(ValueError, match="cls_loss must be one of"):
        build_detector(load_config(None, ["network.type=retinanet", "network.reg_loss=giou", "network.cls_loss=gfl"]))
    for cls in (models.RetinaNet, RetinaHead):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["cls_loss"].default == "focal" and sig["cls_loss_alpha"].default is None and sig["cls_loss_gamma"].default is None


def test_the_quality_experiment_files_load():
    from mxdetection_amd.utils.config import load_config
    base = load_config(os.path.join(ROOT, "configs", "retinanet_r101_fpn_atss.yaml"))
    assert base.network.cls_loss == "focal"
    for k in ("qfl", "vfl"):
        f = load_config(os.path.join(ROOT, "configs", "retinanet_r101_fpn_atss_%s.yaml" % k))
        assert f.network.cls_loss == k and f.network.cls_loss_alpha is None and f.network.cls_loss_gamma is None
        a, b = f.network.to_dict(), base.network.to_dict()
        assert {x: v for x, v in a.items() if x != "cls_loss"} == {x: v for x, v in b.items() if x != "cls_loss"}
        assert {x: v for x, v in f.TRAIN.items()} == {x: v for x, v in base.TRAIN.items()}
        assert (f.network.assigner, f.network.reg_loss, f.network.reg_loss_weight, list(f.network.anchor_ratios)) == ("atss", "giou", 2.0, [1.0])


# ---- tolerances ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_rows(n=N_RANDOM, Cc=8, seed=23):
    """(x [n,Cc], y64 [n,Cc], valid [n,1], y32 [n,Cc]): random anchors on the IoU module's random boxes (stds 1)."""
    rng = np.random.default_rng(seed)
    box, gt, d = T.random_rows(T.RETINA_STDS, n)
    lab = np.where(rng.random(n) < 0.7, rng.integers(1, Cc + 1, n), 0)
    fg = lab > 0
    q64, q32 = np.zeros(n), np.zeros(n, np.float32)
    q64[fg], q32[fg] = Q.quality64(box[fg], gt[fg], d[fg], STDS), Q.quality_fp32(box[fg], gt[fg], d[fg], STDS)
    y64, valid = Q.targets64(lab, q64, Cc)
    y32, _ = Q.targets64(lab, q32, Cc)
    x = T.bf16r(np.clip(rng.standard_normal((n, Cc)) * 2.5 - 1.0, -LOGIT_CLIP, LOGIT_CLIP))
    return T.bf16r(_nudge(x, y64)), y64, valid, y32.astype(np.float32)


@functools.lru_cache(maxsize=None)
def measure_fp32_error():
    """Largest |float32 restatement - float64 reference|: class gradient per element, class loss per anchor."""
    worst = {"grad": 0.0, "loss": 0.0}
    x, y64, valid, y32 = random_rows()
    for cid, cls_loss, alpha, gamma in CLS_SETTINGS:
        for name in DATA_NAMES:
            c = _shape_of(name)
            d, r = _level_data(name), _level_ref(name, cid)
            N, H, W, A, Cc = c["shape"]
            L32, G32 = Q.retina_quality_fp32(d["cls"], d["reg"], A, Cc, d["cls_labels"], d["anchors"], d["matched"], d["gt"], c["off"],
                                             cls_loss, alpha, gamma, STDS)
            G64 = r["grad_cls"][..., :A * Cc].reshape(G32.shape)
            worst["grad"] = max(worst["grad"], float(np.abs(G32 - G64).max()))
            worst["loss"] = max(worst["loss"], float(np.abs(L32 - r["per_anchor"]).max()))
        tables = [(x, y64, valid, y32)]
        for c in PRIM_CASES:                                              # the primitive's tables: qualities given in float32
            if c["cls_id"] == cid:
                d = prim_data(c)
                py, pvalid = Q.targets64(d["labels"], d["q"], c["C"])
                tables.append((d["x"], py, pvalid, py.astype(np.float32)))
        for tx, ty64, tvalid, ty32 in tables:
            L64, G64 = Q.ref_elems(tx, ty64, cls_loss, alpha, gamma)
            L32, G32 = Q.cls_elem_fp32(tx, ty32, cls_loss, alpha, gamma)
            acc = np.zeros(len(tx), np.float32)
            for k in range(tx.shape[1]):
                acc = acc + L32[:, k] * tvalid[:, 0].astype(np.float32)
            worst["grad"] = max(worst["grad"], float(np.abs((G32 - G64) * tvalid).max()))
            worst["loss"] = max(worst["loss"], float(np.abs(acc - (L64 * tvalid).sum(axis=1)).max()))
    return worst


def test_fp32_error_budget():
    w = measure_fp32_error()
    print("quality class loss, float32 restatement vs float64 autograd, max error: gradient %.4e, per-anchor loss %.4e" % (w["grad"], w["loss"]))
    print("bounds by the x4 / power-of-two rule: 2^%d 2^%d" % tuple(math.log2(T._pow2_ceil(4 * w[k])) for k in ("grad", "loss")))
    assert ATOL_CLS_GRAD == T._pow2_ceil(4 * w["grad"]) and ATOL_CLS_LOSS == T._pow2_ceil(4 * w["loss"])
    for k in ("grad", "loss"):
        assert abs(w[k] - MEASURED[k]) <= 0.02 * MEASURED[k], (k, w[k])


def test_references_are_sensitive_to_the_listed_mistakes():
    c = _shape_of("coco")
    d = _level_data("coco")
    N, H, W, A, Cc = c["shape"]
    args = (d["cls"], d["reg"], A, Cc, d["cls_labels"], d["anchors"], d["matched"], d["gt"], 0)
    r = _level_ref("coco", "qfl2")
    lv, q = d["cls_labels"][:, :H * W * A], r["q"]
    G = r["grad_cls"]
    # a hard 0/1 target instead of the quality; the GIoU value 1 - L instead of inter / union; the other kind's formula
    y, valid = Q.targets64(lv, (lv > 0).astype(np.float64), Cc)
    x = d["cls"][..., :A * Cc].reshape(N, -1, Cc)
    hard = Q.ref_elems(x, y, "qfl", 0.0, 2.0)[1] * valid
    assert np.abs(hard - G[..., :A * Cc].reshape(hard.shape)).max() > 1000 * ATOL_CLS_GRAD
    assert np.abs(_level_ref("coco", "vfl")["grad_cls"] - G).max() > 1000 * ATOL_CLS_GRAD
    assert np.abs(_level_ref("coco", "qfl1.5")["grad_cls"] - G).max() > 1000 * ATOL_CLS_GRAD
    stds_wrong = Q.ref_retina_quality(*args, "qfl", 0.0, 2.0, (0.1, 0.1, 0.2, 0.2), 0, 1.0)
    assert np.abs(stds_wrong["grad_cls"] - G).max() > 1000 * ATOL_CLS_GRAD
    assert np.abs(stds_wrong["per_anchor"] - r["per_anchor"]).max() > 1000 * ATOL_CLS_LOSS
