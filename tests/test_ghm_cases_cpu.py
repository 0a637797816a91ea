"""Case tables, references and host-side checks of the gradient-harmonizing losses (GHM-C / GHM-R). No GPU.

The tables (tests/test_gpu_ghm.py runs them): two levels (10 x 13 and 3 x 4 cells, N = 2) that share one histogram, in the
vector form (A = 3, C = 8, ld_cls = ld_reg = 64: 780 anchors = four workgroups, the last one partial, and 72 anchors = less
than one) and the scalar form (A = 1, C = 5, ld 8). One moved element changes every weight of a step, so the tables are
CONSTRUCTED so that no element's float64 gradient norm lies within GUARD = 2^-12 of an interior bin edge k / B, for the
published bin numbers and for 64 bins alike (the outer edges 0 and 1 cannot be crossed: g = 0 and g = 1 are in the first and
the last bin by definition). The guard is asserted here, on the tables themselves; nothing is left out at comparison time.

Element tolerances, by the project's rule (largest difference between the float32 restatement of tests/_ghm_ref.py and
float64 over every table element and 100 000 seeded random ones, times 4, rounded up to a power of two). Measured:
  class  s - t              8.524e-08 -> ATOL_CLS_GRAD = 2^-21       BCE                  4.738e-07 -> ATOL_CLS_LOSS = 2^-19
  box    d / sqrt(d^2+mu^2) 1.347e-07 -> ATOL_REG_GRAD = 2^-20       sqrt(d^2+mu^2) - mu  5.714e-07 -> ATOL_REG_LOSS = 2^-18
Gradients are compared after division by coef * weight * loss_scale; bf16 outputs add 2^-8 |ref|; a summed loss is within
LOSS_RTOL of the float64 sum plus weight * coef * the element bound for every summed element. cnt is exact; coef is within
8 float32 ulp (a moving-average multiply-add, one product, one reciprocal).
"""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import _ghm_ref as G
import test_loss_cases_cpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 2.0 ** -12
DRAW_MARGIN = 2.0 ** -10                                  # the tables are drawn this far from an edge, the guard asks GUARD
ATOL_CLS_GRAD, ATOL_CLS_LOSS = 2.0 ** -21, 2.0 ** -19
ATOL_REG_GRAD, ATOL_REG_LOSS = 2.0 ** -20, 2.0 ** -18
MEASURED = {"cls_grad": 8.5235e-08, "cls_loss": 4.7379e-07, "reg_grad": 1.3472e-07, "reg_loss": 5.7142e-07}
BF16_STEP, LOSS_RTOL, N_RANDOM = T.BF16_STEP, T.LOSS_RTOL, 100000
COEF_ULPS = 8

PUBLISHED = dict(cls_bins=30, cls_momentum=0.75, cls_weight=1.0, reg_bins=10, reg_momentum=0.7, reg_mu=0.02, reg_weight=10.0)
N = 2
SHAPES = ((10, 13), (3, 4))
FORMS = {"vec": dict(A=3, C=8, ldc=64, ldr=64), "scalar": dict(A=1, C=5, ldc=8, ldr=8)}
KINDS = ("a", "b", "nofg", "ignored")
BINS_C, BINS_R = (30, 64), (10, 64)                       # every bin number the tables are guarded for
EMPTY_C = {"a": (12, 13), "b": (12, 13, 20)}              # class bins (of 30) no element may fall in: n < B; 20: call 1 only
EMPTY_R = {"a": (7,), "b": (7, 3)}                        # box bins (of 10)
PAD = 7.0                                                 # what the padding columns of cls / reg hold


def cfg(**kw):
    c = dict(PUBLISHED)
    c.update(kw)
    return c


def bf16(a):
    """float32 values rounded to bfloat16 (nearest even), as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def edge_distance(g, bins):
    """distance of every g to the nearest INTERIOR edge k / B, 0 < k < B, B in bins"""
    edges = np.unique(np.concatenate([np.arange(1, B) / float(B) for B in bins] + [np.array([-1.0])]))
    return np.abs(np.asarray(g, np.float64)[..., None] - edges).min(axis=-1)


def level_offsets(form):
    A = FORMS[form]["A"]
    offs = [0]
    for H, W in SHAPES:
        offs.append(offs[-1] + H * W * A)
    return offs


@functools.lru_cache(maxsize=None)
def _step_data(form, kind):
    f = FORMS[form]
    A, Cc = f["A"], f["C"]
    rng = np.random.default_rng([11, sorted(FORMS).index(form), KINDS.index(kind)])
    offs = level_offsets(form)
    At = offs[-1]
    r = rng.random((N, At))
    lab = np.zeros((N, At), np.int32)
    fg = r < 0.1
    lab[fg] = rng.integers(1, Cc + 1, int(fg.sum()))
    lab[r > 0.95] = -1
    lab[0, 0], lab[0, 1], lab[0, 2], lab[0, 3] = 1, 2, 0, -1          # the anchors that carry the +-90 / +-20 logits
    if kind == "b":
        lab[1][lab[1] > 0] = 0                                        # an image without foreground
    if kind == "nofg":
        lab[lab > 0] = 0
    if kind == "ignored":
        lab[:] = -1
    ek = "b" if kind == "b" else "a"
    mu = PUBLISHED["reg_mu"]
    levels = []
    targets = np.zeros((N, At, 4), np.float32)
    for l, (H, W) in enumerate(SHAPES):
        n = H * W * A
        ll = lab[:, offs[l]:offs[l] + n]
        t = ll[..., None] == np.arange(1, Cc + 1)
        x = bf16(rng.normal(-1.5, 2.5, (N, n, Cc)))
        keep = np.zeros(x.shape, bool)
        if l == 0:
            x[0, 0, :5] = (90.0, 90.0, -90.0, 20.0, -20.0)            # g = 0 (own column), 1, 0, 1 - 2e-9, 2e-9
            x[0, 1, :5] = (-20.0, -90.0, 20.0, 90.0, -90.0)           # own column 1: g = 1
            x[0, 2, :5] = (90.0, -90.0, 20.0, -20.0, 0.5)
            keep[0, :3, :5] = True
        for _ in range(200):
            g = G.cls_g64(x, t)
            bad = (edge_distance(g, BINS_C) < DRAW_MARGIN) | np.isin(np.minimum(29, np.floor(g * 30)), EMPTY_C[ek])
            bad &= ~keep
            if not bad.any():
                break
            x[bad] = bf16(rng.normal(-1.5, 2.5, int(bad.sum())))
        assert not bad.any()
        cls = np.full((N, H, W, f["ldc"]), PAD, np.float32)
        cls[..., :A * Cc] = x.reshape(N, H, W, A * Cc)
        # box: the gradient norm first, away from the edges and the empty bins; then d and the target
        pred = bf16(rng.normal(0.0, 0.5, (N, n, 4)))
        g = rng.uniform(0.0, 0.999, (N, n, 4))
        for _ in range(200):
            bad = (edge_distance(g, BINS_R) < DRAW_MARGIN) | np.isin(np.floor(g * 10), EMPTY_R[ek])
            if not bad.any():
                break
            g[bad] = rng.uniform(0.0, 0.999, int(bad.sum()))
        assert not bad.any()
        if l == 0:
            g[0, 0, 0] = 0.0                                          # d == 0 exactly: the first bin
        d = mu * g / np.sqrt(1.0 - g * g) * rng.choice([-1.0, 1.0], g.shape)
        targets[:, offs[l]:offs[l] + n] = (pred.astype(np.float64) - d).astype(np.float32)
        reg = np.full((N, H, W, f["ldr"]), PAD, np.float32)
        reg[..., :4 * A] = pred.reshape(N, H, W, 4 * A)
        levels.append(dict(cls=cls, reg=reg, A=A, C=Cc, off=offs[l], H=H, W=W))
    return dict(levels=levels, cls_labels=lab, targets=targets, At=At, form=form, kind=kind)


def step_data(form, kind):
    return _step_data(form, kind)


def all_g(d):
    """(class g, box g) float64 of every valid element of the step, levels in order."""
    gc, gr = [], []
    for lv in d["levels"]:
        x, t, v, dl, tg, f = G.level_views(lv, d["cls_labels"], d["targets"])
        gc.append(G.cls_g64(x, t)[v].reshape(-1))
        gr.append(G.reg_g64(dl - tg, PUBLISHED["reg_mu"])[f].reshape(-1))
    return np.concatenate(gc), np.concatenate(gr)


def ulp32(x):
    x = np.abs(np.asarray(x, np.float64))
    return np.where(x > 0, 2.0 ** (np.floor(np.log2(np.where(x > 0, x, 1.0))) - 23), 2.0 ** -149)


def coef_ok(what, got, ref):
    err = np.abs(np.asarray(got, np.float64) - ref) / ulp32(ref)
    print("%s: largest coef error %.2f ulp (bound %d)" % (what, float(err.max()), COEF_ULPS))
    return bool((err <= COEF_ULPS).all()) and bool((np.asarray(got)[np.asarray(ref) == 0] == 0).all())


# ---- the tables are what they say ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kind", KINDS)
def test_tables_keep_the_guard_and_hold_their_cases(form, kind):
    d = step_data(form, kind)
    f = FORMS[form]
    gc, gr = all_g(d)
    if gc.size:
        assert edge_distance(gc, BINS_C).min() >= GUARD
    if gr.size:
        assert edge_distance(gr, BINS_R).min() >= GUARD
    assert gc.min(initial=0.5) >= 0.0 and gc.max(initial=0.5) <= 1.0 and gr.max(initial=0.5) < 1.0
    lab = d["cls_labels"]
    assert d["At"] == 142 * f["A"] and [N * H * W * f["A"] for H, W in SHAPES] == ([780, 72] if form == "vec" else [260, 24])
    assert f["ldc"] > f["A"] * f["C"] and f["ldr"] > 4 * f["A"] and (f["C"] % 8 == 0) == (form == "vec")
    if kind == "ignored":
        assert gc.size == 0 and gr.size == 0 and (lab == -1).all()
        return
    assert (lab == -1).any() and (lab == 0).any()
    assert (gc < 1e-30).any() and (gc == 1.0).any()                     # +-90: exactly the first and the last bin's ends
    bc = np.bincount(np.minimum(29, np.floor(gc * 30).astype(int)), minlength=30)
    ek = "b" if kind == "b" else "a"
    assert all(bc[i] == 0 for i in EMPTY_C[ek]) and bc[0] > 0 and bc[29] > 0 and (bc > 0).sum() == 30 - len(EMPTY_C[ek])
    if kind in ("a", "b"):
        br = np.bincount(np.floor(gr * 10).astype(int), minlength=10)
        assert all(br[i] == 0 for i in EMPTY_R[ek]) and (br > 0).sum() == 10 - len(EMPTY_R[ek]) and (gr == 0.0).any()
        assert (lab[0] > 0).any() and ((lab[1] > 0).any() == (kind == "a"))
    else:
        assert gr.size == 0 and gc.size > 0                            # no foreground: the box histogram is empty
    if kind == "b":                                                    # populated in call 1, empty in call 2
        ga, ra = all_g(step_data(form, "a"))
        assert (np.floor(ga * 30) == 20).any() and (np.floor(ra * 10) == 3).any()


# ---- the float64 loop form against the closed form -------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
def test_loop_form_equals_the_closed_form_over_two_calls(form):
    acc_c, acc_r = np.zeros(30), np.zeros(10)
    cc, cr = np.zeros(30), np.zeros(10)
    c = cfg()
    for kind in ("a", "b", "ignored", "nofg"):
        d = step_data(form, kind)
        before = acc_c.copy(), acc_r.copy()
        r = G.ref_step(d["levels"], d["cls_labels"], d["targets"], "both", c, acc_c, acc_r)
        gc, gr = all_g(d)
        cnt_c, coef_c = G.closed_form(gc, 30, 0.75, cc)
        cnt_r, coef_r = G.closed_form(gr, 10, 0.7, cr)
        assert np.array_equal(r["cnt_c"], cnt_c) and np.array_equal(r["cnt_r"], cnt_r)
        assert np.allclose(r["coef_c"], coef_c, rtol=1e-13, atol=0) and np.allclose(r["coef_r"], coef_r, rtol=1e-13, atol=0)
        assert np.allclose(acc_c, cc, rtol=1e-13, atol=0) and np.allclose(acc_r, cr, rtol=1e-13, atol=0)
        assert int(r["cnt_c"].sum()) == gc.size and int(r["cnt_r"].sum()) == gr.size
        if kind == "ignored":                                          # nothing valid: zero loss and gradients, state untouched
            assert np.array_equal(acc_c, before[0]) and np.array_equal(acc_r, before[1])
            assert not r["coef_c"].any() and not r["coef_r"].any()
            for o in r["levels"]:
                assert o["loss_c"] == 0.0 and o["loss_r"] == 0.0 and not o["grad_cls"].any() and not o["grad_reg"].any()
        else:
            # the weights sum to one bin's worth each: sum over elements of coef = sum_i cnt_i / (n acc_i)
            assert all(np.isfinite(o["loss_c"]) and o["loss_c"] > 0 for o in r["levels"])
            assert all(not o["grad_cls"][..., FORMS[form]["A"] * FORMS[form]["C"]:].any() for o in r["levels"])
    # momentum 0: stateless -- coef = 1 / (n cnt), whatever acc held
    d = step_data(form, "a")
    r = G.ref_step(d["levels"], d["cls_labels"], d["targets"], "both", cfg(cls_momentum=0.0, reg_momentum=0.0),
                   np.full(30, 123.0), np.full(10, 5.0))
    has = r["cnt_c"] > 0
    assert np.allclose(r["coef_c"][has], 1.0 / (has.sum() * r["cnt_c"][has]), rtol=1e-15, atol=0)
    assert abs(sum(o["wsum_c"] for o in r["levels"]) - 1.0) < 1e-12 and abs(sum(o["wsum_r"] for o in r["levels"]) - 1.0) < 1e-12


def test_fp32_bins_are_the_float64_bins_on_the_tables():
    """The restated float32 g of every table element falls in the float64 bin: what the guard is for."""
    for form in sorted(FORMS):
        for kind in ("a", "b", "nofg"):
            d = step_data(form, kind)
            for lv in d["levels"]:
                x, t, v, dl, tg, f = G.level_views(lv, d["cls_labels"], d["targets"])
                g32 = G.cls_elem_fp32(x[v], t[v] > 0)[0]
                g64 = G.cls_g64(x, t)[v]
                for B in BINS_C:
                    assert np.array_equal(G.bin_fp32(g32, B), np.minimum(B - 1, np.floor(g64 * B)).astype(np.int32))
                r32 = G.reg_elem_fp32(dl[f].astype(np.float32), tg[f].astype(np.float32), PUBLISHED["reg_mu"])[0]
                r64 = G.reg_g64(dl - tg, PUBLISHED["reg_mu"])[f]
                for B in BINS_R:
                    assert np.array_equal(G.bin_fp32(r32, B), np.minimum(B - 1, np.floor(r64 * B)).astype(np.int32))


# ---- tolerances ------------------------------------------------------------------------------------------------------
def _pow2_ceil(x):
    return 2.0 ** math.ceil(math.log2(x))


@functools.lru_cache(maxsize=None)
def measure_fp32_error():
    import torch
    import torch.nn.functional as F
    xs, ts, ds, gs = [], [], [], []
    for form in sorted(FORMS):
        for kind in ("a", "b", "nofg"):
            d = step_data(form, kind)
            for lv in d["levels"]:
                x, t, v, dl, tg, f = G.level_views(lv, d["cls_labels"], d["targets"])
                xs.append(x[v].reshape(-1))
                ts.append(t[v].reshape(-1))
                ds.append(dl[f].reshape(-1))
                gs.append(tg[f].reshape(-1))
    rng = np.random.default_rng(29)
    xs.append(bf16(np.clip(rng.normal(0.0, 6.0, N_RANDOM), -90, 90)).astype(np.float64))
    ts.append((rng.random(N_RANDOM) < 0.1).astype(np.float64))
    ds.append(bf16(rng.normal(0.0, 1.0, N_RANDOM)).astype(np.float64))
    gs.append(rng.normal(0.0, 1.0, N_RANDOM).astype(np.float32).astype(np.float64))
    x, t, dl, tg = (np.concatenate(a) for a in (xs, ts, ds, gs))
    _, L32, G32 = G.cls_elem_fp32(x, t > 0)
    xt = torch.from_numpy(x).requires_grad_(True)
    bce = F.binary_cross_entropy_with_logits(xt, torch.from_numpy(t), reduction="none")
    bce.sum().backward()
    mu = PUBLISHED["reg_mu"]
    _, A32, D32 = G.reg_elem_fp32(dl, tg, mu)
    dt = torch.from_numpy(dl).requires_grad_(True)
    asl1 = torch.sqrt((dt - torch.from_numpy(tg)) ** 2 + mu * mu) - mu
    asl1.sum().backward()
    return {"cls_grad": float(np.abs(G32 - xt.grad.numpy()).max()), "cls_loss": float(np.abs(L32 - bce.detach().numpy()).max()),
            "reg_grad": float(np.abs(D32 - dt.grad.numpy()).max()), "reg_loss": float(np.abs(A32 - asl1.detach().numpy()).max()),
            "n": int(x.size + dl.size)}


def test_fp32_error_budget():
    w = measure_fp32_error()
    print("GHM elements, float32 restatement vs float64 autograd over %d elements, max error: s - t %.4e, BCE %.4e, d / r %.4e, "
          "r - mu %.4e" % (w["n"], w["cls_grad"], w["cls_loss"], w["reg_grad"], w["reg_loss"]))
    print("bounds by the x4 / power-of-two rule: " + " ".join("%s 2^%d" % (k, math.log2(_pow2_ceil(4 * w[k]))) for k in MEASURED))
    assert ATOL_CLS_GRAD == _pow2_ceil(4 * w["cls_grad"]) and ATOL_CLS_LOSS == _pow2_ceil(4 * w["cls_loss"])
    assert ATOL_REG_GRAD == _pow2_ceil(4 * w["reg_grad"]) and ATOL_REG_LOSS == _pow2_ceil(4 * w["reg_loss"])
    for k in MEASURED:
        assert abs(w[k] - MEASURED[k]) <= 0.02 * MEASURED[k], (k, w[k])        # the docstring's figures are these


def test_fp32_weights_are_within_the_ulp_bound():
    """The float32 restatement of the weights kernel against float64 over the two calls, state carried: <= COEF_ULPS."""
    for form in sorted(FORMS):
        a64, a32 = np.zeros(30), np.zeros(30, np.float32)
        for kind in ("a", "b", "a", "nofg", "b"):
            gc, _ = all_g(step_data(form, kind))
            cnt, coef = G.closed_form(gc, 30, 0.75, a64)
            a32, c32 = G.weights_fp32(cnt, a32, 0.75)
            assert coef_ok("%s %s" % (form, kind), c32, coef)


# ---- host-side validation (no GPU: every check happens before a launch) ----------------------------------------------
def test_entries_validate_their_arguments():
    from mxdetection_amd import _lib
    L = _lib.load()
    p, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 4)

    def err():
        return L.mxdet_last_error()

    def hist(cls=p, reg=p, shape=(2, 3, 4, 3, 8), ldc=64, ldr=64, lab=p, tgt=p, At=100, off=0, flags=3, bc=30, br=10, mu=0.02, counts=p):
        return L.mxdet_ghm_hist_level(cls, reg, *shape, ldc, ldr, lab, tgt, At, off, flags, bc, br, mu, counts, None)

    def level(cls=p, reg=p, shape=(2, 3, 4, 3, 8), ldc=64, ldr=64, lab=p, tgt=p, At=100, off=0, flags=3, coef=p, bc=30, br=10, wc=1.0,
              mu=0.02, wr=10.0, nfg=p, gc=p, gr=p, part=p):
        return L.mxdet_retina_loss_level_ghm(cls, reg, *shape, ldc, ldr, lab, tgt, At, off, flags, 0.25, 2.0, 3.0, coef, bc, br, wc, mu,
                                             wr, nfg, 1.0, gc, gr, part, None)

    def weights(counts=p, rows=4, bc=30, br=10, mc=0.75, mr=0.7, acc=p, cnt=p, coef=p):
        return L.mxdet_ghm_weights(counts, rows, bc, br, mc, mr, acc, cnt, coef, None)
    buf = (C.c_int32 * 64)()
    L.mxdet_debug_route_probe(1)
    try:
        assert hist() == 0 and level() == 0 and level(flags=1) == 0 and level(flags=2, bc=1, br=64) == 0
        assert L.mxdet_debug_route_read(buf, 4) == 4
        recs = [tuple(buf[16 * i:16 * i + 4]) for i in range(4)]
        K = _lib.ROUTE_KINDS
        assert recs == [(K["GHM_HIST"], 1, 1, 3), (K["RETINA_LOSS_GHM"], 1, 1, 3), (K["RETINA_LOSS_GHM"], 1, 1, 1),
                        (K["RETINA_LOSS_GHM"], 1, 1, 2)]
        L.mxdet_debug_route_probe(1)
        assert hist(shape=(2, 10, 13, 3, 8), At=1000) == 0 and hist(shape=(2, 10, 13, 1, 5), ldc=8, ldr=8, At=1000) == 0
        assert level(cls=odd) == 0 and level(ldr=66) == 0
        assert L.mxdet_debug_route_read(buf, 4) == 4
        assert [tuple(buf[16 * i + 1:16 * i + 3]) for i in range(4)] == [(1, 4), (0, 2), (0, 1), (0, 1)]      # vec / scalar, the grid
        L.mxdet_debug_route_probe(1)
        for fn in (hist, level):
            assert fn(ldc=8) == -2 and b"bad shape" in err()
            assert fn(At=35) == -2 and b"level outside the anchor range" in err()
            assert fn(flags=0) == -1 and fn(flags=4) == -1 and b"flags" in err()
            assert fn(bc=0) == -1 and fn(bc=65) == -1 and fn(br=0) == -1 and fn(br=65) == -1 and b"bins must lie in 1..64" in err()
            assert fn(mu=0.0) == -1 and fn(mu=-1.0) == -1 and b"mu must be positive" in err()
            assert fn(tgt=odd) == -1 and b"16-byte aligned" in err()
            for k in ("cls", "reg", "lab", "tgt"):
                assert fn(**{k: None}) == -1 and b"null pointer" in err(), k
        assert hist(counts=None) == -1
        for k in ("coef", "nfg", "gc", "gr", "part"):
            assert level(**{k: None}) == -1 and b"null pointer" in err(), k
        assert level(wc=0.0) == -1 and level(wr=-1.0) == -1 and b"positive" in err()
        assert L.mxdet_debug_route_read(buf, 4) == 0                     # a rejected call leaves no record
        assert weights() == 0 and err() == b"" and L.mxdet_debug_route_read(buf, 4) == 0      # one route: no launch, no record
    finally:
        L.mxdet_debug_route_probe(0)
    assert weights(rows=0) == -2
    assert weights(bc=0) == -1 and weights(br=65) == -1 and b"bins" in err()
    assert weights(mc=1.0) == -1 and weights(mr=-0.1) == -1 and b"momentum must lie in [0, 1)" in err()
    for k in ("counts", "acc", "cnt", "coef"):
        assert weights(**{k: None}) == -1 and b"null pointer" in err(), k


def test_header_defines_match_the_bindings():
    from mxdetection_amd import _lib
    from mxdetection_amd.core import loss as L
    hdr = open(os.path.join(ROOT, "include", "mxdet.h")).read()
    d = {k: int(v) for k, v in re.findall(r"#define MXDET_GHM_([A-Z_]+) (\d+)", hdr)}
    assert d == {"CLS": 1, "REG": 2, "MAX_BINS": 64}
    assert _lib.GHM_FLAGS == {"cls": d["CLS"], "reg": d["REG"], "both": d["CLS"] | d["REG"]} and _lib.GHM_MAX_BINS == d["MAX_BINS"]
    assert L.GHM_MODES == ("none",) + tuple(_lib.GHM_FLAGS) and L.GHM_DEFAULTS == PUBLISHED
    dbg = open(os.path.join(ROOT, "include", "mxdet_debug.h")).read()
    assert "#define MXDET_ROUTE_RETINA_LOSS_GHM %d\n" % _lib.ROUTE_KINDS["RETINA_LOSS_GHM"] in dbg
    assert "#define MXDET_ROUTE_GHM_HIST %d\n" % _lib.ROUTE_KINDS["GHM_HIST"] in dbg
    for name in ("mxdet_ghm_hist_level", "mxdet_ghm_weights", "mxdet_retina_loss_level_ghm"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr)


# ---- options: defaults, refusals at every layer, config, experiment file ---------------------------------------------
def test_check_ghm_defaults_and_range():
    from mxdetection_amd.core.loss import check_ghm
    assert check_ghm() == PUBLISHED and check_ghm("both") == PUBLISHED
    for mode in ("cls", "reg", "both"):
        got = check_ghm(mode, cls_bins=1, reg_bins=64, cls_momentum=0, reg_momentum=0.999, reg_mu=1e-3, cls_weight=2, reg_weight=0.5)
        assert got == dict(cls_bins=1, cls_momentum=0.0, cls_weight=2.0, reg_bins=64, reg_momentum=0.999, reg_mu=1e-3, reg_weight=0.5)
    check_ghm("reg", cls_loss_alpha=0.5, cls_loss_gamma=1.5)          # the focal half beside GHM-R keeps its alpha / gamma
    check_ghm("none", cls_loss="vfl", reg_loss="giou", reg_max=16, cls_loss_alpha=0.5)      # 'none' constrains nothing
    # the half that is not harmonized is the plain entry's focal / smooth-L1 half: every other mode needs the plain pair
    for mode in ("cls", "reg", "both"):
        for kw, word in ((dict(reg_loss="giou"), "keep reg_loss"), (dict(reg_loss="giou", reg_max=16), "keep reg_loss"),
                         (dict(reg_max=16), "needs plain deltas"), (dict(cls_loss="qfl"), "another class loss"),
                         (dict(cls_loss="vfl", reg_loss="giou"), "another class loss")):
            with pytest.raises(ValueError, match=word):
                check_ghm(mode, **kw)


BAD_OPTIONS = [(dict(ghm="all"), "ghm must be one of"), (dict(ghm="both", ghm_cls_bins=0), "ghm_cls_bins"),
               (dict(ghm="both", ghm_cls_bins=65), "ghm_cls_bins"), (dict(ghm="reg", ghm_reg_bins=10.0), "ghm_reg_bins"),
               (dict(ghm="cls", ghm_cls_bins=True), "ghm_cls_bins"), (dict(ghm="cls", ghm_cls_momentum=1.0), "ghm_cls_momentum"),
               (dict(ghm="reg", ghm_reg_momentum=-0.1), "ghm_reg_momentum"), (dict(ghm="reg", ghm_reg_mu=0.0), "ghm_reg_mu"),
               (dict(ghm="cls", ghm_cls_weight=0), "ghm_cls_weight"), (dict(ghm="reg", ghm_reg_weight="10"), "ghm_reg_weight"),
               (dict(ghm="cls", cls_loss="qfl", reg_loss="giou"), "in place of the focal loss"),
               (dict(ghm="both", cls_loss="vfl", reg_loss="giou"), "in place of the focal loss"),
               (dict(ghm="cls", cls_loss_alpha=0.5), "no alpha / gamma"), (dict(ghm="both", cls_loss_gamma=1.5), "no alpha / gamma"),
               (dict(ghm="reg", reg_loss="giou"), "keep reg_loss = 'smooth_l1'"), (dict(ghm="both", reg_loss="diou"), "keep reg_loss"),
               (dict(ghm="reg", reg_loss="giou", reg_max=16), "keep reg_loss"),
               # 'cls' beside another box loss, 'reg' beside another class loss: the other half would be trained as plain
               (dict(ghm="cls", reg_loss="giou"), "keep reg_loss"), (dict(ghm="cls", reg_loss="diou", reg_loss_weight=2.0), "keep reg_loss"),
               (dict(ghm="cls", reg_loss="giou", reg_max=16), "keep reg_loss"),
               (dict(ghm="reg", cls_loss="qfl", reg_loss="giou"), "another class loss"),
               (dict(ghm="reg", cls_loss="vfl", reg_loss="giou", reg_max=16), "another class loss")]


@pytest.mark.parametrize("kw,word", BAD_OPTIONS, ids=["%s-%d" % (w.split()[0], i) for i, (_, w) in enumerate(BAD_OPTIONS)])
def test_bad_ghm_options_raise_at_every_layer_before_any_allocation(kw, word, monkeypatch):
    from mxdetection_amd import models
    from mxdetection_amd.core.loss import check_ghm
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.models.rpn_heads.retina_head import RetinaHead
    from mxdetection_amd.models.utils import layers
    from mxdetection_amd.utils.config import load_config
    monkeypatch.setattr(layers.ParamArena, "finalize", lambda self: (_ for _ in ()).throw(AssertionError("allocated")))
    monkeypatch.setattr(layers.ParamArena, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("allocated")))
    with pytest.raises(ValueError, match=word):
        models.RetinaNet("cuda", **kw)
    with pytest.raises(ValueError, match=word):
        RetinaHead(256, [8, 16, 32, 64, 128], None, None, "cuda", None, **kw)
    with pytest.raises(ValueError, match=word):
        check_ghm(kw.get("ghm", "none"), kw.get("cls_loss", "focal"), kw.get("reg_loss", "smooth_l1"), kw.get("reg_max", 0),
                  kw.get("cls_loss_alpha"), kw.get("cls_loss_gamma"), **{k[4:]: v for k, v in kw.items() if k.startswith("ghm_")})
    over = ["network.type=retinanet"] + ["network.%s=%s" % (k, "'10'" if v == "10" else v) for k, v in kw.items()]
    with pytest.raises(ValueError, match=word):
        build_detector(load_config(None, over))


@pytest.mark.parametrize("mode", ["cls", "reg", "both"])
def test_reg_max_with_ghm_is_refused(mode):
    from mxdetection_amd.core.loss import check_ghm
    with pytest.raises(ValueError, match="needs plain deltas"):
        check_ghm(mode, reg_loss="smooth_l1", reg_max=16)


def test_config_defaults_are_todays_model_and_the_builder_plumbs_the_keys(monkeypatch):
    import inspect
    from mxdetection_amd import models
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.models.rpn_heads.retina_head import RetinaHead
    from mxdetection_amd.utils.config import DEFAULTS, load_config
    keys = {"ghm_" + k: v for k, v in PUBLISHED.items()}
    net = DEFAULTS["network"]
    assert net["ghm"] == "none" and {k: net[k] for k in keys} == keys
    seen = []
    monkeypatch.setattr(models, "FasterRCNN", lambda device, **kw: seen.append(("frcnn", kw)) or "m")
    monkeypatch.setattr(models, "RetinaNet", lambda device, **kw: seen.append(("retina", kw)) or "m")
    build_detector(load_config(None, ["network.type=retinanet"]))
    assert seen[-1][1]["ghm"] == "none" and {k: seen[-1][1][k] for k in keys} == keys
    other = dict(ghm_cls_bins=20, ghm_cls_momentum=0.5, ghm_cls_weight=2.0, ghm_reg_bins=12, ghm_reg_momentum=0.0, ghm_reg_mu=0.05,
                 ghm_reg_weight=5.0)
    build_detector(load_config(None, ["network.type=retinanet", "network.ghm=both"] + ["network.%s=%s" % kv for kv in other.items()]))
    assert seen[-1][1]["ghm"] == "both" and {k: seen[-1][1][k] for k in other} == other
    for typ in ("faster_rcnn", "mask_rcnn"):
        build_detector(load_config(None, ["network.type=" + typ]))
        assert not [k for k in seen[-1][1] if k.startswith("ghm")]
        for mode in ("cls", "reg", "both"):
            with pytest.raises(ValueError, match="network.ghm"):
                build_detector(load_config(None, ["network.type=" + typ, "network.ghm=" + mode]))
    monkeypatch.undo()
    for cls in (models.RetinaNet, RetinaHead):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["ghm"].default == "none" and {k: sig[k].default for k in keys} == keys


def test_the_ghm_experiment_file_loads():
    from mxdetection_amd.utils.config import load_config
    g = load_config(os.path.join(ROOT, "configs", "retinanet_r101_fpn_ghm.yaml"))
    b = load_config(os.path.join(ROOT, "configs", "retinanet_r101_fpn.yaml"))
    assert g.network.ghm == "both" and b.network.ghm == "none" and g.network.assigner == "max_iou"
    assert {k[4:]: v for k, v in g.network.items() if k.startswith("ghm_")} == PUBLISHED
    assert (g.network.cls_loss, g.network.reg_loss, g.network.reg_max) == ("focal", "smooth_l1", 0)
    assert {k: v for k, v in g.network.items() if k != "ghm"} == {k: v for k, v in b.network.items() if k != "ghm"}
    assert dict(g.TRAIN) == dict(b.TRAIN)
