"""Case tables of the dense conv / weight-gradient route tests, and the proof -- without a GPU -- that every case runs
the kernel instantiation it is named after.

The library's route probe (mxdet_debug_route_probe, include/mxdet_debug.h) makes the launchers record the instantiation
and grid they would launch and return before touching the device, so the real selector (conv.hip launch(); wgrad.hip
plan_wgrad() / single_split() for one call, grouped_split() / group_three_tap_steps() for a group) is asked, not re-stated
here. tests/test_gpu_conv_routes.py runs the same tables on the GPU against fp64.

A route is written  "BMxBN/WMxWN/NS fwd|dgrad [par] T<taps> [chain<C>]"  (T0 = run-time geometry K loop, T1 / T9 = the
unrolled static-tap loops). Tuning keys, the forced configuration and the forced split are always changed inside
`steer(...)`, which restores them; the last test of the module checks that a plain case is back on its default route.
"""
import contextlib
import ctypes as C

import pytest

ESHAPE, EWORKSPACE = -2, -3
DUMMY = C.c_void_p(1 << 20)          # never dereferenced while the probe is on


def lib():
    from mxdetection_amd import _lib
    return _lib.load()


@contextlib.contextmanager
def steer(tune=None, force=0, ksplit=0):
    """Tuning keys (library-wide state), forced conv cfg and forced wgrad split (per calling thread), restored on exit."""
    from mxdetection_amd import _lib
    L = lib()
    tune = tune or {}
    try:
        for k, v in tune.items():
            assert L.mxdet_debug_set_tuning(_lib.TUNING_KEYS[k], v) == 0
        L.mxdet_debug_force_conv_cfg(force)
        L.mxdet_debug_force_wgrad_ksplit(ksplit)
        yield L
    finally:
        for k in tune:
            L.mxdet_debug_set_tuning(_lib.TUNING_KEYS[k], -1)
        L.mxdet_debug_force_conv_cfg(0)
        L.mxdet_debug_force_wgrad_ksplit(0)


@contextlib.contextmanager
def probe():
    """Route probe on; yields a function that reads the records made so far as lists of 16 ints."""
    L = lib()

    def read():
        buf = (C.c_int32 * 64)()
        n = L.mxdet_debug_route_read(buf, 4)
        assert 0 <= n <= 4, "more launches than the probe keeps: %d" % n
        return [list(buf[16 * i:16 * i + 16]) for i in range(n)]
    L.mxdet_debug_route_probe(1)
    try:
        yield read
    finally:
        L.mxdet_debug_route_probe(0)


def desc(c, **kw):
    from mxdetection_amd.ops.dense import conv_desc
    return conv_desc(c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c["KH"], c["KW"], c["s"], c["p"], **kw)


def out_hw(c):
    return (c["H"] + 2 * c["p"] - c["KH"]) // c["s"] + 1, (c["W"] + 2 * c["p"] - c["KW"]) // c["s"] + 1


def rows_cols(c):
    """GEMM rows / columns of a forward or data-gradient case."""
    Ho, Wo = out_hw(c)
    return (c["N"] * c["H"] * c["W"], c["Cin"]) if c["kind"] == "dgrad" else (c["N"] * Ho * Wo, c["Cout"])


def route_name(r):
    assert r[0] in (1, 3)
    s = "%dx%d/%dx%d/%d %s%s T%d" % (r[1], r[2], r[3], r[4], r[5], "dgrad" if r[6] else "fwd", " par" if r[7] else "", r[8])
    return s + (" chain%d" % r[9] if r[9] else "")


def conv_records(c, tune=None, force=None):
    """Records of one forward / dgrad / split-K / chain case under its steering (or the given one)."""
    with steer(c.get("tune") if tune is None else tune, c.get("force", 0) if force is None else force) as L, probe() as read:
        d = desc(c)
        if c["kind"] == "fwd":
            rc = L.mxdet_conv2d_fwd(C.byref(d), DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None)
        elif c["kind"] == "dgrad":
            d.relu = 1
            rc = L.mxdet_conv2d_dgrad(C.byref(d), DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None)
        elif c["kind"] == "splitk":
            rc = L.mxdet_conv2d_fwd_splitk(C.byref(d), DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, c["ksplit"], DUMMY, 1 << 40, None)
        else:
            rc = L.mxdet_conv2d_fwd_chain(C.byref(d), DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 256, 1, DUMMY, DUMMY, DUMMY, DUMMY, 64,
                                          1, DUMMY, None)
        assert rc == 0, L.mxdet_last_error()
        return read()


def baseline_force(taps):
    """The forced configuration that runs 64x64 tiles in the K-loop flavour `taps` (the tile-independence reference)."""
    return 5 if taps == 0 else 40


# ---------------------------------------------------------------------------------------------------------------------
# a / b / c / d: single-launch forward and data gradient
# ---------------------------------------------------------------------------------------------------------------------
def _c(name, kind, N, H, W, Cin, Cout, K, s, p, route, tune=None, force=0, **kw):
    KH, KW = K if isinstance(K, tuple) else (K, K)
    c = dict(name=name, kind=kind, N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW, s=s, p=p, tune=tune or {}, force=force,
             route=route if isinstance(route, list) else [route])
    c.update(kw)
    return c


NOST = {"STATIC_TAPS": 0}
T64LO = {"T64": 1}                      # 64x128 tiles on any size
T128LO = {"T128": 1}                    # the "largest layers" branch on any size (K > 256)
W8 = {"T128W": 1}                       # eight-wave 128x128 tiles on any size (>= 128 columns, static loop)
S128, S64x128, S64 = "128x64/4x1/2", "64x128/2x2/2", "64x64/2x2/3"
S128Q, S128W, S256 = "128x128/2x2/2", "128x128/2x4/2", "256x256/2x4/2"

CONV_CASES = []
_M = {127: (1, 127, 1), 128: (2, 8, 8), 129: (3, 43, 1), 63: (1, 7, 9), 64: (1, 8, 8), 65: (1, 5, 13), 255: (3, 5, 17),
      256: (2, 8, 16), 257: (1, 1, 257), 130: (2, 5, 13), 198: (2, 9, 11), 66: (3, 2, 11), 2: (2, 1, 1)}
# (rows one below / at / one above a multiple of BM; 129 rows = an H x 1 map, 257 = a 1 x W map, 66 = a map two pixels high,
#  198 / 130 / 255 = several images, so tile rows cross image boundaries)
for kind in ("fwd", "dgrad"):
    D = kind
    # `red` = reduction channels (fwd: Cin, dgrad: Cout), `col` = GEMM columns (fwd: Cout, dgrad: Cin)
    def mk(name, rows, red, col, K, s, p, route, tune=None, force=0, **kw):
        N, H, W = _M[rows] if isinstance(rows, int) else rows
        ci, co = (red, col) if D == "fwd" else (col, red)
        CONV_CASES.append(_c("%s_%s" % (D, name), D, N, H, W, ci, co, K, s, p, route, tune, force, **kw))
    for (tag, taps, K, p, tune) in (("1x1", 1, 1, 0, {}), ("3x3", 9, 3, 1, {}), ("1x1_rt", 0, 1, 0, NOST), ("3x3_rt", 0, 3, 1, NOST)):
        T = " %s T%d" % (D, taps)
        big = 320 if K == 1 else 64                        # K > 256 for the T128 branch
        # 128x64/4x1: up to 64 columns (8 and 16 included)
        mk("n64_%s_c8" % tag, 127, 64, 8, K, 1, p, S128 + T, tune)
        mk("n64_%s_c16" % tag, 129, 128, 16, K, 1, p, S128 + T, tune)
        mk("n64_%s_c64" % tag, 256, 64, 64, K, 1, p, S128 + T, tune)
        # 64x64
        mk("t64_%s_c72" % tag, 63, 64, 72, K, 1, p, S64 + T, tune)
        mk("t64_%s_c136" % tag, 128, 128, 136, K, 1, p, S64 + T, tune)
        mk("t64_%s_c200" % tag, 65, 64, 200, K, 1, p, S64 + T, tune)
        # 64x128
        mk("t64x128_%s_c136" % tag, 255, 64, 136, K, 1, p, S64x128 + T, dict(tune, **T64LO))
        mk("t64x128_%s_c200" % tag, 64, 128, 200, K, 1, p, S64x128 + T, dict(tune, **T64LO))
        mk("t64x128_%s_c72" % tag, 257, 64, 72, K, 1, p, S64x128 + T, dict(tune, **T64LO))
        # 128x128 of four waves: production reaches it as the tile of the T128 branch's rows (TAIL = 0); here no whole round
        mk("t128_%s_c136" % tag, 255, big, 136, K, 1, p, S128Q + T, dict(tune, TAIL=0, **T128LO))
        mk("t128_%s_c200" % tag, 129, big, 200, K, 1, p, S128Q + T, dict(tune, TAIL=0, **T128LO))
        mk("t128_%s_c72" % tag, 256, big, 72, K, 1, p, S128Q + T, dict(tune, TAIL=0, **T128LO))
        mk("t128_%s_tail1" % tag, 130, big, 136, K, 1, p, S64x128 + T, dict(tune, TAIL=1, **T128LO))
        mk("t128_%s_tail2" % tag, 66, big, 72, K, 1, p, S64 + T, dict(tune, TAIL=2, **T128LO))
        if taps:   # eight waves: static loop only
            mk("w8_%s_c136" % tag, 257, 64, 136, K, 1, p, S128W + T, dict(tune, **W8))
            mk("w8_%s_c200" % tag, 127, 128, 200, K, 1, p, S128W + T, dict(tune, **W8))
            mk("w8_%s_c128" % tag, 256, 64, 128, K, 1, p, S128W + T, dict(tune, **W8))
    # maps narrower than 3 pixels / one pixel: every 3x3 border case at once
    mk("t64_3x3_2x2map", (5, 2, 2), 64, 72, 3, 1, 1, S64 + " %s T9" % D)
    mk("n64_3x3_1x1map", 2, 64, 64, 3, 1, 1, S128 + " %s T9" % D)
    # forced configurations (what the sweep tools time); 15 (256x256) only with columns % 256 == 0, as production guards it
    for f, r in ((3, "128x128/2x2/4"), (5, S64), (6, S64x128), (7, S128Q), (8, S128), (15, S256)):
        col = 256 if f == 15 else 136
        mk("force%d_1x1" % f, 257, 256, 256 if f == 15 else col, 1, 1, 0, r + " %s T0" % D, None, f)
        mk("force%d_3x3" % f, 198, 64, col, 3, 1, 1, r + " %s T0" % D, None, f)
    for f, r in ((40, S64), (41, S64x128), (45, S128Q), (46, S128), (49, S128W)):
        mk("force%d_1x1" % f, 257, 256, 136, 1, 1, 0, r + " %s T1" % D, None, f)
        mk("force%d_3x3" % f, 198, 64, 136, 3, 1, 1, r + " %s T9" % D, None, f)

# strided forward: 3x3 on the static-9 loop, 1x1 on the run-time loop
CONV_CASES += [
    _c("fwd_s2_3x3_static", "fwd", 2, 13, 21, 64, 136, 3, 2, 1, S64 + " fwd T9"),
    _c("fwd_s2_3x3_static_n64", "fwd", 3, 10, 9, 128, 64, 3, 2, 1, S128 + " fwd T9"),
    _c("fwd_s2_3x3_static_t64x128", "fwd", 2, 12, 22, 64, 200, 3, 2, 1, S64x128 + " fwd T9", T64LO),
    _c("fwd_s2_1x1_rt", "fwd", 2, 13, 21, 64, 136, 1, 2, 0, S64 + " fwd T0"),
    _c("fwd_s2_1x1_rt_n64", "fwd", 2, 14, 22, 128, 16, 1, 2, 0, S128 + " fwd T0"),
]

# 256x256 rounds + tail: 16,744 rows x 1,024 columns (one round of 256 tiles = 16,384 rows; the seam lies inside an image row
# of the second image), and 16,384 rows exactly (no tail launch). TAIL picks the tile of the 360 rows left over.
_BIG = dict(N=2, H=92, W=91)
_R = S256 + " %s T0"
for tail, tname in ((0, S128Q), (1, S64x128), (2, S64)):
    CONV_CASES.append(_c("fwd_256_tail%d_1x1" % tail, "fwd", 2, 92, 91, 320, 1024, 1, 1, 0, [_R % "fwd", tname + " fwd T1"],
                         dict(T128LO, TAIL=tail), big=True))
CONV_CASES += [
    _c("fwd_256_tail2_1x1_rt", "fwd", 2, 92, 91, 320, 1024, 1, 1, 0, [_R % "fwd", S64 + " fwd T0"], dict(T128LO, TAIL=2, **NOST), big=True),
    _c("fwd_256_notail_1x1", "fwd", 2, 64, 128, 320, 1024, 1, 1, 0, [_R % "fwd"], T128LO, big=True),
    _c("fwd_256_tail2_3x3", "fwd", 2, 92, 91, 64, 1024, 3, 1, 1, [_R % "fwd", S64 + " fwd T9"], dict(T128LO, TAIL=2), big=True),
    _c("dgrad_256_tail2_1x1", "dgrad", 2, 92, 91, 1024, 320, 1, 1, 0, [_R % "dgrad", S64 + " dgrad T1"], dict(T128LO, TAIL=2), big=True),
    _c("dgrad_256_tail0_3x3", "dgrad", 2, 92, 91, 1024, 64, 3, 1, 1, [_R % "dgrad", S128Q + " dgrad T9"], dict(T128LO, TAIL=0), big=True),
    # one partial round of 256x256 tiles: forward (160 tiles) and the box head's first FC, data gradient (196 tiles)
    _c("fwd_256_partial", "fwd", 2, 64, 80, 1024, 1024, 1, 1, 0, [_R % "fwd"], big=True),
    _c("dgrad_256_partial_fc1", "dgrad", 1024, 1, 1, 12544, 1024, 1, 1, 0, [_R % "dgrad"], big=True),
]

# b. parity-grouped stride-2 data gradient: all three tiles; K = 3 / pad 1, K = 1 / pad 0, K = 3 / pad 0; H, W odd and even;
#    an empty parity class (H or W = 1)
PAR_LO, PAR_HI = {"PAR64": 1}, {"PAR64": 1 << 30}
for (K, p) in ((3, 1), (1, 0), (3, 0)):
    for (H, W) in ((9, 11), (9, 12), (10, 11), (10, 12), (1, 13), (14, 1)):
        if (H + 2 * p - K) < 0 or (W + 2 * p - K) < 0:
            continue
        g = "k%dp%d_%dx%d" % (K, p, H, W)
        CONV_CASES += [
            _c("dgrad_par_n64_" + g, "dgrad", 3, H, W, 64, 128, K, 2, p, S128 + " dgrad par T0"),
            _c("dgrad_par_64x128_" + g, "dgrad", 3, H, W, 136, 64, K, 2, p, S64x128 + " dgrad par T0", PAR_LO),
            _c("dgrad_par_64x64_" + g, "dgrad", 3, H, W, 200, 64, K, 2, p, S64 + " dgrad par T0", PAR_HI),
        ]

# c. geometries the descriptor admits but the models never use (run-time loop): forward, data gradient (and weight gradient,
#    GEOM_WGRAD below). stride 2 with K = 2 goes to the parity-grouped kernel, stride 3 to the general strided path.
GEOMS = [("3x3p0", 3, 1, 0), ("3x3p2", 3, 1, 2), ("1x1p1", 1, 1, 1), ("5x5p2", 5, 1, 2), ("1x3p1", (1, 3), 1, 1), ("3x1p1", (3, 1), 1, 1),
         ("1x3p0", (1, 3), 1, 0), ("3x3s3p1", 3, 3, 1), ("2x2s2p0", 2, 2, 0), ("5x5s2p2", 5, 2, 2), ("1x1s3p0", 1, 3, 0)]
for g, K, s, p in GEOMS:
    CONV_CASES.append(_c("fwd_geom_" + g, "fwd", 2, 9, 11, 64, 72, K, s, p, S64 + (" fwd T9" if (K, p) == (3, 1) else " fwd T0")))
    CONV_CASES.append(_c("dgrad_geom_" + g, "dgrad", 2, 9, 11, 72, 64, K, s, p, S64 + (" dgrad par T0" if s == 2 else " dgrad T0")))
GEOM_WGRAD = [dict(name="wgrad_geom_" + g, N=2, H=9, W=11, Cin=72, Cout=40, KH=K if isinstance(K, int) else K[0],
                   KW=K if isinstance(K, int) else K[1], s=s, p=p) for g, K, s, p in GEOMS]

CONV_BY_NAME = {c["name"]: c for c in CONV_CASES}
assert len(CONV_BY_NAME) == len(CONV_CASES)

# e. split-K forward: 1,000 rois x 1,024 -> 1,024 (rows not a multiple of any tile; 256 / 64 tiles)
SPLITK_CASES = [dict(name="splitk_tile%d_ks%d" % (t, ks), kind="splitk", N=1000, H=1, W=1, Cin=1024, Cout=1024, KH=1, KW=1, s=1, p=0,
                     tune={"SPLITK_TILE": t}, ksplit=ks, route=[r + " fwd T1"])
                for t, r in ((0, S64), (1, S128Q), (2, S128W)) for ks in (2, 3, 5, 16)]      # 16 slices: 3 -> 6,6,4; 5 -> 4,4,4,4,0
SPLITK_BY_NAME = {c["name"]: c for c in SPLITK_CASES}

# f. chain launch
CHAIN_CASES = [dict(name="chain_ragged", kind="chain", N=2, H=37, W=53, Cin=64, Cout=64, KH=3, KW=3, s=1, p=1, tune={},
                    route=["128x64/4x1/2 fwd T9 chain256"])]

# every instantiation production code (force == 0) or a sweep tool (forced cfg) can reach, derived by reading launch(),
# mxdet_conv2d_fwd_splitk and mxdet_conv2d_fwd_chain in conv.hip. A new route without a case fails test_coverage.
REACHABLE = set()
for D in ("fwd", "dgrad"):
    for t in (S128, S64, S64x128, S128Q):
        REACHABLE |= {"%s %s T%d" % (t, D, k) for k in (0, 1, 9)}
    REACHABLE |= {"%s %s T%d" % (S128W, D, k) for k in (1, 9)}
    REACHABLE |= {"%s %s T0" % (S256, D), "128x128/2x2/4 %s T0" % D}
REACHABLE |= {"%s dgrad par T0" % t for t in (S128, S64x128, S64)}
REACHABLE |= {"128x64/4x1/2 fwd T9 chain256"}
# ... and the roles a launch can play beyond its instantiation
ROLES = {"rounds+tail", "rounds only", "partial round", "splitk 64x64", "splitk 128x128/4", "splitk 128x128/8", "tail 128x128",
         "tail 64x128", "tail 64x64"}


def check_cover(c, recs):
    """The launches of a case cover rows [0, M) exactly once and all columns; returns the case's roles."""
    M, cols = rows_cols(c) if c["kind"] in ("fwd", "dgrad") else (c["N"] * c["H"] * c["W"], c["Cout"])
    roles, at = set(), 0
    for r in recs:
        BM, BN, par, tm, tn, mb = r[1], r[2], r[7], r[10], r[11], r[12]
        assert tn == -(-cols // BN)
        if par:      # four parity classes, each padded to whole tiles
            assert len(recs) == 1 and mb == 0
            s, pd, n = c["s"], c["p"], 0
            for ph in (0, 1):
                for pw in (0, 1):
                    hc = len([h for h in range(c["H"]) if (h + pd) % 2 == ph])
                    wc = len([w for w in range(c["W"]) if (w + pd) % 2 == pw])
                    n += -(-(c["N"] * hc * wc) // BM)
            assert tm == n and s == 2
            at = M
            continue
        assert mb == at, "launch starts at row %d, the previous one ended at %d" % (mb, at)
        at = min(M, mb + tm * BM)
        assert (tm - 1) * BM < at - mb <= tm * BM                  # no tile without a row
    assert at == M, "rows [%d, %d) are not covered" % (at, M)
    if len(recs) == 2:
        assert recs[0][1] == 256 and recs[0][10] * recs[0][11] % 256 == 0      # whole rounds of the chip's 256 CUs
        roles |= {"rounds+tail", "tail %dx%d" % (recs[1][1], recs[1][2])}
    elif recs[0][1] == 256 and not c.get("force"):
        roles.add("rounds only" if recs[0][10] * recs[0][11] % 256 == 0 else "partial round")
    if c["kind"] == "splitk":
        assert recs[0][13] == c["ksplit"] and recs[0][14] == tm * tn * c["ksplit"] and (tm * tn) % 8 == 0
        roles.add("splitk 64x64" if BM == 64 else "splitk 128x128/%d" % (r[3] * r[4]))
    else:
        assert all(r[13] == 0 for r in recs)
    return roles


ALL_SINGLE = CONV_CASES + SPLITK_CASES + CHAIN_CASES


@pytest.mark.parametrize("name", [c["name"] for c in ALL_SINGLE])
def test_case_reaches_its_route(name):
    c = {x["name"]: x for x in ALL_SINGLE}[name]
    recs = conv_records(c)
    assert [route_name(r) for r in recs] == c["route"]
    check_cover(c, recs)
    if c["kind"] in ("fwd", "dgrad") and not any(r[7] for r in recs):
        # the tile-independence reference of each launch's flavour really is the 64x64 tile of that flavour
        for taps in {r[8] for r in recs}:
            b = conv_records(c, tune={}, force=baseline_force(taps))
            assert len(b) == 1 and route_name(b[0]) == "%s %s T%d" % (S64, c["kind"], taps)
    if c["route"] == [S64x128 + " dgrad par T0"]:
        # ... and of the parity-grouped flavour: the same layer under PAR64 high is the 64x64 parity tile
        assert [route_name(r) for r in conv_records(c, tune=PAR_HI)] == [S64 + " dgrad par T0"]


def test_coverage():
    seen, roles = set(), set()
    for c in ALL_SINGLE:
        recs = conv_records(c)
        seen |= {route_name(r) for r in recs}
        roles |= check_cover(c, recs)
    assert REACHABLE - seen == set(), "instantiations without a case: %s" % sorted(REACHABLE - seen)
    assert seen - REACHABLE == set(), "cases on routes the list does not know: %s" % sorted(seen - REACHABLE)
    assert ROLES - roles == set(), "roles without a case: %s" % sorted(ROLES - roles)
    # every route is listed by the cases' own `route` fields, so deleting the only case of a route fails here
    assert {r for c in ALL_SINGLE for r in c["route"]} == REACHABLE


def test_seam_shapes_are_what_the_names_say():
    for c in CONV_CASES:
        if c.get("big") and len(c["route"]) == 2:
            recs = conv_records(c)
            mb = recs[1][12]
            hw = c["H"] * c["W"]
            assert c["N"] >= 2 and mb % hw != 0 and (mb % hw) % c["W"] != 0      # inside an image, inside an image row
    for tile, bm in ((S128, 128), (S64, 64), (S64x128, 64), (S128Q, 128), (S128W, 128)):
        rel = set()
        for c in CONV_CASES:
            if c["route"][0].startswith(tile) and not c.get("big") and " par" not in c["route"][0]:
                M, cols = rows_cols(c)
                rel.add(M % bm)
        assert {bm - 1, 0, 1} <= rel, (tile, sorted(rel))          # rows one below / at / one above a multiple of BM


# ---------------------------------------------------------------------------------------------------------------------
# c. what validate() refuses is refused with MXDET_ESHAPE and a message, before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = lib()
    base = dict(N=1, H=9, W=9, Cin=64, Cout=64, KH=3, KW=3, s=1, p=1)

    def both(d, word):
        for fn in (L.mxdet_conv2d_fwd, L.mxdet_conv2d_dgrad):
            assert fn(C.byref(d), DUMMY, DUMMY, None, None, DUMMY, None) == ESHAPE
            assert word in L.mxdet_last_error(), L.mxdet_last_error()
    with probe() as read:
        both(desc(dict(base, KH=6, KW=5, p=2)), b"25 filter taps")
        d = desc(base)
        d.Ho += 1
        both(d, b"Ho/Wo")
        d = desc(base)
        d.stride = 0
        both(d, b"non-positive")
        d = desc(dict(base, p=0))
        d.pad = -1
        both(d, b"non-positive")
        d = desc(dict(base, Cin=72))
        assert L.mxdet_conv2d_fwd(C.byref(d), DUMMY, DUMMY, None, None, DUMMY, None) == ESHAPE and b"Cin" in L.mxdet_last_error()
        d = desc(dict(base, Cout=72))
        assert L.mxdet_conv2d_dgrad(C.byref(d), DUMMY, DUMMY, None, None, DUMMY, None) == ESHAPE and b"Cout" in L.mxdet_last_error()
        # split-K: tile count not a multiple of 8, more splits than channel slices, not a 1x1
        sk = dict(N=100, H=1, W=1, Cin=1024, Cout=192, KH=1, KW=1, s=1, p=0)
        args = (DUMMY, DUMMY, None, None, DUMMY)
        assert L.mxdet_conv2d_fwd_splitk(C.byref(desc(sk)), *args, 4, DUMMY, 1 << 40, None) == ESHAPE
        assert b"multiple of 8" in L.mxdet_last_error()
        assert L.mxdet_conv2d_fwd_splitk(C.byref(desc(dict(sk, Cout=256, N=128))), *args, 17, DUMMY, 1 << 40, None) == ESHAPE
        assert b"ksplit" in L.mxdet_last_error()
        assert L.mxdet_conv2d_fwd_splitk(C.byref(desc(dict(base, Cin=1024))), *args, 4, DUMMY, 1 << 40, None) == ESHAPE
        assert b"1x1" in L.mxdet_last_error()
        assert L.mxdet_conv2d_fwd_splitk(C.byref(desc(dict(sk, Cout=256, N=128))), *args, 4, DUMMY, 16, None) == EWORKSPACE
        assert read() == []            # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# g. grouped forward / data gradient: 4 tiles x 3 tap classes x 2 kinds
# ---------------------------------------------------------------------------------------------------------------------
LEVELS = [(2, 13, 21), (2, 7, 11), (1, 5, 3)]         # 546 / 154 / 15 rows: block counts that are not multiples of 8
GROUP_TILES = {0: (S128, {}, 8, 46), 1: (S128Q, T128LO, 7, 45), 2: (S64x128, T64LO, 6, 41), 3: (S64, {}, 5, 40)}   # cfg -> tile, steer, forced cfgs
GROUP_CASES = []
for kind in ("fwd", "dgrad"):
    for cfg in range(4):
        for tc, Ks in ((0, (3, 1, 3)), (1, (1, 1, 1)), (2, (3, 3, 3))):
            GROUP_CASES.append(dict(name="group_%s_cfg%d_tc%d" % (kind, cfg, tc), kind=kind, cfg=cfg, tc=tc, Ks=Ks, red=320,
                                    col=64 if cfg == 0 else 136, tune=GROUP_TILES[cfg][1]))
GROUP_BY_NAME = {c["name"]: c for c in GROUP_CASES}


def group_items(c):
    """[(N, H, W, Cin, Cout, K, pad)] of a grouped case."""
    return [(N, H, W) + ((c["red"], c["col"]) if c["kind"] == "fwd" else (c["col"], c["red"])) + (K, K // 2)
            for (N, H, W), K in zip(LEVELS, c["Ks"])]


@pytest.mark.parametrize("name", [c["name"] for c in GROUP_CASES])
def test_grouped_case_reaches_its_route(name):
    from mxdetection_amd import _lib
    c = GROUP_BY_NAME[name]
    items = group_items(c)
    arr = (_lib.ConvItemT * len(items))()
    for it, (N, H, W, Cin, Cout, K, pad) in zip(arr, items):
        it.desc = desc(dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=K, KW=K, s=1, p=pad))
        it.src = it.filt = it.dst = DUMMY.value
    with steer(c["tune"]) as L, probe() as read:
        nbytes = L.mxdet_conv2d_grouped_table_bytes(len(items))
        host = (C.c_ubyte * nbytes)()
        cfg, grid = C.c_int32(-1), C.c_int32(-1)
        k = 0 if c["kind"] == "fwd" else 1
        assert L.mxdet_conv2d_grouped_plan(arr, len(items), k, host, nbytes, C.byref(cfg), C.byref(grid)) == 0, L.mxdet_last_error()
        assert (cfg.value & 3, cfg.value >> 2) == (c["cfg"], c["tc"])
        tile = GROUP_TILES[c["cfg"]][0]
        BM, BN = [int(v) for v in tile.split("/")[0].split("x")]
        blocks = [-(-(N * H * W) // BM) * -(-c["col"] // BN) for (N, H, W) in LEVELS]
        assert any(b % 8 for b in blocks[:-1])                     # alignment padding between items is exercised
        assert grid.value == sum(-(-b // 8) * 8 for b in blocks)
        assert L.mxdet_conv2d_grouped(DUMMY, len(items), k, cfg.value, grid.value, None) == 0
        recs = read()
    taps = {0: 0, 1: 1, 2: 9}[c["tc"]]
    assert len(recs) == 1 and recs[0][0] == 3 and route_name(recs[0]) == "%s %s T%d" % (tile, c["kind"], taps)
    assert recs[0][14] == grid.value
    # the single launch each item is compared with runs the same tile in the same flavour
    f = GROUP_TILES[c["cfg"]][2 if taps == 0 else 3]
    for (N, H, W, Cin, Cout, K, pad) in items:
        one = dict(kind=c["kind"], N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=K, KW=K, s=1, p=pad)
        r = conv_records(one, tune={}, force=f)
        assert [route_name(x) for x in r] == ["%s %s T%d" % (tile, c["kind"], 0 if taps == 0 else K * K)]


def test_grouped_coverage():
    assert {(c["kind"], c["cfg"], c["tc"]) for c in GROUP_CASES} == {(k, g, t) for k in ("fwd", "dgrad") for g in range(4) for t in range(3)}


# ---------------------------------------------------------------------------------------------------------------------
# h. weight gradient, single launch. route = (three-tap, ksplit, ring three-tap, ring one-tap, fold)
# ---------------------------------------------------------------------------------------------------------------------
def _w(name, N, H, W, Cin, Cout, K, s, p, route, ksplit=0, tune=None, bias=True, acc=False):
    return dict(name=name, N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=K, KW=K, s=s, p=p, ksplit=ksplit, tune=tune or {}, bias=bias,
                acc=acc, route=route)


T3OFF = {"T3_ENABLE": 0}
WGRAD_CASES = [
    # one-tap kernel, forced splits: 1 (direct write; accumulate without a fold), 2, uneven (7 steps over 3), = step count
    _w("wg_1x1_ks1", 2, 9, 11, 72, 200, 1, 1, 0, (0, 1, 0, 4, 0), 1),
    _w("wg_1x1_ks1_acc", 2, 9, 11, 72, 200, 1, 1, 0, (0, 1, 0, 4, 0), 1, acc=True),
    _w("wg_1x1_ks2", 2, 9, 11, 200, 72, 1, 1, 0, (0, 2, 0, 4, 1), 2),
    _w("wg_1x1_ks3_uneven", 2, 9, 11, 72, 200, 1, 1, 0, (0, 3, 0, 4, 1), 3, bias=False),
    _w("wg_1x1_ks_steps", 2, 9, 11, 8, 8, 1, 1, 0, (0, 7, 0, 4, 1), 7),
    _w("wg_1x1_ks_over", 2, 9, 11, 8, 72, 1, 1, 0, (0, 7, 0, 4, 1), 50, acc=True),     # more than the step count: clamped
    _w("wg_1x1_below_step", 5, 1, 1, 200, 8, 1, 1, 0, (0, 1, 0, 4, 0)),
    _w("wg_s2_3x3", 2, 13, 21, 72, 136, 3, 2, 1, (0, 2, 0, 4, 1), 2),
    # ring depth 2: more than 512 workgroups (2 x 2 x 9 tiles x 15 splits + bias workgroups)
    _w("wg_3x3_onetap_ns2", 2, 25, 42, 256, 256, 3, 1, 1, (0, None, 0, 2, 1), 15, T3OFF),
    # three-tap kernel: ring depth 2 and 3, and the one-tap kernel on the same shapes
    _w("wg_3x3_t3_ns2", 2, 13, 21, 72, 200, 3, 1, 1, (1, 3, 2, 4, 1), 3),
    _w("wg_3x3_t3_ns3", 2, 13, 21, 72, 200, 3, 1, 1, (1, 3, 3, 4, 1), 3, {"T3_NS": 3}),
    _w("wg_3x3_t3_off", 2, 13, 21, 72, 200, 3, 1, 1, (0, 3, 0, 4, 1), 3, T3OFF),
    _w("wg_3x3_t3_ks1_nobias", 1, 12, 9, 200, 72, 3, 1, 1, (1, 1, 2, 0, 0), 1, bias=False),
    _w("wg_3x3_t3_ks1_acc", 1, 12, 9, 8, 8, 3, 1, 1, (1, 1, 2, 4, 0), 1, acc=True),
    _w("wg_3x3_t3_heuristic", 2, 25, 42, 128, 128, 3, 1, 1, (1, None, 2, 4, 1)),
    # eligibility edge 64 / (W + 1) + 1 <= H, W = 7: H = 8 (one-tap), 9 and 10 (three-tap)
    _w("wg_3x3_elig_below", 2, 8, 7, 72, 72, 3, 1, 1, (0, 2, 0, 4, 1), 2),
    _w("wg_3x3_elig_at", 2, 9, 7, 72, 72, 3, 1, 1, (1, 2, 2, 4, 1), 2),
    _w("wg_3x3_elig_above", 2, 10, 7, 72, 72, 3, 1, 1, (1, 2, 2, 4, 1), 2),
]
WGRAD_BY_NAME = {c["name"]: c for c in WGRAD_CASES}
WGRAD_REACHABLE = {("one-tap", 4), ("one-tap", 2), ("three-tap", 2), ("three-tap", 3), "fold", "direct", "direct+accumulate",
                   "three-tap direct", "three-tap without bias workgroups"}


def wgrad_record(c, ksplit=None, tune=None, ws=1 << 40):
    with steer(c.get("tune") if tune is None else tune, 0, c.get("ksplit", 0) if ksplit is None else ksplit) as L, probe() as read:
        d = desc(c, accumulate=c.get("acc", False))
        rc = L.mxdet_conv2d_wgrad(C.byref(d), DUMMY, DUMMY, DUMMY, DUMMY if c.get("bias", True) else None, DUMMY, ws, None)
        need = L.mxdet_conv2d_wgrad_workspace_bytes(C.byref(d))
        return rc, read(), need


def wgrad_check(c, r):
    """The record is consistent: the splits cover every step, none is empty."""
    M = c["N"] * out_hw(c)[0] * out_hw(c)[1]
    t3, ks, sps, t3s, steps, steps3 = r[1], r[2], r[3], r[4], r[11], r[12]
    assert steps == -(-M // 32)                                # MXDET_WGRAD_BKP = 32 pixels per step (the case table counts on it)
    assert sps * ks >= steps and sps * (ks - 1) < steps, "one-tap / bias ranges: %d splits x %d steps for %d steps" % (ks, sps, steps)
    if t3:
        assert steps3 == -(-(c["N"] * c["H"] * (c["W"] + 1)) // 64)
        assert t3s * ks >= steps3 and t3s * (ks - 1) < steps3, "three-tap ranges: %d x %d for %d steps" % (ks, t3s, steps3)
    assert r[7] == (1 if ks > 1 else 0)


@pytest.mark.parametrize("name", [c["name"] for c in WGRAD_CASES])
def test_wgrad_case_reaches_its_route(name):
    c = WGRAD_BY_NAME[name]
    rc, recs, need = wgrad_record(c)
    assert rc == 0 and len(recs) == 1 and recs[0][0] == 2
    r = recs[0]
    want = c["route"]
    got = (r[1], r[2], r[5], r[6], r[7])
    assert all(w is None or w == g for w, g in zip(want, got)), (got, want)
    wgrad_check(c, r)
    # one byte too little workspace is refused before anything is recorded
    rc, recs, _ = wgrad_record(c, ws=need - 1)
    assert rc == EWORKSPACE and recs == []


def wgrad_roles(c, r):
    roles = {("three-tap", r[5])} if r[1] else {("one-tap", r[6])}
    roles.add("fold" if r[7] else ("direct+accumulate" if r[10] else "direct"))
    if r[1] and not r[7]:
        roles.add("three-tap direct")
    if r[1] and r[6] == 0:
        roles.add("three-tap without bias workgroups")
    return roles


def test_wgrad_coverage():
    seen = set()
    for c in WGRAD_CASES:
        seen |= wgrad_roles(c, wgrad_record(c)[1][0])
    assert WGRAD_REACHABLE - seen == set(), sorted(map(str, WGRAD_REACHABLE - seen))


@pytest.mark.parametrize("g", [g["name"] for g in GEOM_WGRAD])
def test_wgrad_geometries_are_planned(g):
    c = {x["name"]: x for x in GEOM_WGRAD}[g]
    rc, recs, _ = wgrad_record(c, ksplit=2, tune={})
    assert rc == 0 and len(recs) == 1 and recs[0][1] == 0
    wgrad_check(c, recs[0])


# ---------------------------------------------------------------------------------------------------------------------
# i. weight gradient, grouped: the seven-item mix of test_grouped_wgrad_three_tap_tiles + one filter shared by two levels
# ---------------------------------------------------------------------------------------------------------------------
# (N, H, W, Cin, Cout, K, stride, pad, bias, dw slot): items with the same slot share dw / db
WGG_ITEMS = [(2, 25, 42, 256, 256, 3, 1, 1, True, 0), (2, 13, 21, 512, 448, 1, 1, 0, True, 1), (1, 26, 44, 256, 512, 3, 2, 1, False, 2),
             (300, 1, 1, 1024, 256, 1, 1, 0, True, 3), (2, 25, 42, 64, 128, 3, 1, 1, True, 4), (1, 9, 130, 72, 200, 3, 1, 1, True, 5),
             (3, 12, 7, 128, 64, 3, 1, 1, False, 6), (2, 13, 21, 256, 256, 3, 1, 1, True, 7), (2, 7, 11, 256, 256, 3, 1, 1, True, 7)]
ONE_SPLIT = {"WG_TARGET": 1, "WG_MINSTEPS": 1 << 20, "WG_MAXSTEPS": 1 << 20, "T3_TARGET": 1, "T3_MINSTEPS": 1 << 15}
MANY_SPLITS = {"WG_TARGET": 1 << 20, "WG_MINSTEPS": 1, "WG_MAXSTEPS": 2, "T3_TARGET": 1 << 20, "T3_MINSTEPS": 1, "T3_PER_ITEM": 0}
# name -> (tuning, (mixed grid, ring depth three-tap tiles, ring depth one-tap tiles), splits: None / "one" / "many")
WGG_CASES = {
    "wgg_default": ({}, (1, 2, 3), None),
    "wgg_mix2": ({"T3_MIX": 2}, (2, 2, 2), None),
    "wgg_mix0_ns2": ({"T3_MIX": 0, "WG_NS": 2}, (0, 2, 2), None),
    "wgg_mix0_ns3": ({"T3_MIX": 0, "WG_NS": 3}, (0, 2, 3), None),
    "wgg_mix0_ns4_t3ns3": ({"T3_MIX": 0, "WG_NS": 4, "T3_NS": 3}, (0, 3, 4), None),
    "wgg_per_item0": ({"T3_PER_ITEM": 0}, (1, 2, 3), None),
    "wgg_per_item8": ({"T3_PER_ITEM": 8}, (1, 2, 3), "one3"),            # a cap below one split's tiles: every 3x3 layer one split
    "wgg_one_split": (ONE_SPLIT, (1, 2, 3), "one"),
    "wgg_one_split_mix0": (dict(ONE_SPLIT, T3_MIX=0), (0, 2, 2), "one"),
    "wgg_many_splits": (MANY_SPLITS, (1, 2, 3), "many"),
    "wgg_many_splits_mix0_ns4": (dict(MANY_SPLITS, T3_MIX=0, WG_NS=4), (0, 2, 4), "many"),
}
WGG_REACHABLE = {"mixed<2,3>", "mixed<2,2>", "three-tap<2>", "three-tap<3>", "one-tap<2>", "one-tap<3>", "one-tap<4>"}


def _t3(it):
    N, H, W, Cin, Cout, K, s, p = it[:8]
    return K == 3 and s == 1 and p == 1 and 64 // (W + 1) + 1 <= H


def wgg_plan(L, items=WGG_ITEMS, ptr=lambda i, what: 4096 * (1 + 8 * i + what)):
    """mxdet_conv2d_wgrad_grouped_plan of the mix under the steering in effect; ptr(i, 0..3) = address of x / dy / dw / db."""
    from mxdetection_amd import _lib
    arr = (_lib.WgradItemT * len(items))()
    for i, (it, a) in enumerate(zip(items, arr)):
        N, H, W, Cin, Cout, K, s, p, bias, slot = it
        a.desc = desc(dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=K, KW=K, s=s, p=p))
        a.x, a.dy, a.dw, a.db = ptr(i, 0), ptr(i, 1), ptr(slot, 2), (ptr(slot, 3) if bias else None)
    nbytes = L.mxdet_conv2d_wgrad_grouped_table_bytes(len(items))
    host = (C.c_ubyte * nbytes)()
    ws, gw, gb, gr = C.c_size_t(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = L.mxdet_conv2d_wgrad_grouped_plan(arr, len(items), host, nbytes, C.byref(ws), C.byref(gw), C.byref(gb), C.byref(gr))
    assert rc == 0, L.mxdet_last_error()
    return host, ws.value, gw.value, gb.value, gr.value


def wgg_kernels(r):
    assert r[0] == 4
    mix, ns3, ns1 = r[1], r[2], r[3]
    if mix:
        return {"mixed<2,%d>" % ns1}
    return ({"three-tap<%d>" % ns3} if ns3 else set()) | ({"one-tap<%d>" % ns1} if ns1 else set())


def wgg_records(name, parts=7, grids=None):
    tune = WGG_CASES[name][0]
    with steer(tune) as L, probe() as read:
        _, ws, gw, gb, gr = wgg_plan(L)
        if grids:
            gw, gb = grids
        assert L.mxdet_conv2d_wgrad_grouped_parts(DUMMY, len(WGG_ITEMS), gw, gb, gr, parts, DUMMY, 1 << 40, ws, None) == 0
        return read(), (ws, gw, gb, gr)


def _align8(n):
    return -(-n // 8) * 8


@pytest.mark.parametrize("name", list(WGG_CASES))
def test_grouped_wgrad_case_reaches_its_route(name):
    tune, want, splits = WGG_CASES[name]
    recs, (ws, gw, gb, gr) = wgg_records(name)
    assert len(recs) == 1 and tuple(recs[0][1:4]) == want and tuple(recs[0][4:8]) == (gb, gw, gr, 7)
    assert gw > 0 and gb > 0 and gw % 8 == 0 and gb % 8 == 0          # both tile kinds; the plan aligns every item to 8 blocks
    t3_one = sum(_align8(-(-it[4] // 128) * -(-it[3] // 64) * 3) for it in WGG_ITEMS if _t3(it))
    t1_one = sum(_align8(-(-it[4] // 128) * (-(-it[3] // 128) * it[5] * it[5] * (0 if _t3(it) else 1) + (1 if it[8] else 0))) for it in WGG_ITEMS)
    if splits in ("one", "one3"):
        assert gb == t3_one
    if splits == "one":
        assert gw == t1_one
        # no fold but for the filter two items share (its two slabs are summed)
        shared = [it for it in WGG_ITEMS if it[9] == 7][0]
        assert gr == -(-(shared[4] * 9 * shared[3] // 4) // 256) + -(-shared[4] // 256)
    if splits == "many":
        assert gb > 8 * t3_one and gw > 8 * t1_one
    if name == "wgg_per_item0":
        assert gb >= wgg_records("wgg_default")[1][2]                  # no cap: at least as many three-tap workgroups
    # the three parts of mxdet_conv2d_wgrad_grouped_parts, issued separately, never use the mixed grid
    for parts, kern in ((1, "three-tap<%d>" % (3 if tune.get("T3_NS") == 3 else 2)),
                        (2, "one-tap<%d>" % (tune.get("WG_NS", 2))), (4, None)):
        r = wgg_records(name, parts)[0]
        assert len(r) == 1 and r[0][1] == 0 and r[0][7] == parts and wgg_kernels(r[0]) == ({kern} if kern else set())
        assert (r[0][4] > 0, r[0][5] > 0, r[0][6] > 0) == (parts == 1, parts == 2, parts == 4)
    # too little workspace is refused before anything is recorded
    with steer(tune) as L, probe() as read:
        assert L.mxdet_conv2d_wgrad_grouped(DUMMY, len(WGG_ITEMS), gw, gb, gr, DUMMY, ws - 1, ws, None) == EWORKSPACE
        assert read() == []


def test_grouped_wgrad_mixed_grid_falls_back():
    """The mixed grid needs both grids to be multiples of 8 (one group of 8 workgroups per XCD). The plan always aligns them, so
    only a caller that passes other grids reaches the fall-back to two launches: asserted from the probe alone (on the GPU such
    grids would not cover the plan's table)."""
    for name in ("wgg_default", "wgg_mix2"):
        for grids in ((16, 12), (12, 16), (9, 7)):
            r = wgg_records(name, 7, grids)[0][0]
            assert r[1] == 0 and wgg_kernels(r) == {"three-tap<2>", "one-tap<2>"}
        assert wgg_records(name, 7, (16, 24))[0][0][1] == (2 if name == "wgg_mix2" else 1)


def test_grouped_wgrad_coverage():
    seen = set()
    for name in WGG_CASES:
        seen |= wgg_kernels(wgg_records(name)[0][0])
    assert seen == WGG_REACHABLE, (sorted(WGG_REACHABLE - seen), sorted(seen - WGG_REACHABLE))
    assert {s for _, _, s in WGG_CASES.values()} >= {"one", "many"}


# ---------------------------------------------------------------------------------------------------------------------
STEERED_KEYS = sorted({k for c in ALL_SINGLE + GROUP_CASES + WGRAD_CASES for k in c["tune"]} | {k for t, _, _ in WGG_CASES.values() for k in t})


def test_zz_steering_is_restored():
    """Every tuning key a case of this module steers is read back and is at the library's default (what value -1 restores);
    the forced cfg / split and the probe are per thread and are checked through the route of plain cases. Named to sort
    last; it holds wherever it runs, because steer() restores on exit."""
    from mxdetection_amd import _lib
    L = lib()
    assert {"T64", "T128", "PAR64", "TAIL", "STATIC_TAPS", "T128W", "SPLITK_TILE", "T3_ENABLE", "T3_NS", "WG_NS", "T3_MIX", "T3_PER_ITEM",
            "WG_TARGET", "WG_MINSTEPS", "WG_MAXSTEPS", "T3_TARGET", "T3_MINSTEPS"} <= set(STEERED_KEYS)
    for k, i in _lib.TUNING_KEYS.items():
        now = L.mxdet_debug_get_tuning(i)
        L.mxdet_debug_set_tuning(i, -1)
        assert L.mxdet_debug_get_tuning(i) == now, "tuning key %s was left at %d" % (k, now)
    assert L.mxdet_debug_get_tuning(99) == -1 and b"unknown key" in L.mxdet_last_error()
    with steer({"T64": 7}):
        assert L.mxdet_debug_get_tuning(_lib.TUNING_KEYS["T64"]) == 7
    assert L.mxdet_debug_get_tuning(_lib.TUNING_KEYS["T64"]) == 400


def test_zz_default_routes_of_plain_cases():
    """Plain cases (forced cfg / split 0, default tunings) take the default routes, and records stay readable after the probe
    is switched off."""
    plain = dict(kind="fwd", N=2, H=14, W=22, Cin=256, Cout=256, KH=3, KW=3, s=1, p=1)
    with probe() as read:
        L = lib()
        d = desc(plain)
        assert L.mxdet_conv2d_fwd(C.byref(d), DUMMY, DUMMY, None, None, DUMMY, None) == 0
        assert [route_name(r) for r in read()] == [S64 + " fwd T9"]
        big = dict(plain, H=200, W=336)                      # 134,400 rows x 256: two rounds of 256x256 tiles + 64x64 tail (TAIL = 2)
        assert L.mxdet_conv2d_fwd(C.byref(desc(big)), DUMMY, DUMMY, None, None, DUMMY, None) == 0
        assert [route_name(r) for r in read()][1:] == [S256 + " fwd T0", S64 + " fwd T9"]
        L.mxdet_debug_route_probe(1)
        w = dict(plain)
        assert L.mxdet_conv2d_wgrad(C.byref(desc(w)), DUMMY, DUMMY, DUMMY, None, DUMMY, 1 << 40, None) == 0
        r = read()[0]
        assert (r[0], r[1], r[5]) == (2, 1, 2)
    buf = (C.c_int32 * 64)()
    assert lib().mxdet_debug_route_read(buf, 4) >= 1        # records stay readable after the probe is switched off
