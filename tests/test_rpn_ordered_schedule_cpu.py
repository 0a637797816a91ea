"""mxdet_rpn_ordered_schedule (host only): the split parameters it reads off a grouped weight-gradient plan of the RPN
head's ten items partition every level's pixels, slabs in item order, at the default and at forced-deep tunings."""
import ctypes as C

import pytest

LEVELS = {"small": [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)], "bench": [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]}
TUNINGS = [{}, {"T3_MINSTEPS": 2, "WG_MINSTEPS": 2, "WG_MAXSTEPS": 2}, {"T3_ENABLE": 0, "WG_MINSTEPS": 2, "WG_MAXSTEPS": 3}]
N, CH, CO = 2, 256, 64


def _plan(lib, _lib, levels, db=True, dw_shared=True):
    from mxdetection_amd.ops.dense import conv_desc
    L = len(levels)
    items = (_lib.WgradItemT * (2 * L))()
    for q in range(2):
        for l, (h, w) in enumerate(levels):
            it = items[q * L + l]
            it.desc = conv_desc(N, h, w, CH, CH if q else CO, 3 if q else 1, 3 if q else 1, 1, 1 if q else 0, accumulate=False)
            it.x, it.dy = 0x1000, 0x2000                      # the planner only compares and stores the addresses
            it.dw = 0x100000 * (q + 1) + (0 if dw_shared else 0x1000 * l)
            it.db = 0x10000 * (q + 1) if db else None
    nbytes = lib.mxdet_conv2d_wgrad_grouped_table_bytes(2 * L)
    host = (C.c_ubyte * nbytes)()
    ws, gw, gb, gr = C.c_size_t(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    assert lib.mxdet_conv2d_wgrad_grouped_plan(items, 2 * L, host, nbytes, C.byref(ws), C.byref(gw), C.byref(gb), C.byref(gr)) == 0
    return host


@pytest.mark.parametrize("tuning", TUNINGS, ids=["default", "deep", "onetap_deep"])
@pytest.mark.parametrize("pyramid", list(LEVELS))
def test_schedule_partitions_every_level(pyramid, tuning):
    from mxdetection_amd import _lib
    lib = _lib.load()
    levels = LEVELS[pyramid]
    L = len(levels)
    for k, v in tuning.items():
        lib.mxdet_debug_set_tuning(_lib.TUNING_KEYS[k], v)
    try:
        host = _plan(lib, _lib, levels)
        out = (_lib.RpnOrderedItemT * (2 * L))()
        assert lib.mxdet_rpn_ordered_schedule(host, 2 * L, L, out) == 0, lib.mxdet_last_error()
    finally:
        for k in tuning:
            lib.mxdet_debug_set_tuning(_lib.TUNING_KEYS[k], -1)
    for q in range(2):
        items = out[q * L:(q + 1) * L]
        assert items[0].slab0 == 0
        for l, it in enumerate(items):
            h, w = levels[l]
            assert (it.H, it.W) == (h, w) and it.fold_ksplit == items[0].fold_ksplit
            if q == 0 or tuning.get("T3_ENABLE") == 0:
                assert it.kind == 0
            slabs = (items[l + 1].slab0 if l + 1 < L else it.fold_ksplit) - it.slab0
            pixels = N * h * (w + 1 if it.kind else w)
            span = it.halves_per_slab * 32
            assert slabs >= 1 and (slabs - 1) * span < pixels <= slabs * span
            assert it.bias_splits == slabs and it.bias_pixels % 32 == 0
            # (a three-tap item splits its virtual pixels; the bias ranges over the real ones may leave trailing splits empty)
            assert N * h * w <= slabs * it.bias_pixels and (it.kind == 1 or (slabs - 1) * it.bias_pixels < N * h * w)
        if "WG_MAXSTEPS" in tuning:
            assert items[0].fold_ksplit > L                   # forced deep: several slabs per level


def test_schedule_rejects_other_groups():
    from mxdetection_amd import _lib
    lib = _lib.load()
    levels = LEVELS["small"]
    L = len(levels)
    out = (_lib.RpnOrderedItemT * (2 * L))()
    host = _plan(lib, _lib, levels)
    assert lib.mxdet_rpn_ordered_schedule(host, 2 * L - 1, L, out) != 0
    assert lib.mxdet_rpn_ordered_schedule(None, 2 * L, L, out) != 0
    assert lib.mxdet_rpn_ordered_schedule(_plan(lib, _lib, levels, db=False), 2 * L, L, out) != 0
    assert lib.mxdet_rpn_ordered_schedule(_plan(lib, _lib, levels, dw_shared=False), 2 * L, L, out) != 0
