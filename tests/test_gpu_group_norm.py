"""GroupNorm kernels (csrc/group_norm.hip) against the fp64 reference of tests/test_group_norm_cpu.py, evaluated on the
same bf16 inputs.

Bounds. bf16 outputs (y, dx): the project's bf16 bound, |got - ref| <= 2^-7 |ref| + 2^-7 rms(ref) elementwise, no
element exempt. fp32 outputs: the forward-error bound of an fp32 sum of n terms, n * 2^-23 * sum|term| (twice the worst
case of any summation order, covering the rounding of the terms), computed from the fp64 reference: mean (terms x / m),
dgamma (terms g * xh), dbeta (terms g); rstd: relative error n * 2^-23 with n = HW * C / G.
dgamma is a sum of terms g * xh whose factor xh = (x - mean) * rstd is built from backward's INPUTS mean and rstd, which
are fp32 numbers. A stored fp32 value is off by up to 2^-24 relative from its rounding alone, and with |mean| up to 32
standard deviations that half ulp of mean already moves every xh of the group by 32 * 2^-24: more than n * 2^-23 * |xh|
allows for small n, whatever the kernel does. So dgamma is asserted, against the pure fp64 reference, within
    n * 2^-23 * sum|g * xh|  +  2^-22 * sum_n |mean| * rstd * sum_hw|g|  +  2^-22 * sum|g * xh|,
the issue's sum bound plus the first-order effect (d xh / d mean = -rstd, d xh / d rstd = xh / rstd) of TWO ULPS
(2^-22 relative) of each stored statistic: one for the rounding of the store, one for a stable computation of the value.
The allowance is fixed by the number format; it does not grow with the group size m, and it is not taken from what the
kernels return (how far their mean / rstd really are from fp64 is asserted separately, above). Relative to the issue's
bound the two extra terms are 2 * (|mean| / sigma) * sum|g| / (n * sum|g * xh|) + 2 / n with n = N * HW: about 42 / n
on ordinary channels at these inputs. On the two head shapes and the pyramid shape (n >= 33600) the asserted bound is
1.001 to 1.002 times the issue's on every ordinary channel; on the 8 channels of the constant group, where
|mean| * rstd = 5.25 / sqrt(eps) = 1660, it is up to 1.25 times at the pyramid shape (N = 2) and 1.002 at the head shapes.
It is a real widening only where n is small (median over channels 1.1 to 1.5 for n = 50 to 250, 3 for n = 14 to 18, 8
to 26 for n <= 6), which is the conditioning |mean| / sigma of those inputs in an fp32 mean and not slack. On both sides
of the route boundary (n = 2048 / 2050 and 256 / 258) the median is 1.02 and 1.13 to 1.16, the constant group's channels
5 to 6 and 41; on the accumulate cases (n = 3137, 4201) median 1.01, maximum 1.06 and 2.8.
Measured on an MI355X, dgamma error / the issue's bound alone: at most 3.6e-5 on the head and pyramid shapes, 8.4e-3 on
the route-boundary cases, 1.9e-4 on the accumulate cases; above 1 only for [1,3,64] (5.5), [2,3,512] (5.0) and [1,1,64]
(1.3), where n <= 6 and the asserted bound is 17, 8 and 26 times the issue's in the median.
_dgamma_bound prints asserted bound / issue's bound (median and maximum over channels) for every case and asserts
median < 1.01 and maximum < 1.3 whenever n >= 30000, so a wider bound cannot creep in on the named shapes. dbeta does
not depend on the statistics and keeps the plain sum bound.
Under ReLU the backward reference takes its mask from the bf16 y the kernel stored (y itself is checked first): where
the exact y is within rounding of zero the two masks may differ, and the contract is "where y > 0"."""
import numpy as np
import pytest
import torch

from test_group_norm_cpu import gn_ref, gn_ref_backward

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _close(got, ref, what="", tol=2.0 ** -7):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rms = np.sqrt(np.mean(ref ** 2)) + 1e-30
    err = np.abs(got - ref)
    bound = tol * np.abs(ref) + tol * rms
    bad = err > bound
    print("%s: max err %.4g, rms %.4g, worst err/bound %.3f" % (what, err.max(), rms, (err / bound).max()))
    assert not bad.any(), "%s: %d/%d outside tolerance, max err %.4g (rms %.4g)" % (what, bad.sum(), bad.size, err.max(), rms)


STAT_ULPS = 2.0 ** -22      # two ulps of a stored fp32 statistic (module docstring)


def _stat_terms(rmean, rrstd, gmask, xh, G):
    """Per-channel first-order effect on dgamma of STAT_ULPS of relative error in the stored mean and rstd."""
    cpg = gmask.shape[2] // G
    per_c = np.repeat(np.abs(rmean) * rrstd, cpg, axis=1)                                  # [N, C]: |mean| * rstd
    return STAT_ULPS * ((per_c * np.abs(gmask).sum(axis=1)).sum(axis=0) + np.abs(gmask * xh).sum(axis=(0, 1)))


def _dgamma_bound(got, ref, n, terms, extra, what):
    """Asserts dgamma; prints its error against the issue's sum bound alone and how far the asserted bound exceeds it."""
    plain = np.maximum(n * 2.0 ** -23 * terms, 1e-300)
    err = np.abs(np.asarray(got, np.float64) - ref)
    widen = (plain + extra) / plain
    print("%s: err / plain sum bound %.4g; asserted bound / plain sum bound: median %.4g, max %.4g" % (
        what, (err / plain).max(), np.median(widen), widen.max()))
    assert n < 30000 or (np.median(widen) < 1.01 and widen.max() < 1.3), "%s: statistics allowance too wide" % what
    _sum_bound(got, ref, n, terms, what, extra=extra)


def _sum_bound(got, ref, n, abs_terms_sum, what, extra=0.0):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = n * 2.0 ** -23 * abs_terms_sum + extra
    err = np.abs(got - ref)
    print("%s: max err %.4g, worst err/bound %.4g" % (what, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound), "%s: %d outside the fp32 sum bound, max err %.4g" % (what, (err > bound).sum(), err.max())


def _inputs(N, HW, Cc, G, seed):
    """Gaussian data plus a per-(sample, group) offset of up to 32 standard deviations; group 1 % G of sample 0 constant;
    gamma with mixed signs and zeros. Returned as bf16 device tensors and the float64 values of the same bf16 numbers."""
    g = torch.Generator().manual_seed(seed)
    cpg = Cc // G
    x = torch.randn((N, HW, G, cpg), generator=g)
    x = x + (torch.rand((N, 1, G, 1), generator=g) * 64.0 - 32.0)
    x[0, :, 1 % G, :] = 5.25
    x = x.reshape(N, HW, Cc).to(torch.bfloat16)
    dy = torch.randn((N, HW, Cc), generator=g).to(torch.bfloat16)
    gamma = torch.randn((Cc,), generator=g)
    gamma[::7] = 0.0
    beta = torch.randn((Cc,), generator=g) * 0.5
    dev = {"x": x.cuda(), "dy": dy.cuda(), "gamma": gamma.cuda(), "beta": beta.cuda()}
    ref = {k: v.double().numpy() for k, v in (("x", x), ("dy", dy), ("gamma", gamma), ("beta", beta))}
    return dev, ref


def _run(dev, G, relu, with_y=True, accumulate=None):
    from mxdetection_amd.ops import group_norm as GN
    y, mean, rstd = GN.group_norm_forward(dev["x"], dev["gamma"], dev["beta"], G, EPS, relu)
    Cc = dev["x"].shape[-1]
    if accumulate is None:
        dg = torch.full((Cc,), float("nan"), device="cuda")
        db = torch.full((Cc,), float("nan"), device="cuda")
    else:
        dg, db = accumulate[0].clone(), accumulate[1].clone()
    dx = GN.group_norm_backward(dev["x"], dev["dy"], mean, rstd, dev["gamma"], G, dg, db, y=y if with_y else None,
                                beta=dev["beta"], eps=EPS, relu=relu, accumulate=accumulate is not None)
    torch.cuda.synchronize()
    return y, mean, rstd, dx, dg, db


def _check(N, HW, Cc, G, relu, seed=0, route=None):
    from mxdetection_amd.ops import group_norm as GN
    if route is not None:
        assert GN.route((N, HW, Cc), G) == route
    dev, ref = _inputs(N, HW, Cc, G, seed)
    y, mean, rstd, dx, dg, db = _run(dev, G, relu)
    m = HW * Cc // G
    ry, rmean, rrstd = gn_ref(ref["x"], ref["gamma"], ref["beta"], G, EPS, relu)
    tag = "[%d,%d,%d] G=%d relu=%d" % (N, HW, Cc, G, relu)
    _close(y.float().cpu().numpy(), ry, tag + " y")
    absx = np.abs(ref["x"]).reshape(N, HW, G, Cc // G).sum(axis=(1, 3)) / m
    _sum_bound(mean.cpu().numpy(), rmean, m, absx, tag + " mean")
    rel = np.abs(rstd.cpu().numpy().astype(np.float64) / rrstd - 1.0)
    print("%s rstd: max rel err %.4g, bound %.4g" % (tag, rel.max(), m * 2.0 ** -23))
    assert np.all(rel <= m * 2.0 ** -23)
    assert abs(float(rstd[0, 1 % G]) / (1.0 / np.sqrt(EPS)) - 1.0) <= m * 2.0 ** -23     # the constant group
    ymask = (y.float().cpu().numpy() > 0) if relu else None
    rdx, rdg, rdb = gn_ref_backward(ref["x"], ref["dy"], ref["gamma"], ref["beta"], G, EPS, relu, y_mask=ymask)
    _close(dx.float().cpu().numpy(), rdx, tag + " dx")
    # the two parameter sums against the pure fp64 reference
    gmask = ref["dy"] * (ymask if relu else 1.0)
    xh = ((ref["x"].reshape(N, HW, G, Cc // G) - rmean[:, None, :, None]) * rrstd[:, None, :, None]).reshape(N, HW, Cc)
    terms = np.abs(gmask * xh).sum(axis=(0, 1))
    _dgamma_bound(dg.cpu().numpy(), rdg, N * HW, terms, _stat_terms(rmean, rrstd, gmask, xh, G), tag + " dgamma")
    _sum_bound(db.cpu().numpy(), rdb, N * HW, np.abs(gmask).sum(axis=(0, 1)), tag + " dbeta")
    return dev, (y, mean, rstd, dx, dg, db)


RES, TIL = 1, 2


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("N,HW,Cc,G,route", [
    (1024, 49, 256, 32, RES),            # box head
    (256, 196, 256, 32, RES),            # mask head
    (2, 100 * 168, 256, 32, TIL),        # pyramid map
])
def test_head_and_pyramid_shapes(N, HW, Cc, G, route, relu):
    _check(N, HW, Cc, G, relu, seed=1, route=route)


@pytest.mark.parametrize("N,HW,Cc,G,relu", [
    (3, 1, 256, 32, True), (1, 3, 64, 8, False), (5, 50, 64, 8, True), (1, 50, 512, 16, True), (2, 3, 512, 32, False),
    (1, 1, 64, 8, True), (4, 50, 256, 16, False), (2, 9, 1024, 32, True), (2, 7, 192, 8, True), (3, 300, 64, 1, False),
])
def test_small_odd_shapes(N, HW, Cc, G, relu):
    _check(N, HW, Cc, G, relu, seed=2)


@pytest.mark.parametrize("Cc,G", [(64, 8), (512, 16)])
def test_both_sides_of_the_route_boundary(Cc, G):
    """GN.route() is the probe: a host function of the shape that shares gn_plan with the entries, i.e. it reports the
    route the entries select, not a record of a launch. That the two sides really run different kernels shows in their
    workspace needs (the resident forward takes none) and both sides are checked against fp64."""
    from mxdetection_amd.ops import group_norm as GN
    edge0 = 8 * (1024 // (Cc // 8))
    assert GN.workspace_bytes((2, edge0, Cc), G, False) == 0 < GN.workspace_bytes((2, edge0 + 1, Cc), G, False)
    edge = 8 * (1024 // (Cc // 8))
    _check(2, edge, Cc, G, True, seed=3, route=RES)
    _check(2, edge + 1, Cc, G, True, seed=3, route=TIL)


@pytest.mark.parametrize("N,HW,Cc,G", [(64, 49, 256, 32), (2, 2100, 256, 32)])
def test_accumulate_adds_onto_existing_gradients(N, HW, Cc, G):
    dev, ref = _inputs(N, HW, Cc, G, 4)
    g = torch.Generator().manual_seed(5)
    old = (torch.randn((Cc,), generator=g).cuda() * 10, torch.randn((Cc,), generator=g).cuda() * 10)
    y, mean, rstd, dx, dg, db = _run(dev, G, True, accumulate=old)
    ymask = y.float().cpu().numpy() > 0
    _, rdg, rdb = gn_ref_backward(ref["x"], ref["dy"], ref["gamma"], ref["beta"], G, EPS, True, y_mask=ymask)
    _, rmean, rrstd = gn_ref(ref["x"], ref["gamma"], ref["beta"], G, EPS)
    gm = ref["dy"] * ymask
    xh = ((ref["x"].reshape(N, HW, G, Cc // G) - rmean[:, None, :, None]) * rrstd[:, None, :, None]).reshape(N, HW, Cc)
    o0, o1 = old[0].double().cpu().numpy(), old[1].double().cpu().numpy()
    _dgamma_bound(dg.cpu().numpy(), rdg + o0, N * HW + 1, np.abs(gm * xh).sum(axis=(0, 1)) + np.abs(o0),
                  _stat_terms(rmean, rrstd, gm, xh, G), "acc dgamma")
    _sum_bound(db.cpu().numpy(), rdb + o1, N * HW + 1, np.abs(gm).sum(axis=(0, 1)) + np.abs(o1), "acc dbeta")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


@pytest.mark.parametrize("N,HW,Cc,G", [(96, 49, 256, 32), (24, 196, 256, 32), (2, 2100, 256, 32)])
def test_two_runs_agree_bit_for_bit(N, HW, Cc, G):
    dev, _ = _inputs(N, HW, Cc, G, 6)
    a = _run(dev, G, True)
    b = _run(dev, G, True)
    for u, v, name in zip(a, b, ("y", "mean", "rstd", "dx", "dgamma", "dbeta")):
        assert np.array_equal(_bits(u), _bits(v)), name


@pytest.mark.parametrize("N,HW,Cc,G", [(40, 49, 256, 32), (12, 196, 256, 32)])
def test_resident_rows_do_not_depend_on_the_batch(N, HW, Cc, G):
    from mxdetection_amd.ops import group_norm as GN
    assert GN.route((N, HW, Cc), G) == RES
    dev, _ = _inputs(N, HW, Cc, G, 7)
    full = _run(dev, G, True)
    lo, hi = 3, N - 5
    sub = {k: (v[lo:hi].contiguous() if k in ("x", "dy") else v) for k, v in dev.items()}
    part = _run(sub, G, True)
    for i, name in enumerate(("y", "mean", "rstd", "dx")):
        assert np.array_equal(_bits(full[i][lo:hi].contiguous()), _bits(part[i])), name


@pytest.mark.parametrize("N,HW,Cc,G,with_y", [(16, 49, 256, 32, True), (16, 49, 256, 32, False), (2, 2100, 256, 32, True),
                                              (2, 2100, 256, 32, False)])
def test_backward_ignores_dy_where_relu_is_off(N, HW, Cc, G, with_y):
    dev, _ = _inputs(N, HW, Cc, G, 8)
    a = _run(dev, G, True, with_y=with_y)
    off = a[0] == 0
    assert 0.2 < float(off.float().mean()) < 0.9
    dev2 = dict(dev)
    dev2["dy"] = torch.where(off, dev["dy"] * -3.0 + 1.0, dev["dy"])
    b = _run(dev2, G, True, with_y=with_y)
    for i, name in ((3, "dx"), (4, "dgamma"), (5, "dbeta")):
        assert np.array_equal(_bits(a[i]), _bits(b[i])), name


def test_recomputed_mask_equals_the_stored_one():
    """y = NULL: the mask is recomputed from x, gamma, beta with the forward's own expression -- same bits as with y."""
    for shape in ((32, 49, 256, 32), (2, 2100, 256, 32)):
        dev, _ = _inputs(*shape, 9)
        a = _run(dev, shape[3], True, with_y=True)
        b = _run(dev, shape[3], True, with_y=False)
        for i, name in ((3, "dx"), (4, "dgamma"), (5, "dbeta")):
            assert np.array_equal(_bits(a[i]), _bits(b[i])), name
