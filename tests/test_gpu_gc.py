"""The global context entries on the GPU through the C-ABI against tests/_gc_ref.py (fp64) on bf16- / fp32-rounded inputs.

The map kernels' chunk is 64 positions (kGcChunk in csrc/context.hip, _lib.GC_CHUNK): a workgroup of four waves owns 64
consecutive positions of one image, wave w the positions w, w + 4, ... of them. HW covers 1, 2 (fewer positions than waves),
3, chunk - 1, chunk, chunk + 1 and 3 chunks + 9 (four workgroups per image, a tail); N is 1 or 3; (C, P) covers one 16-byte
vector per row (8, 8), a row that is no multiple of anything (72, 8), the three vector counts per lane (512: 1, 1024: 2,
2048: 4) and both ends of the inner width (8, 512). Not the full product: every HW at two small widths, every width at two HW.

Each entry is teacher-forced: its stored inputs are the reference's (rounded to the format the entry reads), so one entry's
error does not hide in the next one's input. What the workspace carries between two entries (the chunk partials) cannot be
forced: transform_fwd is checked behind the device's pool_fwd, transform_bwd behind the device's reduce_bwd; D counts the
whole chain (tests/_gc_ref.py _D).

Tolerances, from the reference alone.
  y, d_t (bf16)   |got - exact| <= 2 E + 2^-9 max |exact|, E = max |emulated - exact| (the one rounding of the output).
  fp32 outputs    |got - exact| <= (D + 4) 2^-23 A per element, nothing added: ref.bounds_forward / ref.bounds_backward.
                  Checked: logits, lse, ctx, h, mean, rstd, add; d_add, d_ctx, d_wk and the six parameter gradients.
A bound that is no small fraction of the output would check nothing, so every case also asserts that each fp32 bound's largest
element is at most ref.fraction_limit of max |exact|: 2^-8, and 2^-3 for the five outputs two or three sums deep
(mean, rstd, the fc1 gradients, d_ctx; tests/_gc_ref.py gives the reasoning); for mean the size is max |h|, the values it averages.
Exempt, by construction and not by result: d_wk when the softmax has one position (HW = 1: dl = 0 identically) or is made
one-hot on purpose (the adversarial cases): there d_wk is the rounding-size remainder of e - S and has no size to compare a
bound with.
Every case prints the bound and the achieved error (DESIGN.md 5u holds the table). Outputs are pre-filled with NaN; bf16 outputs
sit between sentinels.
"""
import ctypes
import functools

import pytest

import _gc_ref as ref

pytestmark = pytest.mark.gpu

CHUNK = 64
HWS = (1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 9)
WIDTHS = ((8, 8), (72, 8), (512, 32), (512, 128), (1024, 64), (2048, 128), (2048, 512))
CASES = [(N, HW, C, P) for HW in HWS for (N, (C, P)) in ((1, (8, 8)), (3, (72, 8)))] + \
        [(N, HW, C, P) for (C, P) in WIDTHS[2:] for (N, HW) in ((3, CHUNK + 1), (1, 3 * CHUNK + 9))]
SENTINEL = 7.0
GUARD = 64
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _reference(N, HW, C, P, kind="plain"):
    """Inputs, exact and emulated results and the fp32 bounds of one case: computed once, never modified."""
    seed = ((N * 1009 + HW) * 31 + C) * 7 + P
    if kind == "wide":          # logits spanning more than +-100: exp overflows fp32 unless the maximum is subtracted
        t, sc, ds, p = ref.random_case(N, HW, C, P, seed, wk_scale=60.0)
    elif kind == "peak":        # one position holds nearly all the weight
        t, sc, ds, p = ref.random_case(N, HW, C, P, seed, peak=(N - 1, HW // 2, 40.0))
    else:
        t, sc, ds, p = ref.random_case(N, HW, C, P, seed)
    f = ref.forward(t, sc, p)
    r = ref.backward(t, p, f, ds)
    E = dict(y=float((ref.round_bf16(f["y"]) - f["y"]).abs().max()), d_t=float((ref.round_bf16(r["d_t"]) - r["d_t"]).abs().max()))
    return dict(t=t, sc=sc, ds=ds, p=p, f=f, r=r, E=E, bf=ref.bounds_forward(t, p, f), bb=ref.bounds_backward(t, p, f, r, ds))


def _guarded(shape, fill):
    """A contiguous bf16 view of `shape` inside a larger allocation full of sentinels; (view, check)."""
    import torch
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.bfloat16, device="cuda")
    view = whole[GUARD:GUARD + n].view(shape)
    view.fill_(fill)

    def intact():
        return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())
    return view, intact


def _dev(x, dtype):
    return x.to(dtype).cuda().contiguous()


def _run(c):
    """All six entries, each teacher-forced; returns cpu float64 outputs and the guards' state."""
    import torch
    from mxdetection_amd.ops.context import ContextPlan
    bf, f32 = torch.bfloat16, torch.float32
    t, sc, ds, p, f, r = c["t"], c["sc"], c["ds"], c["p"], c["f"], c["r"]
    N, HW, C = t.shape
    P = p["fc1.weight"].shape[0]
    plan = ContextPlan(N, HW, C, P)
    for b in (plan.logits, plan.lse, plan.ctx, plan.h, plan.mean, plan.rstd, plan.add, plan.d_add, plan.d_ctx):
        b.fill_(NAN)
    plan.workspace.view(torch.float32).fill_(NAN)
    tg, scg, dsg = _dev(t, bf), _dev(sc, bf), _dev(ds, bf)
    w = {k: _dev(v, bf if k in ("mask.weight", "fc1.weight", "fc2.weight") else f32) for k, v in p.items()}
    out = {}
    # forward: pool -> transform (chained through the workspace), then fuse on the reference's add
    plan.pool_forward(tg, w["mask.weight"])
    plan.transform_forward(w["fc1.weight"], w["fc1.bias"], w["ln.gamma"], w["ln.beta"], w["fc2.weight"], w["fc2.bias"])
    for k in ("logits", "lse", "ctx", "h", "mean", "rstd", "add"):
        out[k] = getattr(plan, k).double().cpu()
    y, y_ok = _guarded((N, HW, C), NAN)
    bits = torch.full((N * HW * C // 8 + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.fuse_forward(tg, scg, y, bits[GUARD:GUARD + N * HW * C // 8], add=_dev(f["add"], f32))
    out["y"], out["bits"] = y.double().cpu(), bits[GUARD:GUARD + N * HW * C // 8].cpu()
    bits_ok = bool((bits[:GUARD] == 0xA5).all()) and bool((bits[GUARD + N * HW * C // 8:] == 0xA5).all())
    # backward: reduce -> transform on the reference's ctx, h, mean, rstd; pool on the reference's logits, lse, d_ctx
    for k in ("ctx", "h", "mean", "rstd", "logits", "lse"):
        getattr(plan, k).copy_(_dev(f[k], f32))
    grads = {k: torch.full(tuple(v.shape), NAN, dtype=f32, device="cuda") for k, v in p.items()}
    plan.reduce_backward(dsg)
    plan.transform_backward(w["fc1.weight"], w["ln.gamma"], w["ln.beta"], w["fc2.weight"], grads["fc1.weight"], grads["fc1.bias"],
                            grads["ln.gamma"], grads["ln.beta"], grads["fc2.weight"], grads["fc2.bias"])
    out["d_add"], out["d_ctx"] = plan.d_add.double().cpu(), plan.d_ctx.double().cpu()
    plan.d_ctx.copy_(_dev(r["d_ctx"], f32))
    d_t, dt_ok = _guarded((N, HW, C), NAN)
    plan.pool_backward(tg, w["mask.weight"], dsg, d_t, grads["mask.weight"])
    torch.cuda.synchronize()
    out["d_t"] = d_t.double().cpu()
    out.update({k: v.double().cpu() for k, v in grads.items()})
    return out, (y_ok(), bits_ok, dt_ok())


def _check(tag, c, out, guards, one_hot=False):
    import torch
    assert guards == (True, True, True), "%s: a sentinel around y / its bit mask / d_t was overwritten %s" % (tag, guards)
    f, r = c["f"], c["r"]
    bad = []
    for name, exact, bound in [(k, f[k], c["bf"][k]) for k in ("logits", "lse", "ctx", "h", "mean", "rstd", "add")] + \
                              [(k, r[k], c["bb"][k]) for k in ("d_add", "d_ctx")] + \
                              [(k, r["grads"][k], c["bb"][k]) for k in ref.PARAMS]:
        got = out[name]
        assert got.shape == exact.shape, (name, got.shape, exact.shape)
        scale = float((f["h"] if name == "mean" else exact).abs().max())
        if not (name == "mask.weight" and (one_hot or f["logits"].shape[1] == 1)):
            assert float(bound.max()) <= ref.fraction_limit(name) * scale, "%s: the bound of %s, %.3e, is no small fraction of %.3e" % (
                tag, name, float(bound.max()), scale)
        finite = bool(torch.isfinite(got).all())
        err = (got - exact).abs() if finite else torch.full_like(exact, float("inf"))
        over = float((err - bound).max())
        print("%s %-11s bound %.3e  achieved %.3e  (max |exact| %.3e)" % (tag, name, float(bound.max()), float(err.max()),
                                                                       float(exact.abs().max())))
        if not finite or over > 0:
            bad.append((name, float(err.max()), float(bound.max())))
    for name, exact in (("y", f["y"]), ("d_t", r["d_t"])):
        got = out[name]
        tol = 2.0 * c["E"][name] + 2.0 ** -9 * float(exact.abs().max())
        err = float((got - exact).abs().max()) if bool(torch.isfinite(got).all()) else float("inf")
        print("%s %-11s E %.3e  tolerance %.3e  achieved %.3e" % (tag, name, c["E"][name], tol, err))
        if not err <= tol:
            bad.append((name, err, tol))
    assert not bad, "%s: %s" % (tag, bad)
    # the bit mask is that of the stored y, in the convolution kernels' layout: byte [pixel][c / 8], bit k = channel 8 i + k
    N, HW, C = f["y"].shape
    want = ((out["y"] > 0).reshape(N * HW * C // 8, 8).to(torch.int32) * (1 << torch.arange(8, dtype=torch.int32))).sum(dim=1)
    assert torch.equal(out["bits"].to(torch.int32), want), "%s: the bit mask is not y > 0" % tag


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-HW%d-C%d-P%d" % c)
def test_parity_with_fp64(hip, case):
    c = _reference(*case)
    out, guards = _run(c)
    _check("N=%d HW=%d C=%d P=%d" % case, c, out, guards)


@pytest.mark.parametrize("kind,case", [("wide", (3, 3 * CHUNK + 9, 72, 8)), ("wide", (1, CHUNK + 1, 512, 32)),
                                       ("peak", (3, 3 * CHUNK + 9, 72, 8)), ("peak", (1, CHUNK + 1, 2048, 128))])
def test_adversarial_logits(hip, kind, case):
    """wide: wk scaled so that the logits span more than +-100 (asserted on the reference): without the maximum subtracted,
    exp overflows fp32. peak: one position's logit stands 40 above the rest: att is 1 there up to e^-30."""
    import torch
    c = _reference(*case, kind=kind)
    lg = c["f"]["logits"]
    if kind == "wide":
        assert float(lg.max()) > 100 and float(lg.min()) < -100
    else:
        assert float(c["f"]["att"].max()) > 1 - 1e-9
    out, guards = _run(c)
    assert all(bool(torch.isfinite(v.double()).all()) for k, v in out.items() if k != "bits")
    _check("%s N=%d HW=%d C=%d P=%d" % ((kind,) + case), c, out, guards, one_hot=True)


def test_repeatable(hip):
    """Every entry twice: every output bit for bit."""
    import torch
    for case in ((3, 3 * CHUNK + 9, 72, 8), (1, 3 * CHUNK + 9, 2048, 128)):
        c = _reference(*case)
        a, _ = _run(c)
        b, _ = _run(c)
        assert sorted(a) == sorted(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (case, k)


def test_accumulate_adds_to_the_gradients(hip):
    """accumulate = 1: the seven parameter gradients are added to what the buffers hold (one more fp32 addition)."""
    import torch
    from mxdetection_amd.ops.context import ContextPlan
    case = (3, CHUNK + 1, 72, 8)
    c = _reference(*case)
    base, _ = _run(c)
    bf, f32 = torch.bfloat16, torch.float32
    t, ds, p, f, r = c["t"], c["ds"], c["p"], c["f"], c["r"]
    plan = ContextPlan(*case)
    w = {k: _dev(v, bf if k in ("mask.weight", "fc1.weight", "fc2.weight") else f32) for k, v in p.items()}
    for k in ("ctx", "h", "mean", "rstd", "logits", "lse"):
        getattr(plan, k).copy_(_dev(f[k], f32))
    grads = {k: torch.full(tuple(v.shape), 0.5, dtype=f32, device="cuda") for k, v in p.items()}
    plan.reduce_backward(_dev(ds, bf))
    plan.transform_backward(w["fc1.weight"], w["ln.gamma"], w["ln.beta"], w["fc2.weight"], grads["fc1.weight"], grads["fc1.bias"],
                            grads["ln.gamma"], grads["ln.beta"], grads["fc2.weight"], grads["fc2.bias"], accumulate=True)
    plan.d_ctx.copy_(_dev(r["d_ctx"], f32))
    d_t = torch.empty(case[:3], dtype=bf, device="cuda")
    plan.pool_backward(_dev(t, bf), w["mask.weight"], _dev(ds, bf), d_t, grads["mask.weight"], accumulate=True)
    torch.cuda.synchronize()
    for k, g in grads.items():
        assert torch.equal(g.cpu(), (0.5 + base[k].float())), k


def test_refusals_leave_the_outputs_alone(hip):
    """Every host check returns its error before any launch."""
    import torch
    from mxdetection_amd import _lib
    from mxdetection_amd.ops import context
    lib = _lib.load()
    N, HW, C, P = 2, 70, 72, 8
    f32 = dict(dtype=torch.float32, device="cuda")
    t = torch.zeros((N, HW, C), dtype=torch.bfloat16, device="cuda")
    y = torch.full((N, HW, C), 3.0, dtype=torch.bfloat16, device="cuda")
    logits, add = torch.full((N, HW), 3.0, **f32), torch.full((N, C), 3.0, **f32)
    wk = torch.zeros((C,), dtype=torch.bfloat16, device="cuda")
    ws = torch.full((context.workspace_bytes(N, HW, C, P),), 3, dtype=torch.uint8, device="cuda")
    p, s = _lib.ptr, _lib.stream_ptr()
    for bad, rc_want, text in ((dict(C=76), -2, b"C 76"), (dict(P=12), -2, b"P 12"), (dict(HW=0), -2, b"HW 0"), (dict(N=0), -2, b"N 0"),
                               (dict(eps=-1.0), -1, b"eps")):
        d = context.make_desc(N, HW, C, P)
        for k, v in bad.items():
            setattr(d, k, v)
        for rc in (lib.mxdet_gc_pool_fwd(ctypes.byref(d), p(t), p(wk), p(logits), p(ws), ws.numel(), s),
                   lib.mxdet_gc_fuse_fwd(ctypes.byref(d), p(t), p(add), p(t), p(y), None, s)):
            assert rc == rc_want and text in lib.mxdet_last_error(), (bad, rc, lib.mxdet_last_error())
    d = context.make_desc(N, HW, C, P)
    assert lib.mxdet_gc_pool_fwd(ctypes.byref(d), p(t), p(wk), p(logits), p(ws), ws.numel() - 16, s) == -3
    assert lib.mxdet_gc_pool_fwd(ctypes.byref(d), p(t), None, p(logits), p(ws), ws.numel(), s) == -1
    assert lib.mxdet_gc_pool_fwd(ctypes.byref(d), p(t), p(wk), ctypes.c_void_p(logits.data_ptr() + 4), p(ws), ws.numel(), s) == -1
    assert lib.mxdet_gc_fuse_fwd(ctypes.byref(d), p(t), p(add), None, p(y), None, s) == -1
    assert lib.mxdet_gc_reduce_bwd(ctypes.byref(d), None, p(ws), ws.numel(), s) == -1
    torch.cuda.synchronize()
    assert bool((y == 3.0).all()) and bool((logits == 3.0).all()) and bool((ws == 3).all())
