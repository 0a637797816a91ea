"""The fused loss kernels (csrc/losses.hip, retina_loss.hip, mask_loss_kernel) on the case tables of tests/test_loss_cases_cpu.py.

For every case: gradients against the float64 autograd reference (after division by norm * loss_scale; ATOL_CE / ATOL_FOCAL
as derived in the CPU module, plus one bf16 step 2^-8 * |ref| for bf16 outputs), loss scalars within 3e-5 of the float64
sum (exactly 0 where nothing contributes), the bit-exact claims the project already makes (rpn / mask gradients and
smooth-L1 against the C oracle, retina vector form == scalar form, a second run == the first), and the written extents:
every output is an interior slice of a buffer filled with a sentinel, which must survive everywhere a kernel has no
business writing.
"""
import numpy as np
import pytest

import test_loss_cases_cpu as T

pytestmark = pytest.mark.gpu

SENT = -24576.0           # bf16-exact, far from every gradient of the tables
GUARD = 64                # elements on either side: keeps 16-byte alignment of the slice for bf16 and f32


def _t(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _np(t):
    return t.double().cpu().numpy()


class Guarded:
    """A tensor of `shape` that is the interior slice [GUARD + offset, ...) of a flat sentinel-filled buffer."""

    def __init__(self, shape, dtype, offset=0, init=None):
        import torch
        self.n = int(np.prod(shape))
        self.flat = torch.full((GUARD + offset + self.n + GUARD,), SENT, dtype=dtype, device="cuda")
        self.lo = GUARD + offset
        self.view = self.flat[self.lo:self.lo + self.n].view(*shape)
        if init is not None:
            self.view.copy_(init)

    def outside_intact(self):
        return bool((self.flat[:self.lo] == SENT).all()) and bool((self.flat[self.lo + self.n:] == SENT).all())


def _grad_ok(what, got, ref, unit, atol, bf16):
    """|got - ref| / unit <= atol (+ 2^-8 |ref| / unit for bf16 outputs); prints the figure first."""
    got, ref = np.asarray(got, np.float64) / unit, np.asarray(ref, np.float64) / unit
    err = np.abs(got - ref)
    bound = atol + (T.BF16_STEP * np.abs(ref) if bf16 else 0.0)
    worst = float(np.max(err - bound)) if err.size else 0.0
    print("%s: max |got-ref|/unit = %.3e, max excess over the bound = %.3e" % (what, float(err.max()) if err.size else 0.0, worst))
    return bool(np.all(err <= bound))


def _loss_ok(what, got, ref, terms):
    """rtol 3e-5 of the float64 sum of `terms` terms (+ 2^-126 per term: below that an fp32 term cannot be held); 0 stays 0."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    print("%s: got %s ref %s" % (what, got, ref))
    return all((g == 0.0) if r == 0.0 else abs(g - r) <= T.LOSS_RTOL * abs(r) + terms * T.F32_MIN_NORMAL for g, r in zip(got, ref))


def _lib():
    from mxdetection_amd import _lib
    return _lib, _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.FOCAL_CASES, ids=T.ids(T.FOCAL_CASES))
def test_focal(hip, c):
    import torch
    from mxdetection_amd.core import loss as L
    B, lib = _lib()
    d = T.focal_data(c)
    ref = d["ref"]
    dt = torch.bfloat16 if c["bf"] else torch.float32
    x, lab = _t(d["logits"], dt), _t(d["labels"])
    ws = L.loss_workspace(c["n"], "cuda")
    runs = []
    for _ in range(2):
        g, loss = Guarded((c["n"], c["C"]), dt), Guarded((1,), torch.float32)
        B.check(lib.mxdet_focal_loss(B.ptr(x), int(c["bf"]), B.ptr(lab), c["n"], c["C"], c["a"], c["g"], float(c["gs"]),
                                     B.ptr(loss.view), B.ptr(g.view), B.ptr(ws), ws.numel(), B.stream_ptr()), "focal_loss")
        torch.cuda.synchronize()
        assert g.outside_intact() and loss.outside_intact()
        runs.append((g, loss))
    (g, loss), (g2, loss2) = runs
    assert torch.equal(loss.view, loss2.view) and torch.equal(g.view, g2.view)
    assert _loss_ok("focal loss", _np(loss.view), ref["loss"], c["n"] * c["C"])
    assert _grad_ok("focal grad", _np(g.view), ref["grad"], ref["unit"], T.ATOL_FOCAL, c["bf"])
    if c["mix"] == "ignore":
        assert not g.view.any()


# ---------------------------------------------------------------------------------------------------------------------
def _run_retina(c, d, off_cls, off_reg):
    """One launch with the (cls, grad_cls) / (reg, grad_reg) views `off_*` BYTES off their aligned places."""
    import torch
    from mxdetection_amd.core import loss as L
    B, lib = _lib()
    N, H, W, A, Cc, ldc, ldr = c["shape"]
    bf = torch.bfloat16
    ec, er = off_cls // 2, off_reg // 2
    cls = Guarded((N, H, W, ldc), bf, ec, _t(d["cls"], bf))
    reg = Guarded((N, H, W, ldr), bf, er, _t(d["reg"], bf))
    gc, gr = Guarded((N, H, W, ldc), bf, ec), Guarded((N, H, W, ldr), bf, er)
    for t, off, al in ((cls, off_cls, 16), (gc, off_cls, 16), (reg, off_reg, 8), (gr, off_reg, 8)):
        assert t.view.data_ptr() % al == off % al
    nparts = L.retina_loss_num_partials(N, H, W, A)
    part, out = Guarded((2 * nparts,), torch.float32), Guarded((2,), torch.float32)
    num_fg = torch.tensor([d["num_fg"]], dtype=torch.int32, device="cuda")
    lab, tgt = _t(d["labels"]), _t(d["targets"])
    B.check(lib.mxdet_retina_loss_level(B.ptr(cls.view), B.ptr(reg.view), N, H, W, A, Cc, ldc, ldr, B.ptr(lab),
                                        B.ptr(tgt), d["A_total"], d["off"], T.RETINA_ALPHA, c["g"], T.RETINA_SIGMA,
                                        B.ptr(num_fg), float(c["ls"]), B.ptr(gc.view), B.ptr(gr.view), B.ptr(part.view),
                                        B.stream_ptr()), "retina_loss_level")
    L.loss_finalize(part.view, nparts, 2, out.view)
    torch.cuda.synchronize()
    for t in (cls, reg, gc, gr, part, out):
        assert t.outside_intact()
    assert torch.equal(cls.view, _t(d["cls"], bf)) and torch.equal(reg.view, _t(d["reg"], bf))
    # columns beyond the real widths are left untouched (include/mxdet.h)
    assert bool((gc.view[..., A * Cc:] == SENT).all()) and bool((gr.view[..., 4 * A:] == SENT).all())
    assert not bool((part.view == SENT).any())
    return gc.view[..., :A * Cc], gr.view[..., :4 * A], out.view


@pytest.mark.parametrize("c", T.RETINA_CASES, ids=T.ids(T.RETINA_CASES))
def test_retina_level(hip, c):
    import torch
    d = T.retina_data(c)
    ref = d["ref"]
    N, H, W, A, Cc, ldc, ldr = c["shape"]
    assert T.retina_route(c)[0] == (c["form"] == "vec")
    gc, gr, out = _run_retina(c, d, c["off_cls"], c["off_reg"])
    gc2, gr2, out2 = _run_retina(c, d, c["off_cls"], c["off_reg"])
    assert torch.equal(out, out2) and torch.equal(gc, gc2) and torch.equal(gr, gr2)
    assert _loss_ok("retina loss", _np(out), ref["loss"], N * H * W * A * Cc)
    assert _grad_ok("retina grad_cls", _np(gc), ref["grad_cls"][..., :A * Cc], ref["unit"], T.ATOL_FOCAL, True)
    assert _grad_ok("retina grad_reg", _np(gr), ref["grad_reg"][..., :4 * A], ref["unit"], T.ATOL_CE, True)
    if c["off_cls"] or c["off_reg"]:
        # the same data through aligned views runs the vector form: bit-identical gradients
        assert T.retina_route(dict(c, off_cls=0, off_reg=0))[0]
        vc, vr, vout = _run_retina(c, d, 0, 0)
        assert np.array_equal(_bits(vc), _bits(gc)) and np.array_equal(_bits(vr), _bits(gr))
        assert _loss_ok("retina loss (vector form)", _np(vout), ref["loss"], N * H * W * A * Cc)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.RPN_CASES, ids=T.ids(T.RPN_CASES))
def test_rpn_level(hip, oracle, c):
    import torch
    from mxdetection_amd.core import loss as L
    d = T.rpn_data(c)
    ref = d["ref"]
    N, H, W, A, Cp = c["shape"]
    head, lab, tgt = _t(d["head"], torch.bfloat16), _t(d["labels"]), _t(d["targets"])
    nparts = L.rpn_loss_num_partials(N, H, W)
    assert nparts == (N * H * W + 255) // 256
    runs = []
    for _ in range(2):
        g = Guarded((N, H, W, Cp), torch.bfloat16)
        part, out = Guarded((2 * nparts,), torch.float32), Guarded((2,), torch.float32)
        L.rpn_loss_level(head, A, lab, tgt, d["off"], T.RPN_SIGMA, T.RPN_NORM, float(c["ls"]), g.view, part.view)
        L.loss_finalize(part.view, nparts, 2, out.view)
        torch.cuda.synchronize()
        assert g.outside_intact() and part.outside_intact() and out.outside_intact()
        runs.append((g, out))
    (g, out), (g2, out2) = runs
    assert torch.equal(out.view, out2.view) and torch.equal(g.view, g2.view)
    assert not bool((g.view == SENT).any())                              # the whole row is written ...
    assert not _bits(g.view)[..., 5 * A:].any()                          # ... channels [5A, Cpad) with zeros
    assert _loss_ok("rpn loss", _np(out.view), ref["loss"], N * H * W * A * 4)
    assert _grad_ok("rpn grad", _np(g.view), ref["grad"], ref["unit"], T.ATOL_CE, True)
    _, w_grad = oracle.rpn_loss_level(d["head"], A, d["labels"], d["targets"], d["off"], T.RPN_SIGMA, T.RPN_NORM, float(c["ls"]))
    assert np.array_equal(_bits(g.view), oracle.f32_to_bf16_bits(w_grad))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.RCNN_CASES, ids=T.ids(T.RCNN_CASES))
def test_rcnn(hip, c):
    import torch
    from mxdetection_amd.core import loss as L
    d = T.rcnn_data(c)
    ref = d["ref"]
    nc, R, rd = c["nc"], c["R"], c["reg_dim"]
    dt = torch.bfloat16 if c["bf"] else torch.float32
    lab, tgt, wgt = _t(d["labels"]), _t(d["tgt"]), _t(d["wgt"])
    ws = L.loss_workspace(R, "cuda")
    runs = []
    for _ in range(2):
        out = Guarded((2,), torch.float32)
        if c["fused"]:
            ld = d["ld"]
            fused = np.full((R, ld), 7.0, np.float32)
            fused[:, :nc], fused[:, nc:nc + rd] = d["cls"], d["reg"]
            x = _t(fused, dt)
            g = Guarded((R, ld), dt)
            L.rcnn_loss(x, x[:, nc:], lab, tgt, wgt, nc, rd, ld, ld, T.RCNN_SIGMA, d["norm"], float(c["ls"]), g.view, g.view[:, nc:],
                        out.view, ws)
            torch.cuda.synchronize()
            assert g.outside_intact() and out.outside_intact()
            assert bool((g.view[:, nc + rd:] == SENT).all())            # columns beyond the real widths: untouched
            gc, gr = g.view[:, :nc], g.view[:, nc:nc + rd]
        else:
            gcg, grg = Guarded((R, nc), dt), Guarded((R, rd), dt)
            L.rcnn_loss(_t(d["cls"], dt), _t(d["reg"], dt), lab, tgt, wgt, nc, rd, nc, rd, T.RCNN_SIGMA, d["norm"], float(c["ls"]),
                        gcg.view, grg.view, out.view, ws)
            torch.cuda.synchronize()
            assert gcg.outside_intact() and grg.outside_intact() and out.outside_intact()
            gc, gr = gcg.view, grg.view
        assert not bool((gc == SENT).any()) and not bool((gr == SENT).any())
        runs.append((gc.clone(), gr.clone(), out.view.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    gc, gr, out = runs[0]
    assert _loss_ok("rcnn loss", _np(out), ref["loss"], R * max(nc, rd))
    assert _grad_ok("rcnn grad_cls", _np(gc), ref["grad_cls"], ref["unit"], T.ATOL_CE, c["bf"])
    assert _grad_ok("rcnn grad_reg", _np(gr), ref["grad_reg"], ref["unit"], T.ATOL_CE, c["bf"])


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.MASK_CASES, ids=T.ids(T.MASK_CASES))
def test_mask(hip, oracle, c):
    import torch
    from mxdetection_amd.core import mask as M_
    d = T.mask_data(c)
    ref = d["ref"]
    R, S, Cp = c["shape"]
    logits, cls, tg = _t(d["logits"], torch.bfloat16), _t(d["cls"]), _t(d["targets"])
    ws = M_.mask_loss_workspace(R, S, "cuda")
    runs = []
    for _ in range(2):
        g, loss = Guarded((R, S, S, Cp), torch.bfloat16), Guarded((1,), torch.float32)
        M_.mask_loss(logits, cls, tg, loss.view, g.view, ws, float(c["ls"]))
        torch.cuda.synchronize()
        assert g.outside_intact() and loss.outside_intact()
        runs.append((g, loss))
    (g, loss), (g2, loss2) = runs
    assert torch.equal(loss.view, loss2.view) and torch.equal(g.view, g2.view)
    assert not bool((g.view == SENT).any())                              # the full row is written
    assert _loss_ok("mask loss", _np(loss.view), ref["loss"], R * S * S)
    assert _grad_ok("mask grad", _np(g.view), ref["grad"], ref["unit"], T.ATOL_CE, True)
    _, w_grad = oracle.mask_loss(d["logits"], d["cls"], d["targets"], float(c["ls"]))
    assert np.array_equal(_bits(g.view), oracle.f32_to_bf16_bits(w_grad))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.SL1_CASES, ids=T.ids(T.SL1_CASES))
def test_smooth_l1(hip, oracle, c):
    import torch
    B, lib = _lib()
    d = T.sl1_data(c)
    ref = d["ref"]
    n, f32 = c["n"], torch.float32
    p, t = _t(d["p"]), _t(d["t"])
    w = None if d["w"] is None else _t(d["w"])
    go = None if d["go"] is None else _t(d["go"])
    w_out, w_g = oracle.smooth_l1(d["p"], d["t"], d["w"], c["sigma"])
    if not c["go"] and not c["acc"]:                                     # forward has neither argument: once per (n, sigma, w)
        out = Guarded((n,), f32)
        B.check(lib.mxdet_smooth_l1_fwd(B.ptr(p), B.ptr(t), B.ptr(w), n, c["sigma"], B.ptr(out.view), B.stream_ptr()), "smooth_l1_fwd")
        torch.cuda.synchronize()
        assert out.outside_intact()
        assert np.array_equal(out.view.cpu().numpy(), w_out)
        assert _grad_ok("smooth_l1 out", _np(out.view), ref["out"], 1.0, T.ATOL_CE, False)
    gp = Guarded((n,), f32, init=_t(d["prefill"]) if c["acc"] else None)
    B.check(lib.mxdet_smooth_l1_bwd(B.ptr(p), B.ptr(t), B.ptr(w), B.ptr(go), n, c["sigma"], int(c["acc"]), B.ptr(gp.view),
                                    B.stream_ptr()), "smooth_l1_bwd")
    torch.cuda.synchronize()
    assert gp.outside_intact()
    want, want64 = w_g, ref["grad"]
    if c["go"]:
        want = want * d["go"]
    if c["acc"]:
        want, want64 = d["prefill"] + want, d["prefill"].astype(np.float64) + want64
    assert want.dtype == np.float32
    assert np.array_equal(gp.view.cpu().numpy(), want)
    assert _grad_ok("smooth_l1 grad", _np(gp.view), want64, 1.0, T.ATOL_CE, False)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.FINALIZE_CASES, ids=T.ids(T.FINALIZE_CASES))
def test_loss_finalize(hip, c):
    import torch
    from mxdetection_amd.core import loss as L
    d = T.finalize_data(c)
    part = _t(d["partial"])
    outs = []
    for _ in range(2):
        out = Guarded((c["ncomp"],), torch.float32)
        L.loss_finalize(part, c["count"], c["ncomp"], out.view)
        torch.cuda.synchronize()
        assert out.outside_intact()
        outs.append(out.view.clone())
    assert torch.equal(outs[0], outs[1])
    assert _loss_ok("loss_finalize", _np(outs[0]), d["ref"], c["count"])
    if c["count"] == 0:
        assert not outs[0].any()
