"""Deformable convolution kernels (csrc/deform_conv.hip) at the shapes where their shape-dependent branches leave the
simplest arm: multi-block and multi-pass scans, lists at and beyond the 64-entry wave sort, col2im_coord segment widths
1 and 2, pad / stride / thin maps, samples exactly on the window edges, and the ResNet-50 layer shapes. Inputs and the
CPU proof that each case reaches its branch: tests/test_deform_shapes_cpu.py. Reference and tolerance: the fp64
deform_conv_ref and _close of tests/test_gpu_deform_conv.py (|got - ref| <= 2^-7 |ref| + 2^-7 rms(ref)); dx and doff
against the reference's autograd fed the same bf16 column gradient the kernels read.
"""
import numpy as np
import pytest

import test_deform_shapes_cpu as S
from test_gpu_deform_conv import _bf16, _close, _gpu_layer, deform_conv_ref

pytestmark = pytest.mark.gpu


def _inputs(c, off, positive=False):
    """bf16-exact numpy x, dcol for case c (and the given offsets)."""
    rng = np.random.default_rng(c["seed"] + 7)
    draw = rng.random if positive else rng.standard_normal
    x = _bf16(draw((c["N"], c["H"], c["W"], c["C"])))
    dcol = _bf16(draw((c["N"], c["Ho"], c["Wo"], 9 * c["C"])))
    assert off.shape == (c["N"], c["Ho"], c["Wo"], c["Coff"])
    return x, dcol


def _cuda(a):
    import torch
    return torch.from_numpy(a).cuda().to(torch.bfloat16)


def _gpu(c, x, off, dcol, what=("col", "dx", "doff")):
    import torch
    from mxdetection_amd.ops import deform_conv as dc
    geo = (c["stride"], c["pad"], c["G"], c["mod"])
    xg, og, dg = _cuda(x), _cuda(off), _cuda(dcol)
    out = {}
    if "col" in what:
        out["col"] = dc.im2col(xg, og, *geo)
    if "dx" in what:
        out["dx"] = dc.col2im(og, dg, xg.shape, *geo)
    if "doff" in what:
        out["doff"] = dc.col2im_coord(xg, og, dg, *geo)
    torch.cuda.synchronize()
    return {k: v.float().cpu().numpy() for k, v in out.items()}


def _ref(c, x, off, dcol):
    import torch
    xr, offr = (torch.from_numpy(a).double().requires_grad_() for a in (x, off))
    w = torch.zeros((1, 3, 3, c["C"]), dtype=torch.float64)
    _, colr = deform_conv_ref(xr, offr, w, c["stride"], c["pad"], c["G"], c["mod"])
    (colr * torch.from_numpy(dcol).double()).sum().backward()
    return dict(col=colr.detach().numpy(), dx=xr.grad.numpy(), doff=offr.grad.numpy())


def _check(c, got, ref, tag):
    G = c["G"]
    nreal = (27 if c["mod"] else 18) * G
    if "col" in got:
        _close(got["col"], ref["col"], tag + " col")
    if "dx" in got:
        _close(got["dx"], ref["dx"], tag + " dx")
    if "doff" in got:
        _close(got["doff"][..., :18 * G], ref["doff"][..., :18 * G], tag + " d offsets")
        if c["mod"]:
            _close(got["doff"][..., 18 * G:nreal], ref["doff"][..., 18 * G:nreal], tag + " d mask logits")
        assert not got["doff"][..., nreal:].any(), tag + ": padding channels of doff must be zero"


def _against_reference(c, off, tag, what=("col", "dx", "doff")):
    x, dcol = _inputs(c, off)
    got = _gpu(c, x, off, dcol, what)
    _check(c, got, _ref(c, x, off, dcol), tag)
    return got


@pytest.mark.parametrize("name", sorted(S.SCAN_CASES))
def test_scan_sizes_match_reference(hip, name):
    """A wrong block offset or carry of the three-kernel scan misplaces every list behind it: dx is plainly wrong."""
    c, _ = S.SCAN_CASES[name]
    _against_reference(c, S.dcn_random_offsets(c), name)


@pytest.mark.parametrize("name", sorted(S.LONG_CASES))
def test_long_lists_match_reference_and_are_bit_reproducible(hip, name):
    """Lists of exactly 63, 64, 65 and a few hundred entries: dx against the reference, and bit-identical over two
    launches, one into a dirty buffer (entries arrive in atomic order; only a correct sort hides that)."""
    import torch
    from mxdetection_amd.ops import deform_conv as dc
    c, targets = S.LONG_CASES[name]
    off = S.dcn_long_list_offsets(c, targets)
    x, dcol = _inputs(c, off)
    got = _gpu(c, x, off, dcol, ("dx",))
    ref = _ref(c, x, off, dcol)
    _close(got["dx"], ref["dx"], name + " dx")
    Cg = c["C"] // c["G"]
    for g, (count, ty, tx) in enumerate(targets):       # the long lists on their own (the rms of the whole map is larger)
        _close(got["dx"][1, ty:ty + 2, tx:tx + 2, g * Cg:(g + 1) * Cg],
               ref["dx"][1, ty:ty + 2, tx:tx + 2, g * Cg:(g + 1) * Cg], "%s dx of the %d-entry lists" % (name, count))
    og, dg = _cuda(off), _cuda(dcol)
    runs = []
    for fill in (0.0, float("nan")):
        dx = torch.full(x.shape, fill, dtype=torch.bfloat16, device="cuda")
        dc.col2im(og, dg, x.shape, c["stride"], c["pad"], c["G"], c["mod"], out=dx)
        runs.append(dx.view(torch.int16).cpu())
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1]), "dx differs between launches"
    assert np.array_equal(runs[0].view(torch.bfloat16).float().numpy(), got["dx"]), "dx differs from the first launch"


@pytest.mark.parametrize("name", ["len65_v1", "len300_v1"])
def test_long_lists_are_summed_in_key_order(hip, name):
    """dx of the long lists equals, bit for bit, the fp32 sum in ascending (output pixel, tap) order of a column
    gradient whose sum depends on the order (a CPU restatement of the promise, not another run of the kernel): a list
    left in atomic arrival order fails whether or not that order changes from launch to launch."""
    c, targets = S.LONG_CASES[name]
    off = S.dcn_long_list_offsets(c, targets)
    x, _ = _inputs(c, off)
    dcol = S.dcn_order_sensitive_dcol(c, targets)
    got = _gpu(c, x, off, dcol, ("dx",))["dx"]
    want = S.dcn_key_order_sum(c, targets, dcol)
    Cg = c["C"] // c["G"]
    for g, (count, ty, tx) in enumerate(targets):
        for y in (ty, ty + 1):
            for xx in (tx, tx + 1):
                assert np.array_equal(got[1, y, xx, g * Cg:(g + 1) * Cg], want[g]), \
                    "%d-entry list of pixel (%d, %d) is not summed in key order" % (count, y, xx)


@pytest.mark.parametrize("name", sorted(S.SEG_CASES))
def test_segment_widths_match_reference(hip, name):
    """col2im_coord with 1 and 2 lanes per (pixel, tap, group), single and strided channel loop, a partial last wave."""
    c, _, _ = S.SEG_CASES[name]
    _against_reference(c, S.dcn_random_offsets(c), name, ("doff", "col"))


@pytest.mark.parametrize("name", sorted(S.GEOM_CASES))
def test_geometry_matches_reference(hip, name):
    c = S.GEOM_CASES[name]
    _against_reference(c, S.dcn_random_offsets(c), name)


@pytest.mark.parametrize("name", sorted(S.INT_CASES))
def test_integer_offsets_copy_pixels_bit_for_bit(hip, name):
    """v1 with integer offsets: col is the shifted, zero-padded x bit for bit (expectation built by indexing alone), and
    doff is the reference's one-sided derivative (the floor is the position itself)."""
    import torch
    from mxdetection_amd.ops import deform_conv as dc
    c = S.INT_CASES[name]
    off = S.dcn_integer_offsets(c)
    x, dcol = _inputs(c, off)
    col = dc.im2col(_cuda(x), _cuda(off), c["stride"], c["pad"], c["G"], False)
    torch.cuda.synchronize()
    bits = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy()
    py, px = S.dcn_positions(c, off)                       # [N,Ho,Wo,G,9]
    inside = (py >= 0) & (py < c["H"]) & (px >= 0) & (px < c["W"])
    yi = np.where(inside, py, 0).astype(np.int64)
    xi = np.where(inside, px, 0).astype(np.int64)
    Cg = c["C"] // c["G"]
    want = np.zeros((c["N"], c["Ho"], c["Wo"], 9, c["C"]), np.int16)
    n = np.arange(c["N"])[:, None, None, None]
    for g in range(c["G"]):
        picked = bits[n, yi[..., g, :], xi[..., g, :]][..., g * Cg:(g + 1) * Cg]      # [N,Ho,Wo,9,Cg]
        want[..., g * Cg:(g + 1) * Cg] = np.where(inside[..., g, :, None], picked, np.int16(0))
    got = col.view(torch.int16).cpu().numpy().reshape(want.shape)
    assert np.array_equal(got, want), "%d column entries differ from the indexed pixels" % (got != want).sum()
    _against_reference(c, off, name, ("doff", "dx"))


@pytest.mark.parametrize("mod", [False, True])
def test_window_edges_are_exact(hip, mod):
    """Samples exactly at -1, L, L - 1 and 2^-7 inside either edge (table in tests/test_deform_shapes_cpu.py): col is
    exactly zero outside the open window and within tolerance elsewhere, each (row kind, column kind) block on its own."""
    c = S.dcn_edge_case(mod)
    off = S.dcn_edge_offsets(c)
    x, dcol = _inputs(c, off)
    got = _gpu(c, x, off, dcol)
    ref = _ref(c, x, off, dcol)
    _check(c, got, ref, "edges")
    nreal = (27 if mod else 18) * c["G"]
    for i in range(S.EDGE_L):
        for j in range(S.EDGE_L):
            if S.EDGE_ZERO[i] or S.EDGE_ZERO[j]:
                assert not got["col"][:, i, j].any(), "col at row kind %d, column kind %d must be zero" % (i, j)
                assert not ref["col"][:, i, j].any()
                assert not got["doff"][:, i, j, :nreal].any(), "doff outside the window must be zero"
            else:
                assert ref["col"][:, i, j].any()
                _close(got["col"][:, i, j], ref["col"][:, i, j], "col at row kind %d, column kind %d" % (i, j))
                _close(got["doff"][:, i, j, :nreal], ref["doff"][:, i, j, :nreal],
                       "doff at row kind %d, column kind %d" % (i, j))


@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("layer", sorted(S.BENCH_LAYERS))
def test_bench_shapes_match_reference(hip, layer, G):
    """The DCN v2 layers of ResNet-50 at 800 x 1344 with offsets of up to +-4 px (5 % far outside): col, dx, doff with the
    column gradient the library's own 1x1 data gradient produced, and the fp64 adjoint identity
    <dcol, im2col(x)> == <col2im(dcol), x> on positive data (bound and reasoning: test_adjoint_identity_at_full_size of
    tests/test_gpu_deform_roi_pool.py)."""
    import torch
    from mxdetection_amd.ops import deform_conv as dc
    c = S.dcn_bench_case(layer, G)
    off = S.dcn_random_offsets(c)
    x, _ = _inputs(c, off)
    rng = np.random.default_rng(c["seed"] + 9)
    Cout = c["C"]
    w = _bf16(rng.standard_normal((Cout, 3, 3, c["C"])) * (2.0 / (9 * c["C"])) ** 0.5)
    dy = _bf16(rng.standard_normal((c["N"], c["Ho"], c["Wo"], Cout)))
    _, col, dcol, doff, dx, _ = _gpu_layer(_cuda(x), _cuda(off), _cuda(w), _cuda(dy), c["stride"], c["pad"], G, True)
    torch.cuda.synchronize()
    got = dict(col=col.float().cpu().numpy(), dx=dx.float().cpu().numpy(), doff=doff.float().cpu().numpy())
    _check(c, got, _ref(c, x, off, dcol.float().cpu().numpy()), "%s G=%d" % (layer, G))
    xp, dp = _inputs(c, off, positive=True)
    colp = dc.im2col(_cuda(xp), _cuda(off), c["stride"], c["pad"], G, True)
    dxp = dc.col2im(_cuda(off), _cuda(dp), xp.shape, c["stride"], c["pad"], G, True)
    torch.cuda.synchronize()
    lhs = float((colp.double().cpu() * torch.from_numpy(dp).double()).sum())
    rhs = float((dxp.double().cpu() * torch.from_numpy(xp).double()).sum())
    assert lhs > 0 and abs(lhs - rhs) <= 2e-3 * abs(lhs), (lhs, rhs)
