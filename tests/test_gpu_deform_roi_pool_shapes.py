"""Deformable RoI pooling kernels (csrc/deform_roi_pool.hip) at the shapes where their shape-dependent branches leave the
simplest arm: more than one 1024-roi round of the feature adjoint's list, more than one (and a partial) 256-channel
chunk, bin grids other than 7 x 7 x 4 x 4, padded and unpadded trans / mask rows, one-level pyramids and maps narrower
than or not aligned to a workgroup's 32-pixel span. Inputs and the CPU proof that each case reaches its branch:
tests/test_deform_shapes_cpu.py. Reference: dpool_ref / dpool_ref_backward of tests/test_deform_roi_pool_cpu.py (fp64);
tolerance: _close of tests/test_gpu_deform_roi_pool.py (|got - ref| <= 2^-7 |ref| + 2^-7 rms(ref)).
"""
import pytest

import test_deform_shapes_cpu as S
from test_deform_roi_pool_cpu import dpool_ref, dpool_ref_backward
from test_gpu_deform_roi_pool import _close

pytestmark = pytest.mark.gpu


def _gpu_all(case, mode="v2"):
    """Forward and the three gradients through the library: (out, d_feats, d_trans, d_mask) as fp32 CPU tensors."""
    import torch
    from mxdetection_amd.ops.deform_roi_pool import dpool_backward_feat, dpool_backward_trans, dpool_forward
    kw = dict(sample_per_part=case["S"], trans_std=case["trans_std"], lvl_min=case["lvl_min"])
    feats = [f.cuda() for f in case["feats"]]
    rois, levels, dout = case["rois"].cuda(), case["levels"].cuda(), case["dout"].cuda()
    trans = case["trans"].cuda() if mode != "notrans" else None
    mask = case["mask"].cuda() if mode == "v2" else None
    out = dpool_forward(feats, case["scales"], rois, levels, pooled=case["pooled"], trans=trans, mask=mask, **kw)
    dmaps = [torch.full_like(f, 7.0) for f in feats]          # overwritten in full (accumulate off)
    dpool_backward_feat(dmaps, case["scales"], rois, levels, dout, trans=trans, mask=mask, **kw)
    d_trans = d_mask = None
    if trans is not None:
        d_trans, d_mask = dpool_backward_trans(feats, case["scales"], rois, levels, dout, trans, mask, **kw)
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.float().cpu()   # noqa: E731
    return cpu(out), [cpu(d) for d in dmaps], cpu(d_trans), cpu(d_mask)


def _ref_all(case, mode="v2"):
    kw = dict(pooled=case["pooled"], sample_per_part=case["S"], trans_std=case["trans_std"], lvl_min=case["lvl_min"])
    f64 = [f.double() for f in case["feats"]]
    rois, levels = case["rois"].double(), [int(v) for v in case["levels"]]
    trans = case["trans"].double() if mode != "notrans" else None
    mask = case["mask"].double() if mode == "v2" else None
    out = dpool_ref(f64, case["scales"], rois, levels, trans=trans, mask_logit=mask, **kw)
    dfeat, dtr, dmk = dpool_ref_backward(f64, case["scales"], rois, levels, case["dout"].double(), trans=trans,
                                         mask_logit=mask, **kw)
    return out, dfeat, dtr, dmk


def _check_all(case, got, ref, tag):
    NB = case["NB"]
    out, dmaps, d_trans, d_mask = got
    rout, rfeat, rtr, rmk = ref
    assert rout.abs().sum() > 0
    _close(out.numpy(), rout.numpy(), tag + " forward")
    for l, (g, w) in enumerate(zip(dmaps, rfeat)):
        _close(g.numpy(), w.numpy(), "%s d_feat level %d" % (tag, l))
    if rtr is not None:
        assert rtr.abs().sum() > 0
        _close(d_trans[:, :2 * NB].numpy(), rtr.numpy(), tag + " d_trans")
        assert not d_trans[:, 2 * NB:].any(), tag + ": padding columns of d_trans must be zero"
    if rmk is not None:
        _close(d_mask[:, :NB].numpy(), rmk.numpy(), tag + " d_mask")
        assert not d_mask[:, NB:].any(), tag + ": padding columns of d_mask must be zero"


@pytest.mark.parametrize("R", sorted(S.ROUND_CASES))
def test_roi_rounds_match_reference_and_are_bit_reproducible(hip, R):
    """1023, 1025 and 2500 heavily overlapping rois (one, two and three list rounds; a block of identical boxes across a
    round boundary): forward and all gradients against the reference, d_feat bit-identical over two launches."""
    import torch
    from mxdetection_amd.ops.deform_roi_pool import dpool_backward_feat
    case = S.dpool_round_case(R)
    got = _gpu_all(case)
    _check_all(case, got, _ref_all(case), "R=%d" % R)
    feats = [f.cuda() for f in case["feats"]]
    again = [torch.full_like(f, float("nan")) for f in feats]
    dpool_backward_feat(again, case["scales"], case["rois"].cuda(), case["levels"].cuda(), case["dout"].cuda(),
                        trans=case["trans"].cuda(), mask=case["mask"].cuda())
    torch.cuda.synchronize()
    for a, b in zip(again, got[1]):
        assert torch.equal(a.float().cpu(), b), "d_feat differs between launches"


def test_no_rois_zero_or_keep_the_gradient_maps(hip):
    """R = 0: accumulate off writes zeros everywhere, accumulate on leaves the maps as they are."""
    import torch
    from mxdetection_amd.ops.deform_roi_pool import dpool_backward_feat, dpool_forward
    case = S.dpool_case(0, 64, seed=77)
    feats = [f.cuda() for f in case["feats"]]
    args = (case["scales"], case["rois"].cuda(), case["levels"].cuda(), case["dout"].cuda())
    kw = {}                                                   # (no trans / mask: an empty tensor has no pointer to pass)
    assert dpool_forward(feats, case["scales"], args[1], args[2]).shape == (0, 7, 7, 64)
    d = [torch.full_like(f, 7.0) for f in feats]
    dpool_backward_feat(d, *args, **kw)
    torch.cuda.synchronize()
    assert all(not t.any() for t in d), "accumulate off must zero the maps"
    d = [torch.full_like(f, 7.0) for f in feats]
    dpool_backward_feat(d, *args, accumulate=True, **kw)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in d), "accumulate on must leave the maps untouched"


@pytest.mark.parametrize("C", [8, 264, 512])
def test_channel_chunks_match_reference(hip, C):
    """One partial 256-channel chunk, a full one followed by 8 channels, and two full ones."""
    case = S.dpool_case(40, C, seed=600 + C)
    _check_all(case, _gpu_all(case), _ref_all(case), "C=%d" % C)
    if C == 264:
        _check_all(case, _gpu_all(case, "notrans"), _ref_all(case, "notrans"), "C=264 no trans")


@pytest.mark.parametrize("trans_std", S.TRANS_STD)
@pytest.mark.parametrize("samples", S.SAMPLES)
@pytest.mark.parametrize("pooled", S.POOLED)
def test_bin_grids_match_reference(hip, pooled, samples, trans_std):
    """pooled 1x1, 3x5, 8x8 (all 64 lanes are bins), 1 / 2 / 16 samples per part, trans_std 0.05 / 0.5, with trans and
    mask rows of exactly 2 PH PW / PH PW columns and with padded rows (same values: one reference)."""
    tag = "pooled %dx%d S=%d std=%g" % (pooled + (samples, trans_std))
    tight = S.dpool_grid_case(pooled, samples, trans_std, False)
    ref = _ref_all(tight)
    _check_all(tight, _gpu_all(tight), ref, tag + " tight rows")
    padded = S.dpool_grid_case(pooled, samples, trans_std, True)
    _check_all(padded, _gpu_all(padded), ref, tag + " padded rows")


@pytest.mark.parametrize("W", S.NARROW_W)
def test_narrow_single_level_maps_match_reference(hip, W):
    case = S.dpool_narrow_case(W)
    for mode in ("v2", "v1"):
        _check_all(case, _gpu_all(case, mode), _ref_all(case, mode), "W=%d %s" % (W, mode))
