"""(Modulated) deformable RoI pooling kernels (include/mxdet.h mxdet_dpool_*) against the fp64 torch reference of
tests/test_deform_roi_pool_cpu.py: forward (no-trans / v1 / v2), d_trans, d_mask and the feature adjoint, on P2-P5 with
rois on every level, clipped and tiny rois and random offsets of up to +-2 bins; bit-reproducibility of the adjoint and an
fp64 adjoint identity at full size.

Tolerance: bf16 storage, fp32 accumulation in another order (as tests/test_gpu_deform_conv.py):
|got - ref| <= 2^-7 * |ref| + 2^-7 * rms(ref) elementwise.
"""
import numpy as np
import pytest

from test_deform_roi_pool_cpu import dpool_ref, dpool_ref_backward

pytestmark = pytest.mark.gpu

STRIDES = (4, 8, 16, 32)
SCALES = [1.0 / s for s in STRIDES]


def _close(got, ref, what="", tol=2.0 ** -7):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rms = np.sqrt(np.mean(ref ** 2)) + 1e-30
    err = np.abs(got - ref)
    bad = err > tol * np.abs(ref) + tol * rms
    assert not bad.any(), "%s: %d/%d outside tolerance, max err %.4g (rms %.4g)" % (what, bad.sum(), bad.size, err.max(), rms)


def _bf16(t):
    import torch
    return t.to(torch.bfloat16)


def _case(C, R=40, N=2, H=256, W=320, seed=0, modulated=True):
    """bf16 P2-P5 of an HxW batch, rois on every level (8..600 px, some clipped past the image border, some zero-size:
    the 0.1 width clamp), trans of up to +-2 bins (trans_std 0.1: 2/7 roi widths = 2.86), some positions pushed off the
    map, mask logits in [-3, 3]."""
    import torch
    from mxdetection_amd.ops.roi_align import fpn_level_map
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    feats = [_bf16(torch.randn((N, (H + s - 1) // s, (W + s - 1) // s, C), generator=g)).cuda() for s in STRIDES]
    sz = np.exp(rng.uniform(np.log(8), np.log(600), (R, 2)))
    x1 = rng.uniform(-40, W - 8, R)
    y1 = rng.uniform(-40, H - 8, R)
    boxes = np.stack([x1, y1, x1 + sz[:, 0], y1 + sz[:, 1]], 1)
    boxes[:4, 2:] = boxes[:4, :2]                      # zero-size rois
    boxes[4:6, 0] = -0.5                               # .5 coordinates (C round: -1)
    boxes[6, 1] = 2.5
    rois = np.concatenate([rng.integers(0, N, (R, 1)), boxes], 1).astype(np.float32)
    rois_t = torch.from_numpy(rois).cuda()
    levels = fpn_level_map(rois_t, 2, 5)
    levels[:2] = 5                                     # zero-size rois on P5 / P4: width 1/32, 1/16 -> clamped to 0.1
    levels[2:4] = 4
    assert sorted(set(levels.cpu().tolist())) == [2, 3, 4, 5]
    trans = torch.zeros((R, 128), dtype=torch.float32)
    trans[:, :98] = (torch.rand((R, 98), generator=g) * 2 - 1) * 2.86
    trans[-3:, :49] = 40.0                              # bins far off the map (count 0)
    mask = torch.zeros((R, 64), dtype=torch.float32)
    mask[:, :49] = (torch.rand((R, 49), generator=g) * 2 - 1) * 3
    trans, mask = _bf16(trans).cuda(), _bf16(mask).cuda()
    dout = _bf16(torch.randn((R, 7, 7, C), generator=g)).cuda()
    return feats, rois_t, levels, trans, (mask if modulated else None), dout


def _ref_inputs(feats, rois, levels, trans, mask):
    import torch
    f64 = [f.double().cpu() for f in feats]
    return (f64, rois.double().cpu(), [int(v) for v in levels.cpu()], None if trans is None else trans.double().cpu(),
            None if mask is None else mask.double().cpu())


MODES = ["notrans", "v1", "v2"]


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("mode", MODES)
def test_forward_matches_reference(hip, C, mode):
    from mxdetection_amd.ops.deform_roi_pool import dpool_forward
    feats, rois, levels, trans, mask, _ = _case(C, seed=1, modulated=(mode == "v2"))
    if mode == "notrans":
        trans = None
    out = dpool_forward(feats, SCALES, rois, levels, trans=trans, mask=mask)
    f64, r64, lv, t64, m64 = _ref_inputs(feats, rois, levels, trans, mask)
    ref = dpool_ref(f64, SCALES, r64, lv, trans=t64, mask_logit=m64)
    assert ref.abs().sum() > 0 and (ref == 0).any()          # some empty bins (outside the map) are covered
    _close(out.float().cpu().numpy(), ref.numpy(), "forward %s C=%d" % (mode, C))


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("mode", MODES)
def test_backward_matches_reference(hip, C, mode):
    import torch
    from mxdetection_amd.ops.deform_roi_pool import dpool_backward_feat, dpool_backward_trans
    feats, rois, levels, trans, mask, dout = _case(C, seed=2, modulated=(mode == "v2"))
    if mode == "notrans":
        trans = None
    dmaps = [torch.full_like(f, 7.0) for f in feats]          # overwritten (accumulate off), untouched pixels too
    dpool_backward_feat(dmaps, SCALES, rois, levels, dout, trans=trans, mask=mask)
    f64, r64, lv, t64, m64 = _ref_inputs(feats, rois, levels, trans, mask)
    dfeat, dtr, dmk = dpool_ref_backward(f64, SCALES, r64, lv, dout.double().cpu(), trans=t64, mask_logit=m64)
    for l, (got, want) in enumerate(zip(dmaps, dfeat)):
        _close(got.float().cpu().numpy(), want.numpy(), "d_feat P%d %s C=%d" % (l + 2, mode, C))
    # accumulate: adds onto what is there
    base = [_bf16(torch.randn(f.shape, device="cuda") * 1e-3) for f in feats]   # small: its rounding stays in the bound
    acc = [b.clone() for b in base]
    dpool_backward_feat(acc, SCALES, rois, levels, dout, trans=trans, mask=mask, accumulate=True)
    for l in range(4):
        _close((acc[l].double() - base[l].double()).cpu().numpy(), dfeat[l].numpy(), "accumulate P%d" % (l + 2),
               tol=2.0 ** -5)
    if trans is None:
        return
    d_trans, d_mask = dpool_backward_trans(feats, SCALES, rois, levels, dout, trans, mask)
    got = d_trans.float().cpu()
    assert not got[:, 98:].any(), "padding columns of d_trans are zero"
    _close(got[:, :98].numpy(), dtr.numpy(), "d_trans %s C=%d" % (mode, C))
    assert got[-3:, :49].abs().sum() == 0                     # bins off the map: no gradient
    if mask is not None:
        gm = d_mask.float().cpu()
        assert not gm[:, 49:].any()
        _close(gm[:, :49].numpy(), dmk.numpy(), "d_mask C=%d" % C)


def test_zero_trans_equals_pass0_and_zero_logit_halves_it(hip):
    import torch
    from mxdetection_amd.ops.deform_roi_pool import dpool_forward
    feats, rois, levels, trans, mask, _ = _case(256, seed=3)
    p0 = dpool_forward(feats, SCALES, rois, levels)
    zt = torch.zeros_like(trans)
    p1 = dpool_forward(feats, SCALES, rois, levels, trans=zt)
    assert torch.equal(p0, p1)
    p2 = dpool_forward(feats, SCALES, rois, levels, trans=zt, mask=torch.zeros_like(mask))
    assert torch.equal(p2.float(), p0.float() * 0.5)


def _full_size(R=1024, C=256, identical=False, seed=5):
    """P2-P5 of a 2 x 800 x 1344 batch, 1024 rois (or 1024 copies of one large roi)."""
    import torch
    from mxdetection_amd.ops.roi_align import fpn_level_map
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    N, H, W = 2, 800, 1344
    feats = [_bf16(torch.rand((N, H // s, W // s, C), generator=g)).cuda() for s in STRIDES]
    if identical:
        rois = np.tile(np.array([[1, 100.0, 80.0, 900.0, 700.0]], np.float32), (R, 1))
    else:
        sz = np.exp(rng.uniform(np.log(16), np.log(800), (R, 2)))
        x1, y1 = rng.uniform(0, W - 16, R), rng.uniform(0, H - 16, R)
        rois = np.stack([rng.integers(0, N, R), x1, y1, np.minimum(x1 + sz[:, 0], W - 1),
                         np.minimum(y1 + sz[:, 1], H - 1)], 1).astype(np.float32)
    rois_t = torch.from_numpy(rois).cuda()
    levels = fpn_level_map(rois_t, 2, 5)
    trans = torch.zeros((R, 128))
    trans[:, :98] = (torch.rand((R, 98), generator=g) * 2 - 1) * 2.86
    mask = torch.zeros((R, 64))
    mask[:, :49] = torch.randn((R, 49), generator=g)
    dout = _bf16(torch.rand((R, 7, 7, C), generator=g)).cuda()
    return feats, rois_t, levels, _bf16(trans).cuda(), _bf16(mask).cuda(), dout


@pytest.mark.parametrize("identical", [False, True])
def test_feature_adjoint_is_bit_reproducible(hip, identical):
    """Two runs write identical bits, also when all 1024 rois are the same box (every pixel of it in 1024 lists)."""
    import torch
    from mxdetection_amd.ops.deform_roi_pool import dpool_backward_feat
    feats, rois, levels, trans, mask, dout = _full_size(identical=identical)
    runs = []
    for _ in range(2):
        d = [torch.zeros_like(f) for f in feats]
        dpool_backward_feat(d, SCALES, rois, levels, dout, trans=trans, mask=mask)
        runs.append(d)
    torch.cuda.synchronize()
    assert any(x.any() for x in runs[0])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("mode", ["notrans", "v2"])
def test_adjoint_identity_at_full_size(hip, mode):
    """<dout, pool(x)> == <adj(dout), x> in fp64 (1024 rois on P2-P5 of an 800x1344 batch; positive data, so the bf16
    roundings of both sides average out far below the bound)."""
    import torch
    from mxdetection_amd.ops.deform_roi_pool import dpool_backward_feat, dpool_forward
    feats, rois, levels, trans, mask, dout = _full_size(seed=6)
    if mode == "notrans":
        trans = mask = None
    out = dpool_forward(feats, SCALES, rois, levels, trans=trans, mask=mask)
    adj = [torch.zeros_like(f) for f in feats]
    dpool_backward_feat(adj, SCALES, rois, levels, dout, trans=trans, mask=mask)
    lhs = float((dout.double() * out.double()).sum())
    rhs = sum(float((a.double() * f.double()).sum()) for a, f in zip(adj, feats))
    assert lhs > 0 and abs(lhs - rhs) <= 2e-3 * abs(lhs), (lhs, rhs)
