"""(Modulated) deformable RoI pooling without a GPU: the fp64 torch reference used by tests/test_gpu_deform_roi_pool.py,
pinned by hand-computed answers and by autograd; the C-ABI's argument checks; the config keys, the mdpool experiment file
and the builder's refusal for RetinaNet."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_round(v):
    """C round(): half away from zero (torch.round rounds half to even)."""
    return math.copysign(math.floor(abs(v) + 0.5), v)


def _geometry(roi, scale, pooled, S):
    PH, PW = pooled
    rsw = c_round(float(roi[1])) * scale - 0.5
    rsh = c_round(float(roi[2])) * scale - 0.5
    rew = (c_round(float(roi[3])) + 1.0) * scale - 0.5
    reh = (c_round(float(roi[4])) + 1.0) * scale - 0.5
    roi_w, roi_h = max(rew - rsw, 0.1), max(reh - rsh, 0.1)
    return rsw, rsh, roi_w, roi_h, roi_w / PW / S, roi_h / PH / S


def _samples(feats, scales, rois, levels, r, trans, pooled, S, trans_std, lvl_min):
    """Sample grid of roi r: (F [H,W,C], valid, corners, weights, position pieces), all [PH,PW,S,S](,C)."""
    PH, PW = pooled
    NB = PH * PW
    l = int(levels[r]) - lvl_min
    F = feats[l][int(rois[r, 0])]
    H, W = F.shape[0], F.shape[1]
    rsw, rsh, roi_w, roi_h, sub_w, sub_h = _geometry(rois[r], scales[l], pooled, S)
    dt = F.dtype
    ph = torch.arange(PH, dtype=dt).view(PH, 1)
    pw = torch.arange(PW, dtype=dt).view(1, PW)
    ws = pw * (roi_w / PW) + rsw
    hs = ph * (roi_h / PH) + rsh
    if trans is not None:
        ws = ws + trans[r, :NB].view(PH, PW) * trans_std * roi_w
        hs = hs + trans[r, NB:2 * NB].view(PH, PW) * trans_std * roi_h
    i = torch.arange(S, dtype=dt)
    w = ws[:, :, None, None] + i.view(1, 1, 1, S) * sub_w
    h = hs[:, :, None, None] + i.view(1, 1, S, 1) * sub_h
    w, h = torch.broadcast_tensors(w, h)
    valid = (w >= -0.5) & (w <= W - 0.5) & (h >= -0.5) & (h <= H - 0.5)
    wc, hc = w.clamp(0, W - 1), h.clamp(0, H - 1)
    x0, x1 = torch.floor(wc).detach().long(), torch.ceil(wc).detach().long()
    y0, y1 = torch.floor(hc).detach().long(), torch.ceil(hc).detach().long()
    dx, dy = wc - x0.to(dt), hc - y0.to(dt)
    return dict(F=F, valid=valid, x0=x0, x1=x1, y0=y0, y1=y1, dx=dx, dy=dy, roi_w=roi_w, roi_h=roi_h, l=l,
                n=int(rois[r, 0]))


def dpool_ref(feats, scales, rois, levels, trans=None, mask_logit=None, pooled=(7, 7), sample_per_part=4,
              trans_std=0.1, lvl_min=2):
    """fp64 torch-CPU restatement of include/mxdet.h mxdet_dpool_fwd: feats[l] [N,H,W,C], rois [R,5], levels [R]
    (int), trans [R, >= 2*PH*PW], mask_logit [R, >= PH*PW] (or None). Differentiable in feats, trans and mask_logit
    (floor / ceil held fixed). Returns [R,PH,PW,C]."""
    PH, PW = pooled
    outs = []
    for r in range(rois.shape[0]):
        s = _samples(feats, scales, rois, levels, r, trans, pooled, sample_per_part, trans_std, lvl_min)
        F, dx, dy = s["F"], s["dx"][..., None], s["dy"][..., None]
        val = ((1 - dx) * (1 - dy) * F[s["y0"], s["x0"]] + (1 - dx) * dy * F[s["y1"], s["x0"]] +
               dx * (1 - dy) * F[s["y0"], s["x1"]] + dx * dy * F[s["y1"], s["x1"]])
        v = s["valid"].to(F.dtype)[..., None]
        cnt = v.sum((2, 3))
        o = torch.where(cnt > 0, (val * v).sum((2, 3)) / cnt.clamp(min=1), torch.zeros_like(cnt))
        if mask_logit is not None:
            o = o * torch.sigmoid(mask_logit[r, :PH * PW].view(PH, PW, 1))
        outs.append(o)
    return torch.stack(outs)


def dpool_ref_backward(feats, scales, rois, levels, dout, trans=None, mask_logit=None, pooled=(7, 7),
                       sample_per_part=4, trans_std=0.1, lvl_min=2):
    """MXNet's backward, stated explicitly (fp64): (d_feats list, d_trans [R, 2*PH*PW] or None, d_mask [R, PH*PW] or
    None). Corners get weight * dout / count (* sigmoid); d_tx = sum (U(y1,x1) dy + U(y0,x1) (1-dy) - U(y1,x0) dy -
    U(y0,x0) (1-dy)) * trans_std * roi_w * dout / count, 0 where x0 == x1; d_mask = sum_c dout * pooled * s (1 - s)."""
    PH, PW = pooled
    NB = PH * PW
    R = rois.shape[0]
    dfeat = [torch.zeros_like(f) for f in feats]
    dtr = torch.zeros((R, 2 * NB), dtype=torch.float64) if trans is not None else None
    dmk = torch.zeros((R, NB), dtype=torch.float64) if mask_logit is not None else None
    for r in range(R):
        s = _samples(feats, scales, rois, levels, r, trans, pooled, sample_per_part, trans_std, lvl_min)
        F, dx, dy, valid = s["F"], s["dx"], s["dy"], s["valid"].to(torch.float64)
        H, W = F.shape[0], F.shape[1]
        cnt = valid.sum((2, 3))
        m = torch.sigmoid(mask_logit[r, :NB].view(PH, PW)) if mask_logit is not None else torch.ones((PH, PW), dtype=F.dtype)
        g = torch.where(cnt > 0, m / cnt.clamp(min=1), torch.zeros_like(cnt))[..., None] * dout[r]     # [PH,PW,C]
        gs = g[:, :, None, None, :] * valid[..., None]                                               # [PH,PW,S,S,C]
        flat = dfeat[s["l"]][s["n"]].view(H * W, -1)
        for yy, xx, wt in ((s["y0"], s["x0"], (1 - dx) * (1 - dy)), (s["y1"], s["x0"], (1 - dx) * dy),
                           (s["y0"], s["x1"], dx * (1 - dy)), (s["y1"], s["x1"], dx * dy)):
            flat.index_add_(0, (yy * W + xx).reshape(-1), (wt[..., None] * gs).reshape(-1, flat.shape[1]))
        U00, U01 = F[s["y0"], s["x0"]], F[s["y1"], s["x0"]]
        U10, U11 = F[s["y0"], s["x1"]], F[s["y1"], s["x1"]]
        dx_, dy_ = dx[..., None], dy[..., None]
        if trans is not None:
            tx = (U11 * dy_ + U10 * (1 - dy_) - U01 * dy_ - U00 * (1 - dy_)) * gs
            ty = (U11 * dx_ + U01 * (1 - dx_) - U10 * dx_ - U00 * (1 - dx_)) * gs
            # exactly 0 where the corners coincide (the sum above cancels only up to rounding there)
            tx = torch.where((s["x0"] == s["x1"])[..., None], torch.zeros_like(tx), tx)
            ty = torch.where((s["y0"] == s["y1"])[..., None], torch.zeros_like(ty), ty)
            dtr[r, :NB] = tx.sum((2, 3, 4)).reshape(-1) * trans_std * s["roi_w"]
            dtr[r, NB:] = ty.sum((2, 3, 4)).reshape(-1) * trans_std * s["roi_h"]
        if mask_logit is not None:
            val = (1 - dx_) * (1 - dy_) * U00 + (1 - dx_) * dy_ * U01 + dx_ * (1 - dy_) * U10 + dx_ * dy_ * U11
            pooled_v = torch.where(cnt[..., None] > 0, (val * valid[..., None]).sum((2, 3)) / cnt.clamp(min=1)[..., None],
                                   torch.zeros_like(dout[r]))
            dmk[r] = ((dout[r] * pooled_v).sum(2) * m * (1 - m)).reshape(-1)
    return dfeat, dtr, dmk


# ---- the reference, pinned by hand ------------------------------------------------------------------------------------

def _one(H, W, C, fill, scale=1.0):
    return [fill(torch.zeros((1, H, W, C), dtype=torch.float64))], [scale]


def _ramp(H=12, W=16, C=2):
    f = torch.arange(W, dtype=torch.float64).view(1, 1, W, 1).expand(1, H, W, C).clone()
    return [f], [1.0]


def test_constant_map_gives_the_constant_where_samples_exist():
    feats, scales = _one(10, 12, 3, lambda t: t.fill_(2.75))
    rois = torch.tensor([[0, 1, 2, 8, 7], [0, -6, -6, 3, 3], [0, 20, 20, 40, 40]], dtype=torch.float64)
    trans = torch.zeros((3, 98), dtype=torch.float64)
    trans[1:, :49] = torch.linspace(-2, 2, 49, dtype=torch.float64)
    out = dpool_ref(feats, scales, rois, [2, 2, 2], trans=trans, trans_std=1.0)
    s = _samples(feats, scales, rois, [2, 2, 2], 1, trans, (7, 7), 4, 1.0, 2)
    cnt = s["valid"].sum((2, 3))
    assert (cnt > 0).any() and (cnt == 0).any()          # the second roi has bins inside and bins outside the map
    assert torch.all(out[0] == 2.75)                      # inside the map, unshifted
    assert torch.equal(out[1][..., 0] == 2.75, cnt > 0) and torch.all(out[1][cnt == 0] == 0)
    assert torch.all(out[2] == 0)                           # fully outside: every bin is 0


def test_ramp_gives_the_mean_sample_position_of_a_worked_roi():
    # scale 1, x1 = 2, x2 = 9: rsw = 1.5, rew = 9.5, roi_w = 8, bin_w = 8/7, sub_w = 2/7: samples 1.5 + pw*8/7 + iw*2/7,
    # all inside the 16-wide map, and bilinear on f = x returns x itself: mean = 1.5 + pw*8/7 + 3/7
    feats, scales = _ramp()
    out = dpool_ref(feats, scales, torch.tensor([[0, 2, 1, 9, 8]], dtype=torch.float64), [2])
    want = torch.tensor([1.5 + pw * 8 / 7 + 3 / 7 for pw in range(7)], dtype=torch.float64)
    for ph in range(7):
        assert torch.allclose(out[0, ph, :, 0], want, rtol=0, atol=1e-12)
    # trans: bin (0, 0) moved by tx = 0.25 * 0.1 roi widths = 0.2 px
    tr = torch.zeros((1, 98), dtype=torch.float64)
    tr[0, 0] = 0.25
    out = dpool_ref(feats, scales, torch.tensor([[0, 2, 1, 9, 8]], dtype=torch.float64), [2], trans=tr)
    assert abs(float(out[0, 0, 0, 0]) - (1.5 + 3 / 7 + 0.2)) < 1e-12


def test_half_coordinates_round_away_from_zero():
    feats, scales = _ramp()
    # x1 = 2.5 -> 3 (torch.round: 2): rsw = 2.5, x2 = 9.5 -> 10: rew = 10.5, roi_w = 8: first bin mean 2.5 + 3/7
    out = dpool_ref(feats, scales, torch.tensor([[0, 2.5, 1, 9.5, 8]], dtype=torch.float64), [2])
    assert abs(float(out[0, 0, 0, 0]) - (2.5 + 3 / 7)) < 1e-12
    assert c_round(-0.5) == -1.0 and c_round(0.5) == 1.0 and c_round(2.5) == 3.0 and float(torch.round(torch.tensor(2.5))) == 2.0


def test_outside_bin_is_zero_and_tiny_roi_is_clamped_to_a_tenth():
    feats, scales = _ramp()
    tr = torch.zeros((1, 98), dtype=torch.float64)
    tr[0, 3] = 100.0                                          # bin (0, 3): 10 roi widths to the right, off the map
    out = dpool_ref(feats, scales, torch.tensor([[0, 2, 1, 9, 8]], dtype=torch.float64), [2], trans=tr)
    assert torch.all(out[0, 0, 3] == 0) and torch.all(out[0, 0, 2] > 0)
    # a degenerate roi at scale 1/8: rew - rsw = 1/8, but at scale 1/32 the width would be 1/32 < 0.1 -> 0.1
    g = _geometry([0, 5, 5, 5, 5], 1 / 32, (7, 7), 4)
    assert abs(g[2] - 0.1) < 1e-15 and abs(g[4] - 0.1 / 28) < 1e-15


def test_integer_positions_have_zero_offset_gradient():
    # pooled 2x2, S = 1, scale 1, x1 = 2, x2 = 9: roi_w = 8, bin_w = 4; trans_std 1, tx = 1/16 -> +0.5 px: w = 2 + 4 pw
    torch.manual_seed(0)
    feats = [torch.randn((1, 12, 16, 3), dtype=torch.float64)]
    rois = torch.tensor([[0, 2, 1, 9, 8]], dtype=torch.float64)
    tr = torch.zeros((1, 8), dtype=torch.float64)
    tr[0, :4] = 1 / 16
    dout = torch.randn((1, 2, 2, 3), dtype=torch.float64)
    _, dtr, _ = dpool_ref_backward(feats, [1.0], rois, [2], dout, trans=tr, pooled=(2, 2), sample_per_part=1,
                                   trans_std=1.0)
    assert torch.all(dtr[0, :4] == 0) and torch.any(dtr[0, 4:] != 0)


def _random_case(seed, R=6, C=5, modulated=True):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn((2, 14, 18, C), dtype=torch.float64, generator=g),
             torch.randn((2, 7, 9, C), dtype=torch.float64, generator=g)]
    scales = [1 / 4, 1 / 8]
    b = torch.rand((R, 4), dtype=torch.float64, generator=g) * torch.tensor([60, 40, 60, 40], dtype=torch.float64)
    rois = torch.cat([torch.randint(0, 2, (R, 1), generator=g).double(), torch.minimum(b[:, :2], b[:, 2:]),
                      torch.maximum(b[:, :2], b[:, 2:]) + 4], 1)
    levels = [2 + int(i % 2) for i in range(R)]
    trans = (torch.rand((R, 98), dtype=torch.float64, generator=g) * 2 - 1) * 4.0 * 1.37
    mask = torch.randn((R, 49), dtype=torch.float64, generator=g) if modulated else None
    dout = torch.randn((R, 7, 7, C), dtype=torch.float64, generator=g)
    return feats, scales, rois, levels, trans, mask, dout


@pytest.mark.parametrize("modulated", [False, True])
def test_reference_backward_matches_autograd(modulated):
    """Random offsets (non-integer positions almost surely): MXNet's explicit adjoint == autograd of the forward."""
    feats, scales, rois, levels, trans, mask, dout = _random_case(3, modulated=modulated)
    fs = [f.clone().requires_grad_(True) for f in feats]
    tr = trans.clone().requires_grad_(True)
    mk = mask.clone().requires_grad_(True) if modulated else None
    out = dpool_ref(fs, scales, rois, levels, trans=tr, mask_logit=mk)
    (out * dout).sum().backward()
    dfeat, dtr, dmk = dpool_ref_backward(feats, scales, rois, levels, dout, trans=trans, mask_logit=mask)
    for a, b in zip(dfeat, fs):
        assert torch.allclose(a, b.grad, rtol=1e-10, atol=1e-12)
    assert dtr.abs().sum() > 0 and torch.allclose(dtr, tr.grad, rtol=1e-10, atol=1e-12)
    if modulated:
        assert torch.allclose(dmk, mk.grad, rtol=1e-10, atol=1e-12)


# ---- the C-ABI's argument checks --------------------------------------------------------------------------------------

def _lib():
    from mxdetection_amd import _lib as L, build
    if not os.path.exists(L.LIB_PATH):
        build.build_hip(verbose=False)
    return L, L.load()


def _desc(L, levels=4, **kw):
    d = L.DpoolDescT()
    d.pyr.num_levels, d.pyr.lvl_min = levels, 2
    for l in range(min(levels, 8)):
        d.pyr.H[l], d.pyr.W[l] = 64 >> l, 80 >> l
        d.pyr.spatial_scale[l] = 1.0 / (4 << l)
        d.pyr.feat[l] = 16
    vals = dict(N=2, C=256, PH=7, PW=7, sample_per_part=4, trans_std=0.1, modulated=1, trans_stride=128, mask_stride=64,
                accumulate=1)
    vals.update(kw)
    for k, v in vals.items():
        setattr(d, k, v)
    return d


def test_dpool_entries_validate_arguments():
    """Bad shapes are MXDET_ESHAPE, null pointers MXDET_EINVAL, a short workspace MXDET_EWORKSPACE: all decided on the
    host before any launch (the pointers below are never dereferenced)."""
    L, lib = _lib()
    p = C.c_void_p(16)
    ok = _desc(L)
    need = lib.mxdet_dpool_bwd_feat_workspace_bytes(C.byref(ok), 1024)
    assert need >= 1024 * 32 * 50
    assert lib.mxdet_dpool_bwd_feat_workspace_bytes(C.byref(_desc(L, PH=9, PW=9)), 1024) == 0
    assert lib.mxdet_dpool_bwd_feat_workspace_bytes(None, 1024) == 0
    for bad in (dict(C=60), dict(C=0), dict(N=0), dict(PH=9, PW=9), dict(PH=0), dict(sample_per_part=0),
                dict(sample_per_part=17), dict(trans_stride=97), dict(mask_stride=48)):
        d = _desc(L, **bad)
        assert lib.mxdet_dpool_fwd(C.byref(d), p, p, 1024, p, p, p, None) == -2, bad
        assert lib.mxdet_dpool_bwd_trans(C.byref(d), p, p, 1024, p, p, p, p, p, None) == -2, bad
        assert lib.mxdet_dpool_bwd_feat(C.byref(d), p, p, 1024, p, p, p, p, 1 << 30, None) == -2, bad
    for R in (-1, 65536):
        assert lib.mxdet_dpool_fwd(C.byref(ok), p, p, R, p, p, p, None) == -2
        assert lib.mxdet_dpool_bwd_feat(C.byref(ok), p, p, R, p, p, p, p, 1 << 30, None) == -2
    for bad in (_desc(L, levels=0), _desc(L, levels=9)):
        assert lib.mxdet_dpool_fwd(C.byref(bad), p, p, 8, p, p, p, None) == -2
    big = _desc(L)
    big.pyr.W[0] = 40000
    assert lib.mxdet_dpool_bwd_feat(C.byref(big), p, p, 8, p, p, p, p, 1 << 30, None) == -2
    assert b"sample_per_part" in (lib.mxdet_dpool_fwd(C.byref(_desc(L, sample_per_part=0)), p, p, 8, p, p, p, None)
                                  and lib.mxdet_last_error())
    # null pointers
    nofeat = _desc(L)
    nofeat.pyr.feat[2] = None
    assert lib.mxdet_dpool_fwd(C.byref(nofeat), p, p, 8, p, p, p, None) == -1
    assert lib.mxdet_dpool_fwd(None, p, p, 8, p, p, p, None) == -1
    assert lib.mxdet_dpool_fwd(C.byref(ok), p, p, 8, p, None, p, None) == -1            # modulated without a mask
    assert lib.mxdet_dpool_fwd(C.byref(ok), p, p, 8, None, p, p, None) == -1            # modulated without trans
    assert lib.mxdet_dpool_fwd(C.byref(ok), None, p, 8, p, p, p, None) == -1
    assert lib.mxdet_dpool_fwd(C.byref(ok), p, p, 8, p, p, None, None) == -1
    assert b"modulated" in (lib.mxdet_dpool_fwd(C.byref(ok), p, p, 8, p, None, p, None) and lib.mxdet_last_error())
    v1 = _desc(L, modulated=0)
    assert lib.mxdet_dpool_bwd_trans(C.byref(v1), p, p, 8, None, None, p, p, None, None) == -1   # needs trans
    assert lib.mxdet_dpool_bwd_trans(C.byref(v1), p, p, 8, p, None, p, None, None, None) == -1   # needs d_trans
    assert lib.mxdet_dpool_bwd_trans(C.byref(ok), p, p, 8, p, p, p, p, None, None) == -1         # v2 needs d_mask
    assert lib.mxdet_dpool_bwd_trans(C.byref(v1), p, p, 8, p, None, None, p, None, None) == -1   # no dout
    assert lib.mxdet_dpool_bwd_feat(C.byref(v1), p, p, 8, None, None, None, p, 1 << 30, None) == -1
    # workspace
    need8 = lib.mxdet_dpool_bwd_feat_workspace_bytes(C.byref(v1), 8)
    assert lib.mxdet_dpool_bwd_feat(C.byref(v1), p, p, 8, None, None, p, p, need8 - 1, None) == -3
    assert lib.mxdet_dpool_bwd_feat(C.byref(v1), p, p, 8, None, None, p, None, need8, None) == -3
    assert b"workspace" in (lib.mxdet_dpool_bwd_feat(C.byref(v1), p, p, 8, None, None, p, None, need8, None)
                            and lib.mxdet_last_error())


# ---- config, experiment file, builder ---------------------------------------------------------------------------------

def test_config_defaults_mdpool_experiment_file_and_builder(monkeypatch):
    from mxdetection_amd import models
    from mxdetection_amd.models import builder
    from mxdetection_amd.utils.config import default_config, load_config
    d = default_config()
    assert d.network.roi_pool == "roi_align" and d.network.dpool_trans_std == 0.1
    assert d.network.dpool_sample_per_part == 4 and d.network.dpool_offset_fcs == 3
    cfg = load_config(os.path.join(ROOT, "configs", "faster_rcnn_r50_fpn_dcn_mdpool.yaml"))
    assert cfg.network.type == "faster_rcnn" and cfg.network.roi_pool == "mdpool"
    assert sorted(cfg.network.dcn_stages) == [3, 4, 5] and cfg.network.dcn_modulated is True
    seen = {}

    class Recorder:
        def __init__(self, device, **kw):
            seen.update(kw)

    monkeypatch.setattr(models, "FasterRCNN", Recorder)
    builder.build_detector(cfg, device="cpu")
    assert seen["roi_pool"] == "mdpool" and seen["dpool_trans_std"] == 0.1 and seen["dpool_sample_per_part"] == 4
    assert seen["dpool_offset_fcs"] == 3 and seen["dcn_stages"] == (3, 4, 5)
    seen.clear()
    builder.build_detector(load_config(None, ["network.roi_pool=dpool", "network.dpool_offset_fcs=1"]), device="cpu")
    assert seen["roi_pool"] == "dpool" and seen["dpool_offset_fcs"] == 1
    seen.clear()
    builder.build_detector(default_config(), device="cpu")
    assert seen["roi_pool"] == "roi_align"
    monkeypatch.setattr(models, "RetinaNet", Recorder)
    with pytest.raises(ValueError, match="roi_pool"):
        builder.build_detector(load_config(None, ["network.type=retinanet", "network.roi_pool=mdpool"]), device="cpu")
    seen.clear()
    builder.build_detector(load_config(None, ["network.type=retinanet"]), device="cpu")
    assert "roi_pool" not in seen


def test_faster_rcnn_refuses_an_unknown_roi_pool():
    from mxdetection_amd.models import FasterRCNN
    with pytest.raises(ValueError, match="roi_pool"):
        FasterRCNN("cpu", roi_pool="psroi")
