"""The Mask Scoring R-CNN entries (mxdet_maskiou_*) through the C-ABI against the numpy-float32 restatement of
tests/_mask_iou_ref.py: bit for bit, except the loss value (fp32 fixed-order sum against float64)."""
import numpy as np
import pytest

import _mask_iou_ref as ref

pytestmark = pytest.mark.gpu

N, G, R = 2, 6, 60
CLASSES = (3, 17, 80, 1, 42)


def _t(a, dt=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dt is None else t.to(dt)


def _bits(t):
    import torch
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _gt(H, W):
    """Five valid boxes per image (two of them touching frame edges) and one padding row."""
    frac = np.array([[0.05, 0.10, 0.45, 0.60], [0.50, 0.05, 0.95, 0.50], [0.30, 0.55, 0.80, 0.95],
                     [0.00, 0.00, 0.20, 0.25], [0.70, 0.60, 1.00, 1.00]])
    gt = -np.ones((N, G, 5), np.float32)
    for n in range(N):
        f = frac if n == 0 else frac[::-1]
        for g in range(5):
            x1, y1, x2, y2 = f[g] * (W - 1, H - 1, W - 1, H - 1)
            gt[n, g] = (np.floor(x1), np.floor(y1), np.ceil(x2), np.ceil(y2), CLASSES[(g + n) % 5])
    return gt


def _rois(gt, H, W):
    """Hand-placed rois: (rois [R,5], matched [R], labels [R], rows whose cls is forced positive with matched = -1)."""
    rows = []
    for n in range(N):
        for g in range(5):
            x1, y1, x2, y2, c = (float(v) for v in gt[n, g])
            cx, cy = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
            rows += [((n, x1 - 1.3, y1 + 0.6, x2 + 0.4, y2 - 1.7), g, c),             # hugging the GT, fractional corners
                     ((n, x1, y1, cx, y2), g, c),                                     # the left half
                     ((n, x1, cy + 0.25, x2, y2), g, c),                              # the bottom half
                     ((n, x1 - W, y1 - H, cx + 2.5, cy + 1.5), g, c),                 # hanging over the top-left frame edge
                     ((n, cx - 3.5, cy - 2.5, x2 + W, y2 + H), g, c)]                 # ... and the bottom-right one
    x1, y1, x2, y2, c = (float(v) for v in gt[0, 0])
    rows.append(((0, np.floor(0.5 * (x1 + x2)), y1, np.floor(0.5 * (x1 + x2)), y2), 0, c))      # one pixel wide
    rows.append(((0, *gt[0, 1, :4]), 0, c))                                           # disjoint from its matched mask
    rows.append(((0, W + 5.0, H + 5.0, W + 50.0, H + 50.0), 0, c))                    # outside the frame: empty clip
    rows.append(((0, 0.5 * (x1 + x2) - 1, 0.5 * (y1 + y2) - 1, 0.5 * (x1 + x2) + 1, 0.5 * (y1 + y2) + 1), 0, c))   # 3x3 inside
    rows.append(((1, 0.0, 0.0, W - 1.0, H - 1.0), 2, float(gt[1, 2, 4])))             # the whole frame
    rows += [((0, 0.0, 0.0, 0.0, 0.0), -1, -1)] * 3                                   # padding rows: zero box, no match
    forced = [len(rows), len(rows) + 1]
    rows += [((1, 10.0, 10.0, 40.0, 40.0), -1, 5), ((0, 0.0, 0.0, 0.0, 0.0), -1, 80)]  # cls > 0 but unmatched
    assert len(rows) == R
    rois = np.array([r[0] for r in rows], np.float32)
    return rois, np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.int32), forced


def _target_case(oracle, H, W, S, Cpad, seed=31):
    rng = np.random.default_rng(seed)
    gt = _gt(H, W)
    masks = ref.ellipse_masks(gt, H, W)
    rois, matched, labels, forced = _rois(gt, H, W)
    tg, cls = oracle.mask_target(rois, matched, labels, masks, S)
    cls = cls.copy()
    cls[forced] = labels[forced]
    logits = rng.standard_normal((R, S, S, Cpad)).astype(np.float32) * 2
    for r in range(R):                       # a noisy prediction of the target on the class channel
        if cls[r] > 0:
            logits[r, :, :, cls[r] - 1] = (tg[r].astype(np.float32) * 2 - 1) * 1.5 + rng.standard_normal((S, S)) * 1.5
    return rois, matched, cls, gt, masks, oracle.round_bf16(logits), tg


@pytest.mark.parametrize("S,Cpad", [(28, 128), (28, 88), (14, 128), (14, 88)])
@pytest.mark.parametrize("frame", [(96, 128), (90, 132), (75, 100)])       # row starts 16-byte aligned only in the first
def test_maskiou_target_bit_exact(hip, oracle, frame, S, Cpad):
    from mxdetection_amd.core import mask as M_
    H, W = frame
    a = _target_case(oracle, H, W, S, Cpad)
    rois, matched, cls, gt, masks, logits, tg = a
    want = ref.maskiou_target(*a)
    counts = ref.target_counts(*a)
    # properties of the inputs, checked on the reference before the kernel runs
    fg = [r for r in range(R) if counts[r] is not None]
    assert sum(0 < want[r] < 1 for r in fg) > len(fg) / 2
    assert any(counts[r][1] < counts[r][0] for r in fg)
    assert any(want[r] == 0 and cls[r] > 0 for r in range(R))
    assert any(counts[r] is None and cls[r] > 0 for r in range(R)) and any(cls[r] < 0 for r in range(R))
    import torch
    args = (_t(rois), _t(matched), _t(cls), _t(gt), _t(masks), _t(logits, torch.bfloat16), _t(tg))
    got = M_.maskiou_target(*args).cpu().numpy()
    again = M_.maskiou_target(*args).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got != want)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def test_maskiou_target_wider_box_table(hip, oracle):
    """gt_boxes with more rows per image than gt_masks has instances (the benchmark's 100 against 16): same result."""
    import torch
    from mxdetection_amd.core import mask as M_
    a = _target_case(oracle, 90, 132, 28, 128)
    rois, matched, cls, gt, masks, logits, tg = a
    wide = -np.ones((N, G + 5, 5), np.float32)
    wide[:, :G] = gt
    got = M_.maskiou_target(_t(rois), _t(matched), _t(cls), _t(wide), _t(masks), _t(logits, torch.bfloat16), _t(tg))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.maskiou_target(*a).view(np.uint32))


def test_maskiou_input_bit_exact(hip, oracle):
    import torch
    from mxdetection_amd.core import mask as M_
    rng = np.random.default_rng(32)
    R_, h, C, Cpad = 7, 14, 256, 128
    mp = oracle.round_bf16(rng.standard_normal((R_, h, h, C)).astype(np.float32))
    lg = oracle.round_bf16((rng.standard_normal((R_, 2 * h, 2 * h, Cpad)) * 3).astype(np.float32))
    cls = np.array([1, 80, -1, 17, 0, 128, 42], np.int32)
    out = torch.full((R_, h, h, ref.CIN), float("nan"), dtype=torch.bfloat16, device="cuda")    # unwritten channels show
    M_.maskiou_input(_t(mp, torch.bfloat16), _t(lg, torch.bfloat16), _t(cls), out=out)
    got = _bits(out)
    want = ref.maskiou_input(oracle, mp, lg, cls)
    assert np.array_equal(got, want)
    assert not got[[2, 4], :, :, C].any() and got[0, :, :, C].any() and not got[..., C + 1:].any()


def test_maskiou_input_bwd_bit_exact(hip, oracle):
    import torch
    from mxdetection_amd.core import mask as M_
    rng = np.random.default_rng(33)
    R_, h, C = 3, 14, 256
    a = oracle.round_bf16(rng.standard_normal((R_, h, h, C)).astype(np.float32))
    b = oracle.round_bf16(rng.standard_normal((R_, h, h, ref.CIN)).astype(np.float32))
    b[..., C:] = np.nan                                  # the mask channel's and the padding's gradients are ignored
    d = _t(a, torch.bfloat16)
    M_.maskiou_input_bwd(_t(b, torch.bfloat16), d)
    want = oracle.f32_to_bf16_bits((a + b[..., :C]).astype(np.float32))
    assert np.array_equal(_bits(d), want)


def test_maskiou_loss(hip, oracle):
    import torch
    from mxdetection_amd.core import mask as M_
    rng = np.random.default_rng(34)
    R_, ld = 40, 128
    pred = oracle.round_bf16(rng.uniform(-0.2, 1.2, (R_, ld)).astype(np.float32))
    cls = rng.integers(-1, 81, R_).astype(np.int32)
    cls[cls == 0] = -1
    cls[:4] = (1, 80, -1, 8)
    t = rng.uniform(0.05, 1.0, R_).astype(np.float32)
    t[5::4] = 0.0                                          # foreground rows whose target is 0: not positive
    assert ((cls > 0) & (t == 0)).any() and ((cls > 0) & (t > 0)).sum() > 10 and (cls < 0).any()
    loss = torch.zeros(1, device="cuda")
    grad = torch.full((R_, ld), float("nan"), dtype=torch.bfloat16, device="cuda")
    M_.maskiou_loss(_t(pred, torch.bfloat16), _t(cls), _t(t), loss, grad, loss_scale=2.0, weight=0.75)
    w_loss, w_grad = ref.maskiou_loss(oracle, pred, cls, t, loss_scale=2.0, weight=0.75)
    assert w_loss > 0 and np.allclose(loss.cpu().numpy(), w_loss, rtol=2e-5, atol=0)      # fp32 fixed-order sum vs float64
    assert np.array_equal(_bits(grad), w_grad)
    # no positive row at all: loss 0, gradient all zero
    grad.fill_(float("nan"))
    loss.fill_(7.0)
    M_.maskiou_loss(_t(pred, torch.bfloat16), _t(cls), _t(np.zeros(R_, np.float32)), loss, grad)
    assert float(loss) == 0.0 and not _bits(grad).any()


def test_maskiou_score_bit_exact(hip, oracle):
    import torch
    from mxdetection_amd.core import mask as M_
    rng = np.random.default_rng(35)
    R_, ld = 23, 128
    pred = oracle.round_bf16(rng.uniform(-0.1, 1.1, (R_, ld)).astype(np.float32))
    dets = np.zeros((R_, 6), np.float32)
    dets[:, 4] = rng.uniform(0.05, 1.0, R_)
    dets[:, 5] = rng.integers(1, 81, R_)
    dets[[3, 11, 22], 4:] = (0.0, -1.0)                    # padding rows
    dets[0, 5], dets[1, 5] = 1, 80
    got = M_.maskiou_score(_t(dets), _t(pred, torch.bfloat16)).cpu().numpy()
    want = ref.maskiou_score(dets, pred)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[[3, 11, 22]].any() and (got[[0, 1, 2]] != 0).all()
