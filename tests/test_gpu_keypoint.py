"""The Keypoint R-CNN entries (mxdet_keypoint_*) through the C-ABI against tests/_keypoint_ref.py: target and decode bit
for bit, the gradient within the tolerance measured in tests/test_keypoint_cpu.py, the loss within LOSS_RTOL of float64."""
import functools

import numpy as np
import pytest

import _keypoint_ref as ref
from test_keypoint_cpu import ATOL_GRAD, LOSS_RTOL

pytestmark = pytest.mark.gpu

GUARD = 64          # elements in front of and behind every output
LOSS_SCALE, WEIGHT = 2.0, 0.75


def _t(a, dt=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dt is None else t.to(dt)


def _guarded(shape, dtype, fill):
    """(whole buffer, view of `shape` in its middle): the elements around the view must keep `fill`."""
    import torch
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(shape)


def _guards_intact(whole, fill):
    import torch
    g = torch.cat([whole[:GUARD], whole[-GUARD:]]).float()
    return bool((g == float(fill)).all())


@functools.lru_cache(maxsize=None)
def _case(S_in, Kpad, K):
    """Inputs and float64 reference of one table shape, computed once and shared (never modified)."""
    from oracle import oracle
    c = ref.case(oracle, S_in, Kpad, K)
    c["loss"], c["grad"], c["k"] = ref.keypoint_loss(c["logits"], c["targets"], LOSS_SCALE, WEIGHT)
    c["decoded"] = ref.keypoint_decode(c["logits"], c["dets"], K)
    return c


@pytest.mark.parametrize("S_in,Kpad,K", ref.SHAPES)
def test_target_bit_exact(hip, S_in, Kpad, K):
    import torch
    from mxdetection_amd.core import mask as M_
    c = _case(S_in, Kpad, K)
    want = c["targets"]
    S = 2 * S_in
    # properties of the rows, checked on the reference before the kernel runs
    assert {0, S - 1, (S - 1) * S, S * S - 1} <= set(want[:4].ravel().tolist())
    assert (want[8] == S * S - 1).all() and (want[10] == -1).all() and (want[12:17] == -1).all() and (want[19:21] == -1).all()
    assert (want[9, 0::2] == -1).all() and (want[11] % S == S - 1).any()
    whole, out = _guarded((ref.R_CASE, K), torch.int32, -77)
    args = (_t(c["rois"]), _t(c["matched"]), _t(c["labels"]), _t(c["gt_kp"]))
    M_.keypoint_target(*args, size_in=S_in, out=out)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)
    assert _guards_intact(whole, -77)
    assert M_.keypoint_target(*(a[:0] if i < 3 else a for i, a in enumerate(args)), size_in=S_in).shape == (0, K)


@pytest.mark.parametrize("S_in,Kpad,K", ref.SHAPES)
def test_loss_and_gradient(hip, oracle, S_in, Kpad, K):
    import torch
    from mxdetection_amd.core import mask as M_
    c = _case(S_in, Kpad, K)
    R = ref.R_CASE
    tg = c["targets"]
    assert (tg >= 0).sum() >= K * 15 and (tg[10] < 0).all()
    lg, tgt = _t(c["logits"], torch.bfloat16), _t(tg)
    ws = M_.keypoint_loss_workspace(R, "cuda")
    runs = []
    for _ in range(2):
        lw, loss = _guarded((1,), torch.float32, 7.0)
        gw, grad = _guarded((R, S_in, S_in, Kpad), torch.bfloat16, 776.0)      # sentinel (exact in bf16): every element must be written
        M_.keypoint_loss(lg, tgt, loss, grad, ws, LOSS_SCALE, WEIGHT)
        torch.cuda.synchronize()
        assert _guards_intact(lw, 7.0) and _guards_intact(gw, 776.0)
        runs.append((loss.cpu().numpy().copy(), grad.view(torch.int16).cpu().numpy().copy(), grad.float().cpu().numpy()))
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32)) and np.array_equal(runs[0][1], runs[1][1])
    loss, _, g = runs[0]
    k = c["k"]
    print("keypoint loss %r (float64 %r), max |grad - ref| / k = %.3e" % (float(loss[0]), c["loss"],
                                                                         np.abs(g - c["grad"]).max() / k))
    assert c["loss"] > 0 and abs(float(loss[0]) - c["loss"]) <= LOSS_RTOL * c["loss"]
    assert (np.abs(g - c["grad"]) <= ATOL_GRAD * k + 2.0 ** -8 * np.abs(c["grad"])).all()
    # fully written: zeros on rows / keypoints that are not trained and on the padding channels
    invalid = np.broadcast_to((tg < 0)[:, None, None, :], (R, S_in, S_in, K))
    assert not g[..., :K][invalid].any() and not g[..., K:].any() and g[..., :K][~invalid].any()


@pytest.mark.parametrize("S_in,Kpad,K", ref.SHAPES)
def test_loss_nothing_valid_and_no_rows(hip, S_in, Kpad, K):
    import torch
    from mxdetection_amd.core import mask as M_
    c = _case(S_in, Kpad, K)
    R = ref.R_CASE
    lg = _t(c["logits"], torch.bfloat16)
    loss = torch.full((1,), 7.0, device="cuda")
    grad = torch.full((R, S_in, S_in, Kpad), 776.0, dtype=torch.bfloat16, device="cuda")
    M_.keypoint_loss(lg, _t(np.full((R, K), -1, np.int32)), loss, grad, M_.keypoint_loss_workspace(R, "cuda"))
    assert float(loss) == 0.0 and not grad.view(torch.int16).any()
    loss.fill_(7.0)
    M_.keypoint_loss(lg[:0], _t(np.zeros((0, K), np.int32)), loss, grad[:0], M_.keypoint_loss_workspace(0, "cuda"))
    assert float(loss) == 0.0


def test_loss_final_sum_order_bit_exact(hip):
    """keypoint_loss_final_kernel's sum of the per-roi partials, bit for bit in its documented order: lane t of the one
    256-thread workgroup adds rows t, t + 256, ... ascending; each wave folds its 64 lanes by the descending tree (lane l
    takes lane l + 32, 16 .. 1); the four wave sums are ((w0 + w1) + w2) + w3; loss = k * sum. 300 rois (every wave
    contributes, 44 lanes hold two rows) whose cross-entropies run from about 1e-6 to 3e3, more than 2^24 apart, so that
    another association gives other bits (asserted on the reference). The partials are read back from the workspace."""
    import torch
    from mxdetection_amd.core import mask as M_
    R, S_in, Kpad, K = 300, 2, 8, 1
    a = np.concatenate([np.linspace(60.0, -30.0, 150), -np.geomspace(1.0, 3000.0, 150)]).astype(np.float32)
    a = a[np.random.default_rng(5).permutation(R)]
    logits = np.zeros((R, S_in, S_in, Kpad), np.float32)
    logits[:, 0, 0, 0] = a                                 # target 0 = the corner, whose upsampled value is the pixel's own
    lg, tgt = _t(logits, torch.bfloat16), _t(np.zeros((R, K), np.int32))
    ws = M_.keypoint_loss_workspace(R, "cuda")
    loss = torch.zeros((1,), device="cuda")
    grad = torch.empty((R, S_in, S_in, Kpad), dtype=torch.bfloat16, device="cuda")
    M_.keypoint_loss(lg, tgt, loss, grad, ws, LOSS_SCALE, WEIGHT)
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    nv = int(raw[:4].view(np.int32)[0])
    p = raw[256:256 + 4 * R].view(np.float32).copy()
    assert nv == R and np.isfinite(p).all() and p.min() > 0 and p.max() / p.min() > 2.0 ** 24
    f32 = np.float32
    lanes = np.zeros(256, f32)
    for r in range(R):
        lanes[r % 256] = f32(lanes[r % 256] + p[r])
    waves = []
    for w in range(4):
        x = lanes[64 * w:64 * w + 64].copy()
        off = 32
        while off > 0:
            x[:off] = x[:off] + x[off:2 * off]
            off >>= 1
        waves.append(x[0])
    total = f32(f32(f32(waves[0] + waves[1]) + waves[2]) + waves[3])
    k = f32(f32(f32(LOSS_SCALE) * f32(WEIGHT)) / f32(nv))
    want = f32(k * total)
    other = f32(0.0)
    for r in range(R):
        other = f32(other + p[r])
    assert other.view(np.uint32) != total.view(np.uint32), "the data does not make the summation order visible"
    got = loss.cpu().numpy()
    print("keypoint final sum %r want %r (row-order sum %r)" % (float(got[0]), float(want), float(f32(k * other))))
    assert got.view(np.uint32)[0] == want.view(np.uint32)


@pytest.mark.parametrize("S_in,Kpad,K", ref.SHAPES)
def test_decode_bit_exact(hip, S_in, Kpad, K):
    import torch
    from mxdetection_amd.core import mask as M_
    c = _case(S_in, Kpad, K)
    want = c["decoded"]
    assert (want[18, :, 0] == want[18, 0, 0]).all() and not want[14:17].any() and not want[13].any()     # tie row; padding
    whole, out = _guarded((ref.R_CASE, K, 3), torch.float32, 7.0)
    lg, dets = _t(c["logits"], torch.bfloat16), _t(c["dets"])
    M_.keypoint_decode(lg, dets, K, out=out)
    got = out.cpu().numpy()
    again = M_.keypoint_decode(lg, dets, K).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got != want)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)) and _guards_intact(whole, 7.0)
    # the constant map's tie goes to index 0: the centre of the first bin
    x1, y1, x2, y2 = c["dets"][18, :4]
    assert got[18, 0, 0] == np.float32(x1 + np.float32(0.5) * (np.float32(max(x2 - x1, 1.0)) / np.float32(2 * S_in)))
    assert M_.keypoint_decode(lg[:0], dets[:0], K).shape == (0, K, 3)
