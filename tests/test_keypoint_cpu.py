"""Keypoint R-CNN without a GPU: the reference restatement (tests/_keypoint_ref.py) against hand-computed answers and
float64 torch, the data path (flip, COCO file, synthetic roidb, loader), OKS / keypoint AP, the config keys, the builder's
refusals and the C-ABI's argument checks.

The gradient tolerance of tests/test_gpu_keypoint.py is measured here (test_gradient_tolerance_is_measured): the float32
restatement of the kernel's formula (ref.keypoint_loss_f32: fp32 upsample, mxdet_expf / mxdet_logf, fp32 sum, quotient and
adjoint in the kernel's tap order, before the bf16 rounding) against the float64 reference over the four shapes of the GPU
table, gradients divided by k. Measured maximum: 1.87e-07 (shape (14, 32, 17)); times 4, rounded up to a power of two:
ATOL_GRAD = 2^-20 = 9.5e-07. The bf16 rounding of the stored gradient is the relative term 2^-8 of the GPU test.
"""
import json
import math
import os

import numpy as np
import pytest

import _keypoint_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "coco_kpt_tiny.json")
ATOL_GRAD = 2.0 ** -20          # on gradients divided by k; see the module docstring
LOSS_RTOL = 3e-5                # fp32 fixed-order sum against float64
f32 = np.float32


def _one(roi, kp, label=1, matched=0, n=0, S_in=2):
    """One roi, one instance with the given keypoints [[x, y, v], ...] -> targets [K]."""
    rois = np.array([[n, *roi]], f32)
    gt = np.array([[kp]], f32)
    return ref.keypoint_target(rois, np.array([matched], np.int32), np.array([label], np.int32), gt, S_in)[0]


def test_targets_by_hand():
    """S_in = 2 -> a 4x4 grid. Roi (10, 20) - (18, 28): 8 pixels wide, 2 pixels per bin."""
    roi = (10, 20, 18, 28)
    # bin (by, bx) of (x, y): bx = floor((x - 10) * 4/8), by = floor((y - 20) * 4/8)
    assert _one(roi, [[10, 20, 2], [13.9, 20, 1], [14, 27.9, 2], [17.99, 24, 1]]).tolist() == [0, 1, 3 * 4 + 2, 2 * 4 + 3]
    # a keypoint ON x2 / y2 belongs to the last bin, not to bin S
    assert _one(roi, [[18, 20, 2], [10, 28, 2], [18, 28, 2]]).tolist() == [3, 12, 15]
    # one pixel outside the roi on either side, in x or in y: not trained
    assert _one(roi, [[19, 24, 2], [9, 24, 2], [14, 29, 2], [14, 19, 2]]).tolist() == [-1, -1, -1, -1]
    # v = 0: not labelled, whatever the coordinates
    assert _one(roi, [[14, 24, 0], [14, 24, 1]]).tolist() == [-1, 2 * 4 + 2]
    # a roi one pixel wide (x2 == x1): rw = max(0, 1) = 1; x == x2 -> the last bin; x = x1 + 0.25 -> bin 1; x1 + 1 is outside
    thin = (10, 20, 10, 28)
    assert _one(thin, [[10, 22, 2], [10.25, 22, 2], [11, 22, 2]]).tolist() == [4 + 3, 4 + 1, -1]
    # rows that read no keypoint memory: background / ignored label, unmatched, instance or image index outside the tensors
    kp = [[14, 24, 2]]
    assert _one(roi, kp).tolist() == [10]
    for kw in (dict(label=0), dict(label=-1), dict(matched=-1), dict(matched=1), dict(n=1), dict(n=-1)):
        assert _one(roi, kp, **kw).tolist() == [-1], kw


def test_upsample_rows_sum_to_one_and_match_torch():
    import torch
    for n in (1, 2, 7, 14, 28):
        A = ref.upsample_matrix(n)
        assert A.shape == (2 * n, n) and np.allclose(A.sum(1), 1.0, atol=0, rtol=0) and (A >= 0).all()
        assert np.allclose(A.sum(0), 2.0, atol=1e-15)                   # the adjoint spreads every output once
    rng = np.random.default_rng(0)
    for n in (2, 7, 14):
        x = rng.standard_normal((3, n, n))
        want = torch.nn.functional.interpolate(torch.from_numpy(x)[None], scale_factor=2, mode="bilinear", align_corners=False)[0]
        A = ref.upsample_matrix(n)
        assert np.allclose(A @ x @ A.T, want.numpy(), rtol=0, atol=1e-14)
        got = ref.upsample2(x.astype(f32))
        assert got.dtype == f32 and got.shape == (3, 2 * n, 2 * n)
        assert np.allclose(got, want.numpy(), rtol=0, atol=4e-6)          # a handful of fp32 roundings
    # the fp32 order of the convention, spelled out on one value: horizontal first, products rounded before the sum
    x = np.array([[1.1, 2.3], [3.7, 0.9]], f32)
    h0 = f32(f32(0.75) * x[0, 0]) + f32(f32(0.25) * x[0, 1])            # row 0, X = 1 (j = 0, neighbour 1)
    h1 = f32(f32(0.75) * x[1, 0]) + f32(f32(0.25) * x[1, 1])
    assert ref.upsample2(x)[1, 1] == f32(f32(0.75) * h0) + f32(f32(0.25) * h1)
    assert ref.upsample2(x)[0, 0] == x[0, 0] and ref.upsample2(x)[3, 3] == x[1, 1]      # corners replicate


def test_reference_loss_and_gradient_match_torch_autograd(oracle):
    import torch
    c = ref.case(oracle, 7, 8, 5)
    loss, grad, k = ref.keypoint_loss(c["logits"], c["targets"], loss_scale=2.0, weight=0.75)
    tg = c["targets"]
    nv = int((tg >= 0).sum())
    assert nv > 50 and abs(k - 1.5 / nv) < 1e-9
    x = torch.from_numpy(c["logits"].astype(np.float64)).requires_grad_(True)
    up = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
    rows, chans = np.nonzero(tg >= 0)
    sel = up[torch.from_numpy(rows), torch.from_numpy(chans)].reshape(len(rows), -1)
    want = torch.nn.functional.cross_entropy(sel, torch.from_numpy(tg[rows, chans].astype(np.int64)), reduction="sum") * k
    want.backward()
    # the reference's softmax input is the fp32 upsample (the convention), torch's the float64 one: ~1e-6 apart at |x| <= 60
    assert abs(loss - float(want.detach())) <= 1e-5 * float(want.detach())
    assert np.abs(grad - x.grad.numpy()).max() <= 2e-5 * k
    assert not grad[..., 5:].any() and not grad[..., :5][np.broadcast_to((tg < 0)[:, None, None, :], grad[..., :5].shape)].any()


def test_gradient_tolerance_is_measured(oracle):
    """See the module docstring: ATOL_GRAD is 4x the measured fp32-vs-float64 difference, rounded up to a power of two."""
    worst = 0.0
    for S_in, Kpad, K in ref.SHAPES:
        c = ref.case(oracle, S_in, Kpad, K)
        l64, g64, k = ref.keypoint_loss(c["logits"], c["targets"], 2.0, 0.75)
        l32, g32 = ref.keypoint_loss_f32(oracle, c["logits"], c["targets"], 2.0, 0.75)
        d = float(np.abs(g32.astype(np.float64) - g64).max()) / k
        print("shape", (S_in, Kpad, K), "max |g32 - g64| / k = %.3e" % d, "loss rel %.2e" % (abs(float(l32) - l64) / l64))
        worst = max(worst, d)
        assert abs(float(l32) - l64) <= LOSS_RTOL * l64
    assert worst > 0 and ATOL_GRAD == 2.0 ** math.ceil(math.log2(4.0 * worst)), worst


def test_decode_reference_by_hand():
    lg = np.zeros((2, 2, 2, 8), f32)
    lg[0, 1, 0, 0] = 4.0                         # channel 0: the peak at input (1, 0) -> upsampled rows 2..3, columns 0..1
    lg[0, :, :, 1] = 0.5                         # channel 1: constant -> the tie goes to index 0
    dets = np.array([[10, 20, 18, 36, 0.9, 1], [0, 0, 0, 0, 0, -1]], f32)
    out = ref.keypoint_decode(lg, dets, 2)
    # h[1][0] = 0.75*4 + 0.25*4 = 4 (column 0 replicates the edge), U[3][0] = 0.75*4 + 0.25*4 = 4 (so does row 3): index 12
    assert out[0, 0].tolist() == [10 + 0.5 * 2, 20 + 3.5 * 4, 4.0]
    assert out[0, 1].tolist() == [11.0, 22.0, 0.5] and not out[1].any()


def test_flip_swaps_pairs_and_twice_is_identity():
    from mxdetection_amd.process_data.transform import COCO_KEYPOINT_FLIP_PAIRS, transform_keypoints
    assert COCO_KEYPOINT_FLIP_PAIRS == ref.COCO_FLIP_PAIRS
    rng = np.random.default_rng(1)
    kp = np.zeros((3, 17, 3), f32)
    kp[..., 0] = rng.integers(0, 100, (3, 17))
    kp[..., 1] = rng.integers(0, 80, (3, 17))
    kp[..., 2] = rng.integers(0, 3, (3, 17))
    kp[kp[..., 2] == 0] = 0
    fl = transform_keypoints(kp, 1.0, True, 100)
    assert np.array_equal(fl, ref.flip_keypoints(kp, 100))
    lab = kp[0, 5, 2] > 0 or kp[0, 6, 2] > 0
    assert lab and np.array_equal(fl[0, 5], [99 - kp[0, 6, 0], kp[0, 6, 1], kp[0, 6, 2]] if kp[0, 6, 2] > 0 else [0, 0, 0])
    assert np.array_equal(fl[:, 0, 1:], kp[:, 0, 1:])                   # the nose has no partner
    assert not fl[fl[..., 2] == 0].any()                                # v = 0 rows stay zero (not w - 1)
    assert np.array_equal(transform_keypoints(fl, 1.0, True, 100), kp)
    # scale after the flip; no flip: only the scale; the input is not modified
    sc = transform_keypoints(kp, 1.5, True, 100)
    assert np.array_equal(sc[..., :2], fl[..., :2] * f32(1.5)) and np.array_equal(sc[..., 2], fl[..., 2])
    assert np.array_equal(transform_keypoints(kp, 2.0, False, 100)[..., :2], kp[..., :2] * 2)
    assert transform_keypoints(np.zeros((0, 17, 3), f32), 2.0, True, 100).shape == (0, 17, 3)
    five = transform_keypoints(kp[:, :5], 1.0, True, 100)               # K = 5: the pairs past K are skipped
    assert np.array_equal(five, fl[:, :5])


def test_coco_keypoint_file_parses():
    from mxdetection_amd.datasets import load_coco_roidb
    plain, names = load_coco_roidb(GOLDEN)
    roidb, names_k = load_coco_roidb(GOLDEN, with_keypoints=True)
    assert names == names_k == ["__background__", "person"] and len(roidb) == 2
    for a, b in zip(plain, roidb):                                      # every existing key exactly as it is
        assert "keypoints" not in a and set(b) == set(a) | {"keypoints"}
        for key in a:
            assert np.array_equal(a[key], b[key]) if isinstance(a[key], np.ndarray) else a[key] == b[key], key
    assert np.array_equal(roidb[0]["boxes"], np.array([[10, 8, 40, 28], [40, 20, 50, 30]], f32))       # the crowd is dropped
    want = np.zeros((2, 5, 3), f32)
    want[0] = [[20, 12, 2], [24, 10, 2], [16, 10, 1], [0, 0, 0], [13, 11, 2]]                            # v = 0 -> zeros
    assert roidb[0]["keypoints"].dtype == f32 and np.array_equal(roidb[0]["keypoints"], want)
    assert roidb[1]["keypoints"].shape == (1, 5, 3) and not roidb[1]["keypoints"].any()                  # no field: zeros
    with open(GOLDEN) as f:
        assert len(json.load(f)["annotations"]) == 4


def test_synthetic_roidb_unchanged_without_keypoints():
    from mxdetection_amd.datasets import synthetic_roidb
    a = synthetic_roidb(6, seed=3)
    b = synthetic_roidb(6, seed=3, num_keypoints=17)
    again = synthetic_roidb(6, seed=3, num_keypoints=17)
    for ea, eb, ec in zip(a, b, again):
        assert "keypoints" not in ea and set(eb) == set(ea) | {"keypoints"}
        for key in ea:
            assert np.array_equal(ea[key], eb[key]) if isinstance(ea[key], np.ndarray) else ea[key] == eb[key], key
        kp, bx = eb["keypoints"], eb["boxes"]
        assert kp.shape == (bx.shape[0], 17, 3) and kp.dtype == f32 and np.array_equal(kp, ec["keypoints"])
        cx, cy = 0.5 * (bx[:, 0] + bx[:, 2]), 0.5 * (bx[:, 1] + bx[:, 3])
        rx, ry = 0.5 * (bx[:, 2] - bx[:, 0]), 0.5 * (bx[:, 3] - bx[:, 1])
        inside = ((kp[..., 0] - cx[:, None]) / rx[:, None]) ** 2 + ((kp[..., 1] - cy[:, None]) / ry[:, None]) ** 2
        lab = kp[..., 2] > 0
        assert lab.any() and (~lab).any() and (inside[lab] <= 1.0).all() and not kp[~lab].any()
    # the first entry against figures recorded before the option existed
    e = synthetic_roidb(2, seed=0)[0]
    assert (e["height"], e["width"], e["boxes"].shape[0], e["seed"]) == (612, 612, 12, 0) and int(e["gt_classes"][0]) == 52


def test_loader_assembles_gt_keypoints():
    from mxdetection_amd.datasets import synthetic_roidb
    from mxdetection_amd.datasets.loader import DetectionLoader
    from mxdetection_amd.process_data import transform as T
    roidb = synthetic_roidb(4, seed=5, num_keypoints=5)
    roidb[1] = dict(roidb[1], flipped=True)
    ld = DetectionLoader(roidb, 2, device="cpu", g_max=20, with_keypoints=True, num_keypoints=5, shuffle=False)
    hb = ld.assemble([0, 1])
    assert hb.kp.shape == (2, 20, 5, 3) and hb.kp.dtype == f32
    for n in range(2):
        e = roidb[n]
        G = e["boxes"].shape[0]
        want = T.transform_keypoints(e["keypoints"], hb.scales[n], n == 1, e["width"])
        assert np.array_equal(hb.kp[n, :G], want) and not hb.kp[n, G:].any()
        lab = want[..., 2] > 0                                          # labelled points lie inside their transformed box
        bx = hb.gt[n, :G, :4]
        assert (want[..., 0][lab] >= np.broadcast_to(bx[:, None, 0], lab.shape)[lab] - 1).all()
        assert (want[..., 0][lab] <= np.broadcast_to(bx[:, None, 2], lab.shape)[lab] + 1).all()
    assert DetectionLoader(roidb, 2, device="cpu", g_max=20).assemble([0, 1]).kp is None


def _person(image_id, kp, area=100.0, **kw):
    xs, ys = [p[0] for p in kp], [p[1] for p in kp]
    return dict(image_id=image_id, category_id=1, keypoints=kp, area=area,
                bbox=[min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1], **kw)


def test_oks_and_keypoint_ap_by_hand():
    from mxdetection_amd.core.evaluation import COCO_KEYPOINT_SIGMAS, _oks, coco_keypoint_eval
    assert np.allclose(COCO_KEYPOINT_SIGMAS, ref.COCO_SIGMAS) and len(COCO_KEYPOINT_SIGMAS) == 17
    K = 17
    gk = [[10.0 + 2 * j, 20.0 + j, 2] for j in range(K)]
    gt = _person(1, gk)
    # a perfect match: OKS 1 at every threshold
    r = coco_keypoint_eval([gt], [_person(1, gk, score=0.9)])
    assert r["AP"] == pytest.approx(1.0) and r["AP50"] == pytest.approx(1.0) and r["AR"] == pytest.approx(1.0)
    # every keypoint displaced by d = 0.8 in x, uniform sigma 0.05, area 100: e = d^2 / (2 * 100 * (2*0.05)^2) = d^2 / 2,
    # OKS = exp(-0.32) = 0.726: a match at the thresholds 0.50 .. 0.70 (five of ten), none above
    dk = [[x + 0.8, y, 1] for x, y, _ in gk]
    sig = [0.05] * K
    o = _oks(np.array([dk], np.float64), np.array([gk], np.float64), np.array([gt["bbox"]], np.float64), np.array([100.0]), sig)
    assert o.shape == (1, 1) and o[0, 0] == pytest.approx(math.exp(-0.32), rel=1e-12)
    r = coco_keypoint_eval([gt], [_person(1, dk, score=0.9)], sigmas=sig)
    assert r["AP"] == pytest.approx(0.5) and r["AP50"] == pytest.approx(1.0) and r["AP75"] == pytest.approx(0.0)
    # with the published sigmas the same displacement: the mean over the keypoints of exp(-0.64 / (2 * 100 * (2 s_i)^2))
    want = np.mean(np.exp(-0.64 / (2 * 100.0 * (2 * ref.COCO_SIGMAS) ** 2)))
    o = _oks(np.array([dk], np.float64), np.array([gk], np.float64), np.array([gt["bbox"]], np.float64), np.array([100.0]),
             COCO_KEYPOINT_SIGMAS)
    assert o[0, 0] == pytest.approx(want, rel=1e-12)
    # only the labelled keypoints count: unlabel the displaced half, displace nothing else
    half = [[x, y, 2 if j % 2 else 0] for j, (x, y, _) in enumerate(gk)]
    dhalf = [[x + (0 if j % 2 else 50), y, 1] for j, (x, y, _) in enumerate(gk)]
    assert coco_keypoint_eval([_person(1, half)], [_person(1, dhalf, score=0.5)])["AP"] == pytest.approx(1.0)
    # a ground truth without a labelled keypoint is ignored: it is no miss, and a detection on it is no false positive
    none = _person(2, [[x, y, 0] for x, y, _ in gk])
    r = coco_keypoint_eval([gt, none], [_person(1, gk, score=0.5), _person(2, gk, score=0.9)])
    assert r["AP"] == pytest.approx(1.0) and r["AR"] == pytest.approx(1.0)
    # ... while the same detection far from everything is one, and outranks the true positive
    far = [[x + 500, y + 500, 1] for x, y, _ in gk]
    r = coco_keypoint_eval([gt, none], [_person(1, gk, score=0.5), _person(2, far, score=0.9)])
    assert r["AP"] == pytest.approx(0.5, abs=0.01) and r["AR"] == pytest.approx(1.0)


def test_detections_to_coco_keypoints():
    from mxdetection_amd.core.evaluation import detections_to_coco_keypoints
    dets = np.zeros((1, 2, 6), f32)
    dets[0, 0] = (10, 20, 30, 60, 0.8, 1)
    kp = np.zeros((1, 2, 3, 3), f32)
    kp[0, 0] = [[12, 22, 5.0], [20, 40, 1.0], [30, 60, -2.0]]
    out = detections_to_coco_keypoints(dets, np.array([1]), kp, [7], [2.0])
    assert len(out) == 1 and out[0]["image_id"] == 7 and out[0]["score"] == pytest.approx(0.8)
    assert out[0]["keypoints"] == [6.0, 11.0, 1.0, 10.0, 20.0, 1.0, 15.0, 30.0, 1.0]


def test_config_keys_and_file():
    from mxdetection_amd.utils import load_config
    cfg = load_config()
    assert cfg.network.keypoints == 0 and cfg.network.keypoint_weight == 1.0 and cfg.network.num_keypoints == 17
    a = load_config(os.path.join(ROOT, "configs", "keypoint_rcnn_r50_fpn.yaml"))     # only known keys load
    assert a.network.type == "faster_rcnn" and a.network.keypoints == 1 and a.network.num_keypoints == 17
    assert load_config(None, ["network.keypoints=1", "network.keypoint_weight=0.5"]).network.keypoint_weight == 0.5


def test_builder_and_model_validation():
    from mxdetection_amd.models import FasterRCNN
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils import load_config
    with pytest.raises(ValueError, match="keypoints.*retinanet has no RoI branch"):
        build_detector(load_config(None, ["network.type=retinanet", "network.keypoints=1"]), device="cpu")
    with pytest.raises(ValueError, match="network.keypoints must be 0 or 1"):
        build_detector(load_config(None, ["network.keypoints=2"]), device="cpu")
    # the model's own checks come before anything is allocated
    for kw, pat in ((dict(num_keypoints=0), "num_keypoints"), (dict(num_keypoints=33), "num_keypoints"),
                    (dict(num_keypoints=17.0), "num_keypoints"), (dict(keypoint_weight=0.0), "keypoint_weight"),
                    (dict(keypoint_weight=float("inf")), "keypoint_weight")):
        with pytest.raises(ValueError, match=pat):
            FasterRCNN("cpu", with_keypoints=True, **kw)


def test_abi_argument_checks():
    """Argument validation happens on the host before any launch: no GPU needed."""
    from mxdetection_amd import _lib
    lib = _lib.load()
    assert lib.mxdet_keypoint_loss_workspace_bytes(256) >= 256 * 4 + 4 and lib.mxdet_keypoint_loss_workspace_bytes(0) > 0
    assert lib.mxdet_keypoint_target(None, None, None, None, 4, 2, 8, 0, 28, None, None) == -2           # K = 0
    assert lib.mxdet_keypoint_target(None, None, None, None, 4, 2, 8, 17, 28, None, None) == -1
    assert lib.mxdet_keypoint_target(None, None, None, None, 0, 2, 8, 17, 28, None, None) == 0           # R = 0: no-op
    loss = (np.ctypeslib.ctypes.c_float * 1)()
    args = (1.0, 1.0, loss, None, None, 0, None)
    assert lib.mxdet_keypoint_loss(None, None, 4, 28, 30, 17, *args) == -2 and b"Kpad" in lib.mxdet_last_error()
    assert lib.mxdet_keypoint_loss(None, None, 4, 28, 32, 33, *args) == -2                               # K > Kpad
    assert lib.mxdet_keypoint_loss(None, None, 4, 33, 32, 17, *args) == -2 and b"S_in" in lib.mxdet_last_error()
    assert lib.mxdet_keypoint_loss(None, None, 4, 28, 48, 48, *args) == -2                               # LDS
    assert lib.mxdet_keypoint_loss(None, None, 4, 28, 32, 17, *args) == -1
    assert lib.mxdet_keypoint_loss(None, None, 4, 28, 32, 17, 1.0, 1.0, None, None, None, 0, None) == -1
    assert lib.mxdet_keypoint_decode(None, None, 4, 28, 32, 0, None, None) == -2
    assert lib.mxdet_keypoint_decode(None, None, 4, 28, 32, 17, None, None) == -1
    assert lib.mxdet_keypoint_decode(None, None, 0, 28, 32, 17, None, None) == 0
