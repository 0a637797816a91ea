"""CARAFE without a GPU: known answers of the fp64 reference (tests/_carafe_ref.py), its autograd backward against an explicit
gather-form restatement of dX / dM (the form the kernels use), and the option checks of the models, builder and config."""
import os

import pytest
import torch

import _carafe_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2
CROPS = ((0, 0), (0, 1), (1, 0), (1, 1))


@pytest.mark.parametrize("k", (3, 5))
def test_zero_logits_give_the_zero_padded_box_mean(k):
    H, W, C = 5, 4, 8
    x, _, _, _ = ref.random_case(N, H, W, C, k, (2 * H, 2 * W), seed=k)
    y = ref.forward(x, torch.zeros((N, H, W, 4 * k * k), dtype=ref.F64), k, (2 * H - 1, 2 * W))
    r = k // 2
    mean = sum(ref.shift(x, a - r, b - r) for a in range(k) for b in range(k)) / (k * k)
    assert float((y - ref.nearest_up(mean, (2 * H - 1, 2 * W))).abs().max()) < 1e-14


@pytest.mark.parametrize("k", (3, 5))
def test_one_hot_tap_shifts_and_the_centre_is_nearest_upsampling(k):
    H, W, C = 4, 6, 8
    r = k // 2
    x, _, _, _ = ref.random_case(N, H, W, C, k, (2 * H, 2 * W), seed=10 + k)
    for tap in range(k * k):
        y = ref.forward(x, ref.one_hot_logits(N, H, W, k, tap), k, (2 * H, 2 * W - 1))
        want = ref.nearest_up(ref.shift(x, tap // k - r, tap % k - r), (2 * H, 2 * W - 1))
        assert float((y - want).abs().max()) < 1e-40, tap      # the other taps weigh e^-100 each
    y = ref.forward(x, ref.one_hot_logits(N, H, W, k, (k * k) // 2), k, (2 * H, 2 * W))
    assert torch.equal(ref.round_bf16(y), ref.nearest_up(x, (2 * H, 2 * W)))


@pytest.mark.parametrize("k", (3, 5))
@pytest.mark.parametrize("hw", ((1, 1), (2, 3), (5, 4)))
def test_gather_form_agrees_with_autograd(hw, k):
    H, W = hw
    for cy, cx in CROPS:
        out_hw = (2 * H - cy, 2 * W - cx)
        x, m, d_out, _ = ref.random_case(N, H, W, 16, k, out_hw, seed=100 * H + 10 * W + k)
        dx, dm = ref.backward(x, m, d_out, k)
        gx, gm = ref.backward_gather(x, m, d_out, k)
        assert float((dx - gx).abs().max()) <= 1e-12 and float((dm - gm).abs().max()) <= 1e-12
        # a cropped sub-position has no gradient
        gm = gm.reshape(N, H, W, k * k, 4)
        if cy:
            assert not gm[:, H - 1, :, :, 2:].any()
        if cx:
            assert not gm[:, :, W - 1, :, 1::2].any()


def test_option_checks_refuse_bad_values():
    from mxdetection_amd.models import FasterRCNN, RetinaNet
    from mxdetection_amd.models.necks import check_upsample
    check_upsample("carafe", 3, 128, 1)
    for kw, what in ((dict(carafe_k=4), "carafe_k"), (dict(carafe_compress=96), "carafe_compress"),
                     (dict(carafe_enc_kernel=2), "carafe_enc_kernel"), (dict(fpn_upsample="bilinear"), "fpn_upsample")):
        with pytest.raises(ValueError, match=what):          # before anything is allocated: no device is touched
            FasterRCNN("cuda", **dict(dict(fpn_upsample="carafe"), **kw))
    with pytest.raises(ValueError, match="RetinaFPN"):
        RetinaNet("cuda", fpn_upsample="carafe")


def test_config_parses_and_the_builder_refuses_retinanet():
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.utils.config import load_config
    cfg = load_config(os.path.join(ROOT, "configs", "faster_rcnn_r50_fpn_carafe.yaml"))
    net = cfg.network
    assert (net.type, net.fpn_upsample, net.carafe_k, net.carafe_compress, net.carafe_enc_kernel) == \
        ("faster_rcnn", "carafe", 5, 64, 3)
    plain = load_config(os.path.join(ROOT, "configs", "faster_rcnn_r50_fpn.yaml"))
    assert plain.network.fpn_upsample == "nearest"
    bad = load_config(os.path.join(ROOT, "configs", "retinanet_r101_fpn.yaml"), ["network.fpn_upsample=carafe"])
    with pytest.raises(ValueError, match="fpn_upsample"):
        build_detector(bad, "cuda")
    bad = load_config(os.path.join(ROOT, "configs", "faster_rcnn_r50_fpn_carafe.yaml"), ["network.carafe_k=4"])
    with pytest.raises(ValueError, match="carafe_k"):
        build_detector(bad, "cuda")


def test_bindings_refuse_bad_descriptors_on_the_host():
    """The argument checks run before any launch: no GPU needed."""
    import ctypes as C
    from mxdetection_amd import _lib
    lib = _lib.load()
    d = _lib.CarafeDescT()
    d.N, d.H, d.W, d.C, d.Cm, d.k, d.Hf, d.Wf = 2, 4, 4, 12, 128, 5, 8, 8
    assert lib.mxdet_carafe_fwd(C.byref(d), None, None, None, None) == -2 and b"multiple of 8" in lib.mxdet_last_error()
    d.C, d.k = 16, 4
    assert lib.mxdet_carafe_bwd(C.byref(d), None, None, None, None, None, 0, None) == -2 and b"3 or 5" in lib.mxdet_last_error()
