"""ATSS assignment without a GPU: the numpy reference of tests/_atss_ref.py on a hand-computed case, its squared threshold
test against `v >= mean + std` in float64, the branches the two GPU fixtures are meant to exercise, and the config keys."""
import os

import numpy as np
import pytest

import _atss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = dict(ratios=(1.0,), scales_per_octave=1, anchor_scale=8.0)     # ATSS's published setting: one square anchor per cell
FIXTURES = {"S": (R.fixture_s, 64, 96), "M": (R.fixture_m, 256, 320)}


def _run(oracle, name, one, topk=9):
    make, H, W = FIXTURES[name]
    anchors, offs = R.pyramid_anchors(oracle, H, W, **(ONE if one else {}))
    return anchors, offs, R.atss_assign(oracle, anchors, offs, make(), topk)


def test_hand_computed_case(oracle):
    """One level of 3 x 3 cells of stride 8, one 8 x 8 anchor per cell: anchor i = y*3 + x is [8x, 8y, 8x+7, 8y+7], centre
    (8x+3.5, 8y+3.5). GT [8, 8, 19, 15] (12 x 8 px), centre (13.5, 11.5). Squared distances: anchor 4 (11.5, 11.5): 4;
    anchor 5 (19.5, 11.5): 36; anchors 1 and 7 (11.5, 3.5 / 19.5): 4 + 64 = 68 -- a tie at the cut, which goes to anchor 1;
    anchor 3: 100. k = 3: candidates {1, 4, 5}.
    IoU: anchor 1 covers rows 0..7, the GT rows 8..15: 0. Anchor 4 lies inside the GT: 64 / 96 = 2/3. Anchor 5 shares the
    columns 16..19: 32 / (64 + 96 - 32) = 1/4. mean = 11/36; deviations -11/36, 13/36, -2/36: ss = 294/1296,
    var = ss / 2 = 147/1296. Anchor 4: 169/1296 >= 147/1296 and 2/3 >= mean: above; its centre is 3.5 px inside the
    nearest GT edge: positive. Anchor 5 is below the mean. Anchor 1 is below the mean (and outside)."""
    anchors = np.array([[8 * x, 8 * y, 8 * x + 7, 8 * y + 7] for y in range(3) for x in range(3)], np.float32)
    gt = np.array([[[8, 8, 19, 15, 4]]], np.float32)
    labels, matched, targets, miou, info = R.atss_assign(oracle, anchors, [0, 9], gt, 3)
    r = info[(0, 0)]
    assert r["cand"].tolist() == [1, 4, 5] and r["tie_at_cut"] == [True] and r["short"] == [False]
    assert r["v"].tolist() == [0.0, np.float32(64.0) / np.float32(96.0), 0.25]
    assert abs(float(r["mean"]) - 11.0 / 36.0) < 1e-7 and abs(float(r["var"]) - 147.0 / 1296.0) < 1e-7
    assert r["pos"].tolist() == [False, True, False]
    assert labels.tolist() == [[0, 0, 0, 0, 1, 0, 0, 0, 0]] and matched.tolist() == [[-1, -1, -1, -1, 0, -1, -1, -1, -1]]
    assert miou[0, 4] == r["v"][1] and not np.delete(miou[0], 4).any()
    # encode: centre shift (13.5 - 11.5) / 8, same centre row, log(12 / 8), log(8 / 8)
    assert np.allclose(targets[0, 4], [0.25, 0.0, np.log(1.5), 0.0], atol=1e-6) and not np.delete(targets[0], 4, 0).any()
    # k larger than the level: every anchor is a candidate
    assert R.atss_assign(oracle, anchors, [0, 9], gt, 16)[4][(0, 0)]["cand"].tolist() == list(range(9))


@pytest.mark.parametrize("name", ["S", "M"])
@pytest.mark.parametrize("one", [False, True], ids=["9", "1"])
def test_squared_threshold_agrees_with_fp64(oracle, name, one):
    """(v >= mean) and (v - mean)^2 >= var in float32 is v >= mean + sqrt(var) evaluated in float64 on the float32 IoUs,
    except within 1e-6 of the threshold."""
    _, _, (_, _, _, _, info) = _run(oracle, name, one)
    checked = 0
    for r in info.values():
        v = r["v"].astype(np.float64)
        thr = v.mean() + (np.sqrt(v.var(ddof=1)) if len(v) > 1 else 0.0)
        t = (r["v"] - r["mean"]).astype(np.float32)
        squared = (r["v"] >= r["mean"]) & ((t * t).astype(np.float32) >= r["var"])
        near = np.abs(v - thr) < 1e-6
        assert np.array_equal(squared[~near], (v >= thr)[~near])
        checked += int((~near).sum())
    assert checked > 100


def test_fixture_s_exercises_its_branches(oracle):
    for one in (False, True):
        anchors, offs, (labels, matched, _, _, info) = _run(oracle, "S", one)
        c = R.branch_counts(info, labels, offs)
        assert anchors.shape[0] == (129 if one else 1161)
        assert c["gts"] == 6 and c["ties_at_cut"] >= 1 and c["multi_gt_anchors"] >= 1 and c["gts_without_positives"] >= 1
        assert c["positives"] >= 1 and not labels[1].any() and np.all(matched[1] == -1)      # image 1: no valid GT
        assert not info[(0, 5)]["pos"].any()                     # the 2 x 2 px box: no anchor centre inside
        assert (c["short_levels"] >= 1) == one                   # one anchor per cell: P5..P7 hold 6, 2 and 1 < k
        # rows 2 and 3 are the same box: every anchor both want goes to row 2
        both = info[(0, 2)]["cand"][info[(0, 2)]["pos"]]
        assert both.size and np.array_equal(both, info[(0, 3)]["cand"][info[(0, 3)]["pos"]]) and not (matched[0] == 3).any()
        assert labels.min() == 0 and labels.max() == 1


def test_fixture_m_exercises_its_branches(oracle):
    for one in (False, True):
        anchors, offs, (labels, _, _, _, info) = _run(oracle, "M", one)
        c = R.branch_counts(info, labels, offs)
        assert anchors.shape[0] == (1706 if one else 15354) and offs[1] == (1280 if one else 11520)   # P3: several passes
        assert c["gts"] == 52 and c["multi_gt_anchors"] >= 1 and c["levels_with_positives"] >= 3
        assert labels[0].any() and labels[1].any()


def test_config_keys_and_builder_errors():
    from mxdetection_amd.models.builder import build_detector
    from mxdetection_amd.models.retinanet import check_anchor_setting
    from mxdetection_amd.models.rpn_heads.retina_head import check_assigner
    from mxdetection_amd.utils.config import default_config, load_config
    net = default_config().network
    assert (net.assigner, net.atss_topk, net.anchor_ratios, net.anchor_scales_per_octave, net.anchor_scale) == \
        ("max_iou", 9, [0.5, 1.0, 2.0], 3, 4.0)
    # the defaults are the head's constructor defaults, bit for bit
    ratios, octave = check_anchor_setting(net.anchor_ratios, net.anchor_scales_per_octave, net.anchor_scale)
    assert ratios == (0.5, 1.0, 2.0) and octave == (1.0, 2.0 ** (1.0 / 3.0), 2.0 ** (2.0 / 3.0))
    cfg = load_config(os.path.join(ROOT, "configs", "retinanet_r101_fpn_atss.yaml"))
    net = cfg.network
    assert (net.type, net.assigner, net.atss_topk, net.anchor_ratios, net.anchor_scales_per_octave, net.anchor_scale) == \
        ("retinanet", "atss", 9, [1.0], 1, 8.0)
    assert (net.reg_loss, net.reg_loss_weight, net.backbone_depth) == ("giou", 2.0, 101)
    assert check_anchor_setting(net.anchor_ratios, net.anchor_scales_per_octave, net.anchor_scale) == ((1.0,), (1.0,))
    for bad in ("ATSS", "", None):
        with pytest.raises(ValueError, match="assigner"):
            check_assigner(bad)
    for bad in (0, 17, 9.0, True):
        with pytest.raises(ValueError, match="atss_topk"):
            check_assigner("atss", bad)
    with pytest.raises(ValueError, match="anchor_ratios"):
        check_anchor_setting([], 1, 8.0)
    with pytest.raises(ValueError, match="anchor_scales_per_octave"):
        check_anchor_setting([1.0], 0, 8.0)
    # the RPN keeps its sampler: raised before any model (or device) is touched
    for typ in ("faster_rcnn", "mask_rcnn"):
        cfg = load_config(None, ["network.type=" + typ, "network.assigner=atss"])
        with pytest.raises(ValueError, match="network.assigner"):
            build_detector(cfg, device="cpu")
    with pytest.raises(KeyError):
        load_config(None, ["network.atss_k=9"])


def test_host_argument_checks_need_no_device():
    """Every violation is caught by the host check before any launch: the code and a message naming the argument."""
    import ctypes as C
    from mxdetection_amd import _lib
    lib = _lib.load()
    assert lib.mxdet_atss_assign_workspace_bytes(2, 1000, 8) >= 2 * 1000 * 8
    assert lib.mxdet_atss_assign_workspace_bytes(0, 1000, 8) == 0
    p = C.c_void_p(256)      # never dereferenced

    def call(offs, A=10, L=None, topk=9, labels=p, ws=p, ws_bytes=1 << 20, N=1, G=4):
        arr = (C.c_int64 * len(offs))(*offs)
        rc = lib.mxdet_atss_assign(p, A, arr, len(offs) - 1 if L is None else L, p, N, G, topk, labels, p, p, None, ws, ws_bytes,
                                   None)
        return rc, lib.mxdet_last_error()

    for topk in (0, 17):
        rc, msg = call([0, 6, 10], topk=topk)
        assert rc == -1 and b"topk" in msg
    rc, msg = call([0, 6, 4, 10])
    assert rc == -2 and b"level_offsets" in msg and b"ascending" in msg
    rc, msg = call([0, 6, 6, 10])                       # an empty level
    assert rc == -2 and b"level_offsets" in msg
    rc, msg = call([0, 6, 9])
    assert rc == -2 and b"A_total" in msg
    rc, msg = call([0, 10], L=9)
    assert rc == -2 and b"L " in msg
    rc, msg = call([0, 6, 10], labels=None)
    assert rc == -1 and b"null output" in msg
    rc, msg = call([0, 6, 10], ws_bytes=8)
    assert rc == -3 and b"workspace" in msg
    rc, msg = call([0, 6, 10], G=2000)
    assert rc == -2 and b"G_max" in msg
