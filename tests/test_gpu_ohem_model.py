"""ohem=True in the assembled Faster R-CNN, at the small shapes of tests/test_gpu_iou_loss_model.py with 64 RoIs per image, so
that the pool (320 rows) exceeds them: the head's training RoIs are tests/_ohem_ref.py's selection from the pool and the scores
the step left on the device; the training pass behind the sampler is the unchanged code (a default model fed the same selection
gives the same bits); replayed steps reproduce eager ones with new ground truth; inference and the initial weights do not depend
on the option; the default model never reaches the new entries; one step each with the mask branches and with the GN head on
deformable RoI pooling."""
import functools

import numpy as np
import pytest

import _ohem_ref as ref
from test_gpu_gn_heads import _inputs

pytestmark = pytest.mark.gpu

N, H, W = 2, 256, 320
KW = dict(seed=7, pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=64)
POOL = 320            # round_up(300 proposals + 16 ground-truth slots, 64)


@functools.lru_cache(maxsize=None)
def _model(ohem):
    from mxdetection_amd.models import FasterRCNN
    return FasterRCNN("cuda", **KW, ohem=ohem)


@functools.lru_cache(maxsize=None)
def _ohem_step():
    """One eager OHEM step (step 2, inputs of seed 1); returns its losses, a copy of the gradient arena and copies of the
    selection the head trained on."""
    import torch
    m = _model(True)
    image, gt, im_info = _inputs(N, H, W, seed=1)
    losses = torch.cat(list(m.forward_backward(image, gt, im_info, step=2))).clone()
    torch.cuda.synchronize()
    h = m.bbox_head
    return losses, m.arena.g.clone(), [t.clone() for t in (h.rois, h.labels, h.tgt, h.wgt, h.matched, h.num_fg)]


def _np(t):
    return None if t is None else t.cpu().numpy()


def test_training_rois_are_the_reference_selection(hip):
    import torch
    image, gt, im_info = _inputs(N, H, W, seed=1)
    _model(True).forward_backward(image, gt, im_info, step=2)
    torch.cuda.synchronize()
    h = _model(True).bbox_head
    R = KW["rois_per_image"]
    assert h.ohem and h.ohem_nms == 0.7 and h.pool_labels.shape == (N, POOL) and h.ohem_score.shape == (N, POOL)
    score, labels, rois = _np(h.ohem_score), _np(h.pool_labels), _np(h.pool_rois)
    matched, tgt, wgt = _np(h.pool_matched), _np(h.pool_tgt), _np(h.pool_wgt)
    cand = (labels >= 0).sum(1)
    assert (cand > R).all() and (score[labels < 0] == -1).all() and (score[labels >= 0] > 0).all()
    # the pool is every candidate, foreground first, then background, then padding
    for n in range(N):
        nfg = int((labels[n] > 0).sum())
        assert (labels[n, :nfg] > 0).all() and (labels[n, nfg:cand[n]] == 0).all() and (labels[n, cand[n]:] == -1).all()
        assert int(h.pool_num_fg[n]) == nfg
    sel, num_sel, num_fg, sup = ref.select(score, labels, rois, R, 0.7)
    # (the proposals left the RPN's own NMS at 0.7, so the dedup at 0.7 finds little here: test_ohem_with_an_iou_loss runs at 0.5)
    assert (num_sel == R).all() and num_fg.sum() >= 8
    assert np.array_equal(_np(h.ohem_sel), sel) and np.array_equal(_np(h.num_fg), num_fg)
    want = ref.gather(sel, rois, labels, matched, tgt, wgt)
    for name, got, w in zip(("rois", "labels", "tgt", "wgt", "matched"), (h.rois, h.labels, h.tgt, h.wgt, h.matched), want):
        assert np.array_equal(_np(got), w), name
    assert h.rois.shape == (N, R, 5) and h.o.shape[0] == N * R           # the training pass ran on the chosen rows
    # hard examples: the chosen rows' mean score is above the pool's
    chosen = np.concatenate([score[n, sel[n]] for n in range(N)])
    assert chosen.mean() > score[labels >= 0].mean()
    assert torch.isfinite(_model(True).arena.g).all()


def test_an_ohem_step_does_not_depend_on_the_sampling_seed(hip):
    """The pool is every candidate: the Philox keys of proposal-target decide nothing. (The RPN's own sampler keeps its seed.)"""
    import torch
    h = _model(True).bbox_head
    image, gt, im_info = _inputs(N, H, W, seed=1)
    _model(True).forward_backward(image, gt, im_info, step=2)
    torch.cuda.synchronize()
    before = [t.clone() for t in (h.rois, h.labels, h.matched, h.ohem_sel)]
    seed = h.seed
    try:
        h.seed = seed + 12345
        _model(True).forward_backward(image, gt, im_info, step=2)
        torch.cuda.synchronize()
    finally:
        h.seed = seed
    for a, b in zip(before, (h.rois, h.labels, h.matched, h.ohem_sel)):
        assert torch.equal(a, b)


def test_the_training_pass_is_the_unchanged_code(hip, monkeypatch):
    """A default model whose sampler is replaced by the OHEM model's selection: the same losses and gradients, bit for bit."""
    import torch
    l_ohem, g_ohem, chosen = _ohem_step()
    m = _model(False)
    assert torch.equal(m.arena.w, _model(True).arena.w) and m.arena.size == _model(True).arena.size
    h = m.bbox_head
    assert not h.ohem

    def fake_sample(rois, num_rois, gt_boxes, step, image_offset, step_dev=None, feats=None):
        h.rois, h.labels, h.tgt, h.wgt, h.matched, h.num_fg = chosen
        h.gt_boxes = gt_boxes
        return h.rois.view(-1, 5)

    monkeypatch.setattr(h, "sample", fake_sample)
    image, gt, im_info = _inputs(N, H, W, seed=1)
    l_def = torch.cat(list(m.forward_backward(image, gt, im_info, step=2))).clone()
    torch.cuda.synchronize()
    assert torch.equal(l_def, l_ohem), (l_def, l_ohem)
    assert torch.equal(m.arena.g, g_ohem)


def test_replayed_steps_reproduce_eager_ones(hip):
    """capture + three replays with two different ground truths: the selection happens on the device, inside the graph."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, gt_a, im_info = _inputs(N, H, W, seed=2)
    _, gt_b, _ = _inputs(N, H, W, seed=3)
    assert not torch.equal(gt_a, gt_b)
    eager = _model(True)
    want, sels = [], []
    for gt in (gt_a, gt_b):
        want.append(torch.cat(list(eager.forward_backward(image, gt, im_info, step=4))).clone())
        sels.append(eager.bbox_head.ohem_sel.clone())
    torch.cuda.synchronize()
    assert not torch.allclose(want[0], want[1], rtol=1e-3) and not torch.equal(sels[0], sels[1])
    m = FasterRCNN("cuda", **KW, ohem=True)
    m.capture(image, gt_a, im_info, lr=0.0, image_offset=0, warmup=1)
    for gt, w, s in zip((gt_a, gt_b, gt_a), want + want[:1], sels + sels[:1]):
        got = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
        torch.cuda.synchronize()
        assert torch.allclose(got, w, rtol=1e-4, atol=1e-5), (got, w)
        assert torch.equal(m.bbox_head.ohem_sel, s)


def test_predict_and_initial_weights_do_not_depend_on_ohem(hip):
    import torch
    from mxdetection_amd.models import FasterRCNN
    image, _, im_info = _inputs(N, H, W, seed=5)
    outs = []
    for ohem in (False, True):
        m = _model(ohem)
        dets, num = m.predict(image, im_info, score_thresh=0.0)
        torch.cuda.synchronize()
        outs.append((dets.clone(), num.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(_model(False).arena.w, _model(True).arena.w)
    assert torch.equal(FasterRCNN("cuda", **KW, ohem=True, ohem_nms=1.0).arena.w, _model(False).arena.w)


def test_default_model_never_calls_the_new_bindings(hip, monkeypatch):
    import torch
    from mxdetection_amd.core import bbox as B
    from mxdetection_amd.core import loss as L
    calls = []
    for mod, name in ((B, "ohem_select"), (B, "ohem_gather"), (B, "ohem_select_workspace"), (L, "ohem_roi_score")):
        fn = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, _fn=fn, _name=name, **k: calls.append(_name) or _fn(*a, **k))
    image, gt, im_info = _inputs(N, H, W, seed=1)
    _model(False).forward_backward(image, gt, im_info, step=1)
    torch.cuda.synchronize()
    assert calls == []
    _model(True).forward_backward(image, gt, im_info, step=1)
    torch.cuda.synchronize()
    assert calls.count("ohem_roi_score") == 1 and calls.count("ohem_select") == 1 and calls.count("ohem_gather") == 1


@pytest.mark.parametrize("reg_loss", ["giou"])
def test_ohem_with_an_iou_loss(hip, reg_loss):
    """The score is the IoU-family entry's, the gather skips targets and weights (nothing reads them), and at ohem_nms = 0.5 --
    below the RPN's own 0.7 -- the dedup removes candidates."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    m = FasterRCNN("cuda", **KW, ohem=True, ohem_nms=0.5, reg_loss=reg_loss, reg_loss_weight=10.0)
    image, gt, im_info = _inputs(N, H, W, seed=1)
    losses = torch.cat(list(m.forward_backward(image, gt, im_info, step=2)))
    torch.cuda.synchronize()
    h = m.bbox_head
    assert h.tgt is None and h.wgt is None and torch.isfinite(losses).all() and torch.isfinite(m.arena.g).all()
    score, labels, rois = _np(h.ohem_score), _np(h.pool_labels), _np(h.pool_rois)
    sel, num_sel, num_fg, sup = ref.select(score, labels, rois, KW["rois_per_image"], 0.5)
    print("ohem giou model: num_sel %s num_fg %s suppressed %s" % (num_sel, num_fg, sup))
    assert (num_sel == KW["rois_per_image"]).all() and sup.sum() >= 1
    assert np.array_equal(_np(h.ohem_sel), sel) and np.array_equal(_np(h.num_fg), num_fg)
    want = ref.gather(sel, rois, labels, _np(h.pool_matched))
    assert np.array_equal(_np(h.rois), want[0]) and np.array_equal(_np(h.labels), want[1]) and np.array_equal(_np(h.matched), want[4])
    assert losses[3] > 0          # the box regression loss of the chosen foreground rows


# mask-scoring: 32 RoIs per image, so that the mask branch's 8 per image are fewer than the ~10 foreground candidates these
# small inputs give an untrained RPN (the pool still exceeds the RoIs tenfold)
@pytest.mark.parametrize("kw", [dict(with_mask=True, mask_iou=True, rois_per_image=32),
                                dict(bbox_head="4conv1fc", head_norm="gn", roi_pool="mdpool")], ids=["mask-scoring", "gn-head-mdpool"])
def test_one_step_with_the_other_options(hip, kw):
    import torch
    from mxdetection_amd.models import FasterRCNN
    m = FasterRCNN("cuda", **dict(KW, ohem=True, **kw))
    masks = kw.get("with_mask", False)
    inp = _inputs(N, H, W, seed=1, masks=masks)
    losses = m.forward_backward(*inp[:3], step=0, gt_masks=inp[3] if masks else None)
    torch.cuda.synchronize()
    assert len(losses) == (4 if masks else 2)
    assert torch.isfinite(torch.cat(list(losses))).all() and torch.isfinite(m.arena.g).all()
    assert m.export_grads()["bbox.fc_out.weight"].abs().sum().item() > 0
    h = m.bbox_head
    R = h.R
    labels, num_fg = _np(h.labels), _np(h.num_fg)
    assert labels.shape == (N, R) and (_np(h.ohem_num_sel) == R).all()
    for n in range(N):        # foreground first: what FCNMaskHead.select_rois relies on
        assert (labels[n, :num_fg[n]] > 0).all() and (labels[n, num_fg[n]:] <= 0).all()
    if masks:
        k = m.mask_head.Rimg
        assert k == R // 4 and (num_fg >= k).all(), num_fg
        assert bool((m.mask_head.roi_labels > 0).all())                  # mask RoIs all foreground
