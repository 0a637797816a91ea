"""RetinaNet with gradient-harmonized losses (GHM-C / GHM-R) at the small shape of tests/test_gpu_retinanet.py
(128 x 192, ResNet-50, nine anchors per cell, max-IoU assigner): a training step whose two losses are the float64 reference
(tests/_ghm_ref.py) evaluated on the head's own outputs from a fresh state, ghm="none" with its keywords spelled out being the default-constructed model bit for bit,
"cls" / "reg" leaving the other loss word untouched, a captured step replayed with new ground truth (stateless and with the
published momenta), and a checkpoint round trip into a plain model."""
import functools

import numpy as np
import pytest

import _ghm_ref as G
import test_ghm_cases_cpu as GT
from test_gpu_gn_heads import _inputs

pytestmark = pytest.mark.gpu

N, H, W = 2, 128, 192
STATELESS = dict(ghm_cls_momentum=0.0, ghm_reg_momentum=0.0)


@functools.lru_cache(maxsize=None)
def _model(ghm, stateless=False, seed=7):
    from mxdetection_amd.models import RetinaNet
    kw = {} if ghm is None else {"ghm": ghm}
    return RetinaNet("cuda", depth=50, seed=seed, **kw, **(STATELESS if stateless else {}))


def _ref_on_head_outputs(h, acc_c, acc_r):
    levels = [dict(cls=co.float().cpu().numpy(), reg=bo.float().cpu().numpy(), A=h.A, C=h.Cn, off=h.level_offsets[l])
              for l, (co, bo) in enumerate(zip(h.co, h.bo))]
    return G.ref_step(levels, h.cls_labels.cpu().numpy(), h.at_out[2].cpu().numpy(), h.ghm, h.ghm_cfg, acc_c, acc_r)


def test_ghm_training_step(hip):
    import torch
    m = _model("both")
    h = m.head
    assert h.ghm == "both" and h.ghm_cfg == GT.PUBLISHED and (h.A, h.Cn, h.ld_cls, h.ld_reg) == (9, 80, 768, 64)
    image, gt, im_info = _inputs(N, H, W, seed=1)
    m.plan(N, H, W, gt.shape[1])
    m.ghm_reset()
    (loss,) = m.forward_backward(image, gt, im_info, step=0)
    torch.cuda.synchronize()
    nfg = int(h.num_fg.item())
    assert nfg >= 8
    acc_c, acc_r = np.zeros(30), np.zeros(10)
    ref = _ref_on_head_outputs(h, acc_c, acc_r)
    cnt, coef = h.ghm_cnt.cpu().numpy(), h.ghm_coef.cpu().numpy()
    print("class bins", cnt[:30].tolist(), "box bins", cnt[30:].tolist())
    assert int(cnt[30:].sum()) == 4 * nfg and int(cnt[:30].sum()) == 80 * int((h.cls_labels >= 0).sum())
    assert np.array_equal(cnt[:30], ref["cnt_c"]) and np.array_equal(cnt[30:], ref["cnt_r"])
    assert GT.coef_ok("model class", coef[:30], ref["coef_c"]) and GT.coef_ok("model box", coef[30:], ref["coef_r"])
    assert np.all(np.abs(h.ghm_acc.cpu().numpy() - np.concatenate([acc_c, acc_r])) <= 4 * GT.ulp32(np.concatenate([acc_c, acc_r])))
    got = loss.cpu().numpy()
    for k, name, w, atol in ((0, "c", 1.0, GT.ATOL_CLS_LOSS), (1, "r", 10.0, GT.ATOL_REG_LOSS)):
        want = sum(o["loss_" + name] for o in ref["levels"])
        wsum = sum(o["wsum_" + name] for o in ref["levels"])
        bound = GT.LOSS_RTOL * abs(want) + w * wsum * atol
        print("ghm %s loss: got %.9g ref %.9g |diff| %.3e (bound %.3e)" % (name, got[k], want, abs(got[k] - want), bound))
        assert abs(got[k] - want) <= bound and got[k] > 0
    assert np.all(np.isfinite(got)) and torch.isfinite(m.arena.g).all()
    grads = m.export_grads()
    for name in ("retina.cls_out.weight", "retina.box_out.weight", "retina.cls0.weight", "retina.box0.weight"):
        assert torch.isfinite(grads[name]).all() and grads[name].abs().sum().item() > 0, name


def test_ghm_none_is_todays_model(hip):
    """ghm="none" with every ghm_* keyword spelled out against a default-constructed model of the same tree: both take the
    plain branch of loss_and_grad, so this shows that the keywords are inert and that nothing is allocated for them -- not
    that the model equals the parent commit's. The evidence for that is outside the suite: the level entry timed beside the
    parent's library and the default benchmark's equal last-step losses."""
    import torch
    from mxdetection_amd.models import RetinaNet
    image, gt, im_info = _inputs(N, H, W, seed=1)
    a = _model(None)
    b = RetinaNet("cuda", depth=50, seed=7, ghm="none", **{"ghm_" + k: v for k, v in GT.PUBLISHED.items()})
    assert a.head.ghm == b.head.ghm == "none" and not hasattr(b.head, "ghm_acc")
    la = a.forward_backward(image, gt, im_info, step=0)[0].clone()
    lb = b.forward_backward(image, gt, im_info, step=0)[0].clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(a.arena.g, b.arena.g)
    ga, gb = a.export_grads(), b.export_grads()
    assert list(ga) == list(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    b.ghm_reset()                                                        # nothing to reset: no error


def test_ghm_cls_and_reg_leave_the_other_loss_word_alone(hip):
    import torch
    image, gt, im_info = _inputs(N, H, W, seed=1)
    out = {}
    for k in (None, "cls", "reg", "both"):
        m = _model(k)
        m.ghm_reset()
        out[k] = m.forward_backward(image, gt, im_info, step=0)[0].clone()
    torch.cuda.synchronize()
    assert torch.equal(out["cls"][1], out[None][1]) and not torch.equal(out["cls"][0], out[None][0])
    assert torch.equal(out["reg"][0], out[None][0]) and not torch.equal(out["reg"][1], out[None][1])
    assert torch.equal(out["both"][0], out["cls"][0]) and torch.equal(out["both"][1], out["reg"][1])


def test_ghm_stateless_replayed_step_equals_the_eager_step(hip):
    """momentum 0: replays with gt_a, gt_b, gt_a give the eager losses of each -- assignment, histograms, weights and loss run
    inside the graph on what gt_boxes holds at replay."""
    import torch
    from mxdetection_amd.models import RetinaNet
    image, gt_a, im_info = _inputs(N, H, W, seed=2)
    _, gt_b, _ = _inputs(N, H, W, seed=3)
    eager = _model("both", True)
    want = []
    for gt in (gt_a, gt_b):
        want.append(torch.cat(list(eager.forward_backward(image, gt, im_info, step=4))).clone())
    torch.cuda.synchronize()
    assert not torch.allclose(want[0], want[1], rtol=1e-3)
    m = RetinaNet("cuda", depth=50, seed=7, ghm="both", **STATELESS)
    m.capture(image, gt_a, im_info, lr=0.0, image_offset=0, warmup=1)
    for gt, w in zip((gt_a, gt_b, gt_a), want + want[:1]):
        got = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
        torch.cuda.synchronize()
        assert torch.allclose(got, w, rtol=1e-4, atol=1e-5), (got, w)


def test_ghm_replayed_sequence_carries_the_state_like_the_eager_one(hip):
    """Published momenta: after ghm_reset() on both models the replayed sequence gt_a, gt_b equals the eager sequence (the
    moving average lives on the device and is updated inside the graph)."""
    import torch
    from mxdetection_amd.models import RetinaNet
    image, gt_a, im_info = _inputs(N, H, W, seed=2)
    _, gt_b, _ = _inputs(N, H, W, seed=3)
    eager = _model("both")
    eager.plan(N, H, W, gt_a.shape[1])
    eager.ghm_reset()
    want, state = [], []
    for gt in (gt_a, gt_b):
        want.append(torch.cat(list(eager.forward_backward(image, gt, im_info, step=4))).clone())
        state.append(eager.head.ghm_acc.clone())
    torch.cuda.synchronize()
    eager.ghm_reset()                                                    # a fresh state gives another second step
    fresh_b = torch.cat(list(eager.forward_backward(image, gt_b, im_info, step=4))).clone()
    assert not torch.equal(fresh_b, want[1])
    m = RetinaNet("cuda", depth=50, seed=7, ghm="both")
    m.capture(image, gt_a, im_info, lr=0.0, image_offset=0, warmup=1)
    torch.cuda.synchronize()
    assert not m.head.ghm_acc.any()                                      # the warm-up step left no counts behind
    m.ghm_reset()
    for gt, w, s in zip((gt_a, gt_b), want, state):
        got = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
        torch.cuda.synchronize()
        assert torch.allclose(got, w, rtol=1e-4, atol=1e-5), (got, w)
        assert torch.allclose(m.head.ghm_acc, s, rtol=1e-6, atol=0)


def test_ghm_checkpoint_loads_into_a_plain_model(hip, tmp_path):
    """The parameter layout does not depend on ghm and the moving average is no parameter: a ghm checkpoint loads into a
    plain model with no missing or unexpected names, and both predict the same detections."""
    import torch
    from mxdetection_amd.models import RetinaNet
    image, gt, im_info = _inputs(N, H, W, seed=4)
    a = RetinaNet("cuda", depth=50, seed=5, ghm="both")
    a.train_step(image, gt, im_info, step=0, lr=0.01)
    a.train_step(image, gt, im_info, step=1, lr=0.01)
    fn = str(tmp_path / "ghm-0001.params")
    a.save_checkpoint(fn)
    b = RetinaNet("cuda", depth=50, seed=11)
    assert b.head.ghm == "none" and b.load_checkpoint(fn) == []
    assert [n for n, _, _, _ in a._named_tensors()] == [n for n, _, _, _ in b._named_tensors()]
    assert not [n for n, _, _, _ in a._named_tensors() if "ghm" in n]
    for (na, _, ta, _), (nb, _, tb, _) in zip(a._named_tensors(), b._named_tensors()):
        assert na == nb and torch.equal(ta, tb), na
    assert torch.equal(a.arena.w, b.arena.w) and torch.equal(a.arena.m, b.arena.m)
    c = RetinaNet("cuda", depth=50, seed=13, ghm="both")
    b.save_checkpoint(str(tmp_path / "plain-0001.params"))
    assert c.load_checkpoint(str(tmp_path / "plain-0001.params")) == [] and torch.equal(c.arena.w, a.arena.w)      # and back
    outs = []
    for m in (a, b):
        dets, num = m.predict(image, im_info, score_thresh=0.0, max_per_image=50)
        torch.cuda.synchronize()
        outs.append((dets.clone(), num.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][0].shape == (N, 50, 6) and torch.isfinite(outs[0][0]).all()
