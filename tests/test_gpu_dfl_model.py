"""RetinaNet with the distribution box head (reg_max = 16: the GFL head) at a small shape (128 x 192,
ResNet-50), on the one-anchor ATSS model of tests/test_gpu_atss_model.py: a training step whose three losses are the float64
reference (tests/_dfl_ref.py) evaluated on the head's own outputs, a captured step replayed with new ground truth, inference,
checkpoints (round trip; the other box layout is refused before anything is written), and reg_max = 0 being today's model
bit for bit."""
import functools

import numpy as np
import pytest

import _dfl_ref as D
import test_dfl_cases_cpu as DT
import test_quality_loss_cases_cpu as QT
from test_gpu_atss_model import CELLS, H, N, ONE, W
from test_gpu_gn_heads import _inputs

pytestmark = pytest.mark.gpu

GFL = dict(cls_loss="qfl", reg_max=16, dfl_weight=0.25)


@functools.lru_cache(maxsize=None)
def _model(gfl=True, seed=7):
    from mxdetection_amd.models import RetinaNet
    return RetinaNet("cuda", depth=50, seed=seed, **ONE, **(GFL if gfl else {}))


def test_gfl_training_step(hip):
    import torch
    m = _model()
    image, gt, im_info = _inputs(N, H, W, seed=1)
    (loss,) = m.forward_backward(image, gt, im_info, step=0)
    torch.cuda.synchronize()
    h = m.head
    assert (h.reg_max, h.dfl_weight, h.cls_loss, h.reg_loss, h.reg_loss_weight) == (16, 0.25, "qfl", "giou", 2.0)
    assert h.A == 1 and h.anchors.shape[0] == CELLS and (h.ld_cls, h.ld_reg, h.reg_ch) == (128, 128, 68)
    assert h.box_out.cout_real == 68 and loss.shape == (3,) and h.partial.numel() == 3 * sum(h.nparts)
    nfg = int(h.num_fg.item())
    assert nfg >= 8
    anchors, matched, gtn = h.anchors.cpu().numpy(), h.matched.cpu().numpy(), gt.cpu().numpy()
    cls_labels = h.cls_labels.cpu().numpy()
    want, n_valid, n_reg = np.zeros(3), 0, 0
    for l, (co, bo) in enumerate(zip(h.co, h.bo)):
        r = D.ref_level(co.float().cpu().numpy(), bo.float().cpu().numpy(), h.A, h.Cn, cls_labels, anchors, matched, gtn,
                        h.level_offsets[l], "qfl", h.cls_alpha, h.cls_gamma, "giou", 16, float(h.strides[l]), 2.0, 0.25, nfg, 1.0)
        want += r["loss"]
        n_valid += r["n_valid"]
        n_reg += r["nfg"]
    got = loss.cpu().numpy()
    print("GFL losses: got %s ref %s over %d anchors, %d regress, %d foreground" % (got, want, n_valid, n_reg, nfg))
    assert n_reg >= 8
    assert abs(got[0] - want[0]) <= DT.LOSS_RTOL * abs(want[0]) + n_valid * QT.ATOL_CLS_LOSS / nfg
    assert abs(got[1] - want[1]) <= DT.LOSS_RTOL * abs(want[1]) + n_reg * DT.ATOL_BOX / nfg
    assert abs(got[2] - want[2]) <= DT.LOSS_RTOL * abs(want[2]) + n_reg * DT.ATOL_DFL / nfg
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    assert torch.isfinite(m.arena.g).all()
    grads = m.export_grads()
    for name in ("retina.cls_out.weight", "retina.box_out.weight", "retina.cls0.weight", "retina.box0.weight"):
        assert grads[name].abs().sum().item() > 0, name
    assert grads["retina.box_out.weight"].shape[0] == 128 and not grads["retina.box_out.weight"][68:].any()


def test_gfl_replayed_step_equals_the_eager_step(hip):
    import torch
    from mxdetection_amd.models import RetinaNet
    image, gt_a, im_info = _inputs(N, H, W, seed=2)
    _, gt_b, _ = _inputs(N, H, W, seed=3)
    eager = _model()
    want = []
    for gt in (gt_a, gt_b):
        want.append(torch.cat(list(eager.forward_backward(image, gt, im_info, step=4))).clone())
    torch.cuda.synchronize()
    assert want[0].shape == (3,) and not torch.allclose(want[0], want[1], rtol=1e-3)
    m = RetinaNet("cuda", depth=50, seed=7, **ONE, **GFL)
    m.capture(image, gt_a, im_info, lr=0.0, image_offset=0, warmup=1)
    for gt, w in zip((gt_a, gt_b, gt_a), want + want[:1]):
        got = torch.cat(list(m.replay(image, gt, im_info, 4))).clone()
        torch.cuda.synchronize()
        assert torch.allclose(got, w, rtol=1e-4, atol=1e-5), (got, w)


def test_gfl_predict_and_checkpoints(hip, tmp_path):
    import torch
    from mxdetection_amd.models import RetinaNet
    image, gt, im_info = _inputs(N, H, W, seed=4)
    a = RetinaNet("cuda", depth=50, seed=5, **ONE, **GFL)
    a.train_step(image, gt, im_info, step=0, lr=0.01)
    a.train_step(image, gt, im_info, step=1, lr=0.01)
    fn = str(tmp_path / "gfl-0001.params")
    a.save_checkpoint(fn)
    b = RetinaNet("cuda", depth=50, seed=11, **ONE, **GFL)
    assert b.load_checkpoint(fn) == []
    for (na, _, ta, _), (nb, _, tb, _) in zip(a._named_tensors(), b._named_tensors()):
        assert na == nb and torch.equal(ta, tb), na
    assert torch.equal(a.arena.w, b.arena.w) and torch.equal(a.arena.m, b.arena.m)
    outs = []
    for m in (a, b):
        dets, num = m.predict(image, im_info, score_thresh=0.0, max_per_image=50)
        torch.cuda.synchronize()
        outs.append((dets.clone(), num.clone()))
    dets, num = outs[0]
    assert torch.equal(dets, outs[1][0]) and torch.equal(num, outs[1][1])
    assert dets.shape == (N, 50, 6) and torch.isfinite(dets).all() and a._det.reg_max == 16
    info = im_info.cpu().numpy()
    for n in range(N):
        k = int(num[n])
        d = dets[n].cpu().numpy()
        assert 0 < k <= 50 and np.all(np.diff(d[:k, 4]) <= 0) and np.all((d[:k, 5] >= 1) & (d[:k, 5] <= 80))
        assert d[:k, :4].min() >= 0 and d[:k, 2].max() <= info[n, 1] - 1 and d[:k, 3].max() <= info[n, 0] - 1      # inside the image
        assert np.all(d[:k, 2] >= d[:k, 0]) and np.all(d[:k, 3] >= d[:k, 1])
    # the other box layout is refused, both ways, before any tensor changes
    plain = RetinaNet("cuda", depth=50, seed=13, **ONE)
    before = [t.clone() for _, _, t, _ in plain._named_tensors()]
    with pytest.raises(ValueError, match=r"68 rows.*reg_max = 16.*4 rows"):
        plain.load_checkpoint(fn)
    assert all(torch.equal(x, t) for x, (_, _, t, _) in zip(before, plain._named_tensors()))
    fn0 = str(tmp_path / "plain-0001.params")
    plain.save_checkpoint(fn0)
    before = [t.clone() for _, _, t, _ in b._named_tensors()]
    with pytest.raises(ValueError, match=r"4 rows.*reg_max = 0.*68 rows"):
        b.load_checkpoint(fn0)
    assert all(torch.equal(x, t) for x, (_, _, t, _) in zip(before, b._named_tensors()))
    assert plain.load_checkpoint(fn0) == []
    # nine plain anchors have 36 box rows, as one anchor with reg_max = 8 has: told apart by retina.cls_out
    nine = RetinaNet("cuda", depth=50, seed=3, reg_loss="giou")
    fn9 = str(tmp_path / "nine-0001.params")
    nine.save_checkpoint(fn9)
    one8 = RetinaNet("cuda", depth=50, seed=17, **ONE, reg_max=8)
    assert nine.head.reg_ch == one8.head.reg_ch == 36
    before = [t.clone() for _, _, t, _ in one8._named_tensors()]
    with pytest.raises(ValueError, match=r"36 rows: 9 anchors per cell x 4 rows per anchor \(reg_max = 0\).*720 rows.*reg_max \+ 1 = 9"):
        one8.load_checkpoint(fn9)
    assert all(torch.equal(x, t) for x, (_, _, t, _) in zip(before, one8._named_tensors()))


def test_reg_max_zero_is_todays_model(hip):
    import torch
    from mxdetection_amd.models import RetinaNet
    image, gt, im_info = _inputs(N, H, W, seed=1)
    a = _model(False)
    b = RetinaNet("cuda", depth=50, seed=7, **ONE, reg_max=0, dfl_weight=0.25)
    assert (b.head.reg_max, b.head.ld_reg, b.head.reg_ch, b.head.ncomp) == (0, 64, 4, 2) == (a.head.reg_max, a.head.ld_reg, a.head.reg_ch, a.head.ncomp)
    la = a.forward_backward(image, gt, im_info, step=0)[0].clone()
    lb = b.forward_backward(image, gt, im_info, step=0)[0].clone()
    torch.cuda.synchronize()
    assert la.shape == (2,) and torch.equal(la, lb) and torch.equal(a.arena.g, b.arena.g)
    ga, gb = a.export_grads(), b.export_grads()
    assert list(ga) == list(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)
