"""The vector / scalar split of the delta-box level entries (mxdet_retina_loss_level, _iou, _quality in csrc/retina_loss.hip):
one kernel template per entry, the two forms sharing the class elements and the box part.

Each entry's `coco` case data (C = 80: the 16-byte form in aligned buffers) is fed again through the `viewcls` / `viewreg`
offset views of tests/test_loss_cases_cpu.py -- cls / grad_cls one bf16 element off, or reg / grad_reg two -- which take the
scalar form. Both gradients must be the vector form's bits (every element is computed by the same code on the same
inputs). The loss sums add the same terms in another order: they agree within the tolerance of the entry's own test file
(LOSS_RTOL of the sum, plus that file's absolute bound per summed term).
"""
import numpy as np
import pytest

import test_iou_loss_cases_cpu as IT
import test_loss_cases_cpu as LT
import test_quality_loss_cases_cpu as QT
from test_gpu_losses import SENT, Guarded, _bits, _run_retina, _t

pytestmark = pytest.mark.gpu

VIEWS = {s[0]: (s[3], s[4]) for s in LT.RETINA_SHAPES if s[0].startswith("view")}      # name -> byte offsets (cls, reg)


def _sums_agree(what, got, want, atol):
    got, want = np.asarray(got.double().cpu()), np.asarray(want.double().cpu())
    err = np.abs(got - want)
    print("%s: scalar form %s vector form %s, max |difference| %.3e (allowed %s)" % (what, got, want, err.max(), LT.LOSS_RTOL * np.abs(want) + atol))
    return bool(np.all(err <= LT.LOSS_RTOL * np.abs(want) + atol))


def test_view_table_is_the_one_meant():
    assert VIEWS == {"viewcls": (2, 0), "viewreg": (0, 4)}


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_smooth_l1_entry_forms_agree(hip, view):
    c = next(x for x in LT.RETINA_CASES if x["name"] == "coco")
    d = LT.retina_data(c)
    N, H, W, A, Cc, ldc, ldr = c["shape"]
    vc, vr, vout = (t.clone() for t in _run_retina(c, d, 0, 0))
    sc, sr, sout = _run_retina(c, d, *VIEWS[view])
    assert np.array_equal(_bits(sc), _bits(vc)) and np.array_equal(_bits(sr), _bits(vr))
    assert _sums_agree("class, box loss", sout, vout, N * H * W * A * Cc * LT.F32_MIN_NORMAL)


def _run_anchor_entry(entry, c, d, num_fg, off_cls, off_reg):
    """mxdet_retina_loss_level_iou / _quality with the (cls, grad_cls) / (reg, grad_reg) views `off_*` BYTES off their aligned places."""
    import torch
    from mxdetection_amd.core import loss as L
    N, H, W, A, Cc = c["shape"]
    ldc, ldr = IT.retina_ld(c)
    bf = torch.bfloat16
    ec, er = off_cls // 2, off_reg // 2
    cls, reg = Guarded((N, H, W, ldc), bf, ec, _t(d["cls"], bf)), Guarded((N, H, W, ldr), bf, er, _t(d["reg"], bf))
    gc, gr = Guarded((N, H, W, ldc), bf, ec), Guarded((N, H, W, ldr), bf, er)
    for t, off, al in ((cls, off_cls, 16), (gc, off_cls, 16), (reg, off_reg, 8), (gr, off_reg, 8)):
        assert t.view.data_ptr() % al == off % al
    nparts = L.retina_loss_num_partials(N, H, W, A)
    part, out = Guarded((2 * nparts,), torch.float32), Guarded((2,), torch.float32)
    nfg = torch.tensor([num_fg], dtype=torch.int32, device="cuda")
    args = (cls.view, reg.view, A, Cc, _t(d["cls_labels"]), _t(d["anchors"]), _t(d["matched"]), _t(d["gt"]), c["off"])
    if entry == "iou":
        L.retina_loss_level_iou(*args, IT.RETINA_ALPHA, IT.RETINA_GAMMA, c["kind"], IT.STDS[IT.RETINA_STDS], c["rw"], nfg, float(c["ls"]),
                                gc.view, gr.view, part.view)
    else:
        L.retina_loss_level_quality(*args, c["cls_loss"], c["alpha"], c["gamma"], c["kind"], QT.STDS, c["rw"], nfg, float(c["ls"]), gc.view,
                                    gr.view, part.view)
    L.loss_finalize(part.view, nparts, 2, out.view)
    torch.cuda.synchronize()
    for t in (cls, reg, gc, gr, part, out):
        assert t.outside_intact()
    assert bool((gc.view[..., A * Cc:] == SENT).all()) and bool((gr.view[..., 4 * A:] == SENT).all())
    assert not bool((part.view == SENT).any())
    return gc.view[..., :A * Cc].clone(), gr.view[..., :4 * A].clone(), part.view.clone(), out.view.clone()


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("kind", IT.KINDS)
def test_iou_entry_forms_agree(hip, kind, view):
    c = dict(next(x for x in IT.RETINA_CASES if x["name"] == "coco" and x["nfg"] == "true"), kind=kind)
    d, ref = IT.retina_data(c), IT.retina_ref(c, kind)
    vc, vr, vpart, vout = _run_anchor_entry("iou", c, d, IT.retina_num_fg(c), 0, 0)
    sc, sr, spart, sout = _run_anchor_entry("iou", c, d, IT.retina_num_fg(c), *VIEWS[view])
    assert np.array_equal(_bits(sc), _bits(vc)) and np.array_equal(_bits(sr), _bits(vr))
    inv = ref["unit"] / c["ls"]
    assert _sums_agree("class loss", sout[0], vout[0], 0.0) and _sums_agree("class partials", spart[0::2], vpart[0::2], 0.0)
    assert _sums_agree("box loss", sout[1], vout[1], ref["nfg"] * IT.ATOL_LOSS * c["rw"] * inv)
    assert _sums_agree("box partials", spart[1::2], vpart[1::2], ref["nfg"] * IT.ATOL_LOSS * c["rw"] * inv)


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("cls_id", [s[0] for s in QT.CLS_SETTINGS])
def test_quality_entry_forms_agree(hip, cls_id, view):
    c = next(x for x in QT.CASES if x["name"] == "coco" and x["cls_id"] == cls_id and x["kind"] == "giou" and x["nfg"] == "true")
    d, ref = QT.level_data(c), QT.level_ref(c)
    vc, vr, vpart, vout = _run_anchor_entry("quality", c, d, QT.num_fg(c), 0, 0)
    sc, sr, spart, sout = _run_anchor_entry("quality", c, d, QT.num_fg(c), *VIEWS[view])
    assert np.array_equal(_bits(sc), _bits(vc)) and np.array_equal(_bits(sr), _bits(vr))
    atol_cls = ref["n_valid"] * QT.ATOL_CLS_LOSS * ref["inv"]
    assert _sums_agree("class loss", sout[0], vout[0], atol_cls) and _sums_agree("class partials", spart[0::2], vpart[0::2], atol_cls)
    nfg = int((d["cls_labels"][:, c["off"]:c["off"] + vr[0].numel() // 4] > 0).sum())
    atol_box = nfg * IT.ATOL_LOSS * c["rw"] * ref["inv"]
    assert _sums_agree("box loss", sout[1], vout[1], atol_box) and _sums_agree("box partials", spart[1::2], vpart[1::2], atol_box)
