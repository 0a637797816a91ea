"""The gradient-harmonizing entries (mxdet_ghm_hist_level, mxdet_ghm_weights, mxdet_retina_loss_level_ghm in
csrc/retina_loss.hip) on the tables of tests/test_ghm_cases_cpu.py: two levels that share one histogram, N = 2, in the vector
form (780 anchors = four workgroups, the last one partial, and 72 = less than one; padding columns present) and the scalar
form.

Per step: cnt equal to the float64 reference bit for bit, coef within 8 float32 ulp, per-level losses within LOSS_RTOL of the
float64 sum plus weight * coef * the measured element bound per summed element, gradients within the measured bound (plus
one bf16 step) after division by coef * weight * loss_scale -- the device's own coef, which the line before has tied to the
reference's. Every output is an interior slice of a sentinel-filled buffer; padding columns keep the sentinel.
"""
import numpy as np
import pytest

import _ghm_ref as G
import test_ghm_cases_cpu as GT
from test_gpu_losses import SENT, Guarded, _bits, _np, _t

pytestmark = pytest.mark.gpu

FOCAL = (0.25, 2.0, 3.0)                                  # alpha, gamma, sigma of the half that is not harmonized


def run_step(form, kind, mode, c, acc, loss_scale=1.0, data=None):
    """One step (histogram passes, weights, loss passes, finalize per level) from the state `acc` (f32 device tensor,
    updated in place). Returns cnt, coef, acc (clones) and per level gc, gr (whole rows), part, out."""
    import torch
    from mxdetection_amd.core import loss as L
    d = data or GT.step_data(form, kind)
    f = GT.FORMS[form]
    A, Cc = f["A"], f["C"]
    bf = torch.bfloat16
    lab, tgt = _t(d["cls_labels"]), _t(d["targets"])
    nfg = torch.tensor([int((d["cls_labels"] > 0).sum())], dtype=torch.int32, device="cuda")
    nb = c["cls_bins"] + c["reg_bins"]
    nparts = [L.retina_loss_num_partials(GT.N, lv["H"], lv["W"], A) for lv in d["levels"]]
    rows = sum(nparts)
    counts = Guarded((rows, nb), torch.int32)
    cnt, coef = Guarded((nb,), torch.int32), Guarded((nb,), torch.float32)
    cls = [_t(lv["cls"], bf) for lv in d["levels"]]
    reg = [_t(lv["reg"], bf) for lv in d["levels"]]
    off = 0
    for l, lv in enumerate(d["levels"]):
        L.ghm_hist_level(cls[l], reg[l], A, Cc, lab, tgt, lv["off"], mode, c["cls_bins"], c["reg_bins"], c["reg_mu"], counts.view[off:])
        off += nparts[l]
    L.ghm_weights(counts.view, rows, c["cls_bins"], c["reg_bins"], c["cls_momentum"], c["reg_momentum"], acc, cnt.view, coef.view)
    out = {"levels": []}
    off = 0
    part = Guarded((2 * rows,), torch.float32)
    for l, lv in enumerate(d["levels"]):
        gc, gr = Guarded(cls[l].shape, bf), Guarded(reg[l].shape, bf)
        res = Guarded((2,), torch.float32)
        L.retina_loss_level_ghm(cls[l], reg[l], A, Cc, lab, tgt, lv["off"], mode, *FOCAL, coef.view, c["cls_bins"], c["reg_bins"],
                                c["cls_weight"], c["reg_mu"], c["reg_weight"], nfg, loss_scale, gc.view, gr.view, part.view[2 * off:])
        L.loss_finalize(part.view[2 * off:], nparts[l], 2, res.view)
        torch.cuda.synchronize()
        assert gc.outside_intact() and gr.outside_intact() and res.outside_intact()
        assert bool((gc.view[..., A * Cc:] == SENT).all()) and bool((gr.view[..., 4 * A:] == SENT).all())      # padding: untouched
        assert not bool((gc.view[..., :A * Cc] == SENT).any()) and not bool((gr.view[..., :4 * A] == SENT).any())
        out["levels"].append(dict(gc=gc.view.clone(), gr=gr.view.clone(), part=part.view[2 * off:2 * (off + nparts[l])].clone(),
                                  out=res.view.clone()))
        off += nparts[l]
    for t in (counts, cnt, coef, part):
        assert t.outside_intact() and not bool((t.view == SENT).any())
    out.update(cnt=cnt.view.clone(), coef=coef.view.clone(), acc=acc.clone(), counts=counts.view.clone(), nfg=nfg, cls=cls, reg=reg,
               lab=lab, tgt=tgt, data=d)
    assert bool(torch.isfinite(out["coef"]).all()) and bool(torch.isfinite(out["acc"]).all())
    assert torch.equal(out["counts"].sum(0), out["cnt"])
    return out


def run_plain(r, form, loss_scale=1.0):
    """mxdet_retina_loss_level on the inputs of a run_step result: per level (gc, gr, part)."""
    import torch
    from mxdetection_amd.core import loss as L
    f = GT.FORMS[form]
    res = []
    for l, lv in enumerate(r["data"]["levels"]):
        gc, gr = torch.full_like(r["cls"][l], SENT), torch.full_like(r["reg"][l], SENT)
        part = torch.zeros((2 * L.retina_loss_num_partials(GT.N, lv["H"], lv["W"], f["A"]),), device="cuda")
        L.retina_loss_level(r["cls"][l], r["reg"][l], f["A"], f["C"], r["lab"], r["tgt"], lv["off"], *FOCAL, r["nfg"], loss_scale, gc, gr,
                            part)
        res.append((gc, gr, part))
    torch.cuda.synchronize()
    return res


def grads_ok(what, got, ref, bins, coef, weight, loss_scale, unit_ref, atol):
    """got (device gradient, whole rows) / (coef[bin] * weight * loss_scale) against ref / unit_ref, element by element;
    where there is no element the device gradient is exactly 0."""
    got, m = np.asarray(got, np.float64), bins >= 0
    if got[~m].any():
        return False
    unit =np.where(m, np.asarray(coef, np.float64)[np.where(m, bins, 0)], 0.0) * weight * loss_scale
    ok = True
    if m.any():
        a, b = got[m] / unit[m], ref[m] / unit_ref[m]
        err, bound = np.abs(a - b), atol + GT.BF16_STEP * np.abs(b)
        print("%s: max |got-ref|/unit = %.3e (atol %.3e), max excess over the bound = %.3e" % (what, err.max(), atol, (err - bound).max()))
        ok = bool((err <= bound).all())
    return ok


def sum_ok(what, got, ref, weight, wsum, atol):
    got, ref = float(got), float(ref)
    bound = GT.LOSS_RTOL * abs(ref) + weight * wsum * atol
    print("%s: got %.9g ref %.9g, |diff| %.3e (bound %.3e)" % (what, got, ref, abs(got - ref), bound))
    return got == 0.0 if wsum == 0.0 else abs(got - ref) <= bound


def check_against_ref(tag, r, ref, form, mode, c, loss_scale):
    f = GT.FORMS[form]
    A, Cc = f["A"], f["C"]
    Bc = c["cls_bins"]
    cnt, coef = r["cnt"].cpu().numpy(), r["coef"].cpu().numpy()
    if mode in ("cls", "both"):
        assert np.array_equal(cnt[:Bc], ref["cnt_c"]), (tag, cnt[:Bc], ref["cnt_c"])
        assert GT.coef_ok(tag + " class", coef[:Bc], ref["coef_c"])
    else:
        assert not cnt[:Bc].any() and not coef[:Bc].any()
    if mode in ("reg", "both"):
        assert np.array_equal(cnt[Bc:], ref["cnt_r"]), (tag, cnt[Bc:], ref["cnt_r"])
        assert GT.coef_ok(tag + " box", coef[Bc:], ref["coef_r"])
    else:
        assert not cnt[Bc:].any() and not coef[Bc:].any()
    for l, (g, o) in enumerate(zip(r["levels"], ref["levels"])):
        gc, gr = _np(g["gc"])[..., :A * Cc], _np(g["gr"])[..., :4 * A]
        if mode in ("cls", "both"):
            bins = o["bin_c"][..., :A * Cc]
            assert not gc[bins < 0].any()                                              # ignored anchors: zero gradient
            assert sum_ok("%s level %d class loss" % (tag, l), g["out"][0], o["loss_c"], c["cls_weight"], o["wsum_c"], GT.ATOL_CLS_LOSS)
            assert grads_ok("%s level %d grad_cls" % (tag, l), gc, o["grad_cls"][..., :A * Cc], bins, coef[:Bc], c["cls_weight"],
                            loss_scale, o["unit_c"][..., :A * Cc], GT.ATOL_CLS_GRAD)
        if mode in ("reg", "both"):
            bins = o["bin_r"][..., :4 * A]
            assert not gr[bins < 0].any()
            assert sum_ok("%s level %d box loss" % (tag, l), g["out"][1], o["loss_r"], c["reg_weight"], o["wsum_r"], GT.ATOL_REG_LOSS)
            assert grads_ok("%s level %d grad_reg" % (tag, l), gr, o["grad_reg"][..., :4 * A], bins, coef[Bc:], c["reg_weight"],
                            loss_scale, o["unit_r"][..., :4 * A], GT.ATOL_REG_GRAD)


@pytest.mark.parametrize("mode", G.MODES)
@pytest.mark.parametrize("form", sorted(GT.FORMS))
def test_two_calls_match_the_reference_and_its_carried_state(hip, form, mode):
    """Calls 1 and 2 (different inputs; a bin populated in call 1 is empty in call 2 and keeps its acc) at the published
    momenta from a zero state. The half that `mode` leaves out is mxdet_retina_loss_level's, bit for bit."""
    import torch
    c = GT.cfg()
    ls = 4.0
    acc = torch.zeros((40,), device="cuda")
    acc_c, acc_r = np.zeros(30), np.zeros(10)
    for kind in ("a", "b"):
        d = GT.step_data(form, kind)
        before = acc.clone()
        r = run_step(form, kind, mode, c, acc, ls)
        ref = G.ref_step(d["levels"], d["cls_labels"], d["targets"], mode, c, acc_c, acc_r, ls)
        check_against_ref("%s %s call %s" % (form, mode, kind), r, ref, form, mode, c, ls)
        held = r["cnt"] == 0
        assert torch.equal(r["acc"][held], before[held])                      # empty bins keep their state
        if kind == "b" and mode != "reg":
            assert float(before[20]) > 0 and int(r["cnt"][20]) == 0 and float(r["acc"][20]) == float(before[20])
        if mode != "both":
            plain = run_plain(r, form, ls)
            for l, (g, (pc, pr, pp)) in enumerate(zip(r["levels"], plain)):
                if mode == "cls":
                    assert np.array_equal(_bits(g["gr"]), _bits(pr)) and torch.equal(g["part"][1::2], pp[1::2])
                    assert not torch.equal(g["part"][0::2], pp[0::2])
                else:
                    assert np.array_equal(_bits(g["gc"]), _bits(pc)) and torch.equal(g["part"][0::2], pp[0::2])
                    assert l > 0 or not torch.equal(g["part"][1::2], pp[1::2])        # the small level may hold no foreground
    ref_acc = np.concatenate([acc_c, acc_r])
    got = acc.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - ref_acc) <= 4 * GT.ulp32(ref_acc))


@pytest.mark.parametrize("form", sorted(GT.FORMS))
def test_momentum_zero_is_stateless(hip, form):
    import torch
    c = GT.cfg(cls_momentum=0.0, reg_momentum=0.0)
    d = GT.step_data(form, "a")
    a = run_step(form, "a", "both", c, torch.zeros((40,), device="cuda"))
    b = run_step(form, "a", "both", c, torch.full((40,), 123.0, device="cuda"))
    assert torch.equal(a["coef"], b["coef"]) and torch.equal(a["cnt"], b["cnt"])
    has = a["cnt"] > 0
    assert torch.equal(a["acc"][has], a["cnt"][has].float()) and torch.equal(b["acc"][~has], torch.full_like(b["acc"][~has], 123.0))
    for x, y in zip(a["levels"], b["levels"]):
        assert all(torch.equal(x[k], y[k]) for k in ("gc", "gr", "part", "out"))
    ref = G.ref_step(d["levels"], d["cls_labels"], d["targets"], "both", c, np.full(30, 7.0), np.full(10, 7.0))
    check_against_ref(form + " momentum 0", a, ref, form, "both", c, 1.0)


@pytest.mark.parametrize("form", sorted(GT.FORMS))
def test_same_call_from_the_same_state_is_bit_identical(hip, form):
    import torch
    c = GT.cfg()
    warm = torch.zeros((40,), device="cuda")
    run_step(form, "a", "both", c, warm)
    a = run_step(form, "b", "both", c, warm.clone(), 512.0)
    b = run_step(form, "b", "both", c, warm.clone(), 512.0)
    for k in ("cnt", "coef", "acc", "counts"):
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(a["levels"], b["levels"]):
        assert all(torch.equal(x[k], y[k]) for k in ("gc", "gr", "part", "out"))
    assert not torch.equal(a["acc"], warm)


@pytest.mark.parametrize("form", sorted(GT.FORMS))
def test_empty_histograms(hip, form):
    """No foreground: the box histogram is empty while the class one is not. Every label ignored: both are empty -- zero loss
    and gradients, cnt and coef 0, the state unchanged bit for bit, nothing NaN or Inf."""
    import torch
    c = GT.cfg()
    f = GT.FORMS[form]
    acc = torch.zeros((40,), device="cuda")
    acc_c, acc_r = np.zeros(30), np.zeros(10)
    d = GT.step_data(form, "a")
    run_step(form, "a", "both", c, acc)
    G.ref_step(d["levels"], d["cls_labels"], d["targets"], "both", c, acc_c, acc_r)
    before = acc.clone()
    d = GT.step_data(form, "nofg")
    r = run_step(form, "nofg", "both", c, acc)
    ref = G.ref_step(d["levels"], d["cls_labels"], d["targets"], "both", c, acc_c, acc_r)
    check_against_ref(form + " nofg", r, ref, form, "both", c, 1.0)
    assert not r["cnt"][30:].any() and not r["coef"][30:].any() and torch.equal(r["acc"][30:], before[30:]) and r["cnt"][:30].any()
    for g in r["levels"]:
        assert float(g["out"][1]) == 0.0 and not g["gr"][..., :4 * f["A"]].any() and float(g["out"][0]) > 0.0
    before = acc.clone()
    r = run_step(form, "ignored", "both", c, acc)
    assert not r["cnt"].any() and not r["coef"].any() and torch.equal(r["acc"], before) and torch.equal(acc, before)
    for g in r["levels"]:
        assert not g["out"].any() and not g["part"].any()
        assert not g["gc"][..., :f["A"] * f["C"]].any() and not g["gr"][..., :4 * f["A"]].any()


@pytest.mark.parametrize("bins", [1, 64])
def test_bin_limits_are_accepted(hip, bins):
    """1 bin: every element weighs 1 / count. 64 bins (the tables are guarded for them too): cnt equals the reference."""
    import torch
    c = GT.cfg(cls_bins=bins, reg_bins=bins, cls_momentum=0.0, reg_momentum=0.0)
    d = GT.step_data("vec", "a")
    r = run_step("vec", "a", "both", c, torch.zeros((2 * bins,), device="cuda"))
    ref = G.ref_step(d["levels"], d["cls_labels"], d["targets"], "both", c, np.zeros(bins), np.zeros(bins))
    check_against_ref("vec %d bins" % bins, r, ref, "vec", "both", c, 1.0)
    gc, gr = GT.all_g(d)
    assert int(r["cnt"][:bins].sum()) == gc.size and int(r["cnt"][bins:].sum()) == gr.size
    if bins == 1:
        assert float(r["coef"][0]) == float(np.float32(1.0) / np.float32(gc.size)) and float(r["coef"][1]) == float(np.float32(1.0) / np.float32(gr.size))


def test_out_of_range_settings_are_refused_with_a_message(hip):
    import torch
    from mxdetection_amd._lib import MxdetError
    for kw, word in ((dict(cls_bins=0), "bins must lie in 1..64"), (dict(reg_bins=65), "bins must lie in 1..64"),
                     (dict(cls_momentum=1.0), r"momentum must lie in \[0, 1\)"), (dict(reg_mu=0.0), "mu must be positive")):
        with pytest.raises(MxdetError, match=word):
            run_step("vec", "a", "both", GT.cfg(**kw), torch.zeros((200,), device="cuda"))
    torch.cuda.synchronize()
