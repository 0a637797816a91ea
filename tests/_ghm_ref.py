"""References of the gradient-harmonizing losses (GHM-C / GHM-R; DESIGN.md 5v, include/mxdet.h). No tests here.

  * float64 on the definition, in mmdetection's form: a loop over the bins with a mask per bin from edge comparisons
    (edges k / B, the last one + 1e-6), tot formed and divided out again, the weights a constant (numpy) of the torch
    autograd loss, the moving average a float64 array the caller carries.
  * numpy float32 restatements in the kernel's operation order (oracle.expf / oracle.logf): CPU stand-ins that measure the
    float32 error, never references.
"""
import numpy as np

import test_loss_cases_cpu as T

MODES = ("cls", "reg", "both")


def O():
    return T.O()


# ---------------------------------------------------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------------------------------------------------
def cls_g64(x, t):
    """|sigmoid(x) - t| float64, elementwise; 1 - sigmoid(x) is taken as sigmoid(-x)."""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    with np.errstate(over="ignore"):
        s, sm = 1.0 / (1.0 + np.exp(-x)), 1.0 / (1.0 + np.exp(x))
    return np.where(t > 0, sm, s)


def reg_g64(d, mu):
    d = np.asarray(d, np.float64)
    return np.abs(d) / np.sqrt(d * d + mu * mu)


def harmonize64(g, B, momentum, acc):
    """mmdetection's GHM weighting of the valid elements g (1-d float64): returns (weights per element = N * coef[bin],
    tot, cnt [B] int64, coef [B] float64); acc [B] float64 is updated in place."""
    g = np.asarray(g, np.float64)
    edges = np.arange(B + 1, dtype=np.float64) / B
    edges[-1] += 1e-6
    weights = np.zeros_like(g)
    tot = max(float(g.size), 1.0)
    cnt = np.zeros((B,), np.int64)
    n = 0
    for i in range(B):
        inds = (g >= edges[i]) & (g < edges[i + 1])
        num = int(inds.sum())
        cnt[i] = num
        if num > 0:
            if momentum > 0:
                acc[i] = momentum * acc[i] + (1 - momentum) * num
                weights[inds] = tot / acc[i]
            else:
                acc[i] = num
                weights[inds] = tot / num
            n += 1
    if n > 0:
        weights = weights / n
    coef = np.zeros((B,), np.float64)
    if n > 0:
        coef[cnt > 0] = 1.0 / (n * acc[cnt > 0])
    return weights, tot, cnt, coef


def level_views(lv, cls_labels, targets):
    """Of one level dict(cls [N,H,W,ldc], reg [N,H,W,ldr], A, C, off): logits x [N,n,C], onehot t [N,n,C], valid [N,n],
    deltas [N,n,4], targets [N,n,4], fg [N,n]."""
    N, H, W, _ = lv["cls"].shape
    A, Cc, off = lv["A"], lv["C"], lv["off"]
    n = H * W * A
    lab = np.asarray(cls_labels)[:, off:off + n]
    x = np.asarray(lv["cls"], np.float64)[..., :A * Cc].reshape(N, n, Cc)
    t = (lab[..., None] == np.arange(1, Cc + 1)).astype(np.float64)
    dl = np.asarray(lv["reg"], np.float64)[..., :4 * A].reshape(N, n, 4)
    tg = np.asarray(targets, np.float64)[:, off:off + n]
    return x, t, lab >= 0, dl, tg, lab > 0


def ref_step(levels, cls_labels, targets, mode, cfg, acc_c, acc_r, loss_scale=1.0):
    """One step over all levels in float64. cfg: the dict of core.loss.check_ghm. acc_c / acc_r: float64 state, updated in
    place for the harmonized halves. Returns a dict: cnt_c / cnt_r, coef_c / coef_r, and per level loss_c, loss_r, grad_cls,
    grad_reg (arrays like the level's cls / reg, zeros in the padding), unit_c / unit_r (coef * weight * loss_scale per
    element, same shapes), bin_c / bin_r (the element's bin, -1 where there is none), wsum_c / wsum_r (sum of coef over the
    level's valid elements). A half that mode leaves out has
    None entries."""
    import torch
    import torch.nn.functional as F
    views = [level_views(lv, cls_labels, targets) for lv in levels]
    out = {"levels": [dict() for _ in levels]}
    do_c, do_r = mode in ("cls", "both"), mode in ("reg", "both")
    if do_c:
        g_all = np.concatenate([cls_g64(x, t)[v] .reshape(-1) for x, t, v, _, _, _ in views])
        w_all, tot, out["cnt_c"], out["coef_c"] = harmonize64(g_all, cfg["cls_bins"], cfg["cls_momentum"], acc_c)
        pos = 0
        for lv, (x, t, v, _, _, _), o in zip(levels, views, out["levels"]):
            k = int(v.sum()) * lv["C"]
            w = np.zeros(x.shape)
            w[v] = w_all[pos:pos + k].reshape(-1, lv["C"])
            pos += k
            xt = torch.from_numpy(x.copy()).requires_grad_(True)
            bce = F.binary_cross_entropy_with_logits(xt, torch.from_numpy(t), reduction="none")
            loss = (bce * torch.from_numpy(w)).sum() / tot * cfg["cls_weight"]
            loss.backward()
            o["loss_c"] = float(loss.detach())
            o["grad_cls"] = _pad_like(lv["cls"], xt.grad.numpy() * loss_scale, lv["A"] * lv["C"])
            o["unit_c"] = _pad_like(lv["cls"], w / tot * cfg["cls_weight"] * loss_scale, lv["A"] * lv["C"])
            o["wsum_c"] = float((w / tot).sum())
            b = np.where(v[..., None], np.minimum(cfg["cls_bins"] - 1, np.floor(cls_g64(x, t) * cfg["cls_bins"])), -1)
            o["bin_c"] = _pad_like(lv["cls"], b, lv["A"] * lv["C"], fill=-1).astype(np.int64)
    if do_r:
        g_all = np.concatenate([reg_g64(dl - tg, cfg["reg_mu"])[f].reshape(-1) for _, _, _, dl, tg, f in views])
        w_all, tot, out["cnt_r"], out["coef_r"] = harmonize64(g_all, cfg["reg_bins"], cfg["reg_momentum"], acc_r)
        pos = 0
        mu = cfg["reg_mu"]
        for lv, (_, _, _, dl, tg, f), o in zip(levels, views, out["levels"]):
            k = int(f.sum()) * 4
            w = np.zeros(dl.shape)
            w[f] = w_all[pos:pos + k].reshape(-1, 4)
            pos += k
            dt = torch.from_numpy(dl.copy()).requires_grad_(True)
            diff = dt - torch.from_numpy(tg)
            asl1 = torch.sqrt(diff * diff + mu * mu) - mu
            loss = (asl1 * torch.from_numpy(w)).sum() / tot * cfg["reg_weight"]
            loss.backward()
            o["loss_r"] = float(loss.detach())
            o["grad_reg"] = _pad_like(lv["reg"], dt.grad.numpy() * loss_scale, 4 * lv["A"])
            o["unit_r"] = _pad_like(lv["reg"], w / tot * cfg["reg_weight"] * loss_scale, 4 * lv["A"])
            o["wsum_r"] = float((w / tot).sum())
            b = np.where(f[..., None], np.minimum(cfg["reg_bins"] - 1, np.floor(reg_g64(dl - tg, mu) * cfg["reg_bins"])), -1)
            o["bin_r"] = _pad_like(lv["reg"], b, 4 * lv["A"], fill=-1).astype(np.int64)
    return out


def _pad_like(like, a, real, fill=0.0):
    N, H, W, ld = like.shape
    out = np.full((N, H, W, ld), fill, np.float64)
    out[..., :real] = a.reshape(N, H, W, real)
    return out


def closed_form(g, B, momentum, acc):
    """cnt, coef by np.bincount on min(B - 1, floor(g * B)) in float64 (the definition's words); acc updated in place."""
    g = np.asarray(g, np.float64)
    cnt = np.bincount(np.minimum(B - 1, np.floor(g * B).astype(np.int64)), minlength=B) if g.size else np.zeros((B,), np.int64)
    has = cnt > 0
    acc[has] = momentum * acc[has] + (1 - momentum) * cnt[has] if momentum > 0 else cnt[has]
    coef = np.zeros((B,), np.float64)
    if has.any():
        coef[has] = 1.0 / (has.sum() * acc[has])
    return cnt, coef


# ---------------------------------------------------------------------------------------------------------------------
# float32 restatements
# ---------------------------------------------------------------------------------------------------------------------
def _u(fn, x):
    u, inv = np.unique(np.asarray(x, np.float32), return_inverse=True)
    return fn(u)[inv].reshape(np.shape(x)).astype(np.float32)


def cls_elem_fp32(x, positive):
    """(g, BCE, s - t) float32 per element, operation for operation ghm_cls_norm / GhmClsElem (sigmoid_logs)."""
    o, f = O(), np.float32
    x = np.asarray(x, f)
    positive = np.asarray(positive, bool)
    one = f(1.0)
    t = _u(o.expf, -np.abs(x))
    d = one + t
    dm1 = d - one
    sp = np.where(dm1 == 0, t, _u(o.logf, d) * (t / np.where(dm1 == 0, one, dm1))).astype(f)
    big, small = one / d, t / d
    p, q = np.where(x >= 0, big, small).astype(f), np.where(x >= 0, small, big).astype(f)
    logp = -(np.where(x < 0, -x, f(0.0)).astype(f) + sp)
    log1mp = -(np.where(x > 0, x, f(0.0)).astype(f) + sp)
    g = np.where(positive, q, p).astype(f)
    L = np.where(positive, -logp, -log1mp).astype(f)
    G = np.where(positive, -q, p).astype(f)
    return g, L, G


def reg_elem_fp32(delta, target, mu):
    """(g, sqrt(d*d + mu*mu) - mu, d / sqrt(..)) float32 per element, as ghm_reg_norm / ghm_box_part."""
    f = np.float32
    d = np.asarray(delta, f) - np.asarray(target, f)
    r = np.sqrt(d * d + f(mu) * f(mu)).astype(f)
    return (np.abs(d) / r).astype(f), (r - f(mu)).astype(f), (d / r).astype(f)


def bin_fp32(g, B):
    """ghm_bin: min(B - 1, (int)(g * (float)B)) in float32."""
    return np.minimum(B - 1, (np.asarray(g, np.float32) * np.float32(B)).astype(np.int32))


def weights_fp32(cnt, acc, momentum):
    """(acc', coef) float32 as ghm_weights_kernel: acc' = fl(fl(m * acc) + fl(fl(1 - m) * cnt)), coef = 1 / fl(n * acc')."""
    f = np.float32
    cnt = np.asarray(cnt)
    acc = np.asarray(acc, f).copy()
    has = cnt > 0
    c = cnt.astype(f)
    if momentum > 0:
        m = f(momentum)
        new = (m * acc + (f(1.0) - m) * c).astype(f)
    else:
        new = c
    acc[has] = new[has]
    coef = np.zeros(acc.shape, f)
    if has.any():
        coef[has] = f(1.0) / (f(int(has.sum())) * acc[has])
    return acc, coef
