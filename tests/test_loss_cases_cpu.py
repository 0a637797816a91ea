"""Case tables and float64 references of the fused loss kernel tests (csrc/losses.hip, csrc/retina_loss.hip, mask_loss_kernel in csrc/mask.hip),
and the proof -- without a GPU -- that every case is what it is named after. tests/test_gpu_losses.py runs the same tables
on the GPU.

References: float64 torch autograd on the textbook definitions only (binary_cross_entropy_with_logits, cross_entropy,
smooth_l1_loss(beta = 1/sigma^2), the sigmoid focal loss written with logsigmoid); nothing from include/mxdet_math.h and
nothing from the C oracle's loss functions. Every reference takes its kernel's argument layout and returns
  loss  float64 array, as the kernel reports it (normalised, NOT multiplied by loss_scale)
  grads float64 arrays in the kernel's layout = d(loss)/d(input) * loss_scale  (zeros where the kernel writes zeros)
  unit  norm * loss_scale (resp. inv_norm * grad_scale): gradients are compared after division by it.

Tolerances of the gradient comparison (on gradients divided by `unit`; bf16 outputs add 2^-8 * |ref|, one bf16 step):
  ATOL_CE    = 2^-20  softmax-CE, BCE and smooth-L1 gradients. The C oracle (an fp32 evaluation of the kernels' formulas on
                      the CPU) differs from the float64 references by at most 1.64e-7 over every case of the rpn, rcnn, mask
                      and smooth-L1 tables below, logits to +-90, weights to 2 (test_references_agree_with_the_c_oracle
                      measures and bounds it); times 4, rounded up to a power of two.
  ATOL_FOCAL = 2^-16  focal gradients. A float32 numpy restatement of the focal formula with oracle.expf / oracle.logf, with q
                      formed as 1.0f - p and softplus as log(1 + t) as the kernels did before these tests, differed from the
                      float64 reference by at most 2.94e-6 over every bf16-exact logit k/2 in [-90, 90], gamma in {0, 0.5,
                      1.5, 2, 5}, both targets (the general branch computes x^gamma as exp(gamma*log(x)), which multiplies
                      log's rounding error by gamma*|log x|); times 4, rounded up to a power of two. With the
                      cancellation-free sigmoid_softplus of csrc/loss_elem.h, which focal_fp32 below restates,
                      test_focal_fp32_error_budget measures 5.6e-7 (grid plus 1500 float32 logits ~ 3*N(0,1)) and bounds it
                      by ATOL_FOCAL / 4; the bound itself is kept at the value derived for the formula as it was.
Loss scalars: rtol 3e-5 against the float64 sum (the bound of the project's fixed-order fp32 reductions), exactly 0 where
no element contributes. A term below 2^-126, the smallest normal float32, cannot be held by an fp32 kernel at all (a
well-classified element at |z| = 90 contributes 1e-98): the comparison allows 2^-126 per summed term on top of the rtol, which
only matters where such terms are the whole sum (the single-element cases).
"""
import ctypes as C
import functools
import os
import re
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL_CE = 2.0 ** -20
ATOL_FOCAL = 2.0 ** -16
BF16_STEP = 2.0 ** -8
LOSS_RTOL = 3e-5
F32_MIN_NORMAL = 2.0 ** -126
GAMMAS = (0.0, 0.5, 1.5, 2.0, 5.0)
FOCAL_MAX_ELEMS_ONE_PASS = 2048 * 256       # cls_loss_kernel's grid cap times its block size


def O():
    from oracle import oracle as o
    o.lib()
    return o


def rng_of(case):
    return np.random.default_rng(zlib.crc32(case["id"].encode()))


def bf16r(x):
    return O().round_bf16(np.asarray(x, np.float32))


def sat_logits(rng, shape):
    """bf16-exact logits k/2, uniform in [-90, 90]: a share of them has fp32 sigmoid exactly 1, or 1 - sigmoid exactly 1."""
    return (rng.integers(-180, 181, size=shape) * 0.5).astype(np.float32)


def _t64(a, grad=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    return t.requires_grad_(True) if grad else t


# ---------------------------------------------------------------------------------------------------------------------
# float64 references (torch autograd)
# ---------------------------------------------------------------------------------------------------------------------
def _focal_terms(z, lab, Cc, alpha, gamma):
    """Sum of the sigmoid focal loss over rows with label >= 0; z [..., Cc] float64 tensor, lab [...] int64 tensor."""
    return _focal_elems(z, lab, Cc, alpha, gamma).sum()


def _focal_elems(z, lab, Cc, alpha, gamma):
    import torch
    import torch.nn.functional as F
    onehot = lab.unsqueeze(-1) == torch.arange(1, Cc + 1)
    valid = (lab >= 0).unsqueeze(-1).to(z.dtype)
    lp, ln = F.logsigmoid(z), F.logsigmoid(-z)                      # log p, log(1 - p)
    pos = -alpha * torch.exp(gamma * ln) * lp                       # -alpha (1-p)^gamma log p
    neg = -(1.0 - alpha) * torch.exp(gamma * lp) * ln               # -(1-alpha) p^gamma log(1-p)
    return torch.where(onehot, pos, neg) * valid


def _sl1_sum(d, sigma):
    import torch
    import torch.nn.functional as F
    return F.smooth_l1_loss(d, torch.zeros_like(d), beta=1.0 / sigma ** 2, reduction="sum")


def ref_focal(logits, labels, alpha, gamma, grad_scale):
    import torch
    z = _t64(logits, True)
    lab = torch.from_numpy(np.asarray(labels, np.int64))
    inv = 1.0 / max(1, int((lab > 0).sum()))
    loss = _focal_terms(z, lab, z.shape[1], alpha, gamma) * inv
    loss.backward()
    return {"loss": np.array([loss.item()]), "grad": z.grad.numpy() * grad_scale, "unit": inv * grad_scale}


def ref_retina(cls, reg, A, Cc, labels, targets, level_offset, alpha, gamma, sigma, num_fg, loss_scale):
    import torch
    N, H, W, _ = cls.shape
    n_lvl = H * W * A
    z, d = _t64(cls, True), _t64(reg, True)
    lab = torch.from_numpy(np.asarray(labels, np.int64))[:, level_offset:level_offset + n_lvl]
    tgt = _t64(targets)[:, level_offset:level_offset + n_lvl]
    inv = 1.0 / max(1, int(num_fg))
    lc = _focal_terms(z[..., :A * Cc].reshape(N, n_lvl, Cc), lab, Cc, alpha, gamma) * inv
    fg = (lab > 0).unsqueeze(-1).to(z.dtype)
    lr = _sl1_sum((d[..., :4 * A].reshape(N, n_lvl, 4) - tgt) * fg, sigma) * inv
    (lc + lr).backward()
    return {"loss": np.array([lc.item(), lr.item()]), "grad_cls": z.grad.numpy() * loss_scale,
            "grad_reg": d.grad.numpy() * loss_scale, "unit": inv * loss_scale}


def ref_rpn(head, A, labels, targets, level_offset, sigma, norm, loss_scale):
    import torch
    import torch.nn.functional as F
    N, H, W, _ = head.shape
    n_lvl = H * W * A
    h = _t64(head, True)
    lab = torch.from_numpy(np.asarray(labels, np.int64))[:, level_offset:level_offset + n_lvl]
    tgt = _t64(targets)[:, level_offset:level_offset + n_lvl]
    z = h[..., :A].reshape(N, n_lvl)
    valid = lab >= 0
    lc = F.binary_cross_entropy_with_logits(z[valid], lab[valid].to(z.dtype), reduction="sum") * norm
    fg = (lab == 1).unsqueeze(-1).to(z.dtype)
    lr = _sl1_sum((h[..., A:5 * A].reshape(N, n_lvl, 4) - tgt) * fg, sigma) * norm
    (lc + lr).backward()
    return {"loss": np.array([lc.item(), lr.item()]), "grad": h.grad.numpy() * loss_scale, "unit": norm * loss_scale}


def ref_rcnn(cls, reg, labels, tgt, wgt, num_classes, reg_dim, sigma, norm, loss_scale):
    """cls [R, >= num_classes], reg [R, >= reg_dim] (only the real widths are read); grads have the real widths."""
    import torch
    import torch.nn.functional as F
    z, d = _t64(np.asarray(cls)[:, :num_classes], True), _t64(np.asarray(reg)[:, :reg_dim], True)
    lab = torch.from_numpy(np.asarray(labels, np.int64))
    valid = lab >= 0
    lc = F.cross_entropy(z[valid], lab[valid], reduction="sum") * norm
    fg = (lab > 0).unsqueeze(-1).to(z.dtype)
    lr = _sl1_sum((d - _t64(tgt)) * _t64(wgt) * fg, sigma) * norm
    (lc + lr + 0.0 * z.sum()).backward()
    return {"loss": np.array([lc.item(), lr.item()]), "grad_cls": z.grad.numpy() * loss_scale,
            "grad_reg": d.grad.numpy() * loss_scale, "unit": norm * loss_scale}


def ref_mask(logits, cls, targets, loss_scale):
    import torch
    import torch.nn.functional as F
    R, S, _, Cpad = logits.shape
    z = _t64(logits, True)
    cls = np.asarray(cls)
    norm = 1.0 / (max(1, int((cls > 0).sum())) * S * S)
    rows = np.nonzero(cls > 0)[0]
    loss = 0.0 * z.sum()
    if len(rows):
        zz = z[torch.from_numpy(rows), :, :, torch.from_numpy(cls[rows].astype(np.int64) - 1)]       # [rows, S, S]
        loss = loss + F.binary_cross_entropy_with_logits(zz, _t64(np.asarray(targets)[rows]), reduction="sum") * norm
    loss.backward()
    return {"loss": np.array([loss.item()]), "grad": z.grad.numpy() * loss_scale, "unit": norm * loss_scale}


def ref_smooth_l1(p, t, w, go, sigma):
    """out = smooth_l1((p - t) * w); grad = d(sum(out * go))/dp."""
    import torch
    import torch.nn.functional as F
    pp = _t64(p, True)
    d = pp - _t64(t)
    if w is not None:
        d = d * _t64(w)
    out = F.smooth_l1_loss(d, torch.zeros_like(d), beta=1.0 / sigma ** 2, reduction="none")
    (out * (_t64(go) if go is not None else 1.0)).sum().backward()
    return {"out": out.detach().numpy(), "grad": pp.grad.numpy()}


# ---------------------------------------------------------------------------------------------------------------------
# case tables: every value the kernels branch on appears in at least one id (test_tables_cover_the_listed_values)
# ---------------------------------------------------------------------------------------------------------------------
def _fid(**k):
    k["id"] = "-".join("%s%s" % (a, ("%g" % v) if isinstance(v, float) else v) for a, v in k.items())
    return k


FOCAL_MIXES = ("ignore", "bg", "one", "random")


def _focal_cases():
    out, i = [], 0
    for (n, Cc) in ((1, 1), (257, 3)):
        for gamma in GAMMAS:
            for bf in (0, 1):
                for mix in FOCAL_MIXES:
                    out.append(_fid(n=n, C=Cc, g=gamma, a=(0.25, 0.5)[i % 2], bf=bf, mix=mix, gs=(1, 1024)[(i // 2) % 2], sat=0))
                    i += 1
                out.append(_fid(n=n, C=Cc, g=gamma, a=(0.25, 0.5)[i % 2], bf=bf, mix="random", gs=(1, 1024)[(i // 2) % 2], sat=1))
                i += 1
    # more than one pass of the grid-stride loop (n*C > 2048*256)
    for gamma, bf, mix, sat in ((2.0, 0, "random", 0), (2.0, 1, "random", 1), (1.5, 1, "random", 0), (0.5, 0, "one", 1),
                                (5.0, 1, "bg", 0), (0.0, 0, "random", 1)):
        out.append(_fid(n=6600, C=80, g=gamma, a=(0.25, 0.5)[i % 2], bf=bf, mix=mix, gs=(1, 1024)[(i // 2) % 2], sat=sat))
        i += 1
    return out


FOCAL_CASES = _focal_cases()


def _labels(rng, mix, shape, Cc):
    if mix == "ignore":
        return np.full(shape, -1, np.int32)
    if mix == "bg":
        return np.zeros(shape, np.int32)
    if mix == "one":
        lab = rng.choice([-1, 0, 0], size=shape).astype(np.int32)
        lab.reshape(-1)[int(rng.integers(0, lab.size))] = int(rng.integers(1, Cc + 1))
        return lab
    return rng.choice(np.arange(-1, Cc + 1), size=shape, p=[0.15, 0.55] + [0.3 / Cc] * Cc).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _focal_data(cid):
    c = next(x for x in FOCAL_CASES if x["id"] == cid)
    rng = rng_of(c)
    z = sat_logits(rng, (c["n"], c["C"])) if c["sat"] else (rng.standard_normal((c["n"], c["C"])) * 3).astype(np.float32)
    if c["bf"]:
        z = bf16r(z)
    d = {"logits": z, "labels": _labels(rng, c["mix"], (c["n"],), c["C"])}
    d["ref"] = ref_focal(z, d["labels"], c["a"], c["g"], float(c["gs"]))
    return d


def focal_data(c):
    return _focal_data(c["id"])


# retina level: (N, H, W, A, C, ld_cls, ld_reg), the form the name claims, byte offsets of the (cls, grad_cls) / (reg, grad_reg) views
RETINA_SHAPES = (
    ("coco", (2, 5, 7, 9, 80, 768, 64), "vec", 0, 0),
    ("voc", (2, 5, 7, 9, 20, 192, 64), "scalar", 0, 0),
    ("a256", (1, 4, 8, 8, 8, 64, 32), "vec", 0, 0),                  # exactly 256 anchors
    ("tight", (2, 2, 2, 9, 16, 144, 36), "vec", 0, 0),               # 72 anchors, ld == real widths
    ("c1", (1, 3, 5, 3, 1, 8, 12), "scalar", 0, 0),
    ("ld28", (1, 3, 5, 3, 8, 28, 12), "scalar", 0, 0),               # C % 8 == 0 but ld_cls % 8 != 0
    ("viewcls", (2, 5, 7, 9, 80, 768, 64), "scalar", 2, 0),          # coco's data, cls / grad_cls one bf16 element off
    ("viewreg", (2, 5, 7, 9, 80, 768, 64), "scalar", 0, 4),          # coco's data, reg / grad_reg two bf16 elements off
)
RETINA_VARIANTS = ((2.0, "true", 1, 0), (1.5, "true", 512, 0), (2.0, "one", 512, 1), (1.5, "zero", 1, 0), (1.5, "true", 1, 1))


def _retina_cases():
    out = []
    for name, shape, form, ocls, oreg in RETINA_SHAPES:
        for gamma, nfg, ls, sat in RETINA_VARIANTS:
            out.append({"id": "%s-%s-g%g-nfg%s-ls%d-sat%d" % (name, form, gamma, nfg, ls, sat), "name": name, "shape": shape,
                        "form": form, "off_cls": ocls, "off_reg": oreg, "g": gamma, "nfg": nfg, "ls": ls, "sat": sat,
                        # the view cases reuse coco's data: same seed
                        "data_id": "%s-g%g-nfg%s-ls%d-sat%d" % ("coco" if name.startswith("view") else name, gamma, nfg, ls, sat)})
    return out


RETINA_CASES = _retina_cases()
RETINA_ALPHA, RETINA_SIGMA = 0.25, 3.0


@functools.lru_cache(maxsize=None)
def _retina_data(data_id):
    c = next(x for x in RETINA_CASES if x["data_id"] == data_id)
    rng = np.random.default_rng(zlib.crc32(data_id.encode()))
    N, H, W, A, Cc, ldc, ldr = c["shape"]
    off = 23
    At = off + H * W * A + 14                                       # level_offset > 0, A_total larger than the level
    cls = sat_logits(rng, (N, H, W, ldc)) if c["sat"] else bf16r(rng.standard_normal((N, H, W, ldc)) * 2 - 2)
    d = {"cls": cls, "reg": bf16r(rng.standard_normal((N, H, W, ldr)) * 0.5), "A_total": At, "off": off,
         "labels": _labels(rng, "random", (N, At), Cc), "targets": (rng.standard_normal((N, At, 4)) * 0.3).astype(np.float32)}
    n_lvl = H * W * A
    d["labels"][0, off], d["labels"][0, off + 1] = Cc, 1            # last and first class on the level's first anchors ...
    d["labels"][-1, off + n_lvl - 1], d["labels"][-1, off + n_lvl - 2] = Cc, -1     # ... and on its last ones
    d["labels"][:, :off], d["labels"][:, off + n_lvl:] = 1, 1       # foreground of other levels: counted, not visited
    d["num_fg"] = {"true": int((d["labels"] > 0).sum()), "one": 1, "zero": 0}[c["nfg"]]
    d["ref"] = ref_retina(cls, d["reg"], A, Cc, d["labels"], d["targets"], off, RETINA_ALPHA, c["g"], RETINA_SIGMA, d["num_fg"],
                          float(c["ls"]))
    return d


def retina_data(c):
    return _retina_data(c["data_id"])


# rpn level: (N, H, W, A, Cpad); the last one is not in the issue's list: the only one with a second, partly empty workgroup
RPN_SHAPES = ((2, 5, 7, 3, 16), (1, 16, 16, 1, 5), (2, 3, 3, 9, 48), (1, 1, 1, 3, 15), (1, 16, 16, 3, 24), (1, 17, 16, 3, 16))
RPN_SIGMA, RPN_NORM = 3.0, 1.0 / 256


def _rpn_cases():
    out, i = [], 0
    for shape in RPN_SHAPES:
        for mix, sat in (("ignore", 0), ("fg", 0), ("random", 0), ("random", 1)):
            ls = (1, 1024)[i % 2]
            out.append({"id": "%s-%s-ls%d-sat%d" % ("x".join(map(str, shape)), mix, ls, sat), "shape": shape, "mix": mix, "ls": ls,
                        "sat": sat})
            i += 1
        i += 1
    return out


RPN_CASES = _rpn_cases()


@functools.lru_cache(maxsize=None)
def _rpn_data(cid):
    c = next(x for x in RPN_CASES if x["id"] == cid)
    rng = rng_of(c)
    N, H, W, A, Cp = c["shape"]
    off = 11
    At = off + H * W * A + 29
    head = sat_logits(rng, (N, H, W, Cp)) if c["sat"] else bf16r(rng.standard_normal((N, H, W, Cp)) * 1.5)
    lab = {"ignore": lambda: np.full((N, At), -1, np.int32), "fg": lambda: np.ones((N, At), np.int32),
           "random": lambda: rng.choice([-1, -1, 0, 1], size=(N, At)).astype(np.int32)}[c["mix"]]()
    d = {"head": head, "labels": lab, "targets": (rng.standard_normal((N, At, 4)) * 0.5).astype(np.float32), "A_total": At, "off": off}
    d["ref"] = ref_rpn(head, A, lab, d["targets"], off, RPN_SIGMA, RPN_NORM, float(c["ls"]))
    return d


def rpn_data(c):
    return _rpn_data(c["id"])


RCNN_CLASSES, RCNN_ROIS = (2, 21, 64, 65, 81, 129), (1, 5, 37)
RCNN_WEIGHTS = (0.0, 0.5, 1.0, 2.0)


def _rcnn_cases():
    out, i = [], 0
    for nc in RCNN_CLASSES:
        for R in RCNN_ROIS:
            for bf in (0, 1):
                agnostic, fused, ls, sat = i % 2, (i // 2) % 2, (1, 256)[(i // 3) % 2], int(i % 5 == 4)
                out.append({"id": "nc%d-R%d-%s-%s-%s-ls%d-sat%d" % (nc, R, "bf16" if bf else "f32", "reg4" if agnostic else "reg4nc",
                                                                  "fused" if fused else "tight", ls, sat),
                            "nc": nc, "R": R, "bf": bf, "reg_dim": 4 if agnostic else 4 * nc, "fused": fused, "ls": ls, "sat": sat})
                i += 1
            i += 1
    return out


RCNN_CASES = _rcnn_cases()
RCNN_SIGMA = 1.0
TIED_ROW, PEAK_ROW = 0, 1                                           # special rows of every case with R >= 5


@functools.lru_cache(maxsize=None)
def _rcnn_data(cid):
    c = next(x for x in RCNN_CASES if x["id"] == cid)
    rng = rng_of(c)
    nc, R, rd = c["nc"], c["R"], c["reg_dim"]
    ld = nc + rd + 11 if c["fused"] else None                       # fused: one buffer, ld > the two widths together
    cls = sat_logits(rng, (R, nc)) if c["sat"] else (rng.standard_normal((R, nc)) * 2).astype(np.float32)
    reg = rng.standard_normal((R, rd)).astype(np.float32)
    labels = rng.integers(-1, nc, R).astype(np.int32)
    if R >= 5:
        cls[TIED_ROW] = -1.0
        cls[TIED_ROW, [0, nc - 1]] = 3.0                            # two equal maxima, first and last class
        labels[TIED_ROW] = nc - 1
        cls[PEAK_ROW] = -80.0
        cls[PEAK_ROW, nc // 2] = 80.0                               # one +80 among -80s; the label is one of the -80s
        labels[PEAK_ROW] = (nc // 2 + 1) % nc
        labels[2], labels[3] = -1, 0                                # an ignored row and a background row
    if c["bf"]:
        cls, reg = bf16r(cls), bf16r(reg)
    d = {"cls": cls, "reg": reg, "labels": labels, "tgt": rng.standard_normal((R, rd)).astype(np.float32),
         "wgt": rng.choice(RCNN_WEIGHTS, size=(R, rd)).astype(np.float32), "ld": ld, "norm": 1.0 / R}
    d["ref"] = ref_rcnn(cls, reg, labels, d["tgt"], d["wgt"], nc, rd, RCNN_SIGMA, d["norm"], float(c["ls"]))
    return d


def rcnn_data(c):
    return _rcnn_data(c["id"])


MASK_SHAPES = ((5, 14, 8), (3, 28, 88), (9, 7, 16), (1, 7, 8))     # (R, S, Cpad)


def _mask_cases():
    out, i = [], 0
    for shape in MASK_SHAPES:
        mixes = (("first", 0), ("last", 0), ("last", 1), ("ignore", 0)) if shape[0] == 1 else \
            (("mixed", 0), ("mixed", 1), ("ignore", 0))
        for mix, sat in mixes:
            ls = (1, 512)[i % 2]
            out.append({"id": "%s-%s-ls%d-sat%d" % ("x".join(map(str, shape)), mix, ls, sat), "shape": shape, "mix": mix, "ls": ls,
                        "sat": sat})
            i += 1
    return out


MASK_CASES = _mask_cases()


@functools.lru_cache(maxsize=None)
def _mask_data(cid):
    c = next(x for x in MASK_CASES if x["id"] == cid)
    rng = rng_of(c)
    R, S, Cp = c["shape"]
    logits = sat_logits(rng, (R, S, S, Cp)) if c["sat"] else bf16r(rng.standard_normal((R, S, S, Cp)) * 2)
    if c["mix"] == "ignore":
        cls = np.full(R, -1, np.int32)
    elif c["mix"] == "first":
        cls = np.ones(R, np.int32)
    elif c["mix"] == "last":
        cls = np.full(R, Cp, np.int32)
    else:
        cls = rng.integers(1, Cp + 1, R).astype(np.int32)
        cls[0], cls[1], cls[2] = 1, Cp, -1                          # first channel, last channel, an ignored roi
    d = {"logits": logits, "cls": cls, "targets": (rng.uniform(size=(R, S, S)) < 0.4).astype(np.uint8)}
    d["ref"] = ref_mask(logits, cls, d["targets"], float(c["ls"]))
    return d


def mask_data(c):
    return _mask_data(c["id"])


SL1_CASES = [{"id": "n%d-s%d-w%d-go%d-acc%d" % (n, s, w, go, acc), "n": n, "sigma": float(s), "w": w, "go": go, "acc": acc}
             for n in (1, 255, 256, 257) for s in (1, 2, 3) for w in (0, 1) for go in (0, 1) for acc in (0, 1)]
SL1_BREAKPOINTS = (0.0, 0.25, -0.25)                                # with sigma = 2: x = 0 and x = +-1/sigma^2, all exact


@functools.lru_cache(maxsize=None)
def _sl1_data(cid):
    c = next(x for x in SL1_CASES if x["id"] == cid)
    rng = rng_of(c)
    n = c["n"]
    t = (rng.integers(-8, 9, n) * 0.25).astype(np.float32)
    p = (t + rng.standard_normal(n).astype(np.float32) * (0.6 / c["sigma"] ** 2 + 0.2)).astype(np.float32)
    w = rng.choice(RCNN_WEIGHTS, size=n).astype(np.float32) if c["w"] else None
    if c["sigma"] == 2.0:
        k = min(n, 3)
        p[:k] = t[:k] + np.array(SL1_BREAKPOINTS[:k], np.float32)   # multiples of 1/4: the differences are exact
        if w is not None:
            w[:k] = 1.0
    d = {"p": p, "t": t, "w": w, "go": rng.uniform(0.25, 1.0, n).astype(np.float32) if c["go"] else None,
         "prefill": (rng.integers(-2, 3, n) * 0.5).astype(np.float32)}
    d["ref"] = ref_smooth_l1(p, t, w, d["go"], c["sigma"])
    return d


def sl1_data(c):
    return _sl1_data(c["id"])


FINALIZE_CASES = [{"id": "count%d-ncomp%d" % (n, k), "count": n, "ncomp": k} for n in (0, 1, 255, 256, 257, 5000) for k in (1, 2, 8)]


def finalize_data(c):
    rng = rng_of(c)
    part = rng.uniform(0.0, 1.0, (max(c["count"], 1), c["ncomp"])).astype(np.float32)     # one spare row when count == 0
    return {"partial": part, "ref": part[:c["count"]].astype(np.float64).sum(axis=0)}


def ids(cases):
    return [c["id"] for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# float32 restatement of focal_cls_elem's formula (CPU; only used to size ATOL_FOCAL, never as a reference)
# ---------------------------------------------------------------------------------------------------------------------
def focal_fp32(z, positive, alpha, gamma):
    """(loss term, d(focal)/dz) per element as focal_cls_elem evaluates them: float32 throughout, oracle.expf / oracle.logf."""
    o, f = O(), np.float32
    z = np.asarray(z, f)
    t = o.expf(-np.abs(z))
    d = f(1.0) + t
    dm1 = d - f(1.0)
    sp = np.where(dm1 == 0, t, o.logf(d) * (t / np.where(dm1 == 0, f(1.0), dm1))).astype(f)
    big, small = f(1.0) / d, t / d
    p, q = np.where(z >= 0, big, small).astype(f), np.where(z >= 0, small, big).astype(f)
    logp = -(np.where(z < 0, -z, f(0.0)).astype(f) + sp)
    log1mp = -(np.where(z > 0, z, f(0.0)).astype(f) + sp)
    al, ga = f(alpha), f(gamma)

    def power(x):
        return x * x if gamma == 2.0 else o.expf(ga * o.logf(np.maximum(x, f(1e-30))))
    gpos = -al * power(q) * (q - ga * p * logp)
    gneg = (f(1.0) - al) * power(p) * (p - ga * q * log1mp)
    lpos, lneg = -al * power(q) * logp, -(f(1.0) - al) * power(p) * log1mp
    return np.where(positive, lpos, lneg).astype(f), np.where(positive, gpos, gneg).astype(f)


# ---------------------------------------------------------------------------------------------------------------------
# proofs
# ---------------------------------------------------------------------------------------------------------------------
def _sigmoid32(z):
    return (1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))).astype(np.float32)


def _assert_saturated(z):
    assert np.array_equal(bf16r(z), z), "saturated logits must be bf16-exact"
    assert np.abs(z).max() <= 90.0
    if z.size >= 64:
        p = _sigmoid32(z)
        assert np.any(p == 1.0), "no element with fp32 sigmoid == 1.0"
        assert np.any(np.float32(1.0) - p == 1.0), "no element with fp32 1 - sigmoid == 1.0"
        assert np.any(np.abs(z) < 10.0)


def test_tables_cover_the_listed_values():
    def vals(cases, key):
        return {c[key] for c in cases}
    assert {(c["n"], c["C"]) for c in FOCAL_CASES} == {(1, 1), (257, 3), (6600, 80)}
    for shape in ((1, 1), (257, 3), (6600, 80)):
        sub = [c for c in FOCAL_CASES if (c["n"], c["C"]) == shape]
        assert vals(sub, "g") == set(GAMMAS) and vals(sub, "bf") == {0, 1} and vals(sub, "sat") == {0, 1}
        assert vals(sub, "a") == {0.25, 0.5} and vals(sub, "gs") == {1, 1024}
    assert vals(FOCAL_CASES, "mix") == set(FOCAL_MIXES)
    for name, *_ in RETINA_SHAPES:
        sub = [c for c in RETINA_CASES if c["name"] == name]
        assert vals(sub, "g") == {2.0, 1.5} and vals(sub, "nfg") == {"zero", "one", "true"}
        assert vals(sub, "ls") == {1, 512} and vals(sub, "sat") == {0, 1}
    for shape in RPN_SHAPES:
        sub = [c for c in RPN_CASES if c["shape"] == shape]
        assert vals(sub, "mix") == {"ignore", "fg", "random"} and vals(sub, "sat") == {0, 1}
    assert vals(RPN_CASES, "ls") == {1, 1024}
    assert {(c["nc"], c["R"], c["bf"]) for c in RCNN_CASES} == {(a, b, d) for a in RCNN_CLASSES for b in RCNN_ROIS for d in (0, 1)}
    for nc in RCNN_CLASSES:
        sub = [c for c in RCNN_CASES if c["nc"] == nc]
        assert vals(sub, "reg_dim") == {4, 4 * nc} and vals(sub, "fused") == {0, 1}
    assert vals(RCNN_CASES, "sat") == {0, 1} and vals(RCNN_CASES, "ls") == {1, 256}
    for shape in MASK_SHAPES:
        sub = [c for c in MASK_CASES if c["shape"] == shape]
        assert "ignore" in vals(sub, "mix") and vals(sub, "sat") == {0, 1}
    assert vals(MASK_CASES, "ls") == {1, 512}
    for table in (FOCAL_CASES, RETINA_CASES, RPN_CASES, RCNN_CASES, MASK_CASES, SL1_CASES, FINALIZE_CASES):
        assert len(set(ids(table))) == len(table)


@pytest.mark.parametrize("c", FOCAL_CASES, ids=ids(FOCAL_CASES))
def test_focal_case_is_what_it_is_named(c):
    d = focal_data(c)
    total, lab = c["n"] * c["C"], d["labels"]
    if c["n"] == 6600:
        assert total > FOCAL_MAX_ELEMS_ONE_PASS and total % (FOCAL_MAX_ELEMS_ONE_PASS) != 0      # second pass, partly idle
    if c["n"] == 257:
        assert 256 < total < FOCAL_MAX_ELEMS_ONE_PASS and total % 256 != 0                       # tail workgroup
    nfg = int((lab > 0).sum())
    assert {"ignore": np.all(lab == -1), "bg": np.all(lab == 0), "one": nfg == 1,
            "random": c["n"] < 200 or (nfg > 1 and np.any(lab == -1) and np.any(lab == 0))}[c["mix"]]
    if c["n"] == 6600 and c["mix"] == "random":
        assert set(np.unique(lab)) == set(range(-1, c["C"] + 1))                                  # first and last class
    if c["bf"] or c["sat"]:
        assert np.array_equal(bf16r(d["logits"]), d["logits"])
    if c["sat"]:
        _assert_saturated(d["logits"])
    if nfg == 0:
        assert d["ref"]["unit"] == c["gs"]
    if c["mix"] == "ignore":
        assert d["ref"]["loss"][0] == 0.0 and not d["ref"]["grad"].any()


def retina_route(c, L=None):
    """(vec, grid) of the case as the library's own selector reports it (route probe; dummy pointers, no device access)."""
    from mxdetection_amd import _lib
    L = L or _lib.load()
    N, H, W, A, Cc, ldc, ldr = c["shape"]
    base = 1 << 20
    pc, pr, dummy = C.c_void_p(base + c["off_cls"]), C.c_void_p(base + c["off_reg"]), C.c_void_p(base)
    L.mxdet_debug_route_probe(1)
    try:
        rc = L.mxdet_retina_loss_level(pc, pr, N, H, W, A, Cc, ldc, ldr, dummy, dummy, 23 + H * W * A + 14, 23, RETINA_ALPHA, c["g"],
                                       RETINA_SIGMA, dummy, float(c["ls"]), pc, pr, dummy, None)
        assert rc == 0, L.mxdet_last_error()
        buf = (C.c_int32 * 64)()
        assert L.mxdet_debug_route_read(buf, 4) == 1
    finally:
        L.mxdet_debug_route_probe(0)
    assert buf[0] == _lib.ROUTE_KINDS["RETINA_LOSS"] and not any(buf[3:16])
    return bool(buf[1]), buf[2]


@pytest.mark.parametrize("c", RETINA_CASES, ids=ids(RETINA_CASES))
def test_retina_case_is_what_it_is_named(c):
    from mxdetection_amd import _lib
    d = retina_data(c)
    N, H, W, A, Cc, ldc, ldr = c["shape"]
    total = N * H * W * A
    vec, grid = retina_route(c)
    assert vec == (c["form"] == "vec")                                      # asked of the library, not re-stated
    assert grid == _lib.load().mxdet_retina_loss_num_partials(N, H, W, A) == (total + 255) // 256
    assert ldc >= A * Cc and ldr >= 4 * A and d["off"] > 0 and d["A_total"] > d["off"] + H * W * A
    assert {"coco": total > 256 and total % 256 != 0 and ldc > A * Cc and ldr > 4 * A, "voc": Cc % 8 != 0 and total % 256 != 0,
            "a256": total == 256, "tight": total < 256 and ldc == A * Cc and ldr == 4 * A, "c1": Cc == 1,
            "ld28": Cc % 8 == 0 and ldc % 8 != 0, "viewcls": c["off_cls"] == 2 and c["off_reg"] == 0,
            "viewreg": c["off_cls"] == 0 and c["off_reg"] == 4}[c["name"]]
    if c["name"].startswith("view"):                                        # the same data, aligned, is a vector case
        assert retina_route(dict(c, off_cls=0, off_reg=0))[0]
        assert d is retina_data(next(x for x in RETINA_CASES if x["name"] == "coco" and x["data_id"] == c["data_id"]))
    lv = d["labels"][:, d["off"]:d["off"] + H * W * A]
    assert np.any(lv > 0) and np.any(lv == 0) and np.any(lv == -1) or total < 64
    if total > 256:
        assert np.any(lv == Cc) and np.any(lv == 1)
    assert d["num_fg"] == {"zero": 0, "one": 1, "true": int((d["labels"] > 0).sum())}[c["nfg"]]
    assert c["nfg"] != "true" or d["num_fg"] > int((lv > 0).sum()) > 0     # the normaliser is global, not the level's count
    if c["sat"]:
        _assert_saturated(d["cls"])


def test_retina_probe_validates_and_leaves_no_state():
    from mxdetection_amd import _lib
    L = _lib.load()
    dummy = C.c_void_p(1 << 20)
    L.mxdet_debug_route_probe(1)
    try:
        # arguments are validated as usual while the probe is on
        assert L.mxdet_retina_loss_level(dummy, dummy, 1, 3, 5, 3, 8, 16, 12, dummy, dummy, 100, 0, 0.25, 2.0, 3.0, dummy, 1.0, dummy,
                                         dummy, dummy, None) == -2
        assert L.mxdet_retina_loss_level(None, dummy, 1, 3, 5, 3, 8, 24, 12, dummy, dummy, 100, 0, 0.25, 2.0, 3.0, dummy, 1.0, dummy,
                                         dummy, dummy, None) == -1
        assert L.mxdet_retina_loss_level(dummy, dummy, 1, 3, 5, 3, 8, 24, 12, dummy, dummy, 44, 0, 0.25, 2.0, 3.0, dummy, 1.0, dummy,
                                         dummy, dummy, None) == -2
        buf = (C.c_int32 * 64)()
        assert L.mxdet_debug_route_read(buf, 4) == 0
    finally:
        L.mxdet_debug_route_probe(0)
    hdr = open(os.path.join(ROOT, "include", "mxdet_debug.h")).read()
    assert {k: int(v) for k, v in re.findall(r"#define MXDET_ROUTE_([A-Z_]+) (\d+)", hdr) if k not in ("WORDS", "MAX")} == _lib.ROUTE_KINDS


@pytest.mark.parametrize("c", RPN_CASES, ids=ids(RPN_CASES))
def test_rpn_case_is_what_it_is_named(c):
    d = rpn_data(c)
    N, H, W, A, Cp = c["shape"]
    cells = N * H * W
    assert {(2, 5, 7, 3, 16): cells < 256 and Cp > 5 * A, (1, 16, 16, 1, 5): cells == 256 and A == 1 and Cp == 5 * A,
            (2, 3, 3, 9, 48): cells < 64 and Cp > 5 * A, (1, 1, 1, 3, 15): cells == 1 and Cp == 5 * A,
            (1, 16, 16, 3, 24): cells == 256 and Cp > 5 * A, (1, 17, 16, 3, 16): 256 < cells < 512}[c["shape"]]
    lv = d["labels"][:, d["off"]:d["off"] + H * W * A]
    assert {"ignore": np.all(lv == -1), "fg": np.all(lv == 1),
            "random": cells == 1 or all(np.any(lv == v) for v in (-1, 0, 1))}[c["mix"]]
    if c["sat"]:
        _assert_saturated(d["head"])
    if c["mix"] == "ignore":
        assert not d["ref"]["loss"].any() and not d["ref"]["grad"].any()
    assert not d["ref"]["grad"][..., 5 * A:].any()


@pytest.mark.parametrize("c", RCNN_CASES, ids=ids(RCNN_CASES))
def test_rcnn_case_is_what_it_is_named(c):
    d = rcnn_data(c)
    nc, R = c["nc"], c["R"]
    assert {2: nc < 64, 21: nc < 64, 64: nc == 64, 65: nc == 65, 81: 64 < nc < 128, 129: nc > 128}[nc]
    assert {1: R < 4, 5: R % 4 == 1, 37: R % 4 == 1 and R > 32}[R]                 # a partly empty last workgroup everywhere
    assert c["reg_dim"] in (4, 4 * nc) and (d["ld"] is None or d["ld"] > nc + c["reg_dim"])
    assert set(np.unique(d["wgt"])) <= set(RCNN_WEIGHTS) and (d["wgt"].size < 16 or len(np.unique(d["wgt"])) == 4)
    if R >= 5:
        row = d["cls"][TIED_ROW]
        assert (row == row.max()).sum() == 2 and row[0] == row[-1] == row.max()
        row = d["cls"][PEAK_ROW]
        assert (row == 80.0).sum() == 1 and (row == -80.0).sum() == nc - 1 and row[d["labels"][PEAK_ROW]] == -80.0
        assert abs(d["ref"]["grad_cls"][PEAK_ROW, d["labels"][PEAK_ROW]] / d["ref"]["unit"] + 1.0) < 1e-12
        assert d["labels"][2] == -1 and not d["ref"]["grad_cls"][2].any() and not d["ref"]["grad_reg"][2].any()
        assert d["labels"][3] == 0 and d["ref"]["grad_cls"][3].any() and not d["ref"]["grad_reg"][3].any()
    if c["bf"] or c["sat"]:
        assert np.array_equal(bf16r(d["cls"]), d["cls"])
    if c["sat"] and R >= 5:
        _assert_saturated(d["cls"][4:])


@pytest.mark.parametrize("c", MASK_CASES, ids=ids(MASK_CASES))
def test_mask_case_is_what_it_is_named(c):
    d = mask_data(c)
    R, S, Cp = c["shape"]
    pix = R * S * S
    assert {(5, 14, 8): Cp == 8 and pix % 256 != 0, (3, 28, 88): Cp % 16 == 8 and pix > 256, (9, 7, 16): pix > 256 and pix % 256 != 0,
            (1, 7, 8): Cp == 8 and pix < 256}[c["shape"]]
    cls = d["cls"]
    assert {"ignore": np.all(cls == -1), "first": np.all(cls == 1), "last": np.all(cls == Cp),
            "mixed": np.any(cls == 1) and np.any(cls == Cp) and np.any(cls == -1)}[c["mix"]]
    if c["sat"]:
        _assert_saturated(d["logits"])
    if c["mix"] == "ignore":
        assert d["ref"]["loss"][0] == 0.0 and not d["ref"]["grad"].any()
    else:
        assert 0 < d["targets"][cls > 0].mean() < 1


@pytest.mark.parametrize("c", SL1_CASES, ids=ids(SL1_CASES))
def test_smooth_l1_case_is_what_it_is_named(c):
    d = sl1_data(c)
    assert (d["w"] is None) == (c["w"] == 0) and (d["go"] is None) == (c["go"] == 0)
    if c["sigma"] == 2.0:
        k = min(c["n"], 3)
        x = (d["p"] - d["t"])[:k]
        assert np.array_equal(x, np.array(SL1_BREAKPOINTS[:k], np.float32))
        assert np.allclose(d["ref"]["out"][:k], np.array([0.0, 0.125, 0.125])[:k], atol=0, rtol=0)
    if c["n"] >= 255:
        inv = 1.0 / c["sigma"] ** 2
        x = np.abs((d["p"] - d["t"]) * (1.0 if d["w"] is None else d["w"]))
        assert np.any(x < inv) and np.any(x > inv)                            # both branches


def test_finalize_cases_straddle_the_workgroup():
    assert [c["count"] for c in FINALIZE_CASES if c["ncomp"] == 1] == [0, 1, 255, 256, 257, 5000]       # 0, <, ==, > 256, many passes
    assert {c["ncomp"] for c in FINALIZE_CASES} == {1, 2, 8}
    assert not finalize_data(FINALIZE_CASES[0])["ref"].any()


# ---- the float64 references against the C oracle: the first check of the shared mxdet_math.h formulas against something
# that does not include them -------------------------------------------------------------------------------------------
def _err(got, ref, unit):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / unit)) if np.size(ref) else 0.0


def test_references_agree_with_the_c_oracle():
    o = O()
    worst = {"rpn": 0.0, "rcnn": 0.0, "mask": 0.0, "sl1": 0.0}
    for c in RPN_CASES:
        d, r = rpn_data(c), rpn_data(c)["ref"]
        loss, grad = o.rpn_loss_level(d["head"], c["shape"][3], d["labels"], d["targets"], d["off"], RPN_SIGMA, RPN_NORM, float(c["ls"]))
        assert np.allclose(loss, r["loss"], rtol=1e-6, atol=0), c["id"]
        worst["rpn"] = max(worst["rpn"], _err(grad, r["grad"], r["unit"]))
    for c in RCNN_CASES:
        d, r = rcnn_data(c), rcnn_data(c)["ref"]
        loss, gc, gr = o.rcnn_loss(d["cls"], d["reg"], d["labels"], d["tgt"], d["wgt"], c["nc"], c["reg_dim"], RCNN_SIGMA, d["norm"],
                                   float(c["ls"]))
        assert np.allclose(loss, r["loss"], rtol=1e-6, atol=0), c["id"]
        worst["rcnn"] = max(worst["rcnn"], _err(gc, r["grad_cls"], r["unit"]), _err(gr, r["grad_reg"], r["unit"]))
    for c in MASK_CASES:
        d, r = mask_data(c), mask_data(c)["ref"]
        loss, grad = o.mask_loss(d["logits"], d["cls"], d["targets"], float(c["ls"]))
        assert np.allclose(loss, r["loss"], rtol=1e-6, atol=0), c["id"]
        worst["mask"] = max(worst["mask"], _err(grad, r["grad"], r["unit"]))
    for c in SL1_CASES:
        d, r = sl1_data(c), sl1_data(c)["ref"]
        out, grad = o.smooth_l1(d["p"], d["t"], d["w"], c["sigma"])
        go = 1.0 if d["go"] is None else d["go"]
        worst["sl1"] = max(worst["sl1"], _err(out, r["out"], 1.0), _err(grad * go, r["grad"], 1.0))
    print("oracle (fp32) vs float64 reference, max gradient error / unit:", worst)
    assert max(worst.values()) <= ATOL_CE / 4, worst


def test_references_agree_with_the_c_oracle_focal_and_retina():
    """oracle_focal_loss is float64 C, written independently of torch: the two must agree to fp32 output rounding."""
    o = O()
    worst = 0.0
    for c in FOCAL_CASES:
        d, r = focal_data(c), focal_data(c)["ref"]
        loss, grad = o.focal_loss(d["logits"], d["labels"], c["a"], c["g"], float(c["gs"]))
        assert np.allclose(loss, r["loss"], rtol=1e-9, atol=0), c["id"]
        worst = max(worst, _err(grad, r["grad"], r["unit"]))
    for c in RETINA_CASES:
        d, r = retina_data(c), retina_data(c)["ref"]
        N, H, W, A, Cc, ldc, ldr = c["shape"]
        n_lvl = H * W * A
        lv = d["labels"][:, d["off"]:d["off"] + n_lvl].reshape(-1)
        loss, grad = o.focal_loss(d["cls"][..., :A * Cc].reshape(-1, Cc), lv, RETINA_ALPHA, c["g"], 1.0)
        lvl_fg, inv = max(1, int((lv > 0).sum())), 1.0 / max(1, d["num_fg"])
        assert np.isclose(loss[0] * lvl_fg * inv, r["loss"][0], rtol=1e-9, atol=0), c["id"]
        worst = max(worst, _err(grad.astype(np.float64) * lvl_fg * r["unit"], r["grad_cls"][..., :A * Cc].reshape(-1, Cc), r["unit"]))
        fg = lv > 0
        l1, g1 = o.smooth_l1(d["reg"][..., :4 * A].reshape(-1, 4)[fg], d["targets"][:, d["off"]:d["off"] + n_lvl].reshape(-1, 4)[fg],
                             None, RETINA_SIGMA)
        assert np.isclose(l1.astype(np.float64).sum() * inv, r["loss"][1], rtol=1e-6, atol=0), c["id"]
        gr = r["grad_reg"][..., :4 * A].reshape(-1, 4)
        assert _err(g1, gr[fg] / r["unit"], 1.0) <= ATOL_CE / 4 and not gr[~fg].any()
        assert not r["grad_cls"][..., A * Cc:].any() and not r["grad_reg"][..., 4 * A:].any()
    print("oracle focal (float64, fp32 output) vs float64 reference, max gradient error / unit:", worst)
    assert worst <= ATOL_FOCAL / 4


def test_focal_fp32_error_budget():
    """ATOL_FOCAL: float32 evaluation of focal_cls_elem's formula (oracle.expf / oracle.logf) against float64 autograd over
    every bf16-exact logit k/2 in [-90, 90], both targets, every gamma of the table."""
    import torch
    z = np.concatenate([np.arange(-180, 181) * 0.5, (np.random.default_rng(5).standard_normal(1500) * 3).astype(np.float32)])
    worst = 0.0
    for gamma in GAMMAS:
        for alpha in (0.25, 0.5):
            for positive in (False, True):
                zt = _t64(z.reshape(-1, 1), True)
                lab = torch.full((z.size,), 1 if positive else 0, dtype=torch.int64)
                _focal_terms(zt, lab, 1, alpha, gamma).backward()
                l32, g32 = focal_fp32(z, positive, alpha, gamma)
                worst = max(worst, float(np.max(np.abs(g32.astype(np.float64) - zt.grad.numpy().reshape(-1)))))
                # the loss term of every single element holds the bound of the sums (what the one-element cases rest on)
                l64 = _focal_elems(zt.detach(), lab, 1, alpha, gamma).numpy().reshape(-1)
                assert np.all(np.abs(l32 - l64) <= LOSS_RTOL * l64 + F32_MIN_NORMAL), (gamma, alpha, positive)
    print("fp32 focal formula vs float64 autograd, max gradient error:", worst)
    assert worst <= ATOL_FOCAL / 4


# ---- the references notice the mistakes the GPU module is there to catch (each re-created on the reference side) ------
def test_references_are_sensitive_to_the_listed_mistakes():
    # dropping the gamma*p*logp term: the fp32 restatement without it leaves the focal tolerance by orders of magnitude
    import torch
    z = np.arange(-16, 17) * 0.5
    zt = _t64(z.reshape(-1, 1), True)
    _focal_terms(zt, torch.ones(z.size, dtype=torch.int64), 1, 0.25, 1.5).backward()
    p = 1.0 / (1.0 + np.exp(-z))
    dropped = -0.25 * (1 - p) ** 1.5 * (1 - p)
    assert np.max(np.abs(dropped - zt.grad.numpy().reshape(-1))) > 1000 * ATOL_FOCAL
    # lab == c instead of c + 1: another column carries the positive term
    c = next(x for x in FOCAL_CASES if x["n"] == 257 and x["mix"] == "random" and not x["sat"])
    d = focal_data(c)
    shifted = ref_focal(d["logits"], np.where(d["labels"] > 0, d["labels"] - 1, d["labels"]), c["a"], c["g"], float(c["gs"]))
    assert np.max(np.abs(shifted["grad"] - d["ref"]["grad"]) / d["ref"]["unit"]) > 1000 * ATOL_FOCAL
    # forgetting the second *w: wrong wherever the weight is 0.5 or 2
    c = next(x for x in RCNN_CASES if x["R"] == 37 and not x["sat"])
    d = rcnn_data(c)
    w = d["wgt"].astype(np.float64)
    once = np.where(w != 0, d["ref"]["grad_reg"] / np.where(w != 0, w, 1.0), 0.0)
    assert np.max(np.abs(once - d["ref"]["grad_reg"]) / d["ref"]["unit"]) > 1000 * ATOL_CE
