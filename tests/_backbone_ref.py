"""fp64 reference of the backbone blocks and the FPN necks (models/backbones/resnet.py, models/necks/fpn.py), forward and an
explicit, hand-written backward, for tests/test_gpu_backbone_blocks.py and tests/test_gpu_fpn_necks.py. torch-CPU float64
throughout; maps are NHWC, filters [Cout, KH, KW, Cin], bf16 tensors are float64 tensors that hold bf16 values.

Every function has emulate=False/True. emulate=True rounds to bf16 every map the device stores -- activations, the projection
shortcut, inner / P maps and each stored data-gradient map (a gradient that is accumulated into a buffer is rounded once more,
as the sum) -- and nothing else: weight and bias gradients stay unrounded (fp32 on the device). The emulated variants exist to
MEASURE the error inherent in the number formats, E = max |emulated - exact|; the GPU tests derive their tolerances from it
(check_rows). No device result enters E.

The backward functions take the ReLU masks as arguments (float64 0/1 maps). Backward through a ReLU is not continuous in the
activation: a device activation that differs from the exact one by a rounding near zero is no error, but it switches a whole
gradient path. The GPU tests therefore pass the masks of the device's stored activations, the ones the model itself uses, and
the backward reference is the exact linear adjoint under those masks; tests/test_backbone_ref_cpu.py passes the masks of the
reference's own forward and compares with torch.autograd of the plain composition.

Gradient convention of the backbone (Bottleneck.backward): a gradient travels "already masked": `ds` is the gradient w.r.t. a
block's pre-activation sum, i.e. the gradient arriving at y times (y > 0), and the returned dx is the total gradient arriving
at x times (x > 0).
"""
import torch
import torch.nn.functional as F

from _carafe_ref import F64, nearest_up, round_bf16


def _st(emulate):
    return round_bf16 if emulate else (lambda t: t)


# ---- single convolutions and their adjoints -------------------------------------------------------------------------------
def _pad(w, pad):
    return w.shape[1] // 2 if pad is None else pad


def conv(x, w, b=None, stride=1, pad=None):
    """x [N, H, W, Cin], w [Cout, KH, KW, Cin] -> [N, Ho, Wo, Cout]; pad defaults to k // 2."""
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, stride=stride, padding=_pad(w, pad))
    return y.permute(0, 2, 3, 1).contiguous()


def conv_dgrad(dy, w, x_shape, stride=1, pad=None):
    """Adjoint of conv w.r.t. x: [N, Ho, Wo, Cout] -> x_shape."""
    N, H, W, Cin = x_shape
    dx = torch.nn.grad.conv2d_input((N, Cin, H, W), w.permute(0, 3, 1, 2).contiguous(), dy.permute(0, 3, 1, 2).contiguous(),
                                    stride=stride, padding=_pad(w, pad))
    return dx.permute(0, 2, 3, 1).contiguous()


def conv_wgrad(x, dy, w, stride=1, pad=None):
    """Adjoint of conv w.r.t. the filter `w` (used for its shape only): -> [Cout, KH, KW, Cin]."""
    Cout, KH, KW, Cin = w.shape
    dw = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).contiguous(), (Cout, Cin, KH, KW),
                                     dy.permute(0, 3, 1, 2).contiguous(), stride=stride, padding=_pad(w, pad))
    return dw.permute(0, 2, 3, 1).contiguous()


def upsample2_backward(dfine, coarse_hw):
    """Adjoint of the nearest x 2 upsample cropped to the fine size: each coarse cell sums the (up to) 2 x 2 fine cells."""
    N, Hf, Wf, C = dfine.shape
    Hc, Wc = coarse_hw
    f = F.pad(dfine, (0, 0, 0, 2 * Wc - Wf, 0, 2 * Hc - Hf))
    return f.reshape(N, Hc, 2, Wc, 2, C).sum(dim=(2, 4))


def subsample2_backward(dy, x_shape):
    """Adjoint of x[:, ::2, ::2]."""
    dx = torch.zeros(tuple(x_shape), dtype=F64)
    dx[:, ::2, ::2] = dy
    return dx


# ---- bottleneck -------------------------------------------------------------------------------------------------------------
def bottleneck_forward(x, p, stride, emulate=False):
    """conv1 1x1 + bias + ReLU, conv2 3x3 / stride + bias + ReLU, conv3 1x1 + bias + shortcut, ReLU. p: "conv1.weight",
    "conv1.bias", ... and, for the projection shortcut (1x1 / stride), "down.weight" / "down.bias". Returns a1, a2, sc, y."""
    st = _st(emulate)
    a1 = st(torch.relu(conv(x, p["conv1.weight"], p["conv1.bias"])))
    a2 = st(torch.relu(conv(a1, p["conv2.weight"], p["conv2.bias"], stride)))
    sc = st(conv(x, p["down.weight"], p["down.bias"], stride, 0)) if "down.weight" in p else x
    y = st(torch.relu(conv(a2, p["conv3.weight"], p["conv3.bias"]) + sc))
    return dict(a1=a1, a2=a2, sc=sc, y=y)


def bottleneck_backward(x, fwd, p, stride, ds, masks, prefill=None, need_dx=True, emulate=False):
    """ds: the gradient w.r.t. the pre-activation sum (masked by y > 0). masks: {"a1", "a2", "x"}. prefill: what the dx
    buffer held before the call (dx_has_grad: an un-masked partial gradient w.r.t. x). Stored maps, in the device's order:
    d_a2, d_a1; with a projection shortcut its data gradient (plus the prefill) is stored in the dx buffer and conv1's data
    gradient reads it back as its residual; without one, a prefill is first summed with ds in the buffer."""
    st = _st(emulate)
    a1, a2 = fwd["a1"], fwd["a2"]
    down = "down.weight" in p
    g = {"conv3.weight": conv_wgrad(a2, ds, p["conv3.weight"])}
    d_a2 = st(masks["a2"] * conv_dgrad(ds, p["conv3.weight"], a2.shape))
    g["conv2.weight"] = conv_wgrad(a1, d_a2, p["conv2.weight"], stride)
    d_a1 = st(masks["a1"] * conv_dgrad(d_a2, p["conv2.weight"], a1.shape, stride))
    g["conv1.weight"] = conv_wgrad(x, d_a1, p["conv1.weight"])
    if down:
        g["down.weight"] = conv_wgrad(x, ds, p["down.weight"], stride, 0)
    out = dict(grads=g, d_a1=d_a1, d_a2=d_a2, dx=None)
    if not need_dx:
        return out
    if down:
        t = conv_dgrad(ds, p["down.weight"], x.shape, stride, 0)
        t = st(t if prefill is None else prefill + t)
    else:
        t = ds if prefill is None else st(prefill + ds)
    out["dx"] = st(masks["x"] * (conv_dgrad(d_a1, p["conv1.weight"], x.shape) + t))
    return out


def block_masks(x, fwd):
    """The masks of a forward's own activations."""
    return {"a1": (fwd["a1"] > 0).to(F64), "a2": (fwd["a2"] > 0).to(F64), "x": (x > 0).to(F64)}


# ---- stage and the C3..C5 walk ----------------------------------------------------------------------------------------------
def stage_forward(x, blocks, emulate=False):
    """blocks: [(p, stride)]. Returns the list of the blocks' forward dicts (each with its input under "x")."""
    fwds = []
    for p, stride in blocks:
        f = bottleneck_forward(x, p, stride, emulate)
        f["x"] = x
        fwds.append(f)
        x = f["y"]
    return fwds


def resnet_forward(c2, stages, emulate=False):
    """stages: the trainable stages (layer2 ...), each a list of (p, stride). Returns [[forward dict per block] per stage]."""
    out, x = [], c2
    for blocks in stages:
        out.append(stage_forward(x, blocks, emulate))
        x = out[-1][-1]["y"]
    return out


def resnet_backward(stages, fwds, dC, masks, emulate=False):
    """ResNet.backward: dC[j] is the lateral gradient w.r.t. the output of stage j (un-masked, except the last, which is
    masked by its output > 0); the walk goes from the last stage to the first. The first block of a stage adds its data
    gradient onto the lateral gradient of the previous stage's output (dx_has_grad); the first block of the first stage
    computes no data gradient (its input is frozen). masks[j][b]: the masks of block b of stage j.
    Returns (dC as the device leaves it, [[gradient dict per block] per stage])."""
    dC = list(dC)
    grads = [[None] * len(blocks) for blocks in stages]
    for j in reversed(range(len(stages))):
        ds = dC[j]
        for b in reversed(range(len(stages[j]))):
            p, stride = stages[j][b]
            f = fwds[j][b]
            first = b == 0
            r = bottleneck_backward(f["x"], f, p, stride, ds, masks[j][b], prefill=dC[j - 1] if first and j > 0 else None,
                                    need_dx=not (first and j == 0), emulate=emulate)
            grads[j][b] = r["grads"]
            if first:
                if j > 0:
                    dC[j - 1] = r["dx"]
            else:
                ds = r["dx"]
    return dC, grads


# ---- plain FPN --------------------------------------------------------------------------------------------------------------
def _top_down(feats, p, base, st):
    L = len(feats)
    inner = [None] * L
    for i in reversed(range(L)):
        t = conv(feats[i], p["fpn.lat%d.weight" % (i + base)], p["fpn.lat%d.bias" % (i + base)])
        if i + 1 < L:
            t = t + nearest_up(inner[i + 1], feats[i].shape[1:3])
        inner[i] = st(t)
    P = [st(conv(inner[i], p["fpn.out%d.weight" % (i + base)], p["fpn.out%d.bias" % (i + base)])) for i in range(L)]
    return inner, P


def _top_down_backward(feats, inner, p, dP, base, st, g):
    """Output convs and the top-down path backwards: the gradients of the out layers into g; returns d(inner), each level's
    stored once after its output conv's data gradient and once more after the finer level's was added."""
    L = len(feats)
    dinner = [None] * L
    for i in range(L):
        name = "fpn.out%d" % (i + base)
        g[name + ".weight"] = conv_wgrad(inner[i], dP[i], p[name + ".weight"])
        g[name + ".bias"] = dP[i].sum(dim=(0, 1, 2))
        dinner[i] = st(conv_dgrad(dP[i], p[name + ".weight"], inner[i].shape))
    for i in range(1, L):
        dinner[i] = st(dinner[i] + upsample2_backward(dinner[i - 1], dinner[i].shape[1:3]))
    for i in range(L):
        name = "fpn.lat%d" % (i + base)
        g[name + ".weight"] = conv_wgrad(feats[i], dinner[i], p[name + ".weight"])
        g[name + ".bias"] = dinner[i].sum(dim=(0, 1, 2))
    return dinner


def fpn_forward(feats, p, extra_p6=True, emulate=False):
    """FPN(upsample="nearest") on C2.. (finest first): inner_i = lat_i(C_i) + up(inner_{i+1}), P_i = out_i(inner_i),
    P6 = P5[:, ::2, ::2]. p: name -> tensor under the layer names of models/necks/fpn.py."""
    inner, P = _top_down(feats, p, 2, _st(emulate))
    if extra_p6:
        P = P + [P[-1][:, ::2, ::2]]
    return dict(inner=inner, P=P)


def fpn_backward(feats, fwd, p, dP, top_mask, c_needs_grad, extra_p6=True, emulate=False):
    """FPN.backward. The P6 gradient is added into dP[L-1] in place (one more stored map); the top level's dC is masked by
    top_mask = (C_top > 0). Returns dC (None where not needed), grads, dinner and dP_top, what dP[L-1] holds afterwards."""
    st = _st(emulate)
    L = len(feats)
    dP = list(dP)
    if extra_p6:
        dP[L - 1] = st(dP[L - 1] + subsample2_backward(dP[L], dP[L - 1].shape))
    g = {}
    dinner = _top_down_backward(feats, fwd["inner"], p, dP, 2, st, g)
    dC = [None] * L
    for i in range(L):
        if c_needs_grad[i]:
            t = conv_dgrad(dinner[i], p["fpn.lat%d.weight" % (i + 2)], feats[i].shape)
            dC[i] = st(top_mask * t if i == L - 1 else t)
    return dict(dC=dC, grads=g, dinner=dinner, dP_top=dP[L - 1])


# ---- RetinaNet FPN ----------------------------------------------------------------------------------------------------------
def retina_forward(feats, p, emulate=False):
    """RetinaFPN on C3..C5: P3..P5 as above, P6 = conv3x3/2(C5), P7 = conv3x3/2(ReLU(P6)). P = [P3, P4, P5, P6, P7]."""
    st = _st(emulate)
    inner, P = _top_down(feats, p, 3, st)
    p6 = st(conv(feats[-1], p["fpn.p6.weight"], p["fpn.p6.bias"], 2))
    p7 = st(conv(torch.relu(p6), p["fpn.p7.weight"], p["fpn.p7.bias"], 2))
    return dict(inner=inner, P=P + [p6, p7])


def retina_backward(feats, fwd, p, dP, p6_mask, top_mask, emulate=False):
    """RetinaFPN.backward. p6_mask = (P6 > 0), top_mask = (C5 > 0). The masked P7 data gradient is stored, then added into
    dP[L] in place (the sum is stored: one extra rounding); P6's data gradient is stored in dC[L-1] and the top lateral's data
    gradient reads it back as its residual. Returns dC, grads and dP6, what dP[L] holds afterwards."""
    st = _st(emulate)
    L = len(feats)
    dP = list(dP)
    g = {}
    p6r = torch.relu(fwd["P"][L])
    g["fpn.p7.weight"] = conv_wgrad(p6r, dP[L + 1], p["fpn.p7.weight"], 2)
    g["fpn.p7.bias"] = dP[L + 1].sum(dim=(0, 1, 2))
    t = st(p6_mask * conv_dgrad(dP[L + 1], p["fpn.p7.weight"], p6r.shape, 2))
    dP[L] = st(dP[L] + t)
    dinner = _top_down_backward(feats, fwd["inner"], p, dP, 3, st, g)
    g["fpn.p6.weight"] = conv_wgrad(feats[-1], dP[L], p["fpn.p6.weight"], 2)
    g["fpn.p6.bias"] = dP[L].sum(dim=(0, 1, 2))
    d6 = st(conv_dgrad(dP[L], p["fpn.p6.weight"], feats[-1].shape, 2))
    dC = [None] * L
    for i in range(L):
        t = conv_dgrad(dinner[i], p["fpn.lat%d.weight" % (i + 3)], feats[i].shape)
        dC[i] = st(top_mask * (t + d6) if i == L - 1 else t)
    return dict(dC=dC, grads=g, dinner=dinner, dP6=dP[L])


# ---- the comparison rule ----------------------------------------------------------------------------------------------------
def check_rows(rows, tag=""):
    """rows: (name, got, exact, emulated), float64 CPU tensors. The rule of the kernel and neck tests:
    |got - exact| <= 2 E + 2^-9 max |exact| with E = max |emulated - exact| from the reference alone. Prints E, the bound and
    the achieved error of every row; returns (violations, worst achieved / bound): [(name, achieved, bound)]."""
    bad, worst = [], 0.0
    for name, got, exact, emu in rows:
        assert tuple(got.shape) == tuple(exact.shape), "%s: shape %s, reference %s" % (name, tuple(got.shape), tuple(exact.shape))
        E = float((emu - exact).abs().max())
        top = float(exact.abs().max())
        tol = 2.0 * E + 2.0 ** -9 * top
        finite = bool(torch.isfinite(got).all())
        err = float((got - exact).abs().max()) if finite else float("inf")
        ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        print("%s%s: E %.3e  bound %.3e  achieved %.3e  ratio %.3f  (max |exact| %.3e)" % (tag, name, E, tol, err, ratio, top))
        if not finite or err > tol:
            bad.append((name, err, tol))
    print("%sworst achieved / bound: %.3f" % (tag, worst))
    return bad, worst
