"""fp64 reference of the CARAFE entries (include/mxdet.h), written as the published composition (Wang et
al., ICCV 2019): unfold the k x k neighbourhoods of X, upsample them nearest by 2, pixel-shuffle the 4 k^2 logits into k^2 maps
at the fine size, softmax over the k^2 taps, weighted sum, crop. torch-CPU float64 throughout; bf16 tensors are float64
tensors that hold bf16 values. The backward is autograd's. Unlike the GPU entries, these functions take only the REAL logit
channels [N, H, W, 4 k^2].

emulate=True rounds exactly what the kernels round: the outputs (Y; dX, dM) to bf16 and, with a prefill (accumulate), the
fp64 sum prefill + dX once. The kernels keep no rounded intermediate (the backward recomputes the fp32 weights from M), so
nothing else is rounded. The emulated variants exist to MEASURE the rounding error inherent in the number formats
(E = max |emulated - exact|), from which the GPU tests derive their backward tolerances; no kernel result enters them.

backward_gather restates dX and dM in the kernels' explicit gather form, independently of autograd (tests/test_carafe_cpu.py
compares the two).
"""
import torch
import torch.nn.functional as F

F64 = torch.float64


def round_bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def weights(logits, k):
    """logits [N, H, W, 4 k^2] -> softmax weights at the fine size [N, k^2, 2H, 2W] (channel t * 4 + s -> tap t at
    sub-position s = (i & 1) * 2 + (j & 1): pixel_shuffle's order)."""
    return torch.softmax(F.pixel_shuffle(logits.permute(0, 3, 1, 2), 2), dim=1)


def forward(x, logits, k, out_hw, emulate=False):
    """x [N, H, W, C], logits [N, H, W, 4 k^2] -> Y [N, Hf, Wf, C]."""
    N, H, W, C = x.shape
    r = k // 2
    cols = F.unfold(x.permute(0, 3, 1, 2), k, padding=r).reshape(N, C, k * k, H, W)        # zero outside the map
    cols = cols.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)                    # nearest x 2
    y = (cols * weights(logits, k)[:, None]).sum(dim=2)[:, :, :out_hw[0], :out_hw[1]]
    y = y.permute(0, 2, 3, 1).contiguous()
    return round_bf16(y) if emulate else y


def backward(x, logits, d_out, k, emulate=False, prefill=None):
    """Autograd gradients (dX, dM) of sum(Y * d_out); prefill: what dX held before an accumulating call."""
    x = x.clone().requires_grad_(True)
    logits = logits.clone().requires_grad_(True)
    y = forward(x, logits, k, d_out.shape[1:3])
    dx, dm = torch.autograd.grad((y * d_out).sum(), (x, logits))
    return emulate_backward(dx, dm, prefill) if emulate else (dx if prefill is None else prefill + dx, dm)


def emulate_backward(dx, dm, prefill=None):
    """The roundings of the backward entry applied to its exact results: one rounding of each output, of the sum with the
    prefill when it accumulates (what backward(emulate=True) returns, without a second autograd pass)."""
    return round_bf16(dx if prefill is None else prefill + dx), round_bf16(dm)


def backward_gather(x, logits, d_out, k):
    """dX[n,p,c] = sum over q within r of p and the s inside Hf x Wf of w[q,s,t(p - q)] dY[n,2q+s,c];
    dM[n,q,t*4+s] = w_t (g_t - sum_u w_u g_u), g_t = sum_c dY[n,2q+s,c] X[n,src(t),c]; explicit loops."""
    N, H, W, C = x.shape
    Hf, Wf = d_out.shape[1:3]
    r, T = k // 2, k * k
    w = torch.softmax(logits.reshape(N, H, W, T, 4), dim=3)
    dx = torch.zeros_like(x)
    dm = torch.zeros_like(logits).reshape(N, H, W, T, 4)
    for qy in range(H):
        for qx in range(W):
            for s in range(4):
                oy, ox = 2 * qy + (s >> 1), 2 * qx + (s & 1)
                if oy >= Hf or ox >= Wf:
                    continue
                g = torch.zeros((N, T), dtype=F64)
                for t in range(T):
                    py, px = qy + t // k - r, qx + t % k - r
                    if 0 <= py < H and 0 <= px < W:
                        dx[:, py, px] += w[:, qy, qx, t, s, None] * d_out[:, oy, ox]
                        g[:, t] = (d_out[:, oy, ox] * x[:, py, px]).sum(dim=1)
                ws = w[:, qy, qx, :, s]
                dm[:, qy, qx, :, s] = ws * (g - (ws * g).sum(dim=1, keepdim=True))
    return dx, dm.reshape(N, H, W, 4 * T)


def nearest_up(x, out_hw):
    """Nearest-neighbour upsample by 2, cropped: what a one-hot centre tap must reproduce."""
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :out_hw[0], :out_hw[1]]


def shift(x, dy, dx):
    """S[n, y, x] = X[n, y + dy, x + dx], zero outside the map."""
    N, H, W, C = x.shape
    out = torch.zeros_like(x)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    yd, xd = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
    out[:, ys, xs] = x[:, yd, xd]
    return out


def one_hot_logits(N, H, W, k, tap, low=-100.0):
    """Tap `tap` at 0 and every other at `low`, for all four sub-positions."""
    m = torch.full((N, H, W, k * k, 4), low, dtype=F64)
    m[:, :, :, tap] = 0.0
    return m.reshape(N, H, W, 4 * k * k)


def random_case(N, H, W, C, k, out_hw, seed, logit_std=1.5):
    """bf16-valued X, real logits, d_out and a prefill for dX."""
    g = torch.Generator().manual_seed(seed)
    x = round_bf16(torch.randn((N, H, W, C), generator=g, dtype=F64))
    m = round_bf16(torch.randn((N, H, W, 4 * k * k), generator=g, dtype=F64) * logit_std)
    d_out = round_bf16(torch.randn((N, out_hw[0], out_hw[1], C), generator=g, dtype=F64) * 0.5)
    pre = round_bf16(torch.randn((N, H, W, C), generator=g, dtype=F64))
    return x, m, d_out, pre


# ---- the neck with CARAFE, for tests/test_gpu_carafe_model.py ----------------------------------------------------------------
def conv(x, w, b=None):
    """x [N, H, W, Cin], w [Cout, KH, KW, Cin] (stride 1, pad k / 2) -> [N, H, W, Cout]."""
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, padding=w.shape[1] // 2)
    return y.permute(0, 2, 3, 1)


class _Stored(torch.autograd.Function):
    """A tensor a layer stores in bf16: the value is rounded on the way forward, its gradient on the way back."""

    @staticmethod
    def forward(ctx, t):
        return round_bf16(t)

    @staticmethod
    def backward(ctx, g):
        return round_bf16(g)


class _GradStored(torch.autograd.Function):
    """One consumer of a stored tensor: its contribution to the gradient is rounded to bf16 before the next is added."""

    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return round_bf16(g)


def fpn_reference(feats, params, d_P, k, emulate=False):
    """The FPN with the CARAFE top-down path on the C maps `feats` (finest first), forward and backward by autograd.
    params: name -> float64 tensor under the layer names of models/necks/fpn.py (filters [Cout, KH, KW, Cin]; the enc
    filters and biases hold only the real 4 k^2 rows). d_P: the gradients w.r.t. the P maps.
    emulate: every map a layer stores (comp's and enc's outputs, the upsampled map, inner, P) is rounded to bf16, and so is
    every gradient map: each consumer's contribution to d(inner) as it is added, the sum, the logits' and comp's gradients.
    Weight gradients stay unrounded (fp32 on the device). Returns dict(inner=[..], P=[..], dC=[..], grads={name: ..})."""
    st = _Stored.apply if emulate else (lambda t: t)
    use = _GradStored.apply if emulate else (lambda t: t)
    feats = [f.clone().requires_grad_(True) for f in feats]
    params = {n: v.clone().requires_grad_(True) for n, v in params.items()}
    L = len(feats)
    inner = [None] * L
    for i in reversed(range(L)):
        lat = conv(feats[i], params["fpn.lat%d.weight" % (i + 2)], params["fpn.lat%d.bias" % (i + 2)])
        if i + 1 < L:
            name = "fpn.carafe%d" % (i + 2)
            comp = st(conv(use(inner[i + 1]), params[name + ".comp.weight"], params[name + ".comp.bias"]))
            logits = st(conv(comp, params[name + ".enc.weight"], params[name + ".enc.bias"]))
            lat = lat + st(forward(use(inner[i + 1]), logits, k, feats[i].shape[1:3]))
        inner[i] = st(lat)
    P = [st(conv(use(inner[i]), params["fpn.out%d.weight" % (i + 2)], params["fpn.out%d.bias" % (i + 2)])) for i in range(L)]
    names = sorted(params)
    loss = sum((p * g).sum() for p, g in zip(P, d_P))
    grads = torch.autograd.grad(loss, feats + [params[n] for n in names])
    dC = [round_bf16(g) if emulate else g for g in grads[:L]]
    return dict(inner=[t.detach() for t in inner], P=[t.detach() for t in P], dC=dC, grads=dict(zip(names, grads[L:])))
