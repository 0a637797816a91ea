"""fp64 reference of the global context block (GCNet; include/mxdet.h): mmcv's ContextBlock with
pooling_type='att' and fusion_types=('channel_add',) after a bottleneck's conv3 and in front of its shortcut add. torch-CPU
float64 throughout; a "bf16 tensor" is a float64 tensor that holds bf16 values. No kernel result ever enters this file.

    t [N,HW,C] (conv3 + bias, no residual, no ReLU), sc the shortcut, P = C / reduction
    logit = t . wk (no bias);  att = softmax over the HW positions;  ctx = sum_p att t                     [N,C]
    h = W1 ctx + b1;  u = relu(gamma (h - mean) rstd + beta) (LayerNorm over the P values, biased variance, eps)
    add = W2 u + b2;  y = relu(t + add + sc)

Two modes. Exact: the formulas on the given (bf16- / fp32-valued) inputs. Emulated (emulate=True): the same with the kernels'
stated roundings -- y and d_t to bf16 and, in the block-level reference, the bf16 storage of t and of every other map the
bottleneck stores (tests/_backbone_ref.py's convention). E = max |emulated - exact| measures what the number formats cost; the
GPU tests take their bf16 tolerances from it.

forward() / backward() are explicit (backward is hand-written: the formulas of DESIGN.md 3); composition() is the same
forward from torch's conv2d 1x1, softmax, matmul, layer_norm and linear, for autograd and as a cross-check.

fp32 outputs: bounds_forward() / bounds_backward() give, per output element, the forward error bound of the documented
summation order, (D + 4) 2^-23 A: A is the output's expression with every term replaced by its absolute value, D the longest
chain of dependent fp32 additions behind one output (DESIGN.md 5u lists the orders: a dot over C is 8 NV adds in a lane, NV =
ceil(C / 512), then a 6-level butterfly; a sum over the positions of a chunk is at most 16 per wave, then 4 waves; the K =
ceil(HW / 64) chunks are folded as 4 contiguous runs of ceil(K / 4), then 4 (ctx, d_add), or as 256 strided runs, a 6-level
butterfly and 4 waves (the scalars S); du is 256 / (P / 8) row slices of ceil(C / slices) rows, then the slices; add and d_ctx
are chains over P; a parameter gradient is a
chain over N; d_wk is 16 runs of ceil(N K / 16) partials, then 16). D counts the whole chain behind an output, through every sum the same entry (and the entry that filled the workspace it reads) makes in
front of it (_D). Nothing is added to that rule: no carried term, no factor for the softmax or the LayerNorm. D and A come
from the shape and the reference alone, never from a result.
"""
import torch
import torch.nn.functional as F

import _backbone_ref as bref
from _carafe_ref import F64, round_bf16

EPS = 1e-5
CHUNK = 64                      # kGcChunk of csrc/context.hip
U = 2.0 ** -23
PARAMS = ("mask.weight", "fc1.weight", "fc1.bias", "ln.gamma", "ln.beta", "fc2.weight", "fc2.bias")


def round_f32(x):
    return x.to(torch.float32).to(F64)


def random_params(C, P, g, zero_fc2=False, wk_scale=1.0):
    """The seven parameters as the kernels read them: bf16 values for the three filters, fp32 values for the 1-D arrays.
    Everything is random (gamma around 1) so that a dropped term shows; zero_fc2: the block's initial state."""
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
    p = {"mask.weight": round_bf16(r(C) * wk_scale * (2.0 / C) ** 0.5), "fc1.weight": round_bf16(r(P, C) * (2.0 / C) ** 0.5),
         "fc1.bias": round_f32(r(P) * 0.1), "ln.gamma": round_f32(1.0 + 0.2 * r(P)), "ln.beta": round_f32(0.2 * r(P)),
         "fc2.weight": round_bf16(r(C, P) * (1.0 / P) ** 0.5), "fc2.bias": round_f32(r(C) * 0.1)}
    if zero_fc2:
        p["fc2.weight"].zero_()
        p["fc2.bias"].zero_()
    return p


def random_case(N, HW, C, P, seed, wk_scale=1.0, peak=None):
    """t, sc, ds (bf16 values; ds masked like a gradient behind a ReLU) and the parameters. peak = (n, p, value): one position
    whose logit stands `value` above the others (its row is a multiple of wk)."""
    g = torch.Generator().manual_seed(seed)
    p = random_params(C, P, g, wk_scale=wk_scale)
    t = torch.randn(N, HW, C, generator=g, dtype=F64)
    if peak is not None:
        wk = p["mask.weight"]
        t[peak[0], peak[1]] = wk * (peak[2] / float((wk * wk).sum()))
    t = round_bf16(t)
    sc = round_bf16(torch.relu(torch.randn(N, HW, C, generator=g, dtype=F64)))
    ds = round_bf16(torch.randn(N, HW, C, generator=g, dtype=F64) * 0.5 * (torch.rand(N, HW, C, generator=g) < 0.6))
    return t, sc, ds, p


# ---- the block's forward and backward ---------------------------------------------------------------------------------------------
def forward(t, sc, p, eps=EPS, emulate=False):
    """t, sc [N,HW,C] -> every intermediate and y. emulate: y rounded to bf16."""
    logits = t @ p["mask.weight"]                                          # [N,HW]
    m = logits.max(dim=1, keepdim=True).values
    lse = (m + torch.log(torch.exp(logits - m).sum(dim=1, keepdim=True)))[:, 0]
    att = torch.exp(logits - lse[:, None])
    ctx = torch.einsum("np,npc->nc", att, t)
    out = dict(logits=logits, lse=lse, att=att, ctx=ctx)
    out.update(transform(ctx, p, eps))
    y = torch.relu(t + out["add"][:, None, :] + sc)
    out["y"] = round_bf16(y) if emulate else y
    return out


def transform(ctx, p, eps=EPS):
    h = ctx @ p["fc1.weight"].T + p["fc1.bias"]
    mean = h.mean(dim=1)
    rstd = 1.0 / torch.sqrt(((h - mean[:, None]) ** 2).mean(dim=1) + eps)
    xh = (h - mean[:, None]) * rstd[:, None]
    z = p["ln.gamma"] * xh + p["ln.beta"]
    u = torch.relu(z)
    return dict(h=h, mean=mean, rstd=rstd, xh=xh, z=z, u=u, add=u @ p["fc2.weight"].T + p["fc2.bias"])


def backward(t, p, f, ds, emulate=False):
    """ds: the gradient at the pre-activation sum (already masked by y > 0). f: forward()'s dict (or any dict with att, ctx,
    xh, z, u, rstd). Returns d_t (rounded to bf16 if emulate), the seven parameter gradients under PARAMS' names, and the
    intermediates."""
    W1, W2, gamma, wk = p["fc1.weight"], p["fc2.weight"], p["ln.gamma"], p["mask.weight"]
    att, ctx, xh, u, rstd = f["att"], f["ctx"], f["xh"], f["u"], f["rstd"]
    d_add = ds.sum(dim=1)                                                  # [N,C]
    g = {"fc2.weight": d_add.T @ u, "fc2.bias": d_add.sum(dim=0)}
    du = d_add @ W2
    gz = du * (f["z"] > 0)
    g["ln.gamma"], g["ln.beta"] = (gz * xh).sum(dim=0), gz.sum(dim=0)
    gg = gz * gamma
    dh = rstd[:, None] * (gg - gg.mean(dim=1, keepdim=True) - xh * (gg * xh).mean(dim=1, keepdim=True))
    g["fc1.weight"], g["fc1.bias"] = dh.T @ ctx, dh.sum(dim=0)
    d_ctx = dh @ W1
    e = torch.einsum("nc,npc->np", d_ctx, t)
    S = (att * e).sum(dim=1)
    dl = att * (e - S[:, None])
    d_t = ds + att[:, :, None] * d_ctx[:, None, :] + dl[:, :, None] * wk
    g["mask.weight"] = torch.einsum("np,npc->c", dl, t)
    return dict(d_t=round_bf16(d_t) if emulate else d_t, grads=g, d_add=d_add, du=du, gz=gz, gg=gg, dh=dh, d_ctx=d_ctx, e=e, S=S,
                dl=dl)


def composition(t, sc, p, eps=EPS):
    """The same forward from torch's building blocks: conv2d 1x1 (on [N,C,HW,1]), softmax, matmul, layer_norm, linear."""
    N, HW, C = t.shape
    x = t.permute(0, 2, 1).reshape(N, C, HW, 1)
    mask = F.conv2d(x, p["mask.weight"].reshape(1, C, 1, 1)).reshape(N, 1, HW)
    mask = torch.softmax(mask, dim=2)
    ctx = torch.matmul(x.reshape(N, C, HW), mask.permute(0, 2, 1))[:, :, 0]          # [N,C]
    h = F.linear(ctx, p["fc1.weight"], p["fc1.bias"])
    u = torch.relu(F.layer_norm(h, (h.shape[1],), p["ln.gamma"], p["ln.beta"], eps))
    add = F.linear(u, p["fc2.weight"], p["fc2.bias"])
    return torch.relu(t + add[:, None, :] + sc), add, ctx


def autograd_backward(t, sc, p, ds_unmasked, eps=EPS):
    """(d_t, d_sc, parameter gradients) of sum(y * ds_unmasked) through composition()."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    t = t.clone().requires_grad_(True)
    sc = sc.clone().requires_grad_(True)
    y, _, _ = composition(t, sc, leaves, eps)
    grads = torch.autograd.grad((y * ds_unmasked).sum(), [t, sc] + [leaves[k] for k in PARAMS])
    return grads[0], grads[1], dict(zip(PARAMS, grads[2:]))


# ---- bounds of the fp32 outputs -------------------------------------------------------------------------------------------------
def _nv(C):
    return 1 if C <= 512 else (2 if C <= 1024 else 4)


def _bound(D, A):
    return (D + 4) * U * A


def _cdiv(a, b):
    return -(-a // b)


def _D(N, HW, C, P):
    """The chain lengths of the documented summation orders at one shape, and the chain behind each checked output: the
    entry's own sums and everything the same entry (or the workspace it reads) puts in front of them."""
    K = _cdiv(HW, CHUNK)
    ns = 256 // (P // 8)
    d = dict(dot=8 * _nv(C) + 6, columns=16 + 4 + _cdiv(K, 4) + 4, scalar=16 + 4 + _cdiv(K, 256) + 6 + 4, du=_cdiv(C, ns) + ns,
             wk=16 + 4 + _cdiv(N * K, 16) + 16)
    # pool_fwd -> transform_fwd
    d["logits"] = d["dot"]
    d["lse"] = d["dot"] + d["scalar"]
    d["ctx"] = d["dot"] + d["columns"] + 2                   # the chunk's rescale and the division by S
    d["h"] = d["ctx"] + d["dot"] + 1
    d["mean"] = d["h"] + P
    d["rstd"] = d["mean"] + P + 2
    d["add"] = d["rstd"] + 3 + P + 1                        # xh, the affine map, then the row of W2 and its bias
    # reduce_bwd -> transform_bwd (ctx, h, mean, rstd given)
    d["d_add"] = d["columns"]
    d["gz"] = d["d_add"] + d["du"] + 3                      # xh and the affine map recomputed for the mask
    d["dh"] = d["gz"] + 1 + 2 * P + 3
    d["fc2.weight"] = d["d_add"] + 3 + N
    d["fc2.bias"] = d["d_add"] + N
    d["ln.gamma"] = d["gz"] + 2 + N
    d["ln.beta"] = d["gz"] + N
    d["fc1.weight"] = d["fc1.bias"] = d["dh"] + N
    d["d_ctx"] = d["dh"] + P
    # pool_bwd (logits, lse, d_ctx given): e, S, dl, then the chunks and the fold
    d["mask.weight"] = d["dot"] + d["scalar"] + 2 + d["wk"]
    return d


# A bound that is no small fraction of its output checks nothing: the tests assert max(bound) <= fraction_limit * max |exact|
# at every case. (D + 4) 2^-23 is below 2^-11 (D <= 4096); evaluating a sum in absolute values enlarges it by about the square root
# of its length where the terms' signs are mixed -- at most 2^5.5 here (C = 2048). An output one such sum behind given values gets
# 2^-8 (the 2^3 left over is the spread of the terms' sizes). mean and rstd (the sum over C inside h, then the sum over P), the fc1
# gradients and d_ctx (the sum over C inside du, then the LayerNorm backward's differences over P, then for d_ctx the sum
# over P) sit two and three such sums deep and get 2^-3.
DEEP = ("mean", "rstd", "fc1.weight", "fc1.bias", "d_ctx")


def fraction_limit(name):
    return 2.0 ** -3 if name in DEEP else 2.0 ** -8


def bounds_forward(t, p, f):
    """Per-element bounds (D + 4) 2^-23 A of logits, lse, ctx, h, mean, rstd and add for pool_fwd -> transform_fwd. A is the
    output's formula evaluated in absolute values: every product and sum the entry itself makes on the way to the output is
    made with the absolute values of its terms, so a sum that cancels counts with its full size. The softmax weights enter at
    their values (exp is no sum of terms). h, mean and rstd are checked as outputs in their own right, so nothing of the
    LayerNorm is carried into add: there u enters at its value.
      logits  sum_c |t| |wk|
      lse     |max| + |ln S| + 1   (S is a sum of positive terms: its relative error is an absolute one of ln S)
      ctx     sum_p att |t|
      h       sum_c |W1| ctx_A + |b1|, ctx_A the line above;  mean = mean_P(h_A)
      rstd    to first order d rstd = -rstd^3 mean_P((h - mean) dh): rstd^3 mean_P(|h - mean| (h_A + mean_A))
      add     sum_j |W2| u + |b2|"""
    N, HW, C = t.shape
    P = p["fc1.weight"].shape[0]
    D = _D(N, HW, C, P)
    wk, W1, W2 = p["mask.weight"].abs(), p["fc1.weight"].abs(), p["fc2.weight"].abs()
    m = f["logits"].max(dim=1).values
    A = {"logits": t.abs() @ wk, "lse": m.abs() + (f["lse"] - m).abs() + 1.0, "ctx": torch.einsum("np,npc->nc", f["att"], t.abs())}
    A["h"] = A["ctx"] @ W1.T + p["fc1.bias"].abs()
    A["mean"] = A["h"].mean(dim=1)
    A["rstd"] = f["rstd"] ** 3 * ((f["h"] - f["mean"][:, None]).abs() * (A["h"] + A["mean"][:, None])).mean(dim=1)
    A["add"] = f["u"].abs() @ W2.T + p["fc2.bias"].abs()
    return {k: _bound(D[k], v) for k, v in A.items()}


def bounds_backward(t, p, f, r, ds):
    """Per-element bounds (D + 4) 2^-23 A of d_add, d_ctx, d_wk and the six parameter gradients of transform_bwd, for the
    teacher-forced calls reduce_bwd -> transform_bwd (ctx, h, mean, rstd given, rounded to fp32) and pool_bwd (logits, lse,
    d_ctx given). The same reading: what the entry computes on the way is evaluated in absolute values; what it is given (d_add
    from reduce_bwd's partials; ctx, h, mean, rstd; logits, lse, d_ctx) enters at its value.
      d_add   sum_p |ds|
      du_A    sum_c |d_add| |W2|;  gz_A = du_A (u > 0);  gg_A = gz_A |gamma|;  xh_A = rstd (|h| + |mean|)
      dh_A    rstd (gg_A + mean_P(gg_A) + xh_A mean_P(gg_A xh_A))
      u_A     |gamma| xh_A + |beta| (the ReLU is 1-Lipschitz: where it is off, u still carries the rounding of its argument)
      dW2 sum_n |d_add| u_A;  db2 sum_n |d_add|;  dgamma sum_n gz_A xh_A;  dbeta sum_n gz_A;  dW1 sum_n dh_A |ctx|;
      db1 sum_n dh_A;  d_ctx sum_j dh_A |W1|
      e_A     sum_c |d_ctx| |t|;  S_A = sum_p att e_A;  dl_A = att (e_A + S_A);  d_wk = sum_{n,p} dl_A |t|."""
    N, HW, C = t.shape
    P = p["fc1.weight"].shape[0]
    D = _D(N, HW, C, P)
    W1, W2 = p["fc1.weight"].abs(), p["fc2.weight"].abs()
    da = r["d_add"].abs()
    rstd = f["rstd"][:, None]
    xh = rstd * (f["h"].abs() + f["mean"].abs()[:, None])
    gz = (da @ W2) * (f["z"] > 0)
    gg = gz * p["ln.gamma"].abs()
    dh = rstd * (gg + gg.mean(dim=1, keepdim=True) + xh * (gg * xh).mean(dim=1, keepdim=True))
    e = torch.einsum("nc,npc->np", r["d_ctx"].abs(), t.abs())
    dl = f["att"] * (e + (f["att"] * e).sum(dim=1, keepdim=True))
    A = {"d_add": ds.abs().sum(dim=1), "fc2.weight": da.T @ (p["ln.gamma"].abs() * xh + p["ln.beta"].abs()), "fc2.bias": da.sum(dim=0),
         "ln.gamma": (gz * xh).sum(dim=0),
         "ln.beta": gz.sum(dim=0), "fc1.weight": dh.T @ f["ctx"].abs(), "fc1.bias": dh.sum(dim=0), "d_ctx": dh @ W1,
         "mask.weight": torch.einsum("np,npc->c", dl, t.abs())}
    return {k: _bound(D[k], v) for k, v in A.items()}


# ---- a bottleneck with the block, for tests/test_gpu_gc_block.py --------------------------------------------------------------------
def bottleneck_forward(x, p, gc, stride, emulate=False, eps=EPS):
    """tests/_backbone_ref.py's bottleneck with the context block between conv3 and the shortcut add. p: the convolutions'
    parameters under that file's names; gc: the block's seven. Stored maps (rounded when emulate): a1, a2, sc, t, y."""
    st = bref._st(emulate)
    a1 = st(torch.relu(bref.conv(x, p["conv1.weight"], p["conv1.bias"])))
    a2 = st(torch.relu(bref.conv(a1, p["conv2.weight"], p["conv2.bias"], stride)))
    sc = st(bref.conv(x, p["down.weight"], p["down.bias"], stride, 0)) if "down.weight" in p else x
    t = st(bref.conv(a2, p["conv3.weight"], p["conv3.bias"]))
    N, H, W, C = t.shape
    f = forward(t.reshape(N, H * W, C), sc.reshape(N, H * W, C), gc, eps, emulate)
    f.update(a1=a1, a2=a2, sc=sc, t=t, y=f["y"].reshape(N, H, W, C))
    return f


def bottleneck_backward(x, f, p, gc, stride, ds, masks, prefill=None, need_dx=True, emulate=False, dcol=False):
    """tests/_backbone_ref.py's bottleneck_backward with the block: conv3's gradients read d_t (stored: rounded when emulate),
    the shortcut and the projection keep ds. dcol: conv2 is a deformable convolution at zero offsets -- the plain convolution,
    whose data gradient the device stores once more on the way (the column tensor's gradient, bf16): emulate rounds it."""
    st = bref._st(emulate)
    a1, a2, t = f["a1"], f["a2"], f["t"]
    N, H, W, C = t.shape
    r = backward(t.reshape(N, H * W, C), gc, f, ds.reshape(N, H * W, C), emulate)
    d_t = r["d_t"].reshape(N, H, W, C)
    g = {"conv3.weight": bref.conv_wgrad(a2, d_t, p["conv3.weight"])}
    d_a2 = st(masks["a2"] * bref.conv_dgrad(d_t, p["conv3.weight"], a2.shape))
    g["conv2.weight"] = bref.conv_wgrad(a1, d_a2, p["conv2.weight"], stride)
    if dcol and emulate:
        # each tap's column gradient is rounded before col2im sums the nine
        taps = sum(_tap_dgrad(d_a2, p["conv2.weight"], ky, kx, a1.shape, stride) for ky in range(3) for kx in range(3))
        d_a1 = st(masks["a1"] * taps)
    else:
        d_a1 = st(masks["a1"] * bref.conv_dgrad(d_a2, p["conv2.weight"], a1.shape, stride))
    g["conv1.weight"] = bref.conv_wgrad(x, d_a1, p["conv1.weight"])
    down = "down.weight" in p
    if down:
        g["down.weight"] = bref.conv_wgrad(x, ds, p["down.weight"], stride, 0)
    out = dict(grads=g, gc_grads=r["grads"], d_t=d_t, d_a1=d_a1, d_a2=d_a2, dx=None)
    if not need_dx:
        return out
    if down:
        s = bref.conv_dgrad(ds, p["down.weight"], x.shape, stride, 0)
        s = st(s if prefill is None else prefill + s)
    else:
        s = ds if prefill is None else st(prefill + ds)
    out["dx"] = st(masks["x"] * (bref.conv_dgrad(d_a1, p["conv1.weight"], x.shape) + s))
    return out


def _tap_dgrad(dy, w, ky, kx, x_shape, stride):
    """The data gradient through tap (ky, kx) of a 3x3 convolution alone, its column gradient dy . w[:, ky, kx] rounded to
    bf16 first (what a deformable convolution stores between its 1x1 data gradient and col2im)."""
    col = round_bf16(dy @ w[:, ky, kx])                                   # [N,Ho,Wo,Cin]
    N, H, Wd, Cin = x_shape
    eye = torch.zeros(Cin, 3, 3, Cin, dtype=F64)
    eye[:, ky, kx] = torch.eye(Cin, dtype=F64)
    return bref.conv_dgrad(col, eye, x_shape, stride)
