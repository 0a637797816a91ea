"""fp64 reference of the attention entries (include/mxdet.h) and of the Balanced Feature Pyramid's
embedded-Gaussian non-local refine built on them. torch-CPU float64 throughout; bf16 tensors are float64 tensors that hold
bf16 values.

  attention_forward / attention_backward   exact: O, LSE and the analytic dQ, dK, dV
  attention_*_emulated                     the same formulas with the roundings of the kernels' number formats: p (forward
                                           and the dV product) and dS (the dK and dQ products) are rounded to bf16 where
                                           the kernels feed them to an MFMA, and the outputs are rounded to bf16
  refine_forward / refine_backward         Rf = B + W_out Attn(theta, phi, g) + b_out with fp64 1x1 convolutions, exact or
                                           emulated (every tensor the layers store is then rounded to bf16 as well)
The emulated variants exist to MEASURE the rounding error inherent in those formats (E = max |emulated - exact|), from which
the GPU tests derive their backward tolerances; no kernel result enters them.
"""
import math

import torch

F64 = torch.float64


def round_bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def _ident(x):
    return x


def attention_forward(q, k, v, scale, emulate=False):
    """q, k, v [N, L, d] float64. Returns (O [N, L, d], LSE [N, L]). emulate: the kernel's roundings -- the row sum is
    taken over the unrounded p, the P V product over bf16(p), and O is rounded once."""
    s = scale * torch.einsum("nic,njc->nij", q, k)
    m = s.max(dim=2, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(dim=2, keepdim=True)
    if emulate:
        o = round_bf16(torch.einsum("nij,njc->nic", round_bf16(p), v) / l)
    else:
        o = torch.einsum("nij,njc->nic", p, v) / l
    return o, (m + torch.log(l))[..., 0]


def attention_backward(q, k, v, d_out, scale, out=None, lse=None, emulate=False):
    """Analytic gradients (dQ, dK, dV) of sum(O * d_out). out / lse: the forward's results (computed when None; the
    emulated variant reads the ROUNDED out for delta, as the kernel does)."""
    if out is None or lse is None:
        out, lse = attention_forward(q, k, v, scale, emulate)
    rnd = round_bf16 if emulate else _ident
    s = scale * torch.einsum("nic,njc->nij", q, k)
    p = torch.exp(s - lse[..., None])
    dp = torch.einsum("nic,njc->nij", d_out, v)
    delta = (d_out * out).sum(dim=2, keepdim=True)
    ds = p * (dp - delta)
    dv = torch.einsum("nij,nic->njc", rnd(p), d_out)
    dk = scale * torch.einsum("nij,nic->njc", rnd(ds), q)
    dq = scale * torch.einsum("nij,njc->nic", rnd(ds), k)
    return rnd(dq), rnd(dk), rnd(dv)


def split_packed(packed, d, q_off, k_off, v_off):
    """The Q, K, V column slices of a packed [N, L, row_stride] tensor."""
    return packed[..., q_off:q_off + d], packed[..., k_off:k_off + d], packed[..., v_off:v_off + d]


# ---- the non-local refine of the balanced map ---------------------------------------------------------------------------
def conv1x1(x, w, b=None):
    """x [..., Cin], w [Cout, Cin] -> [..., Cout]."""
    y = x @ w.t()
    return y if b is None else y + b


def refine_forward(B, w_qkv, b_qkv, w_out, b_out, scale, emulate=False):
    """B [N, h, w, C]; w_qkv [3 Ci, C]; w_out [C, Ci]. Returns (Rf, cache)."""
    rnd = round_bf16 if emulate else _ident
    N, h, w, C = B.shape
    Ci = w_out.shape[1]
    qkv = rnd(conv1x1(B, w_qkv, b_qkv)).reshape(N, h * w, 3 * Ci)
    q, k, v = split_packed(qkv, Ci, 0, Ci, 2 * Ci)
    o, lse = attention_forward(q, k, v, scale, emulate)
    Rf = rnd(B + conv1x1(o, w_out, b_out).reshape(N, h, w, C))
    return Rf, (qkv, o, lse)


def refine_backward(B, dRf, w_qkv, w_out, scale, cache, emulate=False):
    """Returns dict(dB, dw_out, db_out, dw_qkv, db_qkv)."""
    rnd = round_bf16 if emulate else _ident
    N, h, w, C = B.shape
    Ci = w_out.shape[1]
    qkv, o, lse = cache
    q, k, v = split_packed(qkv, Ci, 0, Ci, 2 * Ci)
    g = dRf.reshape(N, h * w, C)
    dy = rnd(g @ w_out)
    dq, dk, dv = attention_backward(q, k, v, dy, scale, o, lse, emulate)
    dqkv = torch.cat([dq, dk, dv], dim=2)
    dB = rnd(dRf + (dqkv @ w_qkv).reshape(N, h, w, C))
    flat = lambda t: t.reshape(-1, t.shape[-1])
    return dict(dB=dB, dw_out=flat(g).t() @ flat(o), db_out=flat(g).sum(0), dw_qkv=flat(dqkv).t() @ flat(B.reshape(N, h * w, C)),
                db_qkv=flat(dqkv).sum(0))


# ---- inputs ------------------------------------------------------------------------------------------------------------
def random_packed(N, L, d, pad, seed, std=0.5):
    """bf16-valued packed [N, L, 3d + pad] tensor (Q | K | V | padding) and a bf16-valued d_out [N, L, d]."""
    g = torch.Generator().manual_seed(seed)
    packed = round_bf16(torch.randn((N, L, 3 * d + pad), generator=g, dtype=F64) * std)
    d_out = round_bf16(torch.randn((N, L, d), generator=g, dtype=F64) * std)
    return packed, d_out


def adversarial_packed(N, L, d, where, seed):
    """Logits s_ij ~ a b_j along one direction e (scale 1, |s| <= 32): where = 'last' puts every row's maximum in the last
    key tile behind steadily growing logits, so the online softmax rescales at every tile; 'first' puts it in the first
    tile with every later logit 60 below, so the later contributions vanish against it."""
    g = torch.Generator().manual_seed(seed)
    e = (torch.randint(0, 2, (d,), generator=g).to(F64) * 2 - 1) / math.sqrt(d)
    a = 4.0
    j = torch.arange(L, dtype=F64)
    if where == "last":
        b = -7.0 + 14.0 * j / max(L - 1, 1)
    else:
        b = torch.where(j < 8, torch.full_like(j, 7.5), torch.full_like(j, -7.5))
    noise = lambda: torch.randn((N, L, d), generator=g, dtype=F64) * 0.005
    q = a * e.expand(N, L, d) + noise()
    k = b[None, :, None] * e[None, None, :] + noise()
    v = torch.randn((N, L, d), generator=g, dtype=F64) * 0.5
    packed = round_bf16(torch.cat([q, k, v], dim=2))
    d_out = round_bf16(torch.randn((N, L, d), generator=g, dtype=F64) * 0.5)
    return packed, d_out
