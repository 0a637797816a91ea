"""The global context block of GCNet (include/mxdet.h): attention pooling over a map, the bottleneck transform
with LayerNorm, and the fused add + shortcut + ReLU, forward and backward.

A ContextPlan holds the descriptor of one (N, HW, C, P) and every buffer the six entries exchange -- logits, lse, ctx, h, mean,
rstd, add, d_add, d_ctx and the workspace -- allocated when the plan is made: a call allocates nothing and never synchronises
the host, so a step can be captured. The workspace carries the chunk partials from one entry to the next: a plan belongs to
one block, and its calls run in the order forward (pool, transform, fuse), backward (reduce, transform, pool) on one stream.
"""
import ctypes

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr

CHUNK = _lib.GC_CHUNK
EPS = 1e-5


def check_shape(C, P):
    """The entries' bounds on the channel widths, as a ValueError."""
    if C % 8 or not 8 <= C <= _lib.GC_MAX_C:
        raise ValueError("global context: C = %r must be a multiple of 8 in [8, %d]" % (C, _lib.GC_MAX_C))
    if P % 8 or not 8 <= P <= _lib.GC_MAX_P:
        raise ValueError("global context: inner width %r must be a multiple of 8 in [8, %d]" % (P, _lib.GC_MAX_P))


def make_desc(N, HW, C, P, eps=EPS):
    d = _lib.GcDescT()
    d.N, d.HW, d.C, d.P, d.eps = N, HW, C, P, eps
    return d


def workspace_bytes(N, HW, C, P, eps=EPS):
    return int(_lib.load().mxdet_gc_workspace_bytes(ctypes.byref(make_desc(N, HW, C, P, eps))))


def _t(t, shape, dtype, what):
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() == shape, \
        "global context: %s must be contiguous cuda %s with %d elements (got %s %s)" % (what, dtype, shape, t.dtype, tuple(t.shape))
    return ptr(t)


class ContextPlan:
    def __init__(self, N, HW, C, P, device="cuda", eps=EPS):
        check_shape(C, P)
        self.N, self.HW, self.C, self.P = N, HW, C, P
        self.desc = make_desc(N, HW, C, P, eps)
        nbytes = workspace_bytes(N, HW, C, P, eps)
        if nbytes == 0:
            raise ValueError("global context: N = %r, HW = %r: %s" % (N, HW, _lib.load().mxdet_last_error().decode()))
        f32 = dict(dtype=torch.float32, device=device)
        self.logits = torch.empty((N, HW), **f32)
        self.lse, self.mean, self.rstd = (torch.empty((N,), **f32) for _ in range(3))
        self.ctx, self.add, self.d_add, self.d_ctx = (torch.empty((N, C), **f32) for _ in range(4))
        self.h = torch.empty((N, P), **f32)
        self.workspace = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        self._ws = (ptr(self.workspace), nbytes)

    # ---- forward
    def pool_forward(self, t, wk):
        """logits and the chunk partials of the attention pooling of t bf16 [N, HW, C] with the mask filter wk bf16 [C]."""
        n = self.N * self.HW * self.C
        check(_lib.load().mxdet_gc_pool_fwd(self.desc, _t(t, n, torch.bfloat16, "t"), _t(wk, self.C, torch.bfloat16, "wk"),
                                            ptr(self.logits), *self._ws, stream_ptr()), "gc_pool_fwd")

    def transform_forward(self, w1, b1, gamma, beta, w2, b2):
        """lse, ctx, h, mean, rstd, add from the chunk partials; returns add f32 [N, C]."""
        C, P, bf, f = self.C, self.P, torch.bfloat16, torch.float32
        check(_lib.load().mxdet_gc_transform_fwd(self.desc, _t(w1, P * C, bf, "W1"), _t(b1, P, f, "b1"), _t(gamma, P, f, "gamma"),
                                                 _t(beta, P, f, "beta"), _t(w2, C * P, bf, "W2"), _t(b2, C, f, "b2"),
                                                 ptr(self.lse), ptr(self.ctx), ptr(self.h), ptr(self.mean), ptr(self.rstd),
                                                 ptr(self.add), *self._ws, stream_ptr()), "gc_transform_fwd")
        return self.add

    def fuse_forward(self, t, sc, y, y_bits=None, add=None):
        """y = bf16(relu(t + add + sc)) and, if given, its 1-bit mask."""
        n = self.N * self.HW * self.C
        bf = torch.bfloat16
        add = self.add if add is None else add
        bits = None if y_bits is None else _t(y_bits, n // 8, torch.uint8, "y_bits")
        check(_lib.load().mxdet_gc_fuse_fwd(self.desc, _t(t, n, bf, "t"), _t(add, self.N * self.C, torch.float32, "add"),
                                            _t(sc, n, bf, "sc"), _t(y, n, bf, "y"), bits, stream_ptr()), "gc_fuse_fwd")
        return y

    # ---- backward
    def reduce_backward(self, ds):
        check(_lib.load().mxdet_gc_reduce_bwd(self.desc, _t(ds, self.N * self.HW * self.C, torch.bfloat16, "ds"), *self._ws,
                                              stream_ptr()), "gc_reduce_bwd")

    def transform_backward(self, w1, gamma, beta, w2, d_w1, d_b1, d_gamma, d_beta, d_w2, d_b2, accumulate=False):
        """d_add and d_ctx into the plan; the six parameter gradients (f32, the parameters' shapes) written or added to."""
        C, P, bf, f = self.C, self.P, torch.bfloat16, torch.float32
        check(_lib.load().mxdet_gc_transform_bwd(
            self.desc, _t(w1, P * C, bf, "W1"), _t(gamma, P, f, "gamma"), _t(beta, P, f, "beta"), _t(w2, C * P, bf, "W2"),
            ptr(self.ctx), ptr(self.h), ptr(self.mean), ptr(self.rstd), ptr(self.d_add), ptr(self.d_ctx),
            _t(d_w1, P * C, f, "dW1"), _t(d_b1, P, f, "db1"), _t(d_gamma, P, f, "dgamma"), _t(d_beta, P, f, "dbeta"),
            _t(d_w2, C * P, f, "dW2"), _t(d_b2, C, f, "db2"), int(bool(accumulate)), *self._ws, stream_ptr()), "gc_transform_bwd")
        return self.d_ctx

    def pool_backward(self, t, wk, ds, d_t, d_wk, accumulate=False):
        """d_t bf16 [N, HW, C] (overwritten) and d_wk f32 [C] (written, or added to with accumulate)."""
        n = self.N * self.HW * self.C
        bf = torch.bfloat16
        check(_lib.load().mxdet_gc_pool_bwd(self.desc, _t(t, n, bf, "t"), _t(wk, self.C, bf, "wk"), _t(ds, n, bf, "ds"),
                                            ptr(self.logits), ptr(self.lse), ptr(self.d_ctx), _t(d_t, n, bf, "d_t"),
                                            _t(d_wk, self.C, torch.float32, "d_wk"), int(bool(accumulate)), *self._ws,
                                            stream_ptr()), "gc_pool_bwd")
        return d_t
