"""CARAFE upsampling by 2 (include/mxdet.h): the content-aware reassembly of a coarse map X with the
kernel logits M, forward and backward.

A CarafePlan holds the descriptor of one geometry. The entries need no workspace (the backward recomputes the weights from
M), so a call allocates nothing and never synchronises the host: it can be captured.
"""
import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr

KERNELS = _lib.CARAFE_KERNELS


def logit_channels(k):
    """(real, padded to the conv kernels' multiple of 64) channels of the logits of a k x k reassembly kernel."""
    real = 4 * k * k
    return real, (real + 63) // 64 * 64


def _bf16c(t):
    assert t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous(), "expected contiguous cuda bfloat16"
    return t


class CarafePlan:
    def __init__(self, x_shape, logit_stride, k, out_hw):
        """x_shape (N, H, W, C) of the coarse map; logit_stride = Cm, the channels of the logit tensor (the first 4 k^2 are
        real); out_hw (Hf, Wf), each 2x or 2x - 1 of the coarse size."""
        N, H, W, C = x_shape
        d = _lib.CarafeDescT()
        d.N, d.H, d.W, d.C, d.Cm, d.k, d.Hf, d.Wf = N, H, W, C, logit_stride, k, out_hw[0], out_hw[1]
        self.desc = d
        self.x_shape, self.m_shape, self.y_shape = (N, H, W, C), (N, H, W, logit_stride), (N, out_hw[0], out_hw[1], C)

    def _as(self, t, shape, what):
        assert tuple(t.shape) == shape, "carafe: %s has shape %s, planned %s" % (what, tuple(t.shape), shape)
        return ptr(_bf16c(t))

    def forward(self, x, logits, out):
        check(_lib.load().mxdet_carafe_fwd(self.desc, self._as(x, self.x_shape, "x"), self._as(logits, self.m_shape, "logits"),
                                           self._as(out, self.y_shape, "out"), stream_ptr()), "carafe_fwd")
        return out

    def backward(self, x, logits, d_out, d_x, d_logits, accumulate=False):
        """d_x (+)= the gradient w.r.t. x; d_logits is overwritten (exact zeros in its padding channels)."""
        check(_lib.load().mxdet_carafe_bwd(self.desc, self._as(x, self.x_shape, "x"), self._as(logits, self.m_shape, "logits"),
                                           self._as(d_out, self.y_shape, "d_out"), self._as(d_x, self.x_shape, "d_x"),
                                           self._as(d_logits, self.m_shape, "d_logits"), int(bool(accumulate)), stream_ptr()),
              "carafe_bwd")
        return d_x, d_logits
