"""Batched single-head softmax attention over a packed [N, L, row_stride] bf16 tensor (include/mxdet.h).

An AttentionPlan holds the descriptor of one geometry, the log-sum-exp the forward entry writes and the backward entry
reads, and the backward entry's workspace; everything is allocated once, nothing in a step.
"""
import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr

HEAD_DIMS = _lib.ATTN_HEAD_DIMS


def _bf16c(t):
    assert t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous(), "expected contiguous cuda bfloat16"
    return t


class AttentionPlan:
    def __init__(self, N, L, d, row_stride, q_off, k_off, v_off, scale, device):
        """Q, K, V: columns [off, off + d) of every row of a [N, L, row_stride] tensor."""
        lib = _lib.load()
        desc = _lib.AttnDescT()
        desc.N, desc.L, desc.d, desc.row_stride = N, L, d, row_stride
        desc.q_off, desc.k_off, desc.v_off, desc.scale = q_off, k_off, v_off, scale
        self.desc = desc
        nbytes = lib.mxdet_attention_workspace_bytes(desc)
        if nbytes == 0:
            raise _lib.MxdetError("attention: %s" % lib.mxdet_last_error().decode("utf-8", "replace"))
        self.N, self.L, self.d, self.row_stride = N, L, d, row_stride
        self.lse = torch.empty((N, L), dtype=torch.float32, device=device)
        self.workspace = torch.empty((nbytes,), dtype=torch.uint8, device=device)

    def _packed(self, t):
        assert t.numel() == self.N * self.L * self.row_stride, "attention: the packed tensor does not have the planned shape"
        return _bf16c(t)

    def _dense(self, t):
        assert t.numel() == self.N * self.L * self.d, "attention: the dense tensor does not have the planned shape"
        return _bf16c(t)

    def forward(self, qkv, out):
        """out [N, L, d] (any view of that many elements, e.g. [N, H, W, d]); the plan's lse is overwritten."""
        check(_lib.load().mxdet_attention_fwd(self.desc, ptr(self._packed(qkv)), ptr(self._dense(out)), ptr(self.lse),
                                              stream_ptr()), "attention_fwd")
        return out

    def backward(self, qkv, out, d_out, d_qkv):
        """d_qkv receives dQ, dK and dV at the plan's offsets; its other columns are left as they are."""
        check(_lib.load().mxdet_attention_bwd(self.desc, ptr(self._packed(qkv)), ptr(self._dense(out)), ptr(self._dense(d_out)),
                                              ptr(self.lse), ptr(self._packed(d_qkv)), ptr(self.workspace),
                                              self.workspace.numel(), stream_ptr()), "attention_bwd")
        return d_qkv
