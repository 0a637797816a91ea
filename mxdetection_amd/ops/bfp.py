"""Balanced Feature Pyramid gather / scatter (include/mxdet.h): one launch per entry for all pyramid levels.

A BfpPlan holds the descriptor of one pyramid geometry and the arg-maxima workspace the forward entries fill and the
backward entries read; nothing is allocated in a step.
"""
import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr

MAX_LEVELS = _lib.BFP_MAX_LEVELS


def _bf16c(t):
    assert t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous(), "expected contiguous cuda bfloat16"
    return t


class BfpPlan:
    def __init__(self, shapes, refine_level, device):
        """shapes: [(N, H, W, C)] of the levels, finest first."""
        lib = _lib.load()
        self.shapes = [tuple(s) for s in shapes]
        self.r = refine_level
        d = _lib.BfpDescT()
        d.num_levels, d.refine_level = len(self.shapes), refine_level
        d.N, d.C = (self.shapes[0][0], self.shapes[0][3]) if self.shapes else (0, 0)
        for l, s in enumerate(self.shapes[:8]):
            d.H[l], d.W[l] = s[1], s[2]
        self.desc = d
        nbytes = lib.mxdet_bfp_workspace_bytes(d)
        if nbytes == 0:
            raise _lib.MxdetError("bfp: %s" % lib.mxdet_last_error().decode("utf-8", "replace"))
        self.workspace = torch.empty((nbytes,), dtype=torch.uint8, device=device)

    @property
    def refine_shape(self):
        return self.shapes[self.r]

    def _bind(self, feats, outs=None):
        assert len(feats) == len(self.shapes) and all(tuple(f.shape) == s for f, s in zip(feats, self.shapes)), \
            "bfp: the pyramid does not have the planned shapes %s" % (self.shapes,)
        for l, f in enumerate(feats):
            self.desc.feat[l] = _bf16c(f).data_ptr()
            self.desc.out[l] = _bf16c(outs[l]).data_ptr() if outs is not None else None
        return self.desc

    def gather_forward(self, feats, out):
        check(_lib.load().mxdet_bfp_gather_fwd(self._bind(feats), ptr(_bf16c(out)), ptr(self.workspace), self.workspace.numel(),
                                               stream_ptr()), "bfp_gather_fwd")
        return out

    def scatter_forward(self, feats, refined, outs):
        check(_lib.load().mxdet_bfp_scatter_fwd(self._bind(feats, outs), ptr(_bf16c(refined)), ptr(self.workspace),
                                                self.workspace.numel(), stream_ptr()), "bfp_scatter_fwd")
        return outs

    def scatter_backward(self, d_outs, d_refined):
        check(_lib.load().mxdet_bfp_scatter_bwd(self._bind(d_outs), ptr(_bf16c(d_refined)), ptr(self.workspace),
                                                self.workspace.numel(), stream_ptr()), "bfp_scatter_bwd")
        return d_refined

    def gather_backward(self, d_outs, d_balanced, d_feats=None):
        """d_feats None: in place over d_outs."""
        d_feats = d_outs if d_feats is None else d_feats
        check(_lib.load().mxdet_bfp_gather_bwd(self._bind(d_outs, d_feats), ptr(_bf16c(d_balanced)), ptr(self.workspace),
                                               self.workspace.numel(), stream_ptr()), "bfp_gather_bwd")
        return d_feats
