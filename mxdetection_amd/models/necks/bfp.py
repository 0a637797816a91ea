"""Balanced Feature Pyramid (Libra R-CNN, Pang et al., CVPR 2019): a second neck stage behind the FPN.

Plugin slot: models/necks (/root/reference/README.md:31). The L pyramid levels are gathered onto the refine level's grid
(adaptive max pool from the finer levels, nearest resize from the coarser ones) and averaged, the balanced map is refined
by one 3x3 convolution (`refine="conv"`; "none": not at all), and the result is scattered back and added to every level
(nearest resize to the finer levels, adaptive max pool to the coarser ones). Gather and scatter are one launch each
(ops/bfp.py); the refine convolution is a ConvLayer like the FPN's output convs. The paper's non-local refine is not
implemented.
"""
import torch

from ...ops.bfp import BfpPlan
from ..utils.layers import ConvLayer, cached_buf

REFINES = ("conv", "none")


def check_neck(neck, bfp_refine="conv"):
    """The neck options of FasterRCNN, checked before anything is allocated."""
    if neck not in ("fpn", "bfp"):
        raise ValueError("neck must be 'fpn' or 'bfp' (got %r)" % (neck,))
    if bfp_refine not in REFINES:
        raise ValueError("bfp_refine must be one of %s (got %r)" % (", ".join(REFINES), bfp_refine))


class BFP:
    def __init__(self, channels, arena, ws, device, gen, refine="conv", refine_level=2):
        """gen: a generator of the BFP's own, so every other parameter of the model starts as without it."""
        check_neck("bfp", refine)
        self.C, self.r, self.device = channels, refine_level, device
        self.refine = None
        if refine == "conv":   # Xavier-style like the FPN's output convs: no ReLU follows
            self.refine = ConvLayer("bfp.refine", channels, channels, 3, init_std=(1.0 / (9 * channels)) ** 0.5, arena=arena,
                                    ws=ws, device=device, gen=gen)
        self.bufs, self.plans = {}, {}
        self.plan_ = self.B = self.Q = None

    def layers(self):
        return [self.refine] if self.refine is not None else []

    def _buf(self, key, shape):
        return cached_buf(self.bufs, key, shape, torch.bfloat16, self.device)

    def plan(self, p_shapes):
        key = tuple(tuple(s) for s in p_shapes)
        p = self.plans.get(key)
        if p is None:
            p = self.plans[key] = BfpPlan(key, self.r, self.device)
            if self.refine is not None:
                self.refine.plan(p.refine_shape)
        self.plan_ = p
        return p

    def forward(self, P):
        """P: the FPN's levels, finest first. Returns Q, the levels everything downstream reads."""
        p = self.plan([tuple(t.shape) for t in P])
        self.B = p.gather_forward(P, self._buf("B", p.refine_shape))
        Rf = self.B if self.refine is None else self.refine.forward(self.B, out=self._buf("Rf", p.refine_shape))
        self.Q = p.scatter_forward(P, Rf, [self._buf("Q%d" % l, s) for l, s in enumerate(p.shapes)])
        return self.Q

    def backward(self, dQ):
        """dQ[l]: the gradient w.r.t. Q_l; overwritten with the gradient w.r.t. P_l."""
        p = self.plan_
        dRf = p.scatter_backward(dQ, self._buf("dRf", p.refine_shape))
        dB = dRf
        if self.refine is not None:
            self.refine.backward_weight(self.B, dRf)
            dB = self.refine.backward_data(dRf, self.B.shape, out=self._buf("dB", p.refine_shape))
        p.gather_backward(dQ, dB)
        return dQ
