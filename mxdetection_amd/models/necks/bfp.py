"""Balanced Feature Pyramid (Libra R-CNN, Pang et al., CVPR 2019): a second neck stage behind the FPN.

Plugin slot: models/necks (/root/reference/README.md:31). The L pyramid levels are gathered onto the refine level's grid
(adaptive max pool from the finer levels, nearest resize from the coarser ones) and averaged, the balanced map is refined,
and the result is scattered back and added to every level (nearest resize to the finer levels, adaptive max pool to the
coarser ones). Gather and scatter are one launch each (ops/bfp.py). The refine step is one of
  "conv"               one 3x3 convolution, a ConvLayer like the FPN's output convs;
  "embedded_gaussian"  the paper's non-local block (Wang et al. 2018, embedded Gaussian): Rf = B + W_out Attn(theta, phi, g) +
                       b_out. [theta | phi | g] is ONE 1x1 ConvLayer C -> 3 Ci (`bfp.nl.qkv`) whose packed output the
                       attention entries read in place (ops/attention.py), `bfp.nl.out` is a 1x1 ConvLayer
                       Ci -> C with the residual add fused, zero at the start: the block starts as the identity;
  "none"               not at all.
Ci = C / nl_reduction must be 64 or 128 (reduction 1, Ci = 256, is not built: DESIGN.md section 8).
"""
import torch

from ...ops.attention import HEAD_DIMS, AttentionPlan
from ...ops.bfp import BfpPlan
from ..utils.layers import ConvLayer, cached_buf

REFINES = ("conv", "none", "embedded_gaussian")


def check_neck(neck, bfp_refine="conv", bfp_nl_reduction=2, bfp_nl_use_scale=False, channels=256):
    """The neck options of FasterRCNN, checked before anything is allocated."""
    if neck not in ("fpn", "bfp"):
        raise ValueError("neck must be 'fpn' or 'bfp' (got %r)" % (neck,))
    if bfp_refine not in REFINES:
        raise ValueError("bfp_refine must be one of %s (got %r)" % (", ".join(REFINES), bfp_refine))
    r = bfp_nl_reduction
    if not isinstance(r, int) or isinstance(r, bool) or r < 1 or channels % r or channels // r not in HEAD_DIMS:
        raise ValueError("bfp_nl_reduction must divide %d channels into one of %s (got %r)" % (channels, HEAD_DIMS, r))
    if not isinstance(bfp_nl_use_scale, (bool, int)):
        raise ValueError("bfp_nl_use_scale must be a bool (got %r)" % (bfp_nl_use_scale,))


class BFP:
    def __init__(self, channels, arena, ws, device, gen, refine="conv", refine_level=2, nl_reduction=2, nl_use_scale=False):
        """gen: a generator of the BFP's own, so every other parameter of the model starts as without it."""
        check_neck("bfp", refine, nl_reduction, nl_use_scale, channels)
        self.C, self.r, self.device = channels, refine_level, device
        self.refine = self.nl_qkv = self.nl_out = None
        if refine == "conv":   # Xavier-style like the FPN's output convs: no ReLU follows
            self.refine = ConvLayer("bfp.refine", channels, channels, 3, init_std=(1.0 / (9 * channels)) ** 0.5, arena=arena,
                                    ws=ws, device=device, gen=gen)
        if refine == "embedded_gaussian":
            # registration = backward completion order: the output conv's weight gradient is final first
            self.Ci = channels // nl_reduction
            self.nl_scale = self.Ci ** -0.5 if nl_use_scale else 1.0
            self.nl_out = ConvLayer("bfp.nl.out", self.Ci, channels, 1, arena=arena, ws=ws, device=device, gen=gen,
                                    zero_init=True)
            self.nl_qkv = ConvLayer("bfp.nl.qkv", channels, 3 * self.Ci, 1, init_std=0.01, arena=arena, ws=ws, device=device,
                                    gen=gen)
        self.bufs, self.plans, self.attn_plans = {}, {}, {}
        self.plan_ = self.attn_ = self.B = self.Q = None

    def layers(self):
        if self.nl_out is not None:
            return [self.nl_out, self.nl_qkv]
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
            if self.nl_out is not None:
                N, h, w, _ = p.refine_shape
                self.nl_qkv.plan(p.refine_shape)
                self.nl_out.plan((N, h, w, self.Ci))
                self.attn_plans[key] = AttentionPlan(N, h * w, self.Ci, 3 * self.Ci, 0, self.Ci, 2 * self.Ci, self.nl_scale,
                                                     self.device)
        self.plan_, self.attn_ = p, self.attn_plans.get(key)
        return p

    def _refine_forward(self, B, shape):
        if self.nl_out is not None:
            N, h, w, _ = shape
            self.qkv = self.nl_qkv.forward(B, out=self._buf("qkv", (N, h, w, 3 * self.Ci)))
            self.O = self.attn_.forward(self.qkv, self._buf("O", (N, h, w, self.Ci)))
            return self.nl_out.forward(self.O, residual=B, out=self._buf("Rf", shape))
        return B if self.refine is None else self.refine.forward(B, out=self._buf("Rf", shape))

    def _refine_backward(self, dRf, shape):
        """The gradient w.r.t. B; the refine layers' weight gradients on the way."""
        if self.nl_out is not None:
            self.nl_out.backward_weight(self.O, dRf)
            dY = self.nl_out.backward_data(dRf, self.O.shape, out=self._buf("dY", self.O.shape))
            dqkv = self.attn_.backward(self.qkv, self.O, dY, self._buf("dqkv", self.qkv.shape))
            self.nl_qkv.backward_weight(self.B, dqkv)
            return self.nl_qkv.backward_data(dqkv, shape, residual=dRf, out=self._buf("dB", shape))
        if self.refine is None:
            return dRf
        self.refine.backward_weight(self.B, dRf)
        return self.refine.backward_data(dRf, shape, out=self._buf("dB", shape))

    def forward(self, P):
        """P: the FPN's levels, finest first. Returns Q, the levels everything downstream reads."""
        p = self.plan([tuple(t.shape) for t in P])
        self.B = p.gather_forward(P, self._buf("B", p.refine_shape))
        Rf = self._refine_forward(self.B, p.refine_shape)
        self.Q = p.scatter_forward(P, Rf, [self._buf("Q%d" % l, s) for l, s in enumerate(p.shapes)])
        return self.Q

    def backward(self, dQ):
        """dQ[l]: the gradient w.r.t. Q_l; overwritten with the gradient w.r.t. P_l."""
        p = self.plan_
        dRf = p.scatter_backward(dQ, self._buf("dRf", p.refine_shape))
        p.gather_backward(dQ, self._refine_backward(dRf, p.refine_shape))
        return dQ
