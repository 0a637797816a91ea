"""Region Proposal Network head over an FPN pyramid: shared 3x3 conv + ReLU, one fused 1x1 conv producing the
objectness logits (channels 0..A-1) and box deltas (channels A..5A-1), RPN targets + losses, proposal generation.

Plugin slot: models/rpn_heads (/root/reference/README.md:28) with ops (README.md:24) and core/anchor, core/loss
(README.md:16,19). Everything (targets, sampling, NMS) stays on the GPU; MXNet-lineage code runs these as
numpy/Cython CustomOps on the host.
"""
import os

import torch

from ...core import anchor as A_
from ...core import loss as L_
from ...ops import dense
from ...ops.proposal import PyramidProposal
from ...ops import rpn_sparse as RS
from ...ops.rpn_sparse import MAX_SLOTS, RPNSparse
from ..utils.layers import ConvLayer, cached_buf

HEAD_CPAD = 64   # fused cls+reg output channels padded so that dgrad's reduction dim is a multiple of 64


RELU_BITS = os.environ.get("MXDET_TUNE_RELU_BITS", "1") == "1"
# backward over the sampled anchors' cells only (ops/rpn_sparse.py). 0: the dense kernels; 1: sparse
# data gradients, weight gradients with the dense bits (RPN_ORDERED below, or the dense kernels on a scattered dt map): every
# result bit-identical to 0; 2: the weight
# gradients over the slots as well (faster; they differ from 0 in fp32 summation order)
RPN_SPARSE = int(os.environ.get("MXDET_TUNE_RPN_SPARSE", "1"))
# mode 1 with grouped weight gradients: 1 = the weight gradients from the active cells too, in the dense split-K summation
# order (bit-identical, no dt map); 0 = the dense kernels on the scattered dt map
RPN_ORDERED = int(os.environ.get("MXDET_TUNE_RPN_ORDERED", "1"))


class RPNHead:
    def __init__(self, channels, strides, arena, ws, device, gen, ratios=(0.5, 1.0, 2.0), scales=(8,),
                 pre_nms_top_n=2000, post_nms_top_n=2000, nms_thresh=0.7, min_size=0.0, batch_size=256,
                 fg_fraction=0.5, fg_thresh=0.7, bg_thresh=0.3, sigma=3.0, seed=99):
        kw = dict(arena=arena, ws=ws, device=device, gen=gen)
        self.A = len(ratios) * len(scales)
        assert 5 * self.A <= HEAD_CPAD
        self.out = ConvLayer("rpn.out", channels, HEAD_CPAD, 1, init_std=0.01, cout_real=5 * self.A, **kw)
        self.conv = ConvLayer("rpn.conv", channels, channels, 3, init_std=0.01, **kw)
        self.strides = list(strides)
        self.base = [torch.from_numpy(A_.generate_base_anchors(s, ratios, scales)).to(device) for s in strides]
        self.proposal = PyramidProposal(self.base, strides, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size)
        self.batch_size, self.fg_fraction, self.fg_thresh, self.bg_thresh = batch_size, fg_fraction, fg_thresh, bg_thresh
        self.sigma, self.seed, self.device, self.C = sigma, seed, device, channels
        self.bufs = {}
        self.anchors = None
        self.level_shapes = None

    def layers(self):
        return [self.out, self.conv]

    def _buf(self, key, shape, dtype=torch.bfloat16, zero=False):
        return cached_buf(self.bufs, key, shape, dtype, self.device, zero)

    def plan(self, p_shapes, g_max):
        for s in p_shapes:
            self.conv.plan(s)
            self.out.plan(s)
        self.level_shapes = [(s[1], s[2]) for s in p_shapes]
        N = p_shapes[0][0]
        self.anchors = torch.cat([A_.generate_anchors(self.base[l], H, W, self.strides[l])
                                  for l, (H, W) in enumerate(self.level_shapes)])
        self.level_offsets = [0]
        for (H, W) in self.level_shapes:
            self.level_offsets.append(self.level_offsets[-1] + H * W * self.A)
        At = self.anchors.shape[0]
        self.at_ws = A_.AnchorTargetWorkspace(N, At, g_max, self.device)
        self.at_out = (torch.empty((N, At), dtype=torch.int32, device=self.device),
                       torch.empty((N, At), dtype=torch.int32, device=self.device),
                       torch.empty((N, At, 4), dtype=torch.float32, device=self.device),
                       torch.empty((N, At), dtype=torch.float32, device=self.device))
        self.nparts = [L_.rpn_loss_num_partials(N, H, W) for (H, W) in self.level_shapes]
        self.partial = torch.zeros((2 * sum(self.nparts),), dtype=torch.float32, device=self.device)
        self.loss = torch.zeros((2,), dtype=torch.float32, device=self.device)
        # the loss leaves at most batch_size sampled anchors per image with a gradient: that many slots
        smax = N * self.batch_size
        self.sparse = (RPNSparse(self.level_shapes, N, self.A, self.C, HEAD_CPAD, smax, self.device)
                       if RPN_SPARSE and 0 < smax <= MAX_SLOTS else None)
        self.sparse_wgrad = int(RPN_SPARSE) == 2
        self.dt_map = None
        if self.sparse is not None and not self.sparse_wgrad:
            # dense dt maps for the dense weight gradient, one flat buffer (cleared by one launch), levels are views
            sizes = [s[0] * s[1] * s[2] * s[3] for s in p_shapes]
            flat = self._buf("dt_map", (sum(sizes),))
            self.dt_map, off = [], 0
            for s, n in zip(p_shapes, sizes):
                self.dt_map.append(flat[off:off + n].view(tuple(s)))
                off += n

    def forward(self, P):
        """The largest level keeps its own launches (it fills the chip and has its own tile path); the remaining levels
        -- a few dozen to a few hundred workgroups each -- share one grouped launch per layer."""
        self.P = P
        tb = [self._buf("t%d" % l, p.shape) for l, p in enumerate(P)]
        hb = [self._buf("h%d" % l, p.shape[:3] + (HEAD_CPAD,)) for l, p in enumerate(P)]
        # 1-bit ReLU masks of the conv activations for the head's data gradient (the P2-level activation is 68.8 MB)
        self.tbits = [self._buf("tb%d" % l, p.shape[:3] + (p.shape[3] // 8,), dtype=torch.uint8) if RELU_BITS else None
                      for l, p in enumerate(P)]
        self.conv.forward(P[0], relu=True, out=tb[0], bits_out=self.tbits[0])
        dense.conv2d_group("fwd", [self.conv.fwd_call(P[l], relu=True, out=tb[l], bits_out=self.tbits[l])
                                   for l in range(1, len(P))], self.device)
        self.out.forward(tb[0], out=hb[0])
        dense.conv2d_group("fwd", [self.out.fwd_call(tb[l], out=hb[l]) for l in range(1, len(P))], self.device)
        self.t, self.h = tb, hb
        return self.h

    def get_proposals(self, im_info):
        return self.proposal(self.h, self.h, im_info, layout="nhwc_fused")

    def assign_targets(self, gt_boxes, im_info, step, image_offset, step_dev=None):
        """Anchor labels / regression targets. They depend on the ground truth and the anchor grid only -- not on any
        network output -- so the caller may issue this long before the head has run."""
        labels, _, targets, _ = A_.assign_anchor(self.anchors, gt_boxes, im_info, self.fg_thresh, self.bg_thresh, 0.0,
                                                 self.batch_size, self.fg_fraction, self.seed, step, image_offset,
                                                 self.at_ws, self.at_out, step_dev)
        self._assigned = (labels, targets)
        if self.sparse is not None:
            self.sparse.build_list(labels)

    def loss_and_grad(self, gt_boxes, im_info, step, image_offset, loss_scale=1.0, step_dev=None, assigned=False):
        """Assign anchors (unless assign_targets() already ran for this step), compute the RPN losses and
        d(loss)/d(head) for every level (bf16)."""
        if not assigned:
            self.assign_targets(gt_boxes, im_info, step, image_offset, step_dev)
        labels, targets = self._assigned
        N = gt_boxes.shape[0]
        norm = 1.0 / float(N * self.batch_size)
        self.gh = []
        off = 0
        for l, h in enumerate(self.h):
            g = self._buf("gh%d" % l, h.shape)
            L_.rpn_loss_level(h, self.A, labels, targets, self.level_offsets[l], self.sigma, norm, loss_scale, g,
                              self.partial[2 * off:])
            off += self.nparts[l]
            self.gh.append(g)
        L_.loss_finalize(self.partial, off, 2, self.loss)
        return self.loss

    def backward(self, dP, dP_has_grad, flush=True):
        """Adds the RPN branch's gradient into dP[l] (overwrites where dP_has_grad[l] is False). flush=False leaves the
        recorded weight gradients pending in the workspace: the caller issues them later (ws.flush())."""
        if self.sparse is not None:
            return self._backward_sparse(dP, dP_has_grad, flush)
        L = len(self.h)
        dt = [self._buf("dt%d" % l, self.t[l].shape) for l in range(L)]
        grouped = self.out.ws.grouping     # grouped form: the plan sums the levels of a shared filter itself
        for l in range(L):
            self.out.backward_weight(self.t[l], self.gh[l], accumulate=(l > 0) and not grouped)
        self.out.backward_data(self.gh[0], self.t[0].shape, relu_mask=self.t[0], out=dt[0], relu_bits=self.tbits[0])
        dense.conv2d_group("dgrad", [self.out.dgrad_call(self.gh[l], self.t[l].shape, relu_mask=self.t[l], out=dt[l],
                                                         relu_bits=self.tbits[l])
                                     for l in range(1, L)], self.device)
        for l in range(L):
            self.conv.backward_weight(self.P[l], dt[l], accumulate=(l > 0) and not grouped)
        self.conv.backward_data(dt[0], self.P[0].shape, accumulate=dP_has_grad[0], out=dP[0])
        dense.conv2d_group("dgrad", [self.conv.dgrad_call(dt[l], self.P[l].shape, accumulate=dP_has_grad[l], out=dP[l])
                                     for l in range(1, L)], self.device)
        if flush:
            self.out.ws.flush()

    def _backward_sparse(self, dP, dP_has_grad, flush=True):
        """The same gradients from the active cells alone (assign_targets listed them): dP is cleared where it holds
        nothing yet, then compact rpn.out data-gradient rows and the rpn.conv data gradient of the touched pixels.
        Weight gradients: the dense kernels as in backward(), rpn.conv's on a dt map that holds the listed rows and zeros
        (same operands bit for bit, so same results); with a grouping workspace (RPN_ORDERED) sums over the active cells in
        the grouped plan's split-K order instead (same bits again), straight into the arena, nothing recorded in the
        workspace and no dt map; or (sparse_wgrad) sums over the slots in slot order, also straight into the arena."""
        g = self.out.arena
        grads = (g.view(self.out.wi, "g"), g.view(self.out.bi, "g"), g.view(self.conv.wi, "g"), g.view(self.conv.bi, "g"))
        if self.sparse_wgrad:
            self.sparse.backward(self.P, self.t, self.tbits, self.gh, dP, dP_has_grad, self.out.wt, self.conv.wt, *grads)
            return
        L = len(self.h)
        grouped = self.out.ws.grouping
        if grouped and RPN_ORDERED and self.out.train_bias and self.conv.train_bias:
            if self.sparse.ordered is None and not torch.cuda.is_current_stream_capturing():
                # the ten items flush() would plan, in the order they are recorded below
                self.sparse.plan_ordered(
                    [(self.t[l], self.gh[l], 1, 1, 1, 0, grads[0], grads[1], False) for l in range(L)] +
                    [(self.P[l], self.dt_map[l], 3, 3, 1, 1, grads[2], grads[3], False) for l in range(L)])
            if self.sparse.ordered is not None:     # (first seen under capture: the dense kernels below)
                self.sparse.backward(self.P, self.t, self.tbits, self.gh, dP, dP_has_grad, self.out.wt, self.conv.wt, *grads,
                                     parts=RS.ZERO | RS.DT | RS.DGRAD | RS.WGRAD_ORDERED)
                return
        for l in range(L):
            self.out.backward_weight(self.t[l], self.gh[l], accumulate=(l > 0) and not grouped)
        self.sparse.backward(self.P, self.t, self.tbits, self.gh, dP, dP_has_grad, self.out.wt, self.conv.wt, *grads,
                             parts=RS.ZERO | RS.DT | RS.DTMAP | RS.DGRAD, dt=self.dt_map)
        for l in range(L):
            self.conv.backward_weight(self.P[l], self.dt_map[l], accumulate=(l > 0) and not grouped)
        if flush:
            self.out.ws.flush()
