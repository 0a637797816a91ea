"""Deformable RoI extractor: (modulated) deformable RoI pooling with its offset head, mmdetection's
(Modulated)DeformRoIPoolingPack on the FPN pyramid (level map as FPNRoIExtractor).

Plugin slot: models/roi_extractors (/root/reference/README.md:32); MXNet role contrib.DeformablePSROIPooling (group_size
1, class-agnostic offsets). One forward is two pooling passes:
  pass 0: pooling without trans -> x0 [R,7,7,C]
  offset head: `offset_fc` (offset_fcs FCs: 1024 hidden, ReLU; the last 7*7*2 outputs padded to 128) and, modulated,
    `mask_fc` (C*49 -> 1024, ReLU, -> 49 padded to 64) on x0; the last FC of each branch starts at zero
  pass 1: pooling with trans = offset_fc(x0) (and mask = sigmoid(mask_fc(x0))) -> the box head's input.
Backward (backward_gather, in the slot of FPNRoIExtractor.backward_gather): pass-1 adjoint into dP plus d_trans / d_mask,
the offset head's backward (weight gradients through Workspace.defer, like every layer's) down to d_x0, then the pass-0
adjoint into dP. Every adjoint is the deterministic gather of csrc/deform_roi_pool.hip.
"""
import torch

from ...ops.deform_roi_pool import (dpool_backward_feat, dpool_backward_feat_workspace, dpool_backward_trans,
                                    dpool_forward)
from ...ops.roi_align import fpn_level_map
from ..utils.layers import LayerChain, buf_cache


class DeformRoIExtractor:
    def __init__(self, strides, channels, arena, ws, device, modulated=True, trans_std=0.1, sample_per_part=4,
                 offset_fcs=3, fc_dim=1024, pooled=(7, 7), lvl_min=2, seed=4711):
        assert offset_fcs >= 1
        self.scales = [1.0 / s for s in strides]
        self.pooled, self.lvl_min = tuple(pooled), lvl_min
        self.lvl_max = lvl_min + len(strides) - 1
        self.modulated, self.trans_std, self.spp = bool(modulated), float(trans_std), int(sample_per_part)
        self.device = device
        nb = self.pooled[0] * self.pooled[1]
        self.in_features = nb * channels
        # hidden FCs draw from a generator of their own: every parameter of the plain model keeps its random draw
        kw = dict(arena=arena, ws=ws, device=device, gen=torch.Generator().manual_seed(seed))

        def branch(name, n, nreal):
            """n FCs: fc_dim hidden with ReLU; the last has nreal outputs (padded to 64s), starts at zero, no ReLU."""
            specs = [dict(name="bbox.%s%d" % (name, i + 1), cin=fc_dim if i else self.in_features, cout=fc_dim, k=1)
                     for i in range(n)]
            specs[-1].update(cout=(nreal + 63) // 64 * 64, cout_real=nreal, zero_init=True, relu=False)
            return LayerChain(specs, **kw)
        # registration order == backward completion order: the last FCs' weight gradients are issued first
        self.offset_chain = branch("offset_fc", offset_fcs, 2 * nb)
        self.mask_chain = branch("mask_fc", 2, nb) if self.modulated else None
        self.offset_fc = self.offset_chain.convs
        self.mask_fc = self.mask_chain.convs if self.modulated else []
        # checkpoint layout (CheckpointMixin._to_mx): 2-D FC weights, the pooled-input ones reordered from (H, W, C) to (C, H, W)
        for l in self.layers():
            l.fc_in_hwc = (self.pooled[0], self.pooled[1], channels) if l.cin == self.in_features else ()
        self.bufs, self._buf = buf_cache(device)

    def layers(self):
        """In registration (= backward completion) order."""
        return self.offset_chain.layers() + (self.mask_chain.layers() if self.modulated else [])

    def plan(self, R):
        for l in self.layers():
            l.plan((R, 1, 1, l.cin))

    def forward(self, feats, rois, prepare_gather=False):
        """feats: P2..P5 (bf16 [N,H,W,C]); rois [R,5] f32 -> pass-1 pooled bf16 [R,PH,PW,C]. (prepare_gather: accepted for
        FPNRoIExtractor's interface; the gather's records depend on the offsets and are built in backward_gather.)"""
        self.feats, self.rois = feats[:len(self.scales)], rois
        self.levels = fpn_level_map(rois, self.lvl_min, self.lvl_max)
        R, Cc = rois.shape[0], feats[0].shape[3]
        PH, PW = self.pooled
        a = dict(pooled=self.pooled, sample_per_part=self.spp, trans_std=self.trans_std, lvl_min=self.lvl_min)
        self.x0 = dpool_forward(self.feats, self.scales, rois, self.levels, out=self._buf("x0", (R, PH, PW, Cc)), **a)
        h = self.x0.view(R, 1, 1, -1)
        self.trans = self.offset_chain.forward(h, self._buf).view(R, -1)
        self.mask = self.mask_chain.forward(h, self._buf).view(R, -1) if self.modulated else None
        return dpool_forward(self.feats, self.scales, rois, self.levels, trans=self.trans, mask=self.mask,
                             out=self._buf("x1", (R, PH, PW, Cc)), **a)

    def backward_gather(self, grad_out, dP, accumulate=True):
        """Adds the gradient of both pooling passes (through the offset head) into the bf16 maps dP[l]; the offset head's
        weight gradients go out like every layer's (Workspace.defer in grouped mode)."""
        R = self.rois.shape[0]
        a = dict(sample_per_part=self.spp, trans_std=self.trans_std, lvl_min=self.lvl_min)
        ws = self.bufs.get(("dpool_ws", R))           # per roi count, never freed (a captured step holds it)
        if ws is None:
            ws = self.bufs[("dpool_ws", R)] = dpool_backward_feat_workspace(R, self.pooled, self.device)
        # 1. pass-1 adjoint: d_trans / d_mask, then the features
        d_trans, d_mask = dpool_backward_trans(self.feats, self.scales, self.rois, self.levels, grad_out, self.trans,
                                               self.mask, d_trans=self._buf("d_trans", self.trans.shape),
                                               d_mask=self._buf("d_mask", self.mask.shape) if self.modulated else None,
                                               **a)
        dpool_backward_feat(dP, self.scales, self.rois, self.levels, grad_out, self.trans, self.mask,
                            accumulate=accumulate, workspace=ws, **a)
        # 2. offset head backward -> d_x0
        d_x0 = self.offset_chain.backward(d_trans.view(R, 1, 1, -1), self._buf)
        if self.modulated:      # the second branch on x0 adds its gradient
            self.mask_chain.backward(d_mask.view(R, 1, 1, -1), self._buf, add_to=d_x0)
        # 3. pass-0 adjoint
        dpool_backward_feat(dP, self.scales, self.rois, self.levels, d_x0.view(self.x0.shape), accumulate=True,
                            workspace=ws, **a)
