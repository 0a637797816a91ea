"""Box heads. BBoxHead (2fc): flatten(7x7x256) -> FC 1024 + ReLU -> FC 1024 + ReLU -> fused (cls 81 | reg 324) FC.

Plugin slot: models/bbox_heads (/root/reference/README.md:29) with core/bbox + core/loss (README.md:17,19).
The FCs run on the same MFMA implicit-GEMM kernels as the convolutions (1x1 on [R,1,1,C] tensors); cls and reg
share one GEMM whose output is padded to 448 columns (a multiple of 64, so dgrad can reduce over it).

ConvFCBBoxHead (4conv1fc, the GN head recipe of Detectron / mmdetection): 4 x (conv3x3 256 -> 256 [-> GroupNorm] -> ReLU)
on [R,7,7,256] -> FC 12544 -> 1024 + ReLU -> the same fused output layer. It shares sampling, loss, the padded output
layer, checkpoint layout and the layers() ordering with BBoxHead.
"""
import os

import torch

from ...core import bbox as B_
from ...core import loss as L_
from ...ops import dense
from ..utils.layers import ConvLayer, GroupNormLayer, cached_buf


class BBoxHead:
    def __init__(self, in_features, arena, ws, device, gen, num_classes=81, fc_dim=1024, rois_per_image=512,
                 fg_fraction=0.25, fg_thresh=0.5, bg_hi=0.5, bg_lo=0.0, stds=(0.1, 0.1, 0.2, 0.2), sigma=1.0,
                 seed=99, reg_loss="smooth_l1", reg_loss_weight=1.0, ohem=False, ohem_nms=0.7):
        """reg_loss: 'smooth_l1' on the encoded deltas (core.loss.rcnn_loss), or 'iou' / 'giou' / 'diou' on the decoded
        box times reg_loss_weight (core.loss.rcnn_loss_iou; the head still predicts deltas, inference is the same).
        ohem / ohem_nms: online hard example mining (sample): the training RoIs are the rois_per_image highest-loss
        candidates of a read-only pass, deduplicated by NMS at ohem_nms (1 = none); fg_fraction is not used."""
        L_.check_reg_loss(reg_loss, reg_loss_weight)
        B_.check_ohem(ohem_nms)
        self.ohem, self.ohem_nms = bool(ohem), float(ohem_nms)
        self.ohem_extractor = None        # the detector's box RoI extractor (set by the detector that owns both)
        self.reg_loss, self.reg_loss_weight = reg_loss, float(reg_loss_weight)
        kw = dict(arena=arena, ws=ws, device=device, gen=gen)
        self.nc = num_classes
        self.reg_dim = 4 * num_classes
        self.ld = (num_classes + self.reg_dim + 63) // 64 * 64
        self.fc_out = ConvLayer("bbox.fc_out", fc_dim, self.ld, 1, init_std=0.01, cout_real=num_classes + self.reg_dim, **kw)
        self._build_trunk(in_features, fc_dim, kw)
        self.fc_out.fc_in_hwc = ()
        self.R, self.fg_fraction, self.fg_thresh, self.bg_hi, self.bg_lo = rois_per_image, fg_fraction, fg_thresh, bg_hi, bg_lo
        self.stds, self.sigma, self.seed, self.device = stds, sigma, seed, device
        self.in_features, self.fc_dim = in_features, fc_dim
        self.fc1_ksplit = int(os.environ.get("MXDET_TUNE_FC1_KSPLIT", "4"))
        self.bufs = {}

    def _build_trunk(self, in_features, fc_dim, kw):
        """The layers in front of fc_out, registered in backward completion order."""
        self.fc2 = ConvLayer("bbox.fc2", fc_dim, fc_dim, 1, **kw)
        self.fc1 = ConvLayer("bbox.fc1", in_features, fc_dim, 1, **kw)
        # checkpoint layout (CheckpointMixin._to_mx): fully connected layers are stored 2-D; fc1's input is the pooled
        # [7,7,C] block flattened (H, W, C) here and (C, H, W) in an MXNet FullyConnected after a Flatten of NCHW
        pooled = 7
        self.fc1.fc_in_hwc = (pooled, pooled, in_features // (pooled * pooled)) if in_features % (pooled * pooled) == 0 else ()
        self.fc2.fc_in_hwc = ()

    def layers(self):
        return [self.fc_out, self.fc2, self.fc1]

    def norm_layers(self):
        return []

    def _buf(self, key, shape, dtype=torch.bfloat16, zero=False):
        return cached_buf(self.bufs, key, shape, dtype, self.device, zero)

    def plan(self, N):
        R = N * self.R
        self.fc1.plan((R, 1, 1, self.in_features))
        self.fc2.plan((R, 1, 1, self.fc_dim))
        self.fc_out.plan((R, 1, 1, self.fc_dim))
        self.loss = torch.zeros((2,), dtype=torch.float32, device=self.device)
        self.loss_ws = L_.loss_workspace(R, self.device)

    def sample(self, rois, num_rois, gt_boxes, step, image_offset, step_dev=None, feats=None):
        """proposal-target: returns rois [N*R,5] and keeps labels / targets / weights (and the ground truth, which the
        IoU-family losses read on the device) for the loss. feats (the pyramid) is read by the OHEM route only."""
        if self.ohem:
            return self._sample_ohem(rois, num_rois, gt_boxes, step, image_offset, step_dev, feats)
        out = B_.sample_rois(rois, num_rois, gt_boxes, self.R, self.fg_fraction, self.fg_thresh, self.bg_hi, self.bg_lo,
                             self.nc, False, (0.0, 0.0, 0.0, 0.0), self.stds, self.seed, step, image_offset, step_dev)
        self.rois, self.labels, self.tgt, self.wgt, self.matched, self.num_fg = out
        self.gt_boxes = gt_boxes
        return self.rois.view(-1, 5)

    def _sample_ohem(self, rois, num_rois, gt_boxes, step, image_offset, step_dev, feats):
        """Online hard example mining (Shrivastava et al. 2016), all on the device:
          1. the pool: proposal-target with rois_per_image = P and fg_fraction = 1 returns EVERY candidate of an image (all
             foreground, then all background, ascending, then padding) -- the Philox keys decide nothing;
          2. a read-only pass of the RoI extractor and of this head over the N * P pool rows, in buffers of that row count
             (nothing of it is read by backward: the training pass runs forward again on the chosen rows);
          3. the per-roi loss, the order by it, NMS dedup, the first R survivors (core.bbox.ohem_select);
          4. their rows, foreground first (FCNMaskHead.select_rois relies on it), in the attributes sample() always fills.
        The pool (pool_*), ohem_score [N,P] and ohem_sel [N,R] stay for inspection."""
        if feats is None or self.ohem_extractor is None:
            raise ValueError("ohem: sample() needs the pyramid (feats) and the box RoI extractor (ohem_extractor)")
        N, S, G = rois.shape[0], rois.shape[1], gt_boxes.shape[1]
        P = B_.ohem_pool_size(S, G)
        pool = B_.sample_rois(rois, num_rois, gt_boxes, P, 1.0, self.fg_thresh, self.bg_hi, self.bg_lo, self.nc, False,
                              (0.0, 0.0, 0.0, 0.0), self.stds, self.seed, step, image_offset, step_dev)
        self.pool_rois, self.pool_labels, self.pool_tgt, self.pool_wgt, self.pool_matched, self.pool_num_fg = pool
        pooled = self.ohem_extractor.forward(feats, self.pool_rois.view(-1, 5), prepare_gather=False)
        o2 = self.forward(pooled).view(N * P, self.ld)
        iou = self.reg_loss != "smooth_l1"
        score = L_.ohem_roi_score(o2, o2[:, self.nc:], self.pool_labels, self.nc, self.reg_dim, self.ld, self.ld, self.reg_loss,
                                  bbox_targets=self.pool_tgt, bbox_weights=self.pool_wgt, sigma=self.sigma,
                                  rois=self.pool_rois, matched_gt=self.pool_matched, gt_boxes=gt_boxes, stds=self.stds,
                                  reg_weight=self.reg_loss_weight, score=self._buf("ohem_score", (N * P,), torch.float32))
        self.ohem_score = score.view(N, P)
        ws = self.bufs.get(("ohem_ws", N, P))
        if ws is None:
            ws = self.bufs[("ohem_ws", N, P)] = B_.ohem_select_workspace(N, P, self.device)
        self.ohem_sel, self.ohem_num_sel, self.num_fg = B_.ohem_select(
            self.ohem_score, self.pool_labels, self.pool_rois, self.R, self.ohem_nms, workspace=ws,
            sel=self._buf("ohem_sel", (N, self.R), torch.int32), num_sel=self._buf("ohem_num_sel", (N,), torch.int32),
            num_fg=self._buf("ohem_num_fg", (N,), torch.int32))
        # the IoU-family losses read neither targets nor weights: their 2 x 4 * num_classes floats per row stay in the pool
        self.rois, self.labels, self.tgt, self.wgt, self.matched = B_.ohem_gather(
            self.ohem_sel, self.pool_rois, self.pool_labels, self.pool_matched, None if iou else self.pool_tgt,
            None if iou else self.pool_wgt)
        self.gt_boxes = gt_boxes
        return self.rois.view(-1, 5)

    def forward(self, pooled):
        R = pooled.shape[0]
        self.x = pooled.view(R, 1, 1, -1)
        # fc1 is 196 K-steps on 16 x 16 tiles of 64 x 64: one latency-bound wave per SIMD on its own (118 us in the step
        # while nothing else runs). Split four ways the grid fills the chip; the fold is deterministic (split order).
        ks = self.fc1_ksplit if (R * self.fc_dim) % (64 * 64 * 8) == 0 and R % 64 == 0 else 1
        if ks > 1:
            need = 4 * ks * R * self.fc_dim
            ws = self._buf("fc1_ws", (need,), dtype=torch.uint8)
            self.h1 = dense.conv2d_forward_splitk(self.x, self.fc1.w_bf16, self.fc1.bias_f32, None, True, ks,
                                                  self._buf("h1", (R, 1, 1, self.fc_dim)), ws)
        else:
            self.h1 = self.fc1.forward(self.x, relu=True, out=self._buf("h1", (R, 1, 1, self.fc_dim)))
        self.h2 = self.fc2.forward(self.h1, relu=True, out=self._buf("h2", (R, 1, 1, self.fc_dim)))
        self.o = self.fc_out.forward(self.h2, out=self._buf("o", (R, 1, 1, self.ld)))
        return self.o

    def loss_and_grad(self, loss_scale=1.0):
        R = self.o.shape[0]
        o2 = self.o.view(R, self.ld)
        self.go = self._buf("go", (R, 1, 1, self.ld), zero=True)   # padding columns stay zero forever
        g2 = self.go.view(R, self.ld)
        if self.reg_loss == "smooth_l1":
            L_.rcnn_loss(o2, o2[:, self.nc:], self.labels, self.tgt, self.wgt, self.nc, self.reg_dim, self.ld, self.ld,
                         self.sigma, 1.0 / R, loss_scale, g2, g2[:, self.nc:], self.loss, self.loss_ws)
        else:
            L_.rcnn_loss_iou(o2, o2[:, self.nc:], self.labels, self.rois, self.matched, self.gt_boxes, self.nc, self.reg_dim,
                             self.ld, self.ld, self.reg_loss, self.stds, self.reg_loss_weight, 1.0 / R, loss_scale, g2,
                             g2[:, self.nc:], self.loss, self.loss_ws)
        return self.loss

    def backward(self):
        R = self.o.shape[0]
        self.fc_out.backward_weight(self.h2, self.go)
        d_h2 = self.fc_out.backward_data(self.go, self.h2.shape, relu_mask=self.h2, out=self._buf("dh2", self.h2.shape))
        self.fc2.backward_weight(self.h1, d_h2)
        d_h1 = self.fc2.backward_data(d_h2, self.h1.shape, relu_mask=self.h1, out=self._buf("dh1", self.h1.shape))
        self.fc1.backward_weight(self.x, d_h1)
        d_x = self.fc1.backward_data(d_h1, self.x.shape, out=self._buf("dx", self.x.shape))
        return d_x


class ConvFCBBoxHead(BBoxHead):
    """4conv1fc. norm = "gn": every conv is bias-free and followed by GroupNorm with the ReLU fused into the GN kernel, so
    the conv's data gradient takes no ReLU mask (the GN backward applies it)."""

    def __init__(self, in_features, arena, ws, device, gen, num_convs=4, conv_dim=256, norm="none", gn_groups=32, **kw):
        self.num_convs, self.conv_dim, self.norm, self.gn_groups = num_convs, conv_dim, norm, gn_groups
        assert in_features == 7 * 7 * conv_dim
        super().__init__(in_features, arena, ws, device, gen, **kw)

    def _build_trunk(self, in_features, fc_dim, kw):
        C = self.conv_dim
        self.fc1 = ConvLayer("bbox.fc1", in_features, fc_dim, 1, **kw)
        self.fc1.fc_in_hwc = (7, 7, C)
        gn = self.norm == "gn"
        self.convs, self.norms = [None] * self.num_convs, [None] * self.num_convs
        for i in reversed(range(self.num_convs)):     # backward completion order: GN i, then conv i
            if gn:
                self.norms[i] = GroupNormLayer("bbox.conv%d_gn" % i, C, self.gn_groups, kw["arena"], kw["device"])
            self.convs[i] = ConvLayer("bbox.conv%d" % i, C, C, 3, bias=not gn, **kw)

    def layers(self):
        return [self.fc_out, self.fc1] + list(reversed(self.convs))

    def norm_layers(self):
        return [n for n in reversed(self.norms) if n is not None]

    def plan(self, N):
        R = N * self.R
        shp = (R, 7, 7, self.conv_dim)
        for c, n in zip(self.convs, self.norms):
            c.plan(shp)
            if n is not None:
                n.plan(shp)
        self.fc1.plan((R, 1, 1, self.in_features))
        self.fc_out.plan((R, 1, 1, self.fc_dim))
        self.loss = torch.zeros((2,), dtype=torch.float32, device=self.device)
        self.loss_ws = L_.loss_workspace(R, self.device)

    def forward(self, pooled):
        R = pooled.shape[0]
        x = pooled.view(R, 7, 7, self.conv_dim)
        self.acts = [x]
        for i, (c, n) in enumerate(zip(self.convs, self.norms)):
            if n is None:
                x = c.forward(x, relu=True, out=self._buf("a%d" % i, x.shape))
            else:
                x = n.forward(c.forward(x, out=self._buf("c%d" % i, x.shape)), relu=True, out=self._buf("a%d" % i, x.shape))
            self.acts.append(x)
        self.x = x.view(R, 1, 1, -1)
        ks = self.fc1_ksplit if (R * self.fc_dim) % (64 * 64 * 8) == 0 and R % 64 == 0 else 1
        if ks > 1:
            ws = self._buf("fc1_ws", (4 * ks * R * self.fc_dim,), dtype=torch.uint8)
            self.h1 = dense.conv2d_forward_splitk(self.x, self.fc1.w_bf16, self.fc1.bias_f32, None, True, ks,
                                                  self._buf("h1", (R, 1, 1, self.fc_dim)), ws)
        else:
            self.h1 = self.fc1.forward(self.x, relu=True, out=self._buf("h1", (R, 1, 1, self.fc_dim)))
        self.o = self.fc_out.forward(self.h1, out=self._buf("o", (R, 1, 1, self.ld)))
        return self.o

    def backward(self):
        """Returns d(loss)/d(pooled) [R,7,7,C]."""
        self.fc_out.backward_weight(self.h1, self.go)
        d_h1 = self.fc_out.backward_data(self.go, self.h1.shape, relu_mask=self.h1, out=self._buf("dh1", self.h1.shape))
        self.fc1.backward_weight(self.x, d_h1)
        last = self.acts[-1]
        gn = self.norm == "gn"
        # without GN the last conv's ReLU is applied here; with GN the GN backward applies it
        g = self.fc1.backward_data(d_h1, self.x.shape, relu_mask=None if gn else last.view(self.x.shape),
                                   out=self._buf("dx", self.x.shape)).view(last.shape)
        for i in reversed(range(self.num_convs)):
            xin = self.acts[i]
            if gn:
                g = self.norms[i].backward(g, out=self._buf("dc%d" % i, xin.shape))
            self.convs[i].backward_weight(xin, g)
            g = self.convs[i].backward_data(g, xin.shape, relu_mask=xin if (i > 0 and not gn) else None,
                                            out=self._buf("g%d" % i, xin.shape))
        return g
