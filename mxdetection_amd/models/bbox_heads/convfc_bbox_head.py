"""Box heads. BBoxHead (2fc): flatten(7x7x256) -> FC 1024 + ReLU -> FC 1024 + ReLU -> fused (cls 81 | reg 324) FC.

Plugin slot: models/bbox_heads (/root/reference/README.md:29) with core/bbox + core/loss (README.md:17,19).
The FCs run on the same MFMA implicit-GEMM kernels as the convolutions (1x1 on [R,1,1,C] tensors); cls and reg
share one GEMM whose output is padded to 448 columns (a multiple of 64, so dgrad can reduce over it).

ConvFCBBoxHead (4conv1fc, the GN head recipe of Detectron / mmdetection): 4 x (conv3x3 256 -> 256 [-> GroupNorm] -> ReLU)
on [R,7,7,256] -> FC 12544 -> 1024 + ReLU -> the same fused output layer. It shares sampling, loss, the padded output
layer, checkpoint layout and the layers() ordering with BBoxHead.
"""
import torch

from ...core import bbox as B_
from ...core import loss as L_
from ..utils.layers import LayerChain, buf_cache


class BBoxHead:
    num_fcs, num_convs, conv_dim, norm, gn_groups = 2, 0, 256, "none", 32      # the 2fc head: no tower

    def __init__(self, in_features, arena, ws, device, gen, num_classes=81, fc_dim=1024, rois_per_image=512,
                 fg_fraction=0.25, fg_thresh=0.5, bg_hi=0.5, bg_lo=0.0, stds=(0.1, 0.1, 0.2, 0.2), sigma=1.0,
                 seed=99, reg_loss="smooth_l1", reg_loss_weight=1.0, ohem=False, ohem_nms=0.7, sampler="random",
                 sampler_bins=3, bl1_alpha=0.5, bl1_gamma=1.5, bl1_beta=1.0):
        """reg_loss: 'smooth_l1' on the encoded deltas (core.loss.rcnn_loss), 'iou' / 'giou' / 'diou' on the decoded
        box times reg_loss_weight (core.loss.rcnn_loss_iou; the head still predicts deltas, inference is the same), or
        'balanced_l1' on the encoded deltas -- Balanced L1(bl1_alpha, bl1_gamma, bl1_beta) times reg_loss_weight
        (core.loss.rcnn_loss_balanced).
        ohem / ohem_nms: online hard example mining (sample): the training RoIs are the rois_per_image highest-loss
        candidates of a read-only pass, deduplicated by NMS at ohem_nms (1 = none); fg_fraction is not used.
        sampler / sampler_bins: 'random' draws the background RoIs uniformly; 'iou_balanced' spreads their quota over
        sampler_bins fixed IoU bins (core.bbox.sample_rois(num_bins=)). Not with ohem, which keeps no quota."""
        L_.check_reg_loss(reg_loss, reg_loss_weight, box_head=True)
        B_.check_ohem(ohem_nms)
        B_.check_sampler(sampler, sampler_bins, ohem=bool(ohem))
        self.bl1 = L_.check_balanced_l1(bl1_alpha, bl1_gamma, bl1_beta)
        if reg_loss == "balanced_l1" and ohem:
            raise ValueError("reg_loss = 'balanced_l1' cannot be combined with ohem: the per-RoI score "
                             "(mxdet_ohem_roi_score) has no Balanced L1 term")
        self.sampler, self.sampler_bins = sampler, sampler_bins
        self.ohem, self.ohem_nms = bool(ohem), float(ohem_nms)
        self.ohem_extractor = None        # the detector's box RoI extractor (set by the detector that owns both)
        self.reg_loss, self.reg_loss_weight = reg_loss, float(reg_loss_weight)
        kw = dict(arena=arena, ws=ws, device=device, gen=gen)
        self.nc = num_classes
        self.reg_dim = 4 * num_classes
        self.ld = (num_classes + self.reg_dim + 63) // 64 * 64
        # registration = backward completion order: the FC trunk (fc_out first), then the tower
        fcs = [dict(name="bbox.fc%d" % (i + 1), cin=fc_dim if i else in_features, cout=fc_dim, k=1, split=i == 0)
               for i in range(self.num_fcs)]
        fcs.append(dict(name="bbox.fc_out", cin=fc_dim, cout=self.ld, k=1, init_std=0.01,
                        cout_real=num_classes + self.reg_dim, relu=False))
        self.fcs = LayerChain(fcs, **kw)
        C = self.conv_dim
        self.tower = LayerChain([dict(name="bbox.conv%d" % i, cin=C, cout=C, k=3) for i in range(self.num_convs)],
                                norm=self.norm, gn_groups=self.gn_groups, **kw)
        self.tower_in = (7, 7, C) if self.num_convs else (1, 1, in_features)
        self.convs, self.norms = self.tower.convs, self.tower.norms
        self.fc1, self.fc_out = self.fcs.convs[0], self.fcs.convs[-1]
        if self.num_fcs == 2:
            self.fc2 = self.fcs.convs[1]
        # checkpoint layout (CheckpointMixin._to_mx): fully connected layers are stored 2-D; fc1's input is the pooled
        # [7,7,C] block flattened (H, W, C) here and (C, H, W) in an MXNet FullyConnected after a Flatten of NCHW
        pooled = 7
        self.fc1.fc_in_hwc = (pooled, pooled, in_features // (pooled * pooled)) if in_features % (pooled * pooled) == 0 else ()
        for l in self.fcs.convs[1:]:
            l.fc_in_hwc = ()
        self.R, self.fg_fraction, self.fg_thresh, self.bg_hi, self.bg_lo = rois_per_image, fg_fraction, fg_thresh, bg_hi, bg_lo
        self.stds, self.sigma, self.seed, self.device = stds, sigma, seed, device
        self.in_features, self.fc_dim = in_features, fc_dim
        self.bufs, self._buf = buf_cache(device)

    def layers(self):
        return self.fcs.layers() + self.tower.layers()

    def norm_layers(self):
        return self.tower.norm_layers()

    def plan(self, N):
        R = N * self.R
        self.tower.plan((R,) + self.tower_in)
        self.fcs.plan((R, 1, 1, self.in_features))
        self.loss = torch.zeros((2,), dtype=torch.float32, device=self.device)
        self.loss_ws = L_.loss_workspace(R, self.device)

    def sample(self, rois, num_rois, gt_boxes, step, image_offset, step_dev=None, feats=None):
        """proposal-target: returns rois [N*R,5] and keeps labels / targets / weights (and the ground truth, which the
        IoU-family losses read on the device) for the loss. feats (the pyramid) is read by the OHEM route only."""
        if self.ohem:
            return self._sample_ohem(rois, num_rois, gt_boxes, step, image_offset, step_dev, feats)
        out = B_.sample_rois(rois, num_rois, gt_boxes, self.R, self.fg_fraction, self.fg_thresh, self.bg_hi, self.bg_lo,
                             self.nc, False, (0.0, 0.0, 0.0, 0.0), self.stds, self.seed, step, image_offset, step_dev,
                             num_bins=self.sampler_bins if self.sampler == "iou_balanced" else None)
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
        self.x = self.tower.forward(pooled.view((R,) + self.tower_in), self._buf).view(R, 1, 1, -1)
        self.o = self.fcs.forward(self.x, self._buf)
        self.acts, self.h1 = self.tower.acts, self.fcs.acts[1]
        return self.o

    def loss_and_grad(self, loss_scale=1.0):
        R = self.o.shape[0]
        o2 = self.o.view(R, self.ld)
        self.go = self._buf("go", (R, 1, 1, self.ld), zero=True)   # padding columns stay zero forever
        g2 = self.go.view(R, self.ld)
        if self.reg_loss == "smooth_l1":
            L_.rcnn_loss(o2, o2[:, self.nc:], self.labels, self.tgt, self.wgt, self.nc, self.reg_dim, self.ld, self.ld,
                         self.sigma, 1.0 / R, loss_scale, g2, g2[:, self.nc:], self.loss, self.loss_ws)
        elif self.reg_loss == "balanced_l1":
            L_.rcnn_loss_balanced(o2, o2[:, self.nc:], self.labels, self.tgt, self.wgt, self.nc, self.reg_dim, self.ld, self.ld,
                                  *self.bl1, self.reg_loss_weight, 1.0 / R, loss_scale, g2, g2[:, self.nc:], self.loss,
                                  self.loss_ws)
        else:
            L_.rcnn_loss_iou(o2, o2[:, self.nc:], self.labels, self.rois, self.matched, self.gt_boxes, self.nc, self.reg_dim,
                             self.ld, self.ld, self.reg_loss, self.stds, self.reg_loss_weight, 1.0 / R, loss_scale, g2,
                             g2[:, self.nc:], self.loss, self.loss_ws)
        return self.loss

    def backward(self):
        """Returns d(loss)/d(pooled), in the tower's input shape."""
        m = self.tower.out_mask           # fc1's data gradient applies the last conv's ReLU
        g = self.fcs.backward(self.go, self._buf, first_mask=None if m is None else m.view(self.x.shape))
        return self.tower.backward(g.view(self.tower.acts[-1].shape), self._buf)


class ConvFCBBoxHead(BBoxHead):
    """4conv1fc. norm = "gn": every conv is bias-free and followed by GroupNorm with the ReLU fused into the GN kernel, so
    the conv's data gradient takes no ReLU mask (the GN backward applies it)."""
    num_fcs = 1

    def __init__(self, in_features, arena, ws, device, gen, num_convs=4, conv_dim=256, norm="none", gn_groups=32, **kw):
        self.num_convs, self.conv_dim, self.norm, self.gn_groups = num_convs, conv_dim, norm, gn_groups
        assert in_features == 7 * 7 * conv_dim
        super().__init__(in_features, arena, ws, device, gen, **kw)
