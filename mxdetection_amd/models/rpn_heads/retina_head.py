"""RetinaNet dense head: two 4-conv towers (class / box) shared across P3..P7, 9 anchors per cell, sigmoid focal loss
and smooth-L1 box loss on every anchor (no sampling, no proposals). Targets: max-IoU assignment with fixed thresholds, or
ATSS (`assigner="atss"`, core.anchor.atss_assign; its published setting is one square anchor of scale 8 per cell).

Declared slot: the reference only names `rpn_heads` / `bbox_heads` for dense heads (/root/reference/README.md:28-29);
RetinaNet is BASELINE.json config 5. Class logits are padded 9*80 = 720 -> 768 channels and deltas 36 -> 64 so that
dgrad's reduction dim is a multiple of 64.
"""
import math

import torch

from ...core import anchor as A_
from ...core import loss as L_
from ...ops import dense
from ..utils.layers import ConvLayer, cached_buf


ASSIGNERS = ("max_iou", "atss")


def check_assigner(assigner, atss_topk=9):
    if assigner not in ASSIGNERS:
        raise ValueError("assigner = %r: expected one of %s" % (assigner, ", ".join(ASSIGNERS)))
    if isinstance(atss_topk, bool) or not isinstance(atss_topk, int) or not 1 <= atss_topk <= 16:
        raise ValueError("atss_topk = %r: expected an integer in 1..16" % (atss_topk,))


class RetinaHead:
    def __init__(self, channels, strides, arena, ws, device, gen, num_classes=80, num_convs=4, ratios=(0.5, 1.0, 2.0),
                 octave_scales=(1.0, 2.0 ** (1.0 / 3.0), 2.0 ** (2.0 / 3.0)), anchor_scale=4.0, fg_thresh=0.5,
                 bg_thresh=0.4, alpha=0.25, gamma=2.0, sigma=3.0, prior=0.01, reg_loss="smooth_l1", reg_loss_weight=1.0,
                 assigner="max_iou", atss_topk=9, cls_loss="focal", cls_loss_alpha=None, cls_loss_gamma=None, reg_max=0,
                 dfl_weight=0.25, ghm="none", ghm_cls_bins=30, ghm_cls_momentum=0.75, ghm_cls_weight=1.0, ghm_reg_bins=10,
                 ghm_reg_momentum=0.7, ghm_reg_mu=0.02, ghm_reg_weight=10.0):
        """assigner: 'max_iou' (fg_thresh / bg_thresh) or 'atss' (the atss_topk nearest anchors per level and GT).
        reg_loss: 'smooth_l1' on the encoded deltas (core.loss.retina_loss_level), or 'iou' / 'giou' / 'diou' on the
        decoded box times reg_loss_weight (core.loss.retina_loss_level_iou; stds 1, as the inference decode).
        cls_loss: 'focal' (alpha / gamma above, today's calls), or 'qfl' / 'vfl': the matched class column is trained
        against the IoU of the decoded box with its ground truth (core.loss.retina_loss_level_quality; needs an IoU-family
        reg_loss). cls_loss_alpha / cls_loss_gamma: None = the kind's published setting (QFL beta = 2 in gamma; VFL
        alpha = 0.75, gamma = 2); with 'focal' they replace alpha / gamma when given.
        reg_max / dfl_weight: reg_max > 0 makes the box branch a distribution head (GFL, Li et al. 2020): 4 * (reg_max + 1)
        logits per anchor, the box their integral decode, reg_loss on that box plus dfl_weight * DFL, any cls_loss
        (core.loss.retina_loss_level_dfl; needs an IoU-family reg_loss). reg_max = 0: the plain deltas, today's calls.
        ghm / ghm_*: 'cls', 'reg' or 'both' harmonize the class and / or the box term by the step's gradient-norm histogram
        (GHM, Li et al. 2019; core.loss.check_ghm: needs cls_loss 'focal' without alpha / gamma, reg_loss 'smooth_l1',
        reg_max 0). The histograms and their moving average (ghm_acc, zeroed by ghm_reset) live on the device, per rank, and
        are no parameters. 'none': today's calls."""
        if isinstance(num_convs, bool) or not isinstance(num_convs, int) or num_convs < 1:
            # without a tower layer backward() would mask cls_out's data gradient by P > 0 and never write dP
            raise ValueError("num_convs = %r: expected an integer >= 1" % (num_convs,))
        self.ghm = ghm
        self.ghm_cfg = L_.check_ghm(ghm, cls_loss, reg_loss, reg_max, cls_loss_alpha, cls_loss_gamma, ghm_cls_bins,
                                    ghm_cls_momentum, ghm_cls_weight, ghm_reg_bins, ghm_reg_momentum, ghm_reg_mu, ghm_reg_weight)
        L_.check_reg_loss(reg_loss, reg_loss_weight)
        check_assigner(assigner, atss_topk)
        L_.check_reg_max(reg_max, reg_loss, dfl_weight)
        self.reg_max, self.dfl_weight = int(reg_max), float(dfl_weight)
        self.ncomp = 3 if self.reg_max > 0 else 2             # loss components: class, box (, DFL)
        quality = L_.check_cls_loss(cls_loss, reg_loss, cls_loss_alpha, cls_loss_gamma)
        self.cls_loss = cls_loss
        if quality is not None:
            self.cls_alpha, self.cls_gamma = quality
        else:
            alpha = alpha if cls_loss_alpha is None else float(cls_loss_alpha)
            gamma = gamma if cls_loss_gamma is None else float(cls_loss_gamma)
        self.assigner, self.atss_topk = assigner, int(atss_topk)
        self.reg_loss, self.reg_loss_weight = reg_loss, float(reg_loss_weight)
        kw = dict(arena=arena, ws=ws, device=device, gen=gen)
        self.A, self.Cn = len(ratios) * len(octave_scales), num_classes
        self.ld_cls = (self.A * num_classes + 63) // 64 * 64
        self.reg_ch = self.A * 4 * (self.reg_max + 1)       # real box channels: 4 deltas, or 4 sides of reg_max + 1 bins
        self.ld_reg = (self.reg_ch + 63) // 64 * 64
        # registration = backward completion order
        self.cls_out = ConvLayer("retina.cls_out", channels, self.ld_cls, 3, init_std=0.01, cout_real=self.A * num_classes, **kw)
        self.box_out = ConvLayer("retina.box_out", channels, self.ld_reg, 3, init_std=0.01, cout_real=self.reg_ch, **kw)
        self.cls_convs = [ConvLayer("retina.cls%d" % i, channels, channels, 3, init_std=0.01, **kw)
                          for i in reversed(range(num_convs))][::-1]
        self.box_convs = [ConvLayer("retina.box%d" % i, channels, channels, 3, init_std=0.01, **kw)
                          for i in reversed(range(num_convs))][::-1]
        self.prior_bias = -math.log((1.0 - prior) / prior)
        self.strides = list(strides)
        scales = [anchor_scale * o for o in octave_scales]
        self.base = [torch.from_numpy(A_.generate_base_anchors(s, ratios, scales)).to(device) for s in strides]
        self.fg_thresh, self.bg_thresh, self.alpha, self.gamma, self.sigma = fg_thresh, bg_thresh, alpha, gamma, sigma
        self.device, self.C = device, channels
        self.bufs = {}

    def layers(self):
        return [self.cls_out, self.box_out] + list(reversed(self.cls_convs)) + list(reversed(self.box_convs))

    def post_materialize(self):
        b = self.cls_out.bias_f32
        b.zero_()
        b[: self.A * self.Cn] = self.prior_bias      # focal-loss prior: every anchor starts at p = 0.01

    def _buf(self, key, shape, dtype=torch.bfloat16, zero=False):
        return cached_buf(self.bufs, key, shape, dtype, self.device, zero)

    def plan(self, p_shapes, g_max):
        for s in p_shapes:
            for c in self.cls_convs + self.box_convs + [self.cls_out, self.box_out]:
                c.plan(s)
        self.level_shapes = [(s[1], s[2]) for s in p_shapes]
        N = p_shapes[0][0]
        self.anchors = torch.cat([A_.generate_anchors(self.base[l], H, W, self.strides[l])
                                  for l, (H, W) in enumerate(self.level_shapes)])
        self.level_offsets = [0]
        for (H, W) in self.level_shapes:
            self.level_offsets.append(self.level_offsets[-1] + H * W * self.A)
        At = self.anchors.shape[0]
        dev = self.device
        self.at_ws = (A_.AtssWorkspace if self.assigner == "atss" else A_.AnchorTargetWorkspace)(N, At, g_max, dev)
        self.at_out = (torch.empty((N, At), dtype=torch.int32, device=dev), torch.empty((N, At), dtype=torch.int32, device=dev),
                       torch.empty((N, At, 4), dtype=torch.float32, device=dev), torch.empty((N, At), dtype=torch.float32, device=dev))
        self.cls_labels = torch.empty((N, At), dtype=torch.int32, device=dev)
        self.num_fg = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.nparts = [L_.retina_loss_num_partials(N, H, W, self.A) for (H, W) in self.level_shapes]
        self.partial = torch.zeros((self.ncomp * sum(self.nparts),), dtype=torch.float32, device=dev)
        self.loss = torch.zeros((self.ncomp,), dtype=torch.float32, device=dev)
        if self.ghm != "none":        # one row of counts per workgroup of the step; the moving average survives a re-plan
            nb = self.ghm_cfg["cls_bins"] + self.ghm_cfg["reg_bins"]
            self.ghm_counts = torch.zeros((sum(self.nparts), nb), dtype=torch.int32, device=dev)
            self.ghm_cnt = torch.zeros((nb,), dtype=torch.int32, device=dev)
            self.ghm_coef = torch.zeros((nb,), dtype=torch.float32, device=dev)
            if getattr(self, "ghm_acc", None) is None:
                self.ghm_acc = torch.zeros((nb,), dtype=torch.float32, device=dev)

    def ghm_reset(self):
        """Zero the moving average of the gradient-norm histograms (a memset; call it outside any captured graph)."""
        if getattr(self, "ghm_acc", None) is not None:
            self.ghm_acc.zero_()

    def ghm_state(self):
        """A copy of the moving average, or None while there is none (ghm 'none', or not planned yet: a zero state)."""
        acc = getattr(self, "ghm_acc", None)
        return None if acc is None else acc.clone()

    def ghm_set_state(self, state):
        """Put back what ghm_state returned (None: zero). Outside any captured graph."""
        if getattr(self, "ghm_acc", None) is not None:
            if state is None:
                self.ghm_acc.zero_()
            else:
                self.ghm_acc.copy_(state)

    def _ghm_loss_and_grad(self, targets, loss_scale):
        """Histogram passes over all levels, the weights kernel, then the loss passes: one histogram per term and step."""
        g = self.ghm_cfg
        off = 0
        for l in range(len(self.co)):
            L_.ghm_hist_level(self.co[l], self.bo[l], self.A, self.Cn, self.cls_labels, targets, self.level_offsets[l], self.ghm,
                              g["cls_bins"], g["reg_bins"], g["reg_mu"], self.ghm_counts[off:])
            off += self.nparts[l]
        L_.ghm_weights(self.ghm_counts, off, g["cls_bins"], g["reg_bins"], g["cls_momentum"], g["reg_momentum"], self.ghm_acc,
                       self.ghm_cnt, self.ghm_coef)
        off = 0
        for l in range(len(self.co)):
            gc = self._buf("gco%d" % l, self.co[l].shape, zero=True)     # padding channels stay zero
            gb = self._buf("gbo%d" % l, self.bo[l].shape, zero=True)
            L_.retina_loss_level_ghm(self.co[l], self.bo[l], self.A, self.Cn, self.cls_labels, targets, self.level_offsets[l],
                                     self.ghm, self.alpha, self.gamma, self.sigma, self.ghm_coef, g["cls_bins"], g["reg_bins"],
                                     g["cls_weight"], g["reg_mu"], g["reg_weight"], self.num_fg, loss_scale, gc, gb,
                                     self.partial[2 * off:])
            off += self.nparts[l]
            self.gco.append(gc)
            self.gbo.append(gb)
        L_.loss_finalize(self.partial, off, self.ncomp, self.loss)
        return self.loss

    def forward(self, P):
        """Layer i of BOTH towers on ALL levels is one grouped launch (10 independent convolutions): 5 launches for the
        whole head instead of 50; the small levels ride in the shadow of P3."""
        self.P = P
        L, n = len(P), len(self.cls_convs)
        self.cact = [[p] for p in P]
        self.bact = [[p] for p in P]
        for i in range(n):
            calls = []
            for l, p in enumerate(P):
                co = self._buf("c%d_%d" % (l, i), p.shape)
                bo = self._buf("b%d_%d" % (l, i), p.shape)
                calls.append(self.cls_convs[i].fwd_call(self.cact[l][-1], relu=True, out=co))
                calls.append(self.box_convs[i].fwd_call(self.bact[l][-1], relu=True, out=bo))
                self.cact[l].append(co)
                self.bact[l].append(bo)
            dense.conv2d_group("fwd", calls, self.device)
        self.co = [self._buf("co%d" % l, p.shape[:3] + (self.ld_cls,)) for l, p in enumerate(P)]
        self.bo = [self._buf("bo%d" % l, p.shape[:3] + (self.ld_reg,)) for l, p in enumerate(P)]
        dense.conv2d_group("fwd", [self.cls_out.fwd_call(self.cact[l][-1], out=self.co[l]) for l in range(L)] +
                           [self.box_out.fwd_call(self.bact[l][-1], out=self.bo[l]) for l in range(L)], self.device)
        return self.co, self.bo

    def loss_and_grad(self, gt_boxes, im_info, loss_scale=1.0):
        if self.assigner == "atss":
            labels, matched, targets, _ = A_.atss_assign(self.anchors, self.level_offsets, gt_boxes, self.atss_topk,
                                                         self.at_ws, self.at_out)
        else:
            labels, matched, targets, _ = A_.assign_anchor(self.anchors, gt_boxes, im_info, self.fg_thresh, self.bg_thresh,
                                                           1.0e6, 0, 0.5, 0, 0, 0, self.at_ws, self.at_out)
        L_.anchor_class_labels(labels, matched, gt_boxes, self.cls_labels, self.num_fg)
        self.matched = matched
        self.gco, self.gbo = [], []
        if self.ghm != "none":
            return self._ghm_loss_and_grad(targets, loss_scale)
        off = 0
        for l in range(len(self.co)):
            gc = self._buf("gco%d" % l, self.co[l].shape, zero=True)     # padding channels stay zero
            gb = self._buf("gbo%d" % l, self.bo[l].shape, zero=True)
            if self.reg_max > 0:
                alpha, gamma = (self.alpha, self.gamma) if self.cls_loss == "focal" else (self.cls_alpha, self.cls_gamma)
                L_.retina_loss_level_dfl(self.co[l], self.bo[l], self.A, self.Cn, self.cls_labels, self.anchors, matched, gt_boxes,
                                         self.level_offsets[l], self.cls_loss, alpha, gamma, self.reg_loss, self.reg_max,
                                         float(self.strides[l]), self.reg_loss_weight, self.dfl_weight, self.num_fg, loss_scale,
                                         gc, gb, self.partial[3 * off:])
            elif self.reg_loss == "smooth_l1":
                L_.retina_loss_level(self.co[l], self.bo[l], self.A, self.Cn, self.cls_labels, targets, self.level_offsets[l],
                                     self.alpha, self.gamma, self.sigma, self.num_fg, loss_scale, gc, gb, self.partial[2 * off:])
            elif self.cls_loss != "focal":
                L_.retina_loss_level_quality(self.co[l], self.bo[l], self.A, self.Cn, self.cls_labels, self.anchors, matched,
                                             gt_boxes, self.level_offsets[l], self.cls_loss, self.cls_alpha, self.cls_gamma,
                                             self.reg_loss, (1.0, 1.0, 1.0, 1.0), self.reg_loss_weight, self.num_fg, loss_scale,
                                             gc, gb, self.partial[2 * off:])
            else:
                L_.retina_loss_level_iou(self.co[l], self.bo[l], self.A, self.Cn, self.cls_labels, self.anchors, matched, gt_boxes,
                                         self.level_offsets[l], self.alpha, self.gamma, self.reg_loss, (1.0, 1.0, 1.0, 1.0),
                                         self.reg_loss_weight, self.num_fg, loss_scale, gc, gb, self.partial[2 * off:])
            off += self.nparts[l]
            self.gco.append(gc)
            self.gbo.append(gb)
        L_.loss_finalize(self.partial, off, self.ncomp, self.loss)
        return self.loss

    def backward(self, dP):
        """Writes d(loss)/d(P_l) into dP[l] (overwrites). Same grouping as forward; weight gradients of a filter are
        summed over the levels (by the grouped plan when the workspace groups, by accumulate flags otherwise)."""
        n, L = len(self.cls_convs), len(self.co)
        grouped = self.cls_out.ws.grouping
        dbuf = lambda key, l, i, shape: self._buf("d%s%d_%d" % (key, l, i), shape)   # noqa: E731
        dc = [None] * L
        db = [None] * L
        calls = []
        for l in range(L):
            xc, xb = self.cact[l][-1], self.bact[l][-1]
            self.cls_out.backward_weight(xc, self.gco[l], accumulate=(l > 0) and not grouped)
            self.box_out.backward_weight(xb, self.gbo[l], accumulate=(l > 0) and not grouped)
            dc[l], db[l] = dbuf("c", l, n, xc.shape), dbuf("b", l, n, xb.shape)
            calls.append(self.cls_out.dgrad_call(self.gco[l], xc.shape, relu_mask=xc, out=dc[l]))
            calls.append(self.box_out.dgrad_call(self.gbo[l], xb.shape, relu_mask=xb, out=db[l]))
        dense.conv2d_group("dgrad", calls, self.device)
        for i in reversed(range(n)):
            calls_c, calls_b = [], []
            for l in range(L):
                xc, xb = self.cact[l][i], self.bact[l][i]
                self.cls_convs[i].backward_weight(xc, dc[l], accumulate=(l > 0) and not grouped)
                self.box_convs[i].backward_weight(xb, db[l], accumulate=(l > 0) and not grouped)
                if i > 0:
                    nc, nb = dbuf("c", l, i, xc.shape), dbuf("b", l, i, xb.shape)
                    calls_c.append(self.cls_convs[i].dgrad_call(dc[l], xc.shape, relu_mask=xc, out=nc))
                    calls_b.append(self.box_convs[i].dgrad_call(db[l], xb.shape, relu_mask=xb, out=nb))
                    dc[l], db[l] = nc, nb
                else:   # into the pyramid gradient: the class tower writes, then the box tower adds
                    calls_c.append(self.cls_convs[i].dgrad_call(dc[l], xc.shape, out=dP[l]))
                    calls_b.append(self.box_convs[i].dgrad_call(db[l], xb.shape, accumulate=True, out=dP[l]))
            if i > 0:
                dense.conv2d_group("dgrad", calls_c + calls_b, self.device)
            else:
                dense.conv2d_group("dgrad", calls_c, self.device)
                dense.conv2d_group("dgrad", calls_b, self.device)
