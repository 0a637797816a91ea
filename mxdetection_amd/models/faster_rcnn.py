"""Faster R-CNN ResNet-FPN: one training step = forward, targets, losses, explicit backward, gradient
all-reduce (RCCL, overlapped with backward), SGD-momentum update. Every arithmetic step is a hand-written
HIP kernel reached through the C-ABI; torch supplies device memory, streams and torch.distributed only.

Assembles the plugin parts the reference declares (/root/reference/README.md:27-32). The training loop
itself is not declared anywhere in the reference tree; this is the build's own.
"""
import torch

from ..core import mask as M_
from ..core.bbox import check_ohem, check_sampler
from ..core.loss import check_balanced_l1, check_reg_loss
from .backbones import ResNet
from .backbones.resnet import check_gcb
from .bbox_heads import BBoxHead, ConvFCBBoxHead
from .mask_heads import FCNMaskHead, KeypointHead, MaskIoUHead
from .necks import BFP, FPN, check_neck, check_upsample
from .roi_extractors import DeformRoIExtractor, FPNRoIExtractor
from .rpn_heads import RPNHead
from .utils.detector import DetectorBase
from .utils.layers import Workspace


def check_head_options(bbox_head, head_norm, gn_groups, with_mask):
    """The head options of FasterRCNN, checked before anything is allocated."""
    if bbox_head not in ("2fc", "4conv1fc"):
        raise ValueError("bbox_head must be '2fc' or '4conv1fc' (got %r)" % (bbox_head,))
    if head_norm not in ("none", "gn"):
        raise ValueError("head_norm must be 'none' or 'gn' (got %r)" % (head_norm,))
    if head_norm == "gn":
        if bbox_head == "2fc" and not with_mask:
            raise ValueError("head_norm='gn' with nothing to normalise: the 2fc box head has no convolutions and there "
                             "is no mask head")
        g = gn_groups
        if not isinstance(g, int) or isinstance(g, bool) or g <= 0 or 256 % g or (256 // g) % 8:
            raise ValueError("gn_groups = %r does not divide 256 channels into groups of a multiple of 8" % (g,))


def check_loss_weight(name, w):
    """A branch's loss weight: a positive finite number, not a bool."""
    if not (isinstance(w, (int, float)) and not isinstance(w, bool) and 0.0 < float(w) < float("inf")):
        raise ValueError("%s must be a positive finite number (got %r)" % (name, w))


class FasterRCNN(DetectorBase):
    def __init__(self, device="cuda", depth=50, num_classes=81, seed=7, rpn_seed=99, rois_per_image=512,
                 pre_nms_top_n=2000, post_nms_top_n=2000, with_mask=False, dcn_stages=(), dcn_modulated=True,
                 dcn_groups=1, roi_pool="roi_align", dpool_trans_std=0.1, dpool_sample_per_part=4, dpool_offset_fcs=3,
                 bbox_head="2fc", head_norm="none", gn_groups=32, reg_loss="smooth_l1", reg_loss_weight=1.0,
                 mask_iou=False, mask_iou_weight=1.0, ohem=False, ohem_nms=0.7, with_keypoints=False, num_keypoints=17,
                 keypoint_weight=1.0, neck="fpn", bfp_refine="conv", sampler="random", sampler_bins=3, bl1_alpha=0.5,
                 bl1_gamma=1.5, bl1_beta=1.0, bfp_nl_reduction=2, bfp_nl_use_scale=False, fpn_upsample="nearest", carafe_k=5,
                 carafe_compress=64, carafe_enc_kernel=3, gcb_stages=(), gcb_reduction=16):
        """dcn_stages / dcn_modulated / dcn_groups: deformable conv2 in those backbone stages (backbones.ResNet).
        gcb_stages / gcb_reduction: GCNet (Cao et al. 2019) -- a global context block (attention pooling, a bottleneck
        transform C -> C / gcb_reduction -> C with LayerNorm, broadcast add) in every bottleneck of those backbone stages
        (trainable ones among 3, 4, 5), after conv3 and in front of the shortcut add, on fused kernels (backbones.ResNet,
        utils.layers.ContextBlock); 16 and 4 are the published reductions. The blocks draw from a generator of their own and
        start as the identity (their last layer is zero), so every other parameter starts exactly as in the model without
        them; composes with dcn_stages and every other option.
        roi_pool: the box branch's RoI pooling -- 'roi_align', or deformable RoI pooling with its offset head, 'dpool'
        (v1) / 'mdpool' (v2, modulated) (roi_extractors.DeformRoIExtractor, options dpool_*). The mask branch keeps its
        14x14 RoIAlign.
        bbox_head: '2fc' (two FCs) or '4conv1fc' (four 3x3 convs + one FC). head_norm: 'none' or 'gn' -- GroupNorm with
        gn_groups groups after every conv of the 4conv1fc box head and of the mask head (bbox_heads.ConvFCBBoxHead,
        mask_heads.FCNMaskHead).
        reg_loss / reg_loss_weight: the box head's regression loss -- 'smooth_l1' on the encoded deltas, or 'iou' / 'giou' /
        'diou' on the decoded box times reg_loss_weight (bbox_heads.BBoxHead). The RPN keeps smooth-L1.
        mask_iou / mask_iou_weight: Mask Scoring R-CNN -- a MaskIoU head on the mask branch (mask_heads.MaskIoUHead) whose
        L2 loss, times mask_iou_weight, is the step's fourth loss; predict(with_masks=True) then also returns the mask
        scores. Needs with_mask. The head draws its initial weights from a generator of its own, so every other parameter
        starts exactly as in the model without it.
        ohem / ohem_nms: online hard example mining (Shrivastava et al. 2016) -- the box head trains on the rois_per_image
        highest-loss RoIs of a read-only pass over every candidate of the image (proposals and ground truth), deduplicated
        by NMS at IoU ohem_nms in (0, 1] (1 = none), with no fg:bg quota (bbox_heads.BBoxHead.sample). It adds no parameter.
        with_keypoints / num_keypoints / keypoint_weight: Keypoint R-CNN -- a keypoint head (mask_heads.KeypointHead) on a
        14x14 RoIAlign of its own over the foreground rois, with or without the mask branch; its heatmap loss, times
        keypoint_weight, is the LAST of the step's losses, training takes gt_keypoints [N,G,num_keypoints,3], and
        predict(with_keypoints=True) returns the decoded keypoints. The head draws its initial weights from a generator of
        its own, so every other parameter starts exactly as in the model without it.
        Libra R-CNN (Pang et al. 2019), three independent parts: neck = 'bfp' / bfp_refine -- the Balanced Feature Pyramid
        behind the FPN (necks.BFP; refine 'conv' = one 3x3 convolution, 'embedded_gaussian' = the paper's non-local block on
        the attention entries with Ci = 256 / bfp_nl_reduction (2 or 4) and logits scaled by 1 / sqrt(Ci) if
        bfp_nl_use_scale, 'none'); every head, the RPN and predict then read the balanced levels, and the refine layers draw
        from a generator of their own. sampler = 'iou_balanced' /
        sampler_bins -- the box head's background RoIs keep a quota per IoU bin (not with ohem). reg_loss = 'balanced_l1' /
        bl1_alpha, bl1_gamma, bl1_beta -- Balanced L1 on the encoded deltas, times reg_loss_weight (not with ohem).
        fpn_upsample = 'carafe' / carafe_k, carafe_compress, carafe_enc_kernel: CARAFE (Wang et al. 2019) in place of the
        FPN's nearest-neighbour top-down upsample (necks.FPN): per merge a 1x1 conv 256 -> carafe_compress (a multiple of 64)
        and a carafe_enc_kernel (1 or 3) conv onto the 4 k^2 logits of a carafe_k x carafe_k (3 or 5) reassembly kernel. The
        new layers draw from a generator of their own; composes with every other option, neck = 'bfp' included."""
        check_upsample(fpn_upsample, carafe_k, carafe_compress, carafe_enc_kernel)
        check_gcb(gcb_stages, gcb_reduction)
        check_neck(neck, bfp_refine, bfp_nl_reduction, bfp_nl_use_scale)
        check_head_options(bbox_head, head_norm, gn_groups, with_mask)
        if mask_iou and not with_mask:
            raise ValueError("mask_iou needs the mask branch (with_mask=True): the MaskIoU head scores the mask head's output")
        if mask_iou:
            check_loss_weight("mask_iou_weight", mask_iou_weight)
        if not isinstance(with_keypoints, (bool, int)):
            raise ValueError("with_keypoints must be a bool (got %r)" % (with_keypoints,))
        if with_keypoints:
            if not isinstance(num_keypoints, int) or isinstance(num_keypoints, bool) or not 1 <= num_keypoints <= 32:
                raise ValueError("num_keypoints must be an integer in [1, 32] (got %r)" % (num_keypoints,))
            check_loss_weight("keypoint_weight", keypoint_weight)
        check_reg_loss(reg_loss, reg_loss_weight, box_head=True)
        if not isinstance(ohem, (bool, int)):
            raise ValueError("ohem must be a bool (got %r)" % (ohem,))
        check_ohem(ohem_nms)
        check_sampler(sampler, sampler_bins, ohem=bool(ohem))
        check_balanced_l1(bl1_alpha, bl1_gamma, bl1_beta)
        if reg_loss == "balanced_l1" and ohem:
            raise ValueError("reg_loss = 'balanced_l1' cannot be combined with ohem: the per-RoI score "
                             "(mxdet_ohem_roi_score) has no Balanced L1 term")
        if roi_pool not in ("roi_align", "dpool", "mdpool"):
            raise ValueError("roi_pool must be 'roi_align', 'dpool' or 'mdpool' (got %r)" % (roi_pool,))
        self.roi_pool = roi_pool
        gen = torch.Generator().manual_seed(seed)
        self._init_base(device)
        self.strides = [4, 8, 16, 32, 64]
        # registration order == backward completion order (buckets become final early)
        self.with_mask = with_mask
        # RoIAlign backward: deterministic gather form (no atomics, no fp32 accumulators, writes the bf16 maps directly);
        # False selects the fp32-atomic scatter form (310 us + zero-fill + finalize at the benchmark shape)
        self.roi_bwd_gather = True
        self.mask_head = self.mask_iou_head = self.keypoint_head = None
        self.with_keypoints = bool(with_keypoints)
        if self.with_keypoints:   # Keypoint R-CNN: the keypoint branch's backward runs before the mask branch's
            self.keypoint_head = KeypointHead(256, self.arena, self.ws, device, torch.Generator().manual_seed(seed + 104729),
                                              num_keypoints=num_keypoints, rois_per_image=max(1, rois_per_image // 4),
                                              weight=keypoint_weight)
            self.keypoint_roi_extractor = FPNRoIExtractor([4, 8, 16, 32], pooled=(14, 14), device=device)
        if with_mask:   # Mask R-CNN (BASELINE.json config 4): the mask branch's backward runs first
            if mask_iou:    # ... and within it the MaskIoU head's, which sits behind the mask head's output
                self.mask_iou_head = MaskIoUHead(256, self.arena, self.ws, device, torch.Generator().manual_seed(seed + 7919),
                                                 num_classes=num_classes, rois_per_image=max(1, rois_per_image // 4),
                                                 weight=mask_iou_weight)
            self.mask_head = FCNMaskHead(256, self.arena, self.ws, device, gen, num_classes=num_classes,
                                         rois_per_image=max(1, rois_per_image // 4), norm=head_norm, gn_groups=gn_groups)
            self.mask_roi_extractor = FPNRoIExtractor([4, 8, 16, 32], pooled=(14, 14), device=device)
        self.mark_mask = self.arena.size
        libra = dict(sampler=sampler, sampler_bins=sampler_bins, bl1_alpha=bl1_alpha, bl1_gamma=bl1_gamma, bl1_beta=bl1_beta)
        if bbox_head == "4conv1fc":
            self.bbox_head = ConvFCBBoxHead(7 * 7 * 256, self.arena, self.ws, device, gen, norm=head_norm, gn_groups=gn_groups,
                                            num_classes=num_classes, rois_per_image=rois_per_image, seed=rpn_seed,
                                            reg_loss=reg_loss, reg_loss_weight=reg_loss_weight, ohem=ohem, ohem_nms=ohem_nms,
                                            **libra)
        else:
            self.bbox_head = BBoxHead(7 * 7 * 256, self.arena, self.ws, device, gen, num_classes=num_classes,
                                      rois_per_image=rois_per_image, seed=rpn_seed, reg_loss=reg_loss,
                                      reg_loss_weight=reg_loss_weight, ohem=ohem, ohem_nms=ohem_nms, **libra)
        self.dpool = None
        if roi_pool != "roi_align":
            # the offset head belongs to the head bucket: its backward runs in the slot of the RoI extractor's
            self.dpool = DeformRoIExtractor(self.strides[:4], 256, self.arena, self.ws, device,
                                            modulated=(roi_pool == "mdpool"), trans_std=dpool_trans_std,
                                            sample_per_part=dpool_sample_per_part, offset_fcs=dpool_offset_fcs)
        self.mark_head = self.arena.size
        # own wgrad scratch: the RPN training branch runs on its own stream (enable_branch_stream) and must not
        # share the split-K slabs with the weight-gradient stream of the rest of the model
        self.ws_rpn = Workspace(device)
        self.rpn_head = RPNHead(256, self.strides, self.arena, self.ws_rpn, device, gen, pre_nms_top_n=pre_nms_top_n,
                                post_nms_top_n=post_nms_top_n, seed=rpn_seed)
        self.mark_rpn = self.arena.size
        # Balanced Feature Pyramid: its refine layers' backward completes before the FPN's, so they are registered first
        # among the neck's layers (inside the FPN bucket)
        self.bfp = BFP(256, self.arena, self.ws, device, torch.Generator().manual_seed(seed + 15485863),
                       refine=bfp_refine, nl_reduction=bfp_nl_reduction,
                       nl_use_scale=bool(bfp_nl_use_scale)) if neck == "bfp" else None
        self.neck = FPN([256, 512, 1024, 2048], 256, self.arena, self.ws, device, gen, upsample=fpn_upsample,
                        carafe_k=carafe_k, carafe_compress=carafe_compress, carafe_enc_kernel=carafe_enc_kernel,
                        carafe_gen=torch.Generator().manual_seed(seed + 32452843))
        self.mark_fpn = self.arena.size
        self.backbone = ResNet(depth, self.arena, self.ws, device, gen, dcn_stages=dcn_stages,
                               dcn_modulated=dcn_modulated, dcn_groups=dcn_groups, gcb_stages=gcb_stages,
                               gcb_reduction=gcb_reduction, gcb_gen=torch.Generator().manual_seed(seed + 49979687))
        self.roi_extractor = self.dpool if self.dpool is not None else FPNRoIExtractor(self.strides[:4], device=device)
        self.bbox_head.ohem_extractor = self.roi_extractor
        layers = self.bbox_head.layers() + (self.dpool.layers() if self.dpool is not None else [])
        layers += self.rpn_head.layers() + (self.bfp.layers() if self.bfp is not None else [])
        layers += self.neck.layers() + self.backbone.layers()
        norms = self.bbox_head.norm_layers()
        if with_mask:
            layers = self.mask_head.layers() + layers
            if self.mask_iou_head is not None:
                layers = self.mask_iou_head.layers() + layers
            norms = self.mask_head.norm_layers() + norms
        if self.keypoint_head is not None:
            layers = self.keypoint_head.layers() + layers
        self._finalize_params(layers, norm_layers=norms + self.backbone.norm_layers())

    def plan(self, N, H, W, g_max):
        key = (N, H, W, g_max)
        if self.planned == key:
            return
        self._guard_replan(key)
        dev = self.device
        c_shapes = self.backbone.plan((N, 3, H, W))
        self.neck.plan(c_shapes)
        p_shapes = [(s[0], s[1], s[2], 256) for s in c_shapes]
        p_shapes.append((N, (p_shapes[-1][1] + 1) // 2, (p_shapes[-1][2] + 1) // 2, 256))
        if self.bfp is not None:
            self.bfp.plan(p_shapes)
        self.rpn_head.plan(p_shapes, g_max)
        self.bbox_head.plan(N)
        if self.dpool is not None:
            self.dpool.plan(N * self.bbox_head.R)
        if self.with_mask:
            self.mask_head.plan(N)
            if self.mask_iou_head is not None:
                self.mask_iou_head.plan(N, g_max)
        if self.keypoint_head is not None:
            self.keypoint_head.plan(N)
        self.ws.get()
        self.ws_rpn.get()
        # one flat bf16 buffer (levels are views, finest first): the RoI extractor finalizes P2..P5 with one launch
        sizes = [s[0] * s[1] * s[2] * s[3] for s in p_shapes]
        self.dP_flat = torch.empty((sum(sizes),), dtype=torch.bfloat16, device=dev)
        self.dP, off = [], 0
        for s, n in zip(p_shapes, sizes):
            self.dP.append(self.dP_flat[off:off + n].view(s))
            off += n
        self.dC = [None] + [torch.empty(s, dtype=torch.bfloat16, device=dev) for s in c_shapes[1:]]
        self.planned = key

    def forward_backward(self, image, gt_boxes, im_info, step=0, image_offset=0, step_dev=None, gt_masks=None,
                         gt_keypoints=None):
        """image NCHW [N,3,H,W]; gt_boxes [N,G,5] f32 (class < 0 padding); im_info [N,3] f32; gt_masks [N,G,H,W] u8 (mask
        branch); gt_keypoints [N,G,K,3] f32 = (x, y, v) (keypoint branch)."""
        N, _, H, W = image.shape
        self.plan(N, H, W, gt_boxes.shape[1])
        early = self.branch is not None
        if early:
            # anchor assignment needs the ground truth only: on the branch stream it runs underneath the backbone forward,
            # and the RPN branch proper starts with its losses and heavy convolutions instead of ~100 us of small kernels
            # (+0.9 % on the step)
            with self._branch_ctx():
                self.rpn_head.assign_targets(gt_boxes, im_info, step, image_offset, step_dev)
        C = self.backbone.forward(image)
        P = self._neck_forward(C)
        self.rpn_head.forward(P)
        # The RPN training branch (anchor targets, RPN losses, RPN head backward: MFMA-heavy) depends only on the
        # head outputs; the proposal -> RoI -> box-head chain (long, low-occupancy selection/NMS kernels) does not
        # depend on it. They run on two streams and meet at dP.
        # The RPN head's weight gradients leave the branch and run on the side stream, with the head bucket, underneath
        # the RoIAlign gather (+0.8 % on the step).
        defer_rpn = (self.roi_bwd_gather and self.ws.side is not None and self.ws_rpn.grouping and self.ws.grouping
                     and self._bucket_here(0))
        with self._branch_ctx():
            rpn_loss = self.rpn_head.loss_and_grad(gt_boxes, im_info, step, image_offset, step_dev=step_dev, assigned=early)
            self.rpn_head.backward(self.dP, [False] * 5, flush=not defer_rpn)
        rois, _, _, num_rois = self.rpn_head.get_proposals(im_info)
        rois_s = self.bbox_head.sample(rois, num_rois, gt_boxes, step, image_offset, step_dev, feats=P)
        pooled = self.roi_extractor.forward(P, rois_s, prepare_gather=self.roi_bwd_gather)
        self.bbox_head.forward(pooled)
        rcnn_loss = self.bbox_head.loss_and_grad()
        mask_loss = maskiou_loss = None
        iou_head = self.mask_iou_head
        if self.with_mask:
            mrois = self.mask_head.select_rois(self.bbox_head)
            self.mask_head.targets(gt_masks)
            mpooled = self.mask_roi_extractor.forward(P, mrois, prepare_gather=self.roi_bwd_gather)
            self.mask_head.forward(mpooled)
            mask_loss = self.mask_head.loss_and_grad()
            if iou_head is not None:
                iou_head.targets(self.mask_head, gt_boxes, gt_masks)
                iou_head.forward(mpooled, self.mask_head.o, self.mask_head.cls)
                maskiou_loss = iou_head.loss_and_grad()
        kpt_head, kpt_loss = self.keypoint_head, None
        if kpt_head is not None:
            if gt_keypoints is None:
                raise ValueError("a model with the keypoint head trains on gt_keypoints [N,G,%d,3]" % kpt_head.K)
            krois = kpt_head.select_rois(self.bbox_head)
            kpt_head.targets(gt_keypoints)
            kpooled = self.keypoint_roi_extractor.forward(P, krois, prepare_gather=self.roi_bwd_gather)
            kpt_head.forward(kpooled)
            kpt_loss = kpt_head.loss_and_grad()
        # ---- backward ----
        d_kpooled = kpt_head.backward() if kpt_head is not None else None
        if self.with_mask:
            # the MaskIoU head's backward completes first; its input gradient joins the mask head's at the RoI features
            # (the mask channel of its input is a constant: nothing flows into the mask logits)
            d_iou_in = iou_head.backward() if iou_head is not None else None
            d_mpooled = self.mask_head.backward()
            if iou_head is not None:
                M_.maskiou_input_bwd(d_iou_in, d_mpooled)
        d_pooled = self.bbox_head.backward()
        if self.roi_bwd_gather:
            self._join_branch()                                       # dP[l] holds the RPN part
            # (defer_rpn: the RPN head's weight gradients -- MFMA-bound -- go to the side stream with this bucket instead of
            # lengthening the branch.) The gather is issued FIRST and the head bucket's weight gradients, update and filter
            # transposes behind it (round 3: with the three-tap weight-gradient kernel the gather beside a 2,000-workgroup
            # MFMA grid took 235-310 us instead of its 70-90 us alone; alone first, then the bucket beside the P2 data
            # gradients, is +0.3 % on the step). Deformable RoI pooling needs this order: its offset head's weight gradients
            # belong to the head bucket, so the bucket closes behind the extractor's backward.
            lo = 0
            self.roi_extractor.backward_gather(d_pooled.view(pooled.shape), self.dP[:4], accumulate=True)
            if self.with_mask:
                self.mask_roi_extractor.backward_gather(d_mpooled, self.dP[:4], accumulate=True)
            if kpt_head is not None:
                self.keypoint_roi_extractor.backward_gather(d_kpooled, self.dP[:4], accumulate=True)
            if self._bucket_here(0):
                self._reduce(0, self.mark_rpn, pre=self.ws_rpn if defer_rpn else None)
                lo = self.mark_rpn
        else:
            assert self.dpool is None, "deformable RoI pooling has the gather-form backward only (roi_bwd_gather)"
            acc = self.roi_extractor.backward(d_pooled.view(pooled.shape), self.dP[:4], finalize=False)
            if self.with_mask:
                self.mask_roi_extractor.backward(d_mpooled, self.dP[:4], shared_acc=acc, zero=False, finalize=False)
            if kpt_head is not None:
                self.keypoint_roi_extractor.backward(d_kpooled, self.dP[:4], shared_acc=acc, zero=False, finalize=False)
            self._join_branch()
            self.roi_extractor.finalize(self.dP[:4], accumulate=True)     # dP[l] = RPN part + RoI part
            self._reduce(0, self.mark_rpn)
            lo = self.mark_rpn
        if self.bfp is not None:
            self.bfp.backward(self.dP)          # d/dQ -> d/dP in place: the FPN's backward runs unchanged behind it
        self.neck.backward(self.dP, self.dC, [False, True, True, True])
        if self._bucket_here(1):
            self._reduce(lo, self.mark_fpn)
            lo = self.mark_fpn
        self._backbone_backward(lo)
        losses = (rpn_loss, rcnn_loss)
        if self.with_mask:
            losses += (mask_loss,)
        if iou_head is not None:
            losses += (maskiou_loss,)
        if kpt_head is not None:
            losses += (kpt_loss,)           # always the last
        return losses

    def _neck_forward(self, C):
        """The pyramid every consumer reads: the FPN's levels, balanced by the BFP if the model has one."""
        P = self.neck.forward(C)
        return P if self.bfp is None else self.bfp.forward(P)

    def predict(self, image, im_info, score_thresh=0.05, nms_thresh=0.5, max_per_image=100, with_masks=False,
                mask_thresh=0.5, nms_method="hard", soft_sigma=0.5, with_keypoints=False):
        """Inference: forward, proposals, box head, then softmax / decode / per-class NMS / top-k on the GPU
        (core/evaluation); nms_method "linear" / "gaussian": Soft-NMS per class. Returns (dets [N,max_per_image,6] = x1,y1,x2,y2,score,class;
        num_dets [N]); with_masks (Mask R-CNN) adds the pasted-back instance masks [N,max_per_image,H,W] u8 in the
        frame of the network input: mask head on the detected boxes, sigmoid, bilinear resize into the box, threshold. A
        model with the MaskIoU head (mask_iou) returns a fourth value, the mask scores [N,max_per_image] f32: the
        detection's score times the IoU the head predicts for its class (0 on padding rows); dets are unchanged.
        with_keypoints (a model with the keypoint head) appends keypoints [N,max_per_image,K,3] f32 = (x, y, score) in the
        frame of the network input as the LAST value: the keypoint head on the detected boxes, the argmax of each keypoint's
        x2 upsampled heatmap placed in the box, the maximal logit as score; zeros on padding rows."""
        from ..core.evaluation import DetectionPostprocess
        N, _, H, W = image.shape
        g_max = self.planned[3] if self.planned is not None and self.planned[:3] == (N, H, W) else 100
        self.plan(N, H, W, g_max)
        P = self._neck_forward(self.backbone.forward(image))
        self.rpn_head.forward(P)
        rois, _, _, num_rois = self.rpn_head.get_proposals(im_info)
        pooled = self.roi_extractor.forward(P, rois.view(-1, 5))
        o = self.bbox_head.forward(pooled)
        o2 = o.view(o.shape[0], -1)
        key = (score_thresh, nms_thresh, max_per_image, nms_method, soft_sigma)
        if getattr(self, "_post_key", None) != key:
            self._post = DetectionPostprocess(self.bbox_head.nc, score_thresh, nms_thresh, max_per_image,
                                              stds=self.bbox_head.stds, nms_method=nms_method, soft_sigma=soft_sigma)
            self._post_key = key
        dets, num = self._post(o2[:, :self.bbox_head.nc], o2[:, self.bbox_head.nc:], rois.view(-1, 5), num_rois, im_info)
        if not with_masks and not with_keypoints:
            return dets, num
        assert self.with_mask or not with_masks, "with_masks needs a model built with the mask head"
        assert self.keypoint_head is not None or not with_keypoints, "with_keypoints needs a model built with the keypoint head"
        M = dets.shape[1]
        flat = dets.view(N * M, 6)
        drois = torch.empty((N * M, 5), dtype=torch.float32, device=dets.device)
        drois[:, 0] = torch.arange(N, device=dets.device, dtype=torch.float32).repeat_interleave(M)
        drois[:, 1:] = flat[:, :4]            # padding rows are zero boxes with class -1: pasted as empty masks
        kpts = ()
        if with_keypoints:
            kh = self.keypoint_head
            klogits = kh.forward(self.keypoint_roi_extractor.forward(P, drois))
            kpts = (M_.keypoint_decode(klogits, flat, kh.K).view(N, M, kh.K, 3),)
        if not with_masks:
            return (dets, num) + kpts
        mpooled = self.mask_roi_extractor.forward(P, drois)
        logits = self.mask_head.forward(mpooled)
        masks = M_.mask_paste(logits, flat, H, W, mask_thresh)
        if self.mask_iou_head is None:
            return (dets, num, masks.view(N, M, H, W)) + kpts
        pred = self.mask_iou_head.forward(mpooled, logits, flat[:, 5].to(torch.int32))
        scores = M_.maskiou_score(flat, pred.view(N * M, -1))
        return (dets, num, masks.view(N, M, H, W), scores.view(N, M)) + kpts
