"""RetinaNet ResNet-FPN (BASELINE.json config 5: ResNet-101-FPN, dense 9-anchor heads, focal loss): one training step
on hand-written HIP kernels, same arena / graph / data-parallel machinery as Faster R-CNN."""
import torch

from ..core.loss import check_cls_loss, check_ghm, check_reg_loss, check_reg_max
from .backbones import ResNet
from .backbones.resnet import check_gcb
from .necks.fpn import RetinaFPN
from .rpn_heads.retina_head import RetinaHead, check_assigner
from .utils.detector import DetectorBase


def check_anchor_setting(anchor_ratios, anchor_scales_per_octave, anchor_scale):
    """-> (ratios, octave_scales) of RetinaHead. The defaults give the head's own defaults bit for bit."""
    ratios = tuple(float(r) for r in anchor_ratios)
    if not ratios or any(not r > 0.0 for r in ratios):
        raise ValueError("anchor_ratios = %r: expected a non-empty list of positive numbers" % (anchor_ratios,))
    n = anchor_scales_per_octave
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= 8:
        raise ValueError("anchor_scales_per_octave = %r: expected an integer in 1..8" % (n,))
    if not float(anchor_scale) > 0.0:
        raise ValueError("anchor_scale = %r: expected a positive number" % (anchor_scale,))
    return ratios, tuple(2.0 ** (float(i) / n) for i in range(n))


class RetinaNet(DetectorBase):
    def __init__(self, device="cuda", depth=101, num_classes=80, seed=7, dcn_stages=(), dcn_modulated=True, dcn_groups=1,
                 reg_loss="smooth_l1", reg_loss_weight=1.0, assigner="max_iou", atss_topk=9, anchor_ratios=(0.5, 1.0, 2.0),
                 anchor_scales_per_octave=3, anchor_scale=4.0, cls_loss="focal", cls_loss_alpha=None, cls_loss_gamma=None,
                 reg_max=0, dfl_weight=0.25, fpn_upsample="nearest", gcb_stages=(), gcb_reduction=16, ghm="none",
                 ghm_cls_bins=30, ghm_cls_momentum=0.75, ghm_cls_weight=1.0, ghm_reg_bins=10, ghm_reg_momentum=0.7,
                 ghm_reg_mu=0.02, ghm_reg_weight=10.0):
        """dcn_stages / dcn_modulated / dcn_groups: deformable conv2 in those backbone stages (backbones.ResNet).
        gcb_stages / gcb_reduction: a global context block (GCNet) with inner width C / gcb_reduction in every bottleneck of
        those backbone stages (backbones.ResNet); the blocks draw from a generator of their own.
        reg_loss / reg_loss_weight: the head's box loss -- 'smooth_l1', or 'iou' / 'giou' / 'diou' on the decoded box times
        reg_loss_weight (rpn_heads.RetinaHead).
        assigner / atss_topk: 'max_iou' (thresholds 0.5 / 0.4) or 'atss' (core.anchor.atss_assign).
        anchor_ratios / anchor_scales_per_octave / anchor_scale: the head's anchors per cell -- every ratio at the sizes
        anchor_scale * 2^(i / scales_per_octave) * stride, i < scales_per_octave (ATSS as published: (1.0,), 1, 8.0).
        cls_loss / cls_loss_alpha / cls_loss_gamma: the head's class loss -- 'focal', or 'qfl' / 'vfl' against the IoU of the
        decoded box (rpn_heads.RetinaHead; needs an IoU-family reg_loss). The parameter layout does not depend on it.
        reg_max / dfl_weight: reg_max > 0 = the distribution box head of Generalized Focal Loss -- retina.box_out emits
        4 * (reg_max + 1) logits per anchor, the box is their integral decode (training and predict), the loss gains a third
        component dfl_weight * DFL (rpn_heads.RetinaHead; needs an IoU-family reg_loss). As published: 16, 0.25 with ATSS,
        qfl and reg_loss_weight 2. The layout of retina.box_out depends on it; load_checkpoint refuses the other layout.
        ghm / ghm_*: 'cls' / 'reg' / 'both' = gradient harmonizing (GHM-C / GHM-R, Li et al. 2019) in place of the focal and / or
        the smooth-L1 term (rpn_heads.RetinaHead; core.loss.check_ghm). The defaults are the published settings. The
        histograms' moving average is device state of the head, per rank; it is not part of a checkpoint (head.ghm_reset()
        zeroes it) and the parameter layout does not depend on ghm.
        fpn_upsample: 'nearest' only -- CARAFE is an option of the R-CNN models' FPN (necks.FPN), not of RetinaFPN."""
        if fpn_upsample != "nearest":
            raise ValueError("fpn_upsample = %r: RetinaNet's pyramid (RetinaFPN) upsamples nearest-neighbour only; CARAFE is "
                             "a FasterRCNN option" % (fpn_upsample,))
        check_gcb(gcb_stages, gcb_reduction)
        check_reg_loss(reg_loss, reg_loss_weight)
        check_reg_max(reg_max, reg_loss, dfl_weight)
        check_cls_loss(cls_loss, reg_loss, cls_loss_alpha, cls_loss_gamma)
        check_assigner(assigner, atss_topk)
        ghm_kw = dict(ghm_cls_bins=ghm_cls_bins, ghm_cls_momentum=ghm_cls_momentum, ghm_cls_weight=ghm_cls_weight,
                      ghm_reg_bins=ghm_reg_bins, ghm_reg_momentum=ghm_reg_momentum, ghm_reg_mu=ghm_reg_mu,
                      ghm_reg_weight=ghm_reg_weight)
        check_ghm(ghm, cls_loss, reg_loss, reg_max, cls_loss_alpha, cls_loss_gamma, **{k[4:]: v for k, v in ghm_kw.items()})
        ratios, octave_scales = check_anchor_setting(anchor_ratios, anchor_scales_per_octave, anchor_scale)
        gen = torch.Generator().manual_seed(seed)
        self._init_base(device)
        self.strides = [8, 16, 32, 64, 128]
        self.head = RetinaHead(256, self.strides, self.arena, self.ws, device, gen, num_classes=num_classes,
                               ratios=ratios, octave_scales=octave_scales, anchor_scale=float(anchor_scale),
                               reg_loss=reg_loss, reg_loss_weight=reg_loss_weight, assigner=assigner, atss_topk=atss_topk,
                               cls_loss=cls_loss, cls_loss_alpha=cls_loss_alpha, cls_loss_gamma=cls_loss_gamma,
                               reg_max=reg_max, dfl_weight=dfl_weight, ghm=ghm, **ghm_kw)
        self.mark_head = self.arena.size
        self.neck = RetinaFPN([512, 1024, 2048], 256, self.arena, self.ws, device, gen)
        self.mark_fpn = self.arena.size
        self.backbone = ResNet(depth, self.arena, self.ws, device, gen, dcn_stages=dcn_stages,
                               dcn_modulated=dcn_modulated, dcn_groups=dcn_groups, gcb_stages=gcb_stages,
                               gcb_reduction=gcb_reduction, gcb_gen=torch.Generator().manual_seed(seed + 49979687))
        self._finalize_params(self.head.layers() + self.neck.layers() + self.backbone.layers(),
                              norm_layers=self.backbone.norm_layers())
        self.head.post_materialize()

    def plan(self, N, H, W, g_max):
        key = (N, H, W, g_max)
        if self.planned == key:
            return
        self._guard_replan(key)
        c_shapes = self.backbone.plan((N, 3, H, W))
        p_shapes = self.neck.plan(c_shapes[1:])
        self.head.plan(p_shapes, g_max)
        self.ws.get()
        dev = self.device
        self.dP = [torch.empty(s, dtype=torch.bfloat16, device=dev) for s in p_shapes]
        self.dC = [None] + [torch.empty(s, dtype=torch.bfloat16, device=dev) for s in c_shapes[1:]]
        self.planned = key

    def ghm_reset(self):
        """Zero the head's gradient-norm moving average (ghm != 'none'; outside any captured graph)."""
        self.head.ghm_reset()

    # The eager warm-up steps of capture() DO run the weights kernel, so they move the head's GHM moving average like any
    # training step; DetectorBase._weights_restored puts it back with the parameters, so replay(step=0) stays the first step.
    def _step_state(self):
        return self.head.ghm_state()

    def _set_step_state(self, state):
        self.head.ghm_set_state(state)

    def predict(self, image, im_info, score_thresh=0.05, nms_thresh=0.5, max_per_image=100, pre_nms_top_n=1000,
                nms_method="hard", soft_sigma=0.5):
        """Inference: forward, then per-level top-k / decode / per-class NMS / top-k on the GPU (core/evaluation
        RetinaDetect; nms_method "linear" / "gaussian": Soft-NMS per class). Returns (dets [N,max_per_image,6] = x1,y1,x2,y2,score,class in 1..C; num_dets [N])."""
        from ..core.evaluation import RetinaDetect
        N, _, H, W = image.shape
        g_max = self.planned[3] if self.planned is not None and self.planned[:3] == (N, H, W) else 100
        self.plan(N, H, W, g_max)
        P = self.neck.forward(self.backbone.forward(image)[1:])
        co, bo = self.head.forward(P)
        key = (score_thresh, nms_thresh, max_per_image, pre_nms_top_n, nms_method, soft_sigma)
        if getattr(self, "_det_key", None) != key:
            self._det = RetinaDetect(self.head.Cn, self.strides, self.head.base, pre_nms_top_n, score_thresh, nms_thresh,
                                     max_per_image, nms_method=nms_method, soft_sigma=soft_sigma, reg_max=self.head.reg_max)
            self._det_key = key
        return self._det(co, bo, im_info)

    def load_checkpoint(self, path, strict=True):
        """DetectorBase.load_checkpoint, after checking that the file's output layers have this head's layout: a plain-delta
        file (4 rows per anchor) would otherwise load into the first rows of a distribution head, and the reverse fail
        half way. The anchors per cell come from retina.cls_out (rows / classes), so 9 plain anchors (36 box rows) are not
        taken for one anchor with reg_max = 8. Raises ValueError before any tensor is changed. The file is parsed once."""
        from ..utils import load_params
        blob = load_params(path)
        h = self.head
        box, cls = blob.get("arg:retina.box_out.weight"), blob.get("arg:retina.cls_out.weight")
        fa = cls.shape[0] // h.Cn if cls is not None and cls.shape[0] % h.Cn == 0 else None    # the file's anchors per cell
        bad_cls = cls is not None and cls.shape[0] != h.A * h.Cn
        if (box is not None and box.shape[0] != h.reg_ch) or bad_cls:
            rows = box.shape[0] if box is not None else None
            a = fa if fa else h.A
            if rows is not None and rows % (4 * a) == 0:
                theirs = "%d anchors per cell x %d rows per anchor (reg_max = %d)" % (a, rows // a, rows // (4 * a) - 1)
            else:
                theirs = "no layout of %d anchors per cell" % a
            raise ValueError("checkpoint retina.box_out has %s rows: %s; retina.cls_out has %s rows. The model's box_out has %d "
                             "rows: %d anchors per cell x 4 x (reg_max + 1 = %d), its cls_out %d -- the layouts differ, build the "
                             "model with the file's anchors and reg_max"
                             % (rows, theirs, None if cls is None else cls.shape[0], h.reg_ch, h.A, h.reg_max + 1, h.A * h.Cn))
        return super().load_checkpoint(path, strict, blob=blob)

    def forward_backward(self, image, gt_boxes, im_info, step=0, image_offset=0, step_dev=None, gt_masks=None):
        N, _, H, W = image.shape
        self.plan(N, H, W, gt_boxes.shape[1])
        C = self.backbone.forward(image)
        P = self.neck.forward(C[1:])
        self.head.forward(P)
        loss = self.head.loss_and_grad(gt_boxes, im_info)
        self.head.backward(self.dP)
        lo = 0
        if self._bucket_here(0):
            self._reduce(0, self.mark_head)
            lo = self.mark_head
        self.neck.backward(self.dP, self.dC[1:])
        if self._bucket_here(1):
            self._reduce(lo, self.mark_fpn)
            lo = self.mark_fpn
        self._backbone_backward(lo)
        return (loss,)
