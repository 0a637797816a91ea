"""core/loss (/root/reference/README.md:19): smooth-L1, RPN / box-head losses, sigmoid focal loss."""
import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr

_DT = {torch.float32: 0, torch.bfloat16: 1}


def smooth_l1(pred, target, weight=None, sigma=1.0):
    lib = _lib.load()
    out = torch.empty_like(pred)
    check(lib.mxdet_smooth_l1_fwd(ptr(pred), ptr(target), ptr(weight), pred.numel(), sigma, ptr(out), stream_ptr()),
          "smooth_l1_fwd")
    return out


def smooth_l1_backward(pred, target, weight=None, grad_out=None, sigma=1.0, grad_pred=None, accumulate=False):
    lib = _lib.load()
    if grad_pred is None:
        grad_pred = torch.empty_like(pred)
    check(lib.mxdet_smooth_l1_bwd(ptr(pred), ptr(target), ptr(weight), ptr(grad_out), pred.numel(), sigma,
                                  int(accumulate), ptr(grad_pred), stream_ptr()), "smooth_l1_bwd")
    return grad_pred


def loss_workspace(n, device):
    lib = _lib.load()
    return torch.empty((lib.mxdet_loss_workspace_bytes(n),), dtype=torch.uint8, device=device)


def focal_loss(logits, labels, alpha=0.25, gamma=2.0, grad_scale=1.0, workspace=None):
    """Sigmoid focal loss fwd+bwd. logits [n,C] (f32|bf16), labels [n] i32. Returns (loss[1] f32, grad)."""
    lib = _lib.load()
    n, Cc = logits.shape
    if workspace is None:
        workspace = loss_workspace(n, logits.device)
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
    grad = torch.empty_like(logits)
    check(lib.mxdet_focal_loss(ptr(logits), _DT[logits.dtype], ptr(labels), n, Cc, alpha, gamma, grad_scale,
                               ptr(loss), ptr(grad), ptr(workspace), workspace.numel(), stream_ptr()), "focal_loss")
    return loss, grad


def rpn_loss_level(head, A, labels, bbox_targets, level_offset, sigma, norm, loss_scale, grad_head, partial):
    """One pyramid level of the RPN loss; head/grad_head bf16 [N,H,W,Cpad]; partial: f32 view for this level."""
    lib = _lib.load()
    N, H, W, Cpad = head.shape
    check(lib.mxdet_rpn_loss_level(ptr(head), N, H, W, A, Cpad, ptr(labels), ptr(bbox_targets), labels.shape[1],
                                   level_offset, sigma, norm, loss_scale, ptr(grad_head), ptr(partial),
                                   stream_ptr()), "rpn_loss_level")


def rpn_loss_num_partials(N, H, W):
    return _lib.load().mxdet_rpn_loss_num_partials(N, H, W)


def loss_finalize(partial, count, ncomp, out):
    check(_lib.load().mxdet_loss_finalize(ptr(partial), count, ncomp, ptr(out), stream_ptr()), "loss_finalize")


def rcnn_loss(cls_logits, bbox_pred, labels, bbox_targets, bbox_weights, num_classes, reg_dim, ld_cls, ld_reg,
              sigma, norm, loss_scale, grad_cls, grad_reg, loss_out, workspace):
    """Box-head losses fwd+bwd over R rois; tensors may be column views of one fused head output."""
    lib = _lib.load()
    R = labels.numel()
    check(lib.mxdet_rcnn_loss(ptr(cls_logits), ptr(bbox_pred), _DT[cls_logits.dtype], ld_cls, ld_reg, ptr(labels),
                              ptr(bbox_targets), ptr(bbox_weights), R, num_classes, reg_dim, sigma, norm, loss_scale,
                              ptr(loss_out), ptr(grad_cls), ptr(grad_reg), ptr(workspace), workspace.numel(),
                              stream_ptr()), "rcnn_loss")


def anchor_class_labels(labels, matched_gt, gt_boxes, cls_labels, num_fg):
    """RetinaNet: labels/matched [N,A] i32 -> cls_labels [N,A] (class id for fg), num_fg i32[1]."""
    lib = _lib.load()
    N, A = labels.shape
    check(lib.mxdet_anchor_class_labels(ptr(labels), ptr(matched_gt), ptr(gt_boxes), N, A, gt_boxes.shape[1],
                                        ptr(cls_labels), ptr(num_fg), stream_ptr()), "anchor_class_labels")


def retina_loss_num_partials(N, H, W, A):
    return _lib.load().mxdet_retina_loss_num_partials(N, H, W, A)


def retina_loss_level(cls, reg, A, C, cls_labels, bbox_targets, level_offset, alpha, gamma, sigma, num_fg, loss_scale,
                      grad_cls, grad_reg, partial):
    lib = _lib.load()
    N, H, W, ld_cls = cls.shape
    check(lib.mxdet_retina_loss_level(ptr(cls), ptr(reg), N, H, W, A, C, ld_cls, reg.shape[3], ptr(cls_labels),
                                      ptr(bbox_targets), cls_labels.shape[1], level_offset, alpha, gamma, sigma,
                                      ptr(num_fg), loss_scale, ptr(grad_cls), ptr(grad_reg), ptr(partial), stream_ptr()),
          "retina_loss_level")


# ---- IoU / GIoU / DIoU losses on the decoded box (include/mxdet.h) ----
IOU_LOSS_KINDS = _lib.IOU_LOSS_KINDS
REG_LOSSES = ("smooth_l1",) + tuple(IOU_LOSS_KINDS)
BOX_HEAD_REG_LOSSES = REG_LOSSES + ("balanced_l1",)       # Balanced L1 (Libra R-CNN) is the box head's alone


def check_reg_loss(reg_loss, reg_loss_weight, box_head=False):
    """The regression-loss options of the box heads (box_head: 'balanced_l1' too) and the RetinaNet head, checked before
    anything is allocated."""
    if reg_loss == "balanced_l1" and not box_head:
        raise ValueError("reg_loss = 'balanced_l1' is an option of the R-CNN box head only (the RetinaNet head keeps %s)"
                         % ", ".join(REG_LOSSES))
    allowed = BOX_HEAD_REG_LOSSES if box_head else REG_LOSSES
    if reg_loss not in allowed:
        raise ValueError("reg_loss must be one of %s (got %r)" % (", ".join(allowed), reg_loss))
    w = reg_loss_weight
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not w > 0:
        raise ValueError("reg_loss_weight must be a positive number (got %r)" % (w,))
    if reg_loss == "smooth_l1" and w != 1:
        raise ValueError("reg_loss_weight = %r needs an IoU-family reg_loss: smooth_l1 takes no weight" % (w,))


# ---- Balanced L1 of the box head (Libra R-CNN, Pang et al. 2019; include/mxdet.h) ----
BL1_DEFAULTS = (0.5, 1.5, 1.0)          # alpha, gamma, beta as published


def check_balanced_l1(alpha=0.5, gamma=1.5, beta=1.0):
    """alpha, gamma, beta of Balanced L1: positive finite numbers. Returns them as floats."""
    for name, v in (("bl1_alpha", alpha), ("bl1_gamma", gamma), ("bl1_beta", beta)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < float(v) < float("inf"):
            raise ValueError("%s must be a positive finite number (got %r)" % (name, v))
    return float(alpha), float(gamma), float(beta)


def balanced_l1_b(alpha, gamma):
    """b = float32(exp(gamma / alpha) - 1), evaluated in double: the constant that joins Balanced L1's two branches."""
    import math
    return float(torch.tensor(math.exp(float(gamma) / float(alpha)) - 1.0, dtype=torch.float64).to(torch.float32))


def rcnn_loss_balanced(cls_logits, bbox_pred, labels, bbox_targets, bbox_weights, num_classes, reg_dim, ld_cls, ld_reg, alpha,
                       gamma, beta, reg_weight, norm, loss_scale, grad_cls, grad_reg, loss_out, workspace):
    """rcnn_loss with Balanced L1(alpha, gamma, beta) times reg_weight in place of smooth-L1."""
    lib = _lib.load()
    alpha, gamma, beta = check_balanced_l1(alpha, gamma, beta)
    R = labels.numel()
    check(lib.mxdet_rcnn_loss_balanced(ptr(cls_logits), ptr(bbox_pred), _DT[cls_logits.dtype], ld_cls, ld_reg, ptr(labels),
                                       ptr(bbox_targets), ptr(bbox_weights), R, num_classes, reg_dim, alpha, gamma, beta,
                                       balanced_l1_b(alpha, gamma), reg_weight, norm, loss_scale, ptr(loss_out), ptr(grad_cls),
                                       ptr(grad_reg), ptr(workspace), workspace.numel(), stream_ptr()), "rcnn_loss_balanced")


def box_iou_loss(boxes, gt, deltas, kind="giou", stds=(1.0, 1.0, 1.0, 1.0), weight=None, grad_scale=1.0, loss=None,
                 grad_deltas=None):
    """Unfused IoU-family loss fwd+bwd: boxes / gt [n,4] f32, deltas [n,ld>=4] (f32|bf16; may be a column view of a wider
    buffer). Returns (loss [n] f32, grad_deltas like deltas; only columns 0..3 are written)."""
    lib = _lib.load()
    n = boxes.shape[0]
    if loss is None:
        loss = torch.empty((n,), dtype=torch.float32, device=boxes.device)
    ld = deltas.stride(0) if n > 1 else max(4, deltas.shape[1])
    if grad_deltas is None:     # same leading dimension as deltas
        grad_deltas = torch.zeros((n, ld), dtype=deltas.dtype, device=deltas.device)[:, :deltas.shape[1]]
    check(lib.mxdet_box_iou_loss(ptr(boxes), ptr(gt), ptr(deltas), _DT[deltas.dtype], ld, ptr(weight), n,
                                 IOU_LOSS_KINDS[kind], stds[0], stds[1], stds[2], stds[3], grad_scale, ptr(loss),
                                 ptr(grad_deltas), stream_ptr()), "box_iou_loss")
    return loss, grad_deltas


def rcnn_loss_iou(cls_logits, bbox_pred, labels, rois, matched_gt, gt_boxes, num_classes, reg_dim, ld_cls, ld_reg, kind,
                  stds, reg_weight, norm, loss_scale, grad_cls, grad_reg, loss_out, workspace):
    """rcnn_loss with an IoU-family regression term on the decoded box: rois [R,5], matched_gt [R], gt_boxes [N,G,5]."""
    lib = _lib.load()
    R = labels.numel()
    check(lib.mxdet_rcnn_loss_iou(ptr(cls_logits), ptr(bbox_pred), _DT[cls_logits.dtype], ld_cls, ld_reg, ptr(labels),
                                  ptr(rois), ptr(matched_gt), ptr(gt_boxes), gt_boxes.shape[0], gt_boxes.shape[1], R,
                                  num_classes, reg_dim, IOU_LOSS_KINDS[kind], stds[0], stds[1], stds[2], stds[3], reg_weight,
                                  norm, loss_scale, ptr(loss_out), ptr(grad_cls), ptr(grad_reg), ptr(workspace),
                                  workspace.numel(), stream_ptr()), "rcnn_loss_iou")


def retina_loss_level_iou(cls, reg, A, C, cls_labels, anchors, matched_gt, gt_boxes, level_offset, alpha, gamma, kind, stds,
                          reg_weight, num_fg, loss_scale, grad_cls, grad_reg, partial):
    """retina_loss_level with an IoU-family box term: anchors [A_total,4], matched_gt [N,A_total], gt_boxes [N,G,5]."""
    lib = _lib.load()
    N, H, W, ld_cls = cls.shape
    check(lib.mxdet_retina_loss_level_iou(ptr(cls), ptr(reg), N, H, W, A, C, ld_cls, reg.shape[3], ptr(cls_labels),
                                          ptr(anchors), ptr(matched_gt), ptr(gt_boxes), gt_boxes.shape[1],
                                          cls_labels.shape[1], level_offset, alpha, gamma, IOU_LOSS_KINDS[kind], stds[0],
                                          stds[1], stds[2], stds[3], reg_weight, ptr(num_fg), loss_scale, ptr(grad_cls),
                                          ptr(grad_reg), ptr(partial), stream_ptr()), "retina_loss_level_iou")


# ---- quality-aware class losses of the RetinaNet head: QFL / Varifocal (include/mxdet.h) ----
CLS_LOSS_KINDS = _lib.CLS_LOSS_KINDS
CLS_LOSSES = ("focal",) + tuple(CLS_LOSS_KINDS)
CLS_LOSS_DEFAULTS = {"qfl": (0.0, 2.0), "vfl": (0.75, 2.0)}        # (alpha, gamma) as published; QFL: beta in gamma, no alpha


def check_cls_loss(cls_loss, reg_loss, alpha=None, gamma=None):
    """The class-loss options of the RetinaNet head, checked before anything is allocated. alpha / gamma None = the kind's
    published default (focal: the head's own alpha / gamma). Returns (alpha, gamma) for a quality loss, None for focal."""
    if cls_loss not in CLS_LOSSES:
        raise ValueError("cls_loss must be one of %s (got %r)" % (", ".join(CLS_LOSSES), cls_loss))
    for name, v in (("cls_loss_alpha", alpha), ("cls_loss_gamma", gamma)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float))):
            raise ValueError("%s must be a number or None (got %r)" % (name, v))
    if gamma is not None and not gamma > 0:
        raise ValueError("cls_loss_gamma must be positive (got %r)" % (gamma,))
    if alpha is not None and not 0 <= alpha <= 1:
        raise ValueError("cls_loss_alpha must lie in [0, 1] (got %r)" % (alpha,))
    if cls_loss == "focal":
        return None
    if reg_loss not in IOU_LOSS_KINDS:
        raise ValueError("cls_loss = %r needs an IoU-family reg_loss (%s): the quality is the decoded box's IoU, "
                         "reg_loss = %r decodes none" % (cls_loss, ", ".join(IOU_LOSS_KINDS), reg_loss))
    a0, g0 = CLS_LOSS_DEFAULTS[cls_loss]
    return float(a0 if alpha is None else alpha), float(g0 if gamma is None else gamma)


def quality_focal_loss(logits, labels, quality, cls_loss="qfl", alpha=None, gamma=None, grad_scale=1.0, workspace=None):
    """QFL / Varifocal loss fwd+bwd on given qualities. logits [n,C] (f32|bf16), labels [n] i32, quality [n] f32 (the
    target of row r's column labels[r] - 1). Returns (loss[1] f32, grad like logits)."""
    lib = _lib.load()
    if cls_loss not in CLS_LOSS_KINDS:
        raise ValueError("cls_loss must be one of %s (got %r)" % (", ".join(CLS_LOSS_KINDS), cls_loss))
    a0, g0 = CLS_LOSS_DEFAULTS[cls_loss]
    alpha, gamma = (a0 if alpha is None else alpha), (g0 if gamma is None else gamma)
    n, Cc = logits.shape
    if workspace is None:
        workspace = loss_workspace(n, logits.device)
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
    grad = torch.empty_like(logits)
    check(lib.mxdet_quality_focal_loss(ptr(logits), _DT[logits.dtype], ptr(labels), ptr(quality), n, Cc,
                                       CLS_LOSS_KINDS[cls_loss], alpha, gamma, grad_scale, ptr(loss), ptr(grad), ptr(workspace),
                                       workspace.numel(), stream_ptr()), "quality_focal_loss")
    return loss, grad


def retina_loss_level_quality(cls, reg, A, C, cls_labels, anchors, matched_gt, gt_boxes, level_offset, cls_loss, alpha, gamma,
                              kind, stds, reg_weight, num_fg, loss_scale, grad_cls, grad_reg, partial):
    """retina_loss_level_iou with the class term 'qfl' (beta in gamma) or 'vfl' on the decoded box's IoU."""
    lib = _lib.load()
    if cls_loss not in CLS_LOSS_KINDS:
        raise ValueError("cls_loss must be one of %s (got %r)" % (", ".join(CLS_LOSS_KINDS), cls_loss))
    if kind not in IOU_LOSS_KINDS:
        raise ValueError("cls_loss = %r needs an IoU-family reg_loss (got %r)" % (cls_loss, kind))
    N, H, W, ld_cls = cls.shape
    check(lib.mxdet_retina_loss_level_quality(ptr(cls), ptr(reg), N, H, W, A, C, ld_cls, reg.shape[3], ptr(cls_labels),
                                              ptr(anchors), ptr(matched_gt), ptr(gt_boxes), gt_boxes.shape[1],
                                              cls_labels.shape[1], level_offset, CLS_LOSS_KINDS[cls_loss], alpha, gamma,
                                              IOU_LOSS_KINDS[kind], stds[0], stds[1], stds[2], stds[3], reg_weight, ptr(num_fg),
                                              loss_scale, ptr(grad_cls), ptr(grad_reg), ptr(partial), stream_ptr()),
          "retina_loss_level_quality")


# ---- distribution box regression of the RetinaNet head: integral decode + DFL (include/mxdet.h) ----
CLS_LOSS_KINDS_DFL = _lib.CLS_LOSS_KINDS_DFL
REG_MAX_LIMIT = _lib.REG_MAX_LIMIT


def check_reg_max(reg_max, reg_loss, dfl_weight=0.25):
    """The distribution-head options, checked before anything is allocated: reg_max = 0 (plain deltas) or the last bin
    1..REG_MAX_LIMIT (each side a distribution over 0..reg_max strides; needs an IoU-family reg_loss, which acts on the
    integral-decoded box); dfl_weight > 0."""
    if isinstance(reg_max, bool) or not isinstance(reg_max, int) or not 0 <= reg_max <= REG_MAX_LIMIT:
        raise ValueError("reg_max must be an integer in 0..%d (got %r)" % (REG_MAX_LIMIT, reg_max))
    w = dfl_weight
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not w > 0:
        raise ValueError("dfl_weight must be a positive number (got %r)" % (w,))
    if reg_max > 0 and reg_loss not in IOU_LOSS_KINDS:
        raise ValueError("reg_max = %r needs an IoU-family reg_loss (%s): the box loss acts on the integral-decoded box, "
                         "reg_loss = %r decodes none" % (reg_max, ", ".join(IOU_LOSS_KINDS), reg_loss))


def box_dist_loss(boxes, gt, logits, reg_max, stride, kind="giou", reg_weight=1.0, dfl_weight=0.25, grad_scale=1.0,
                  grad_logits=None, want_quality=True):
    """Unfused distribution box loss fwd+bwd: boxes / gt [n,4] f32, logits [n,ld>=4*(reg_max+1)] (f32|bf16; may be a column
    view of a wider buffer). Returns (loss_box [n], loss_dfl [n], quality [n] or None, grad_logits like logits; only the
    first 4*(reg_max+1) columns are written)."""
    lib = _lib.load()
    if kind not in IOU_LOSS_KINDS:
        raise ValueError("kind must be one of %s (got %r)" % (", ".join(IOU_LOSS_KINDS), kind))
    check_reg_max(reg_max, kind, dfl_weight)
    n = boxes.shape[0]
    dev = boxes.device
    loss_box = torch.empty((n,), dtype=torch.float32, device=dev)
    loss_dfl = torch.empty((n,), dtype=torch.float32, device=dev)
    quality = torch.empty((n,), dtype=torch.float32, device=dev) if want_quality else None
    ld = logits.stride(0) if n > 1 else logits.shape[1]
    if grad_logits is None:     # same leading dimension as logits
        grad_logits = torch.zeros((n, ld), dtype=logits.dtype, device=logits.device)[:, :logits.shape[1]]
    for name, t in (("logits", logits), ("grad_logits", grad_logits)):      # one leading dimension serves both
        if t.dtype != logits.dtype or t.shape[1] < 4 * (reg_max + 1) or (n > 0 and t.stride(1) != 1) or (n > 1 and t.stride(0) != ld):
            raise ValueError("box_dist_loss: %s must hold rows of >= %d contiguous %s elements with the row stride of logits "
                             "(%d); got shape %s, strides %s, %s" % (name, 4 * (reg_max + 1), logits.dtype, ld, tuple(t.shape),
                                                                       tuple(t.stride()), t.dtype))
    check(lib.mxdet_box_dist_loss(ptr(boxes), ptr(gt), ptr(logits), _DT[logits.dtype], ld, n, reg_max, stride,
                                  IOU_LOSS_KINDS[kind], reg_weight, dfl_weight, grad_scale, ptr(loss_box), ptr(loss_dfl),
                                  ptr(quality), ptr(grad_logits), stream_ptr()), "box_dist_loss")
    return loss_box, loss_dfl, quality, grad_logits


def retina_loss_level_dfl(cls, reg, A, C, cls_labels, anchors, matched_gt, gt_boxes, level_offset, cls_loss, alpha, gamma,
                          kind, reg_max, stride, reg_weight, dfl_weight, num_fg, loss_scale, grad_cls, grad_reg, partial):
    """The level loss of the distribution head: class term 'focal' / 'qfl' / 'vfl', box term `kind` on the integral-decoded
    box, DFL. reg / grad_reg [N,H,W,ld_reg >= 4*(reg_max+1)*A]; partial: THREE f32 words per workgroup."""
    lib = _lib.load()
    if cls_loss not in CLS_LOSS_KINDS_DFL:
        raise ValueError("cls_loss must be one of %s (got %r)" % (", ".join(CLS_LOSS_KINDS_DFL), cls_loss))
    if kind not in IOU_LOSS_KINDS:
        raise ValueError("reg_max = %r needs an IoU-family reg_loss (got %r)" % (reg_max, kind))
    N, H, W, ld_cls = cls.shape
    check(lib.mxdet_retina_loss_level_dfl(ptr(cls), ptr(reg), N, H, W, A, C, ld_cls, reg.shape[3], ptr(cls_labels),
                                          ptr(anchors), ptr(matched_gt), ptr(gt_boxes), gt_boxes.shape[1],
                                          cls_labels.shape[1], level_offset, CLS_LOSS_KINDS_DFL[cls_loss], alpha, gamma,
                                          IOU_LOSS_KINDS[kind], reg_max, stride, reg_weight, dfl_weight, ptr(num_fg),
                                          loss_scale, ptr(grad_cls), ptr(grad_reg), ptr(partial), stream_ptr()),
          "retina_loss_level_dfl")


# ---- gradient harmonizing of the RetinaNet head: GHM-C / GHM-R (include/mxdet.h) ----
GHM_MODES = ("none", "cls", "reg", "both")
GHM_FLAGS = _lib.GHM_FLAGS
GHM_MAX_BINS = _lib.GHM_MAX_BINS
GHM_DEFAULTS = dict(cls_bins=30, cls_momentum=0.75, cls_weight=1.0, reg_bins=10, reg_momentum=0.7, reg_mu=0.02,
                    reg_weight=10.0)                                   # as published (Li et al. 2019; mmdetection)


def check_ghm(ghm="none", cls_loss="focal", reg_loss="smooth_l1", reg_max=0, cls_loss_alpha=None, cls_loss_gamma=None,
              cls_bins=30, cls_momentum=0.75, cls_weight=1.0, reg_bins=10, reg_momentum=0.7, reg_mu=0.02, reg_weight=10.0):
    """The gradient-harmonizing options of the RetinaNet head, checked before anything is allocated. ghm: 'none', or which
    terms are harmonized: 'cls' replaces the focal loss, 'reg' the smooth-L1 loss, 'both'. Every mode but 'none' needs
    cls_loss 'focal', reg_loss 'smooth_l1' and reg_max 0 (the half that is not harmonized is the plain entry's); 'cls' and
    'both' take no cls_loss_alpha / cls_loss_gamma (GHM-C has neither; with 'reg' they are the focal half's). Returns the
    seven settings as a dict of ints / floats (the keys of GHM_DEFAULTS)."""
    if ghm not in GHM_MODES:
        raise ValueError("ghm must be one of %s (got %r)" % (", ".join(GHM_MODES), ghm))
    for name, b in (("ghm_cls_bins", cls_bins), ("ghm_reg_bins", reg_bins)):
        if isinstance(b, bool) or not isinstance(b, int) or not 1 <= b <= GHM_MAX_BINS:
            raise ValueError("%s must be an integer in 1..%d (got %r)" % (name, GHM_MAX_BINS, b))
    for name, m in (("ghm_cls_momentum", cls_momentum), ("ghm_reg_momentum", reg_momentum)):
        if isinstance(m, bool) or not isinstance(m, (int, float)) or not 0 <= m < 1:
            raise ValueError("%s must lie in [0, 1) (got %r)" % (name, m))
    for name, v in (("ghm_cls_weight", cls_weight), ("ghm_reg_weight", reg_weight), ("ghm_reg_mu", reg_mu)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 < v < float("inf"):
            raise ValueError("%s must be a positive finite number (got %r)" % (name, v))
    cfg = dict(cls_bins=int(cls_bins), cls_momentum=float(cls_momentum), cls_weight=float(cls_weight), reg_bins=int(reg_bins),
               reg_momentum=float(reg_momentum), reg_mu=float(reg_mu), reg_weight=float(reg_weight))
    if ghm == "none":
        return cfg
    # The level entry's other half is the focal / smooth-L1 half of retina_loss_level and nothing else, so EVERY mode needs
    # the plain pair: 'cls' beside giou would otherwise train smooth-L1 without saying so, and beside reg_max > 0 walk a
    # distribution head's channels as four deltas.
    if cls_loss != "focal":
        raise ValueError("ghm = %r harmonizes the sigmoid cross-entropy in place of the focal loss, or keeps the focal loss "
                         "beside a harmonized box term: cls_loss = %r is another class loss (GHM with qfl / vfl is not built)"
                         % (ghm, cls_loss))
    if reg_loss != "smooth_l1":
        raise ValueError("ghm = %r works on the encoded deltas, harmonized ('reg', 'both') or as smooth-L1 beside a harmonized "
                         "class term ('cls'): reg_loss = %r acts on the decoded box (GHM with the IoU family is not built); "
                         "keep reg_loss = 'smooth_l1'" % (ghm, reg_loss))
    if reg_max != 0:
        raise ValueError("ghm = %r needs plain deltas: reg_max = %r makes the box branch a distribution head" % (ghm, reg_max))
    if ghm in ("cls", "both") and (cls_loss_alpha is not None or cls_loss_gamma is not None):
        raise ValueError("ghm = %r: GHM-C has no alpha / gamma (cls_loss_alpha = %r, cls_loss_gamma = %r); its settings "
                         "are ghm_cls_bins / ghm_cls_momentum / ghm_cls_weight" % (ghm, cls_loss_alpha, cls_loss_gamma))
    return cfg


def _ghm_flags(ghm):
    if ghm not in GHM_FLAGS:
        raise ValueError("ghm must be one of %s (got %r)" % (", ".join(GHM_FLAGS), ghm))
    return GHM_FLAGS[ghm]


def ghm_hist_level(cls, reg, A, C, cls_labels, bbox_targets, level_offset, ghm, cls_bins, reg_bins, reg_mu, counts):
    """Histogram pass of one level: counts = this level's rows ([retina_loss_num_partials, cls_bins + reg_bins] int32) of
    the step's count table; ghm 'cls' / 'reg' / 'both' = the halves that are counted."""
    lib = _lib.load()
    N, H, W, ld_cls = cls.shape
    check(lib.mxdet_ghm_hist_level(ptr(cls), ptr(reg), N, H, W, A, C, ld_cls, reg.shape[3], ptr(cls_labels), ptr(bbox_targets),
                                   cls_labels.shape[1], level_offset, _ghm_flags(ghm), cls_bins, reg_bins, reg_mu, ptr(counts),
                                   stream_ptr()), "ghm_hist_level")


def ghm_weights(counts, rows, cls_bins, reg_bins, cls_momentum, reg_momentum, acc, cnt, coef):
    """The step's weights from the first `rows` rows of the count table: acc (the moving average, f32) is updated in place,
    cnt (i32) and coef (f32) are written; all three [cls_bins + reg_bins], class bins first."""
    check(_lib.load().mxdet_ghm_weights(ptr(counts), rows, cls_bins, reg_bins, cls_momentum, reg_momentum, ptr(acc), ptr(cnt),
                                        ptr(coef), stream_ptr()), "ghm_weights")


def retina_loss_level_ghm(cls, reg, A, C, cls_labels, bbox_targets, level_offset, ghm, alpha, gamma, sigma, coef, cls_bins,
                          reg_bins, cls_weight, reg_mu, reg_weight, num_fg, loss_scale, grad_cls, grad_reg, partial):
    """retina_loss_level with the class ('cls'), the box ('reg') or both terms harmonized by coef (ghm_weights); the other
    half is retina_loss_level's, bit for bit."""
    lib = _lib.load()
    N, H, W, ld_cls = cls.shape
    check(lib.mxdet_retina_loss_level_ghm(ptr(cls), ptr(reg), N, H, W, A, C, ld_cls, reg.shape[3], ptr(cls_labels),
                                          ptr(bbox_targets), cls_labels.shape[1], level_offset, _ghm_flags(ghm), alpha, gamma,
                                          sigma, ptr(coef), cls_bins, reg_bins, cls_weight, reg_mu, reg_weight, ptr(num_fg),
                                          loss_scale, ptr(grad_cls), ptr(grad_reg), ptr(partial), stream_ptr()),
          "retina_loss_level_ghm")


# ---- online hard example mining for the box head (include/mxdet.h) ----
def ohem_roi_score(cls_logits, bbox_pred, labels, num_classes, reg_dim, ld_cls, ld_reg, reg_loss="smooth_l1", bbox_targets=None,
                   bbox_weights=None, sigma=1.0, rois=None, matched_gt=None, gt_boxes=None, stds=(0.1, 0.1, 0.2, 0.2),
                   reg_weight=1.0, score=None):
    """The per-roi loss rcnn_loss (reg_loss 'smooth_l1': bbox_targets / bbox_weights / sigma) or rcnn_loss_iou (an IoU kind:
    rois / matched_gt / gt_boxes / stds / reg_weight) reports for each row alone, cls + reg, as f32 [R]; -1 for label < 0.
    No gradients are written."""
    lib = _lib.load()
    if reg_loss not in REG_LOSSES:
        raise ValueError("reg_loss must be one of %s (got %r)" % (", ".join(REG_LOSSES), reg_loss))
    R = labels.numel()
    if score is None:
        score = torch.empty((R,), dtype=torch.float32, device=labels.device)
    kind = -1 if reg_loss == "smooth_l1" else IOU_LOSS_KINDS[reg_loss]
    N, G = (gt_boxes.shape[0], gt_boxes.shape[1]) if gt_boxes is not None else (0, 0)
    check(lib.mxdet_ohem_roi_score(ptr(cls_logits), ptr(bbox_pred), _DT[cls_logits.dtype], ld_cls, ld_reg, ptr(labels),
                                   ptr(bbox_targets), ptr(bbox_weights), ptr(rois), ptr(matched_gt), ptr(gt_boxes), N, G, R,
                                   num_classes, reg_dim, kind, sigma, stds[0], stds[1], stds[2], stds[3], reg_weight, ptr(score),
                                   stream_ptr()), "ohem_roi_score")
    return score
