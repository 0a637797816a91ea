"""Experiment configuration (/root/reference/README.md:13 `configs`, README.md:49-52
easydict). An attribute dictionary with the lineage's rule that an experiment file may only set keys that exist in the
defaults (typos fail loudly). Files are YAML, read with yaml.safe_load -- the lineage executes python config modules;
nothing is executed here."""
import copy

import yaml


class Config(dict):
    """dict with attribute access, recursively (easydict's behaviour for the subset used here)."""

    def __init__(self, d=None):
        super().__init__()
        for k, v in (d or {}).items():
            self[k] = v

    def __setitem__(self, k, v):
        super().__setitem__(k, Config(v) if isinstance(v, dict) and not isinstance(v, Config) else v)

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v

    def to_dict(self):
        return {k: (v.to_dict() if isinstance(v, Config) else copy.deepcopy(v)) for k, v in self.items()}


DEFAULTS = {
    "network": {
        "type": "faster_rcnn",            # faster_rcnn | mask_rcnn | retinanet
        "backbone_depth": 50,
        "num_classes": 81,                # incl. background for the two-stage models; retinanet uses num_classes - 1
        "pretrained": "",                 # MXNet .params with ImageNet ResNet weights (utils.params_io)
        "seed": 7,
        "dcn_stages": [],                 # backbone stages (subset of 3, 4, 5) whose conv2 is deformable (contrib.DeformableConvolution)
        "dcn_modulated": True,            # DCN v2 (sigmoid mask) when true, v1 otherwise
        "dcn_groups": 1,                  # deformable groups
        "gcb_stages": [],                 # backbone stages (subset of 3, 4, 5) whose bottlenecks get a global context block (GCNet; Cao et al. 2019)
        "gcb_reduction": 16,              # inner width of the block's transform = C / gcb_reduction (a multiple of 8, at most 512); published: 16 | 4
        "roi_pool": "roi_align",          # box branch pooling: roi_align | dpool | mdpool (contrib.DeformablePSROIPooling)
        "dpool_trans_std": 0.1,           # scale of the predicted bin offsets (in roi widths / heights)
        "dpool_sample_per_part": 4,       # samples per bin and axis
        "bbox_head": "2fc",               # box head trunk: 2fc | 4conv1fc (four 3x3 convs + one FC)
        "head_norm": "none",              # none | gn: GroupNorm after every conv of the 4conv1fc box head and of the mask head
        "gn_groups": 32,                  # GroupNorm groups (256 / gn_groups must be a multiple of 8)
        "reg_loss": "smooth_l1",          # box regression loss of the box head / the RetinaNet head: smooth_l1 | iou | giou | diou | balanced_l1 (box head only)
        "reg_loss_weight": 1.0,           # weight of an IoU-family reg_loss (on the decoded box); smooth_l1 takes none. The RPN keeps smooth-L1
        "cls_loss": "focal",              # retinanet class loss: focal | qfl (Li et al. 2020) | vfl (Zhang et al. 2021); qfl / vfl need an IoU-family reg_loss
        "cls_loss_alpha": None,           # null = the kind's published setting (focal 0.25, vfl 0.75; qfl takes none)
        "cls_loss_gamma": None,           # null = the kind's published setting (focal 2, qfl beta = 2, vfl 2)
        "reg_max": 0,                     # retinanet box branch: 0 = deltas (dx, dy, dw, dh); R > 0 = each side a distribution over 0..R strides, integral decode + DFL (Li et al. 2020; published 16; needs an IoU-family reg_loss)
        "dfl_weight": 0.25,               # weight of the Distribution Focal Loss (reg_max > 0)
        "ghm": "none",                    # retinanet: none | cls | reg | both -- gradient harmonizing (GHM-C / GHM-R; Li et al. 2019) in place of the focal / smooth-L1 term; needs cls_loss focal without alpha / gamma, reg_loss smooth_l1, reg_max 0
        "ghm_cls_bins": 30,               # GHM-C: gradient-norm bins (1..64) ...
        "ghm_cls_momentum": 0.75,         # ... moving average of the bin counts, in [0, 1); 0 = the step's own counts ...
        "ghm_cls_weight": 1.0,            # ... weight of the term, as published
        "ghm_reg_bins": 10,               # GHM-R: bins (1..64) ...
        "ghm_reg_momentum": 0.7,          # ... momentum ...
        "ghm_reg_mu": 0.02,               # ... mu of the authentic smooth-L1 sqrt(d^2 + mu^2) - mu ...
        "ghm_reg_weight": 10.0,           # ... weight of the term, as published
        "assigner": "max_iou",            # retinanet targets: max_iou (thresholds 0.5 / 0.4) | atss (Zhang et al. 2020). The RPN keeps its sampler
        "atss_topk": 9,                   # ATSS: candidates per ground-truth box and pyramid level (1..16)
        "anchor_ratios": [0.5, 1.0, 2.0],  # retinanet anchors per cell: these h/w ratios ...
        "anchor_scales_per_octave": 3,    # ... times this many sizes per octave ...
        "anchor_scale": 4.0,              # ... starting at anchor_scale * stride (ATSS as published: [1.0], 1, 8.0)
        "dpool_offset_fcs": 3,            # FCs of the offset head (1: Deformable-ConvNets' FPN head, 3: DCN v2 / mmdetection)
        "mask_iou": False,                # mask_rcnn: Mask Scoring R-CNN's MaskIoU head (Huang et al. 2019); segm detections are scored box score x predicted mask IoU
        "mask_iou_weight": 1.0,           # weight of the MaskIoU head's L2 loss
        "ohem": False,                    # faster_rcnn / mask_rcnn: online hard example mining (Shrivastava et al. 2016) -- the box head trains on the batch_rois highest-loss RoIs of a read-only pass over every candidate, no fg:bg quota
        "ohem_nms": 0.7,                  # IoU above which a higher-loss RoI suppresses a lower-loss one before the choice, in (0, 1]; 1 = no dedup
        "keypoints": 0,                   # faster_rcnn / mask_rcnn: 1 = Keypoint R-CNN's keypoint head (He et al. 2017); training then reads the roidb's keypoints
        "keypoint_weight": 1.0,           # weight of the keypoint heatmap loss
        "num_keypoints": 17,              # keypoints per instance (COCO person: 17)
        "neck": "fpn",                    # faster_rcnn / mask_rcnn: fpn | bfp (Libra R-CNN's Balanced Feature Pyramid behind the FPN; Pang et al. 2019)
        "bfp_refine": "conv",             # refine step of the balanced map: conv (one 3x3 convolution) | embedded_gaussian (the paper's non-local block) | none
        "bfp_nl_reduction": 2,            # embedded_gaussian: inner channels Ci = 256 / reduction; 2 or 4 (Ci = 128 or 64)
        "bfp_nl_use_scale": False,        # embedded_gaussian: logits times 1 / sqrt(Ci)
        "fpn_upsample": "nearest",        # faster_rcnn / mask_rcnn: nearest | carafe (CARAFE in the FPN's top-down path; Wang et al. 2019)
        "carafe_k": 5,                    # carafe: reassembly kernel, 3 | 5
        "carafe_compress": 64,            # carafe: channels of the 1x1 compressor, a multiple of 64
        "carafe_enc_kernel": 3,           # carafe: kernel of the logit encoder, 1 | 3
        "sampler": "random",              # box head's RoI sampler: random | iou_balanced (background quota per IoU bin; not with ohem)
        "sampler_bins": 3,                # IoU bins of the iou_balanced sampler (1..8)
        "bl1_alpha": 0.5,                 # Balanced L1 (reg_loss: balanced_l1, box head only; times reg_loss_weight): alpha ...
        "bl1_gamma": 1.5,                 # ... gamma ...
        "bl1_beta": 1.0,                  # ... beta, as published
    },
    "dataset": {
        "type": "synthetic",              # synthetic | coco | voc (ann_file = Annotations directory)
        "ann_file": "", "image_dir": "",
        "num_images": 64,                 # synthetic only
        "target_size": 800, "max_size": 1333,
        "pixel_means": [123.68, 116.779, 103.939], "pixel_stds": [1.0, 1.0, 1.0], "swap_rb": False,
        "fixed_shape": [800, 1344],       # one batch shape (hipGraph replay); [] = per-batch shapes (eager launches)
        "max_gt": 100,
    },
    "TRAIN": {
        "batch_images": 2,                # per GPU
        "lr": 0.02, "lr_reference_batch": 16, "lr_step": [8, 11], "lr_factor": 0.1,
        "warmup": True, "warmup_lr": 0.00667, "warmup_step": 500, "warmup_mode": "linear",
        "momentum": 0.9, "wd": 0.0001,
        "begin_epoch": 0, "end_epoch": 12,
        "flip": True, "shuffle": True, "aspect_grouping": True, "seed": 0,
        "rpn_pre_nms_top_n": 2000, "rpn_post_nms_top_n": 2000, "batch_rois": 512,
        "graph": True,                    # hipGraph replay of the step
        "checkpoint_prefix": "", "checkpoint_period": 1, "resume": "",
        "log_period": 20, "max_iters": 0,
    },
    "TEST": {
        "batch_images": 2, "score_thresh": 0.05, "nms": 0.5, "max_per_image": 100,
        "bbox_means": [0.0, 0.0, 0.0, 0.0], "bbox_stds": [0.1, 0.1, 0.2, 0.2],
        "nms_method": "hard",             # per-class stage: "hard" (greedy NMS) | "linear" | "gaussian" (Soft-NMS)
        "soft_sigma": 0.5,                # sigma of the Gaussian Soft-NMS weight exp(-iou^2 / sigma)
    },
}


def default_config():
    return Config(copy.deepcopy(DEFAULTS))


def update_config(cfg, d, _path=""):
    """Merge d into cfg; every key must already exist (lineage `update_config`)."""
    for k, v in d.items():
        if k not in cfg:
            raise KeyError("unknown config key %s%s" % (_path, k))
        if isinstance(cfg[k], Config):
            if not isinstance(v, dict):
                raise TypeError("config key %s%s is a section" % (_path, k))
            update_config(cfg[k], v, _path + k + ".")
        else:
            cfg[k] = v
    return cfg


def load_config(path=None, overrides=()):
    """defaults <- YAML file <- "SECTION.key=value" overrides (values parsed as YAML scalars/lists)."""
    cfg = default_config()
    if path:
        with open(path, "r") as f:
            update_config(cfg, yaml.safe_load(f) or {})
    for o in overrides:
        key, _, val = o.partition("=")
        if not _:
            raise ValueError("override %r is not KEY=VALUE" % (o,))
        node = {}
        cur = node
        parts = key.split(".")
        for p in parts[:-1]:
            cur[p] = {}
            cur = cur[p]
        cur[parts[-1]] = yaml.safe_load(val)
        update_config(cfg, node)
    return cfg
