"""Config -> detector (the README's "Modular Design" -- a model is a choice of backbone,
neck, heads named in an experiment file, /root/reference/README.md:7,13)."""


def build_detector(cfg, device="cuda"):
    from . import FasterRCNN, RetinaNet
    net, tr = cfg.network, cfg.TRAIN
    dcn = dict(dcn_stages=tuple(net.dcn_stages), dcn_modulated=bool(net.dcn_modulated), dcn_groups=int(net.dcn_groups),
               gcb_stages=tuple(net.gcb_stages), gcb_reduction=net.gcb_reduction)
    reg = dict(reg_loss=str(net.reg_loss), reg_loss_weight=net.reg_loss_weight)
    if net.type in ("faster_rcnn", "mask_rcnn"):
        if net.cls_loss != "focal":
            raise ValueError("network.cls_loss = %r: %s keeps softmax cross-entropy (qfl / vfl are retinanet options)"
                             % (net.cls_loss, net.type))
        if net.reg_max != 0:
            raise ValueError("network.reg_max = %r: %s regresses plain deltas (the distribution box head is a retinanet "
                             "option)" % (net.reg_max, net.type))
        if net.assigner != "max_iou":
            raise ValueError("network.assigner = %r: %s keeps the RPN's sampler (atss is a retinanet option)"
                             % (net.assigner, net.type))
        if net.ghm != "none":
            raise ValueError("network.ghm = %r: %s keeps its RPN and box-head losses (gradient harmonizing is a retinanet "
                             "option)" % (net.ghm, net.type))
        if net.mask_iou and net.type != "mask_rcnn":
            raise ValueError("network.mask_iou = %r: %s has no mask branch to score (the MaskIoU head is a mask_rcnn option)"
                             % (net.mask_iou, net.type))
        if net.keypoints not in (0, 1, False, True):
            raise ValueError("network.keypoints must be 0 or 1 (got %r)" % (net.keypoints,))
        kpt = dict(with_keypoints=bool(net.keypoints), num_keypoints=net.num_keypoints, keypoint_weight=net.keypoint_weight)
        dpool = dict(roi_pool=str(net.roi_pool), dpool_trans_std=float(net.dpool_trans_std),
                     dpool_sample_per_part=int(net.dpool_sample_per_part), dpool_offset_fcs=int(net.dpool_offset_fcs))
        heads = dict(bbox_head=str(net.bbox_head), head_norm=str(net.head_norm), gn_groups=net.gn_groups)
        libra = dict(neck=str(net.neck), bfp_refine=str(net.bfp_refine), sampler=str(net.sampler), sampler_bins=net.sampler_bins,
                     bl1_alpha=net.bl1_alpha, bl1_gamma=net.bl1_gamma, bl1_beta=net.bl1_beta,
                     bfp_nl_reduction=net.bfp_nl_reduction, bfp_nl_use_scale=net.bfp_nl_use_scale)
        carafe = dict(fpn_upsample=str(net.fpn_upsample), carafe_k=net.carafe_k, carafe_compress=net.carafe_compress,
                      carafe_enc_kernel=net.carafe_enc_kernel)
        model = FasterRCNN(device, depth=net.backbone_depth, num_classes=net.num_classes, seed=net.seed,
                           rois_per_image=tr.batch_rois, pre_nms_top_n=tr.rpn_pre_nms_top_n,
                           post_nms_top_n=tr.rpn_post_nms_top_n, with_mask=(net.type == "mask_rcnn"), **dcn, **dpool, **heads,
                           **reg, mask_iou=bool(net.mask_iou), mask_iou_weight=net.mask_iou_weight, ohem=bool(net.ohem),
                           ohem_nms=net.ohem_nms, **kpt, **libra, **carafe)
    elif net.type == "retinanet":
        if net.ohem:
            raise ValueError("network.ohem = %r: retinanet has no box head to mine RoIs for (OHEM is a faster_rcnn / mask_rcnn "
                             "option)" % (net.ohem,))
        if net.keypoints:
            raise ValueError("network.keypoints = %r: retinanet has no RoI branch to put a keypoint head on (Keypoint R-CNN is "
                             "a faster_rcnn / mask_rcnn option)" % (net.keypoints,))
        if net.mask_iou:
            raise ValueError("network.mask_iou = %r: retinanet has no mask branch to score (the MaskIoU head is a mask_rcnn "
                             "option)" % (net.mask_iou,))
        if net.roi_pool != "roi_align":
            raise ValueError("network.roi_pool = %r: retinanet has no RoI branch" % (net.roi_pool,))
        if net.neck != "fpn":
            raise ValueError("network.neck = %r: retinanet keeps its own pyramid (the Balanced Feature Pyramid is a "
                             "faster_rcnn / mask_rcnn option)" % (net.neck,))
        if net.bfp_nl_reduction != 2 or net.bfp_nl_use_scale:
            raise ValueError("network.bfp_nl_reduction / network.bfp_nl_use_scale = %r / %r: retinanet has no Balanced Feature "
                             "Pyramid to refine (faster_rcnn / mask_rcnn options)" % (net.bfp_nl_reduction, net.bfp_nl_use_scale))
        if net.fpn_upsample != "nearest":
            raise ValueError("network.fpn_upsample = %r: retinanet keeps its own pyramid, whose top-down path upsamples "
                             "nearest-neighbour (CARAFE is a faster_rcnn / mask_rcnn option)" % (net.fpn_upsample,))
        if net.sampler != "random":
            raise ValueError("network.sampler = %r: retinanet has no RoI sampler (iou_balanced is a faster_rcnn / mask_rcnn "
                             "option)" % (net.sampler,))
        if net.reg_loss == "balanced_l1":
            raise ValueError("network.reg_loss = 'balanced_l1': Balanced L1 is the R-CNN box head's loss (retinanet keeps "
                             "smooth_l1 | iou | giou | diou)")
        if net.bbox_head != "2fc" or net.head_norm != "none":
            raise ValueError("network.bbox_head / network.head_norm: retinanet has no RoI heads")
        model = RetinaNet(device, depth=net.backbone_depth, num_classes=net.num_classes - 1, seed=net.seed, **dcn, **reg,
                          assigner=str(net.assigner), atss_topk=net.atss_topk, anchor_ratios=tuple(net.anchor_ratios),
                          anchor_scales_per_octave=net.anchor_scales_per_octave, anchor_scale=float(net.anchor_scale),
                          cls_loss=str(net.cls_loss), cls_loss_alpha=net.cls_loss_alpha, cls_loss_gamma=net.cls_loss_gamma,
                          reg_max=net.reg_max, dfl_weight=net.dfl_weight, ghm=str(net.ghm), ghm_cls_bins=net.ghm_cls_bins,
                          ghm_cls_momentum=net.ghm_cls_momentum, ghm_cls_weight=net.ghm_cls_weight,
                          ghm_reg_bins=net.ghm_reg_bins, ghm_reg_momentum=net.ghm_reg_momentum, ghm_reg_mu=net.ghm_reg_mu,
                          ghm_reg_weight=net.ghm_reg_weight)
    else:
        raise ValueError("unknown network.type %r" % (net.type,))
    if net.pretrained:
        from ..utils import load_pretrained_backbone
        load_pretrained_backbone(model, net.pretrained, depth=net.backbone_depth)
    return model


def build_loader(cfg, device="cuda", rank=0, world=1, train=True, with_masks=None):
    """Config -> (roidb, class names, DetectionLoader). With network.keypoints the roidb carries keypoints and training
    batches carry gt_keypoints."""
    import numpy as np
    from ..datasets import append_flipped, filter_roidb, load_coco_roidb, synthetic_roidb
    from ..datasets.loader import DetectionLoader
    from ..datasets.synthetic import synthetic_reader
    from ..process_data import BatchPreprocessor
    ds = cfg.dataset
    kpt = bool(cfg.network.keypoints)
    if ds.type == "synthetic":
        roidb = synthetic_roidb(ds.num_images, seed=1, num_classes=cfg.network.num_classes - 1,
                                num_keypoints=int(cfg.network.num_keypoints) if kpt else 0)
        names, reader = None, synthetic_reader
    elif ds.type == "coco":
        roidb, names = load_coco_roidb(ds.ann_file, ds.image_dir, with_keypoints=kpt)
        # frames are stored as uint8 [h,w,3] .npy arrays next to / instead of the JPEGs (no decoder in the image)
        reader = lambda e: np.load(e["image"] if e["image"].endswith(".npy") else e["image"].rsplit(".", 1)[0] + ".npy")  # noqa: E731
    elif ds.type == "voc":
        from ..datasets import load_voc_roidb
        roidb, names = load_voc_roidb(ds.ann_file, image_dir=ds.image_dir)       # ann_file = the Annotations directory
        reader = lambda e: np.load(e["image"].rsplit(".", 1)[0] + ".npy")  # noqa: E731
    else:
        raise ValueError("unknown dataset.type %r" % (ds.type,))
    if train:
        roidb = filter_roidb(roidb)
        if cfg.TRAIN.flip:
            roidb = append_flipped(roidb)
    fixed = tuple(ds.fixed_shape) if ds.fixed_shape else None
    pre = BatchPreprocessor(ds.target_size, ds.max_size, ds.pixel_means, ds.pixel_stds, ds.swap_rb,
                            pad_to=fixed, fit_inside=fixed is not None)
    tr = cfg.TRAIN
    loader = DetectionLoader(roidb, tr.batch_images if train else cfg.TEST.batch_images, device=device, rank=rank, world=world,
                             reader=reader, preprocessor=pre, g_max=ds.max_gt,
                             with_masks=(train and cfg.network.type == "mask_rcnn") if with_masks is None else with_masks,
                             shuffle=train and tr.shuffle, aspect_grouping=train and tr.aspect_grouping, seed=tr.seed,
                             with_keypoints=train and kpt, num_keypoints=int(cfg.network.num_keypoints))
    return roidb, names, loader
