"""Training throughput of Faster R-CNN R50-FPN with deformable convolutions in the backbone, one configuration per
process, on the synthetic batch and with the warm-up / capture / replay protocol of bench.py (2 images of 3x800x1333
padded to 1344, weight gradients grouped on a side stream, RPN branch on its own stream, whole step replayed).

    python tools/bench_dcn.py --dcn-stages 3,4,5 --modulated 1 --groups 1 --steps 30 --warmup 5
    python tools/bench_dcn.py --dcn-stages ''              # the plain model, same protocol
    python tools/bench_dcn.py --dcn-stages 3,4,5 --roi-pool mdpool     # + deformable RoI pooling in the box branch
    python tools/bench_dcn.py --dcn-stages '' --bbox-head 4conv1fc --head-norm gn     # the GN box head on the plain backbone
    python tools/bench_dcn.py --dcn-stages '' --mask 1 --bbox-head 4conv1fc --head-norm gn     # Mask R-CNN, GN in both heads
    python tools/bench_dcn.py --dcn-stages '' --reg-loss giou --reg-loss-weight 10     # GIoU loss on the decoded box in the box head
    python tools/bench_dcn.py --dcn-stages '' --mask 1 --mask-iou 1     # Mask Scoring R-CNN: the MaskIoU head on the mask branch
    python tools/bench_dcn.py --dcn-stages '' --ohem 1 --ohem-nms 0.7   # online hard example mining in the box head
    python tools/bench_dcn.py --dcn-stages '' --keypoints 1             # Keypoint R-CNN: the keypoint head beside the box head
    python tools/bench_dcn.py --dcn-stages '' --neck bfp --sampler iou_balanced --reg-loss balanced_l1     # Libra R-CNN
    python tools/bench_dcn.py --dcn-stages '' --neck bfp --bfp-refine embedded_gaussian --sampler iou_balanced --reg-loss balanced_l1     # ... with the paper's non-local refine
    python tools/bench_dcn.py --dcn-stages '' --fpn-upsample carafe     # CARAFE in the FPN's top-down path
    python tools/bench_dcn.py --dcn-stages '' --gcb-stages 3,4,5 --gcb-reduction 16     # GCNet's global context blocks in C3..C5

Prints one JSON line: {"dcn_stages", "modulated", "groups", "roi_pool", "mask", "mask_iou", "ohem", "keypoints", "neck", "bfp_refine", "fpn_upsample", "gcb_stages", "gcb_reduction", "sampler", "img_per_s", "step_ms", "losses"}.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dcn-stages", default="3,4,5", help="comma-separated subset of 3,4,5; empty = plain model")
    ap.add_argument("--modulated", type=int, default=1)
    ap.add_argument("--groups", type=int, default=1)
    ap.add_argument("--roi-pool", default="roi_align", choices=("roi_align", "dpool", "mdpool"))
    ap.add_argument("--bbox-head", default="2fc", choices=("2fc", "4conv1fc"))
    ap.add_argument("--head-norm", default="none", choices=("none", "gn"))
    ap.add_argument("--gn-groups", type=int, default=32)
    ap.add_argument("--reg-loss", default="smooth_l1", choices=("smooth_l1", "iou", "giou", "diou", "balanced_l1"))
    ap.add_argument("--reg-loss-weight", type=float, default=1.0)
    ap.add_argument("--mask", type=int, default=0, help="1 = Mask R-CNN (ground-truth masks: an ellipse in every box, as bench.py)")
    ap.add_argument("--mask-iou", type=int, default=0, help="1 = Mask Scoring R-CNN's MaskIoU head (needs --mask 1)")
    ap.add_argument("--mask-iou-weight", type=float, default=1.0)
    ap.add_argument("--ohem", type=int, default=0, choices=(0, 1), help="1 = online hard example mining in the box head")
    ap.add_argument("--ohem-nms", type=float, default=0.7, help="dedup IoU of --ohem 1, in (0, 1]; 1 = none")
    ap.add_argument("--keypoints", type=int, default=0, choices=(0, 1),
                    help="1 = Keypoint R-CNN's keypoint head (ground-truth keypoints: 17 points inside every box)")
    ap.add_argument("--neck", default="fpn", choices=("fpn", "bfp"), help="bfp = Balanced Feature Pyramid behind the FPN")
    ap.add_argument("--bfp-refine", default="conv", choices=("conv", "none", "embedded_gaussian"),
                    help="embedded_gaussian = the non-local block on the attention entries")
    ap.add_argument("--bfp-nl-reduction", type=int, default=2, choices=(2, 4))
    ap.add_argument("--bfp-nl-use-scale", type=int, default=0, choices=(0, 1))
    ap.add_argument("--fpn-upsample", default="nearest", choices=("nearest", "carafe"),
                    help="carafe = CARAFE in the FPN's top-down path (k 5, compressor 64, encoder 3 x 3)")
    ap.add_argument("--gcb-stages", default="", help="comma-separated subset of 3,4,5 whose bottlenecks get a global context block")
    ap.add_argument("--gcb-reduction", type=int, default=16, help="inner width of the blocks = C / reduction (published: 16, 4)")
    ap.add_argument("--sampler", default="random", choices=("random", "iou_balanced"))
    ap.add_argument("--sampler-bins", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.mask_iou and not args.mask:
        ap.error("--mask-iou 1 needs --mask 1: the MaskIoU head scores the mask head's output")
    import torch
    from bench import BATCH_PER_GPU, IM_H, PAD_W, synth_batch
    from mxdetection_amd.models import FasterRCNN
    stages = tuple(int(s) for s in args.dcn_stages.split(",") if s.strip())
    gcb_stages = tuple(int(s) for s in args.gcb_stages.split(",") if s.strip())
    device = "cuda"
    model = FasterRCNN(device, depth=50, seed=7, dcn_stages=stages, dcn_modulated=bool(args.modulated),
                       dcn_groups=args.groups, roi_pool=args.roi_pool, bbox_head=args.bbox_head,
                       head_norm=args.head_norm, gn_groups=args.gn_groups, with_mask=bool(args.mask),
                       reg_loss=args.reg_loss, reg_loss_weight=args.reg_loss_weight, mask_iou=bool(args.mask_iou),
                       mask_iou_weight=args.mask_iou_weight, ohem=bool(args.ohem), ohem_nms=args.ohem_nms,
                       with_keypoints=bool(args.keypoints), neck=args.neck, bfp_refine=args.bfp_refine, sampler=args.sampler,
                       sampler_bins=args.sampler_bins, bfp_nl_reduction=args.bfp_nl_reduction,
                       bfp_nl_use_scale=bool(args.bfp_nl_use_scale), fpn_upsample=args.fpn_upsample,
                       gcb_stages=gcb_stages, gcb_reduction=args.gcb_reduction)
    model.enable_wgrad_stream()
    model.enable_branch_stream()
    model.enable_grouped_wgrad()
    lr = 0.02 * BATCH_PER_GPU / 16.0 / 3.0
    batches = [synth_batch(0, s, device) for s in range(4)]
    masks = [None] * len(batches)
    if args.mask:   # filled ellipse inside every GT box, [N,16,H,W] u8 (GT rows 0..15 are the valid ones)
        yy = torch.arange(IM_H, device=device).view(1, 1, IM_H, 1).float()
        xx = torch.arange(PAD_W, device=device).view(1, 1, 1, PAD_W).float()
        for k, (_, gt, _) in enumerate(batches):
            b = gt[:, :16]
            cx, cy = 0.5 * (b[..., 0] + b[..., 2]), 0.5 * (b[..., 1] + b[..., 3])
            rx, ry = 0.5 * (b[..., 2] - b[..., 0]) + 0.5, 0.5 * (b[..., 3] - b[..., 1]) + 0.5
            m = (((xx - cx[..., None, None]) / rx[..., None, None]) ** 2 +
                 ((yy - cy[..., None, None]) / ry[..., None, None]) ** 2) <= 1.0
            masks[k] = (m & (b[..., 4] >= 0)[..., None, None]).to(torch.uint8).contiguous()
    kps = [{}] * len(batches)
    if args.keypoints:   # 17 labelled points inside every GT box (GT rows 0..15 are the valid ones), zeros on padding rows
        gen = torch.Generator().manual_seed(17)
        kps = []
        for _, gt, _ in batches:
            b = gt[:, :16]
            u = torch.rand((b.shape[0], 16, 17, 2), generator=gen).to(device) * 0.8 + 0.1
            kp = torch.ones((b.shape[0], 16, 17, 3), device=device)
            kp[..., 0] = b[..., None, 0] + u[..., 0] * (b[..., None, 2] - b[..., None, 0])
            kp[..., 1] = b[..., None, 1] + u[..., 1] * (b[..., None, 3] - b[..., None, 1])
            kps.append({"gt_keypoints": (kp * (b[..., 4] >= 0)[..., None, None]).contiguous()})
    model.capture(*batches[0], lr=lr, image_offset=0, gt_masks=masks[0], **kps[0])
    for i in range(args.warmup):
        img, gt, info = batches[i % len(batches)]
        model.replay(img, gt, info, i, gt_masks=masks[i % len(batches)], **kps[i % len(batches)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        img, gt, info = batches[(args.warmup + i) % len(batches)]
        losses = model.replay(img, gt, info, args.warmup + i, gt_masks=masks[(args.warmup + i) % len(batches)],
                              **kps[(args.warmup + i) % len(batches)])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    vals = [float(v) for v in torch.cat(list(losses)).cpu().numpy()]
    print(json.dumps({"dcn_stages": list(stages), "modulated": bool(args.modulated), "groups": args.groups,
                      "roi_pool": args.roi_pool, "mask": bool(args.mask), "mask_iou": bool(args.mask_iou), "ohem": bool(args.ohem), "keypoints": bool(args.keypoints), "neck": args.neck, "bfp_refine": args.bfp_refine, "fpn_upsample": args.fpn_upsample, "gcb_stages": list(gcb_stages), "gcb_reduction": args.gcb_reduction, "sampler": args.sampler, "bbox_head": args.bbox_head, "head_norm": args.head_norm,
                      "reg_loss": args.reg_loss,
                      "img_per_s": round(BATCH_PER_GPU * args.steps / dt, 2),
                      "step_ms": round(1e3 * dt / args.steps, 3), "losses": vals}), flush=True)


if __name__ == "__main__":
    main()
