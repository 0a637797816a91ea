"""Cost of the distribution box head (integral decode + DFL), modelled on tools/bench_quality_loss.py. Two modes.

level (default): mxdet_retina_loss_level_dfl (reg_max 16, 128 box channels) beside mxdet_retina_loss_level_quality (4 deltas, 64
box channels) on the five RetinaNet levels of the benchmark input (2 x 800 x 1344, 80 classes, one anchor per cell, QFL +
GIoU, one finalize). With --lib PATH a third column is the `_quality` entry of THAT library (the parent commit's build): it
must sit where this tree's does. Device events around `iters` back-to-back calls after a warm-up; the entries alternate over
`rounds` rounds, so their spread is seen beside their difference. One JSON line.

step: RetinaNet R101-FPN with ATSS + QFL + GIoU at reg_max 0 against reg_max 16, bench.py's protocol -- its synthetic
batches, capture, warm-up, timed replays, images/s from the wall clock after a device drain -- both models in one process,
alternating over `rounds` rounds. One JSON line.

    python tools/bench_dfl.py [--mode level|step] [--lib parent/libmxdet_hip.so] [--reg-max 16] [--kind giou]
                              [--iters 200] [--warmup 20] [--rounds 3] [--steps 20] [--step-warmup 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_iou_loss import G_MAX, RETINA_LEVELS, boxes_near, ground_truth, rounds_of   # noqa: E402
from mxdetection_amd import _lib   # noqa: E402
from mxdetection_amd.core import loss as L   # noqa: E402
from mxdetection_amd._lib import ptr, stream_ptr   # noqa: E402

STRIDES = (8, 16, 32, 64, 128)
ATSS_QFL = dict(assigner="atss", anchor_ratios=(1.0,), anchor_scales_per_octave=1, anchor_scale=8.0, reg_loss_weight=2.0,
                cls_loss="qfl")


def other_library(path):
    """The `_quality` entry and finalize of another build of the library, bound with this tree's signatures."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("mxdet_retina_loss_level_quality", "mxdet_loss_finalize", "mxdet_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def bench_level(args, g):
    N, C, A, R = 2, 80, 1, args.reg_max
    ldc, ldr, ldd = (A * C + 63) // 64 * 64, (A * 4 + 63) // 64 * 64, (A * 4 * (R + 1) + 63) // 64 * 64
    offs = [0]
    for h, w in RETINA_LEVELS:
        offs.append(offs[-1] + h * w * A)
    At = offs[-1]
    gt = ground_truth(N, g)
    near = torch.arange(At) % G_MAX
    anchors = boxes_near(gt[0, near, :4], g).cuda().contiguous()
    matched = near.int().repeat(N, 1).cuda().contiguous()
    fg = torch.rand((N, At), generator=g) < 0.002 * 9 / A                             # ~400 foreground anchors, as bench_iou_loss
    cls_labels = torch.where(fg, gt[torch.arange(N)[:, None], near[None], 4].int(), torch.zeros((N, At), dtype=torch.int32)).cuda()
    num_fg = fg.sum().int().view(1).cuda()
    gt = gt.cuda().contiguous()
    co = [(torch.randn((N, h, w, ldc), generator=g) - 4.0).to(torch.bfloat16).cuda() for h, w in RETINA_LEVELS]
    bo = [(torch.randn((N, h, w, ldr), generator=g) * 0.3).to(torch.bfloat16).cuda() for h, w in RETINA_LEVELS]
    do = [torch.randn((N, h, w, ldd), generator=g).to(torch.bfloat16).cuda() for h, w in RETINA_LEVELS]
    gc, gb, gd = [torch.zeros_like(x) for x in co], [torch.zeros_like(x) for x in bo], [torch.zeros_like(x) for x in do]
    nparts = [L.retina_loss_num_partials(N, h, w, A) for h, w in RETINA_LEVELS]
    partial, loss = torch.zeros(3 * sum(nparts), device="cuda"), torch.zeros(3, device="cuda")
    other = other_library(args.lib) if args.lib else None
    kind = L.IOU_LOSS_KINDS[args.kind]

    def run(which):
        off = 0
        for l, (h, w) in enumerate(RETINA_LEVELS):
            if which == "dfl":
                L.retina_loss_level_dfl(co[l], do[l], A, C, cls_labels, anchors, matched, gt, offs[l], "qfl", 0.0, 2.0, args.kind, R,
                                        float(STRIDES[l]), 2.0, 0.25, num_fg, 1.0, gc[l], gd[l], partial[3 * off:])
            elif which == "quality":
                L.retina_loss_level_quality(co[l], bo[l], A, C, cls_labels, anchors, matched, gt, offs[l], "qfl", 0.0, 2.0, args.kind,
                                            (1.0, 1.0, 1.0, 1.0), 2.0, num_fg, 1.0, gc[l], gb[l], partial[2 * off:])
            else:
                rc = other.mxdet_retina_loss_level_quality(ptr(co[l]), ptr(bo[l]), N, h, w, A, C, ldc, ldr, ptr(cls_labels), ptr(anchors),
                                                           ptr(matched), ptr(gt), G_MAX, At, offs[l], 1, 0.0, 2.0, kind, 1.0, 1.0, 1.0, 1.0,
                                                           2.0, ptr(num_fg), 1.0, ptr(gc[l]), ptr(gb[l]), ptr(partial[2 * off:]),
                                                           stream_ptr())
                assert rc == 0, other.mxdet_last_error()
            off += nparts[l]
        L.loss_finalize(partial, off, 3 if which == "dfl" else 2, loss)
    fns = {"quality": lambda: run("quality"), "dfl": lambda: run("dfl")}
    if other is not None:
        fns = {"quality_other_lib": lambda: run("other"), **fns}
    t = rounds_of(fns, args)
    best = {k: min(v) for k, v in t.items()}
    print(json.dumps({"shape": "retinanet 5 levels of 2x800x1344, A=%d C=%d, %d anchors, reg_max %d (%d box channels)"
                               % (A, C, N * At, R, ldd), "box": args.kind, "us_per_call": t,
                      "dfl_over_quality": round(best["dfl"] / best["quality"], 4)}), flush=True)


def bench_step(args):
    import bench
    from mxdetection_amd.models import RetinaNet
    lr = 0.02 * bench.BATCH_PER_GPU / 16.0 / 3.0
    batches = [bench.synth_batch(0, s, "cuda") for s in range(4)]
    models = {}
    for k in (0, args.reg_max):
        m = RetinaNet("cuda", depth=101, seed=7, reg_loss=args.kind, reg_max=k, **ATSS_QFL)
        m.enable_wgrad_stream()
        m.enable_branch_stream()
        m.enable_grouped_wgrad()
        m.capture(*batches[0], lr=lr, image_offset=0)
        models["reg_max_%d" % k] = m
    out = {k: [] for k in models}
    losses = {}
    for _ in range(args.rounds):
        for k, m in models.items():
            for i in range(args.step_warmup):
                m.replay(*batches[i % 4], i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                last = m.replay(*batches[(args.step_warmup + i) % 4], args.step_warmup + i)
            torch.cuda.synchronize()
            out[k].append(round(args.steps * bench.BATCH_PER_GPU / (time.perf_counter() - t0), 3))
            losses[k] = [round(float(v), 6) for v in torch.cat(list(last)).cpu().numpy()]
    a, b = "reg_max_0", "reg_max_%d" % args.reg_max
    print(json.dumps({"model": "retinanet r101-fpn, atss + qfl + %s, 2 x 800 x 1344" % args.kind, "images_per_sec": out, "losses": losses,
                      "dfl_over_plain": round(max(out[b]) / max(out[a]), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="level", choices=("level", "step"))
    ap.add_argument("--lib", default=None, help="level mode: another build of libmxdet_hip.so for a second _quality column (the parent commit's)")
    ap.add_argument("--reg-max", type=int, default=16)
    ap.add_argument("--kind", default="giou", choices=tuple(L.IOU_LOSS_KINDS))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    L.check_reg_max(args.reg_max, args.kind)
    assert args.reg_max > 0, "--reg-max must be positive: the comparison is against reg_max 0"
    if args.mode == "step":
        bench_step(args)
        return
    bench_level(args, torch.Generator().manual_seed(0))


if __name__ == "__main__":
    main()
