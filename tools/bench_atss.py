"""Cost of the ATSS assignment, alone and inside the RetinaNet step.

assign: mxdet_atss_assign beside mxdet_anchor_target in its RetinaNet setting (thresholds 0.5 / 0.4, no sampling) on the
same anchors -- N = 2 images of 800 x 1344, G_max = 100 with 8 and with 60 valid boxes, 9 anchors per cell (201,600) and
1 per cell (22,400). Device events around `iters` back-to-back calls after a warm-up; the variants alternate over `rounds`
rounds, so their spread is seen beside their difference. `--lib` takes mxdet_anchor_target from another build of the library
(the parent commit's), not from the code under test. Microseconds per call; the two ops do different work, so there is no
ratio to pass.

step: RetinaNet R101-FPN, batch 2, assigner atss against max_iou, both with 9 anchors per cell and smooth-L1, so the only
difference is the assignment; bench.py's synthetic batches and warm-up / capture / replay protocol, both models in this
process, `pairs` alternating timed windows of `steps` replayed steps each.

    python tools/bench_atss.py assign [--iters 200] [--warmup 20] [--rounds 3] [--lib PATH]
    python tools/bench_atss.py step [--steps 20] [--warmup 5] [--pairs 3]

One JSON line per shape (assign) or one line (step). Accuracy is not measured here or anywhere: there is no dataset.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IM_H, IM_W, G_MAX, STRIDES = 800, 1344, 100, (8, 16, 32, 64, 128)


def timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters     # microseconds


def boxes(rng, n_valid):
    """gt [2,100,5]: bench.py's box distribution (log-uniform sides 16..600 inside the image), n_valid rows per image."""
    gt = -np.ones((2, G_MAX, 5), np.float32)
    for n in range(2):
        for k in range(n_valid):
            w = min(float(np.exp(rng.uniform(np.log(16), np.log(600)))), IM_W - 1)
            h = min(float(np.exp(rng.uniform(np.log(16), np.log(600)))), IM_H - 1)
            x1, y1 = float(rng.uniform(0, IM_W - w)), float(rng.uniform(0, IM_H - h))
            gt[n, k] = [x1, y1, x1 + w - 1, y1 + h - 1, float(rng.integers(1, 81))]
    return gt


def bench_assign(args):
    import torch
    from mxdetection_amd import _lib
    from mxdetection_amd.core import anchor as A_
    lib = _lib.load()
    ref = lib
    if args.lib:      # the existing entry from another build, bound with this tree's signature table (the entry is unchanged)
        ref = C.CDLL(os.path.abspath(args.lib))
        for name in ("mxdet_anchor_target", "mxdet_anchor_target_workspace_bytes"):
            getattr(ref, name).restype, getattr(ref, name).argtypes = _lib.SIGNATURES[name]
    rng = np.random.default_rng(0)
    info = torch.tensor([[IM_H, IM_W, 1.0]] * 2, device="cuda")
    for per_cell, kw in ((9, dict(ratios=(0.5, 1.0, 2.0), scales=[4.0 * 2.0 ** (i / 3.0) for i in range(3)])),
                         (1, dict(ratios=(1.0,), scales=[8.0]))):
        levels, offs = [], [0]
        for s in STRIDES:
            H, W = -(-IM_H // s), -(-IM_W // s)
            base = torch.from_numpy(A_.generate_base_anchors(s, kw["ratios"], kw["scales"])).cuda()
            levels.append(A_.generate_anchors(base, H, W, s))
            offs.append(offs[-1] + levels[-1].shape[0])
        anchors = torch.cat(levels)
        At = anchors.shape[0]
        out = (torch.empty((2, At), dtype=torch.int32, device="cuda"), torch.empty((2, At), dtype=torch.int32, device="cuda"),
               torch.empty((2, At, 4), device="cuda"), torch.empty((2, At), device="cuda"))
        ws_atss = A_.AtssWorkspace(2, At, G_MAX, "cuda")
        nb = ref.mxdet_anchor_target_workspace_bytes(2, At, G_MAX)
        ws_ref = torch.empty((nb,), dtype=torch.uint8, device="cuda")
        for n_valid in (8, 60):
            gt = torch.from_numpy(boxes(rng, n_valid)).cuda()

            def max_iou():
                _lib.check(ref.mxdet_anchor_target(_lib.ptr(anchors), At, _lib.ptr(gt), 2, G_MAX, _lib.ptr(info), 0.5, 0.4, 1.0e6, 0,
                                                   0.5, 0, 0, None, 0, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]),
                                                   _lib.ptr(out[3]), _lib.ptr(ws_ref), nb, _lib.stream_ptr()), "anchor_target")

            def atss():
                A_.atss_assign(anchors, offs, gt, 9, ws_atss, out)

            fns = {"anchor_target_max_iou": max_iou, "atss_assign": atss}
            us = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    us[k].append(round(timed(fn, args.iters, args.warmup), 2))
            max_iou()
            torch.cuda.synchronize()
            fg_max_iou = int((out[0] == 1).sum())
            atss()
            torch.cuda.synchronize()
            print(json.dumps({"shape": "N=2 %dx%d G_max=%d valid=%d anchors=%d (%d per cell) topk=9" %
                              (IM_H, IM_W, G_MAX, n_valid, At, per_cell), "us_per_call": us,
                              "positives": {"anchor_target_max_iou": fg_max_iou, "atss_assign": int(out[0].sum())},
                              "anchor_target_from": args.lib or "this build"}), flush=True)


def bench_step(args):
    import torch
    from bench import BATCH_PER_GPU, synth_batch
    from mxdetection_amd.models import RetinaNet
    batches = [synth_batch(0, s, "cuda") for s in range(4)]
    lr = 0.02 * BATCH_PER_GPU / 16.0 / 3.0
    models = {}
    for name in ("max_iou", "atss"):
        m = RetinaNet("cuda", depth=101, seed=7, assigner=name)
        m.enable_wgrad_stream()
        m.enable_branch_stream()
        m.enable_grouped_wgrad()
        m.capture(*batches[0], lr=lr, image_offset=0)
        for i in range(args.warmup):
            m.replay(*batches[i % len(batches)], i)
        torch.cuda.synchronize()
        models[name] = m
    ms = {k: [] for k in models}
    losses = {}
    step = args.warmup
    for _ in range(args.pairs):
        for name, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                out = m.replay(*batches[(step + i) % len(batches)], step + i)
            torch.cuda.synchronize()
            ms[name].append(round(1e3 * (time.perf_counter() - t0) / args.steps, 3))
            losses[name] = [float(v) for v in torch.cat(list(out)).cpu().numpy()]
        step += args.steps
    print(json.dumps({"model": "RetinaNet R101-FPN, batch %d, 9 anchors per cell, smooth-L1" % BATCH_PER_GPU, "step_ms": ms,
                      "num_fg_last_step": {k: int(m.head.num_fg.item()) for k, m in models.items()}, "losses": losses}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("assign", "step"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=None, help="default: 20 calls (assign), 5 steps (step)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--lib", default="", help="another build of libmxdet_hip.so whose mxdet_anchor_target is timed (the parent commit's)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    if args.warmup is None:
        args.warmup = 20 if args.what == "assign" else 5
    (bench_assign if args.what == "assign" else bench_step)(args)


if __name__ == "__main__":
    main()
