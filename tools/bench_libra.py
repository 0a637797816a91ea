"""Device times of the Libra R-CNN entries on their own at the benchmark's shape: N = 2 images of 800 x 1344,
pyramid P2..P6 = 200x336, 100x168, 50x84, 25x42, 13x21 with 256 channels, refine level P4; 2000 proposals + 100 ground-truth
slots, 512 RoIs per image, 81 classes, the box head's fused bf16 output of 448 columns. The four Balanced Feature Pyramid
kernels stand beside their byte floor, the IoU-balanced sampler beside mxdet_proposal_target, and mxdet_rcnn_loss_balanced
beside mxdet_rcnn_loss. Each entry is captured `reps` times into a hipGraph and the replay is timed with device events (no
launch gaps in the window); `rounds` repeats show the spread.

    python tools/bench_libra.py [--reps 20] [--rounds 3]

One JSON line per entry: {"entry", "us" (per call, one value per round), "bytes", "GBps" (bytes over the best time)}.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxdetection_amd.core import bbox as B_   # noqa: E402
from mxdetection_amd.core import loss as L_   # noqa: E402
from mxdetection_amd.ops.bfp import BfpPlan   # noqa: E402


def graph_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps     # microseconds per call


def report(name, fn, nbytes, args, **extra):
    us = [round(graph_time(fn, args.reps), 2) for _ in range(args.rounds)]
    rec = {"entry": name, "us": us}
    if nbytes:
        rec.update(bytes=int(nbytes), GBps=round(float(nbytes) / min(us) / 1e3, 1))
    print(json.dumps(dict(rec, **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = "cuda"
    N, C, r = 2, 256, 2
    sizes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    shapes = [(N, h, w, C) for h, w in sizes]
    gen = torch.Generator().manual_seed(0)
    rnd = lambda s: torch.randn(s, generator=gen).to(torch.bfloat16).to(dev)     # noqa: E731
    P, dQ = [rnd(s) for s in shapes], [rnd(s) for s in shapes]
    Q, dP = [torch.empty_like(p) for p in P], [torch.empty_like(p) for p in P]
    Bm, Rf, dRf, dB = (torch.empty(shapes[r], dtype=torch.bfloat16, device=dev) for _ in range(4))
    Rf.copy_(rnd(shapes[r]))
    dB.copy_(rnd(shapes[r]))
    plan = BfpPlan(shapes, r, dev)
    pyr = sum(p.numel() for p in P) * 2                     # bytes of the pyramid
    ref = Bm.numel() * 2                                    # ... of one map on the refine level
    amax_g = sum(Bm.numel() for l in range(len(P)) if l < r)            # arg-maxima, one byte per pooled element
    amax_s = sum(P[l].numel() for l in range(len(P)) if l > r)
    report("bfp_gather_fwd", lambda: plan.gather_forward(P, Bm), pyr + ref + amax_g, args)
    report("bfp_scatter_fwd", lambda: plan.scatter_forward(P, Rf, Q), 2 * pyr + ref + amax_s, args)
    report("bfp_scatter_bwd", lambda: plan.scatter_backward(dQ, dRf), pyr + ref + amax_s, args)
    report("bfp_gather_bwd", lambda: plan.gather_backward(dQ, dB, dP), 2 * pyr + ref + amax_g, args)
    report("bfp_gather_bwd in place", lambda: plan.gather_backward(dQ, dB), 2 * pyr + ref + amax_g, args)

    # ---- sampler: jittered ground truth and random boxes, as tools/bench_ohem.py ----
    S, G, R, NC, LD, H, W = 2000, 100, 512, 81, 448, 800, 1344
    D = 4 * NC
    rng = np.random.default_rng(0)
    gt = -np.ones((N, G, 5), np.float32)
    rois = np.zeros((N, S, 5), np.float32)
    for n in range(N):
        for g in range(16):
            bw, bh = np.exp(rng.uniform(np.log(32), np.log(600))), np.exp(rng.uniform(np.log(32), np.log(500)))
            x1, y1 = rng.uniform(0, W - 1 - bw), rng.uniform(0, H - 1 - bh)
            gt[n, g] = (x1, y1, x1 + bw, y1 + bh, rng.integers(1, NC))
        near = gt[n, rng.integers(0, 16, S // 2), :4] + rng.uniform(-12, 12, (S // 2, 4))
        bw, bh = np.exp(rng.uniform(np.log(16), np.log(400), S - S // 2)), np.exp(rng.uniform(np.log(16), np.log(400), S - S // 2))
        x1, y1 = rng.uniform(0, W - 1 - bw), rng.uniform(0, H - 1 - bh)
        rois[n, :, 0] = n
        rois[n, :, 1:] = np.concatenate([near, np.stack([x1, y1, x1 + bw, y1 + bh], 1)])
    rois_d, gt_d = torch.from_numpy(rois).to(dev), torch.from_numpy(gt).to(dev)
    num_rois = torch.full((N,), S, dtype=torch.int32, device=dev)
    for bins in (None, 1, 3, 8):
        f = lambda bins=bins: B_.sample_rois(rois_d, num_rois, gt_d, R, 0.25, 0.5, 0.5, 0.0, NC, False, (0.0,) * 4,  # noqa: E731
                                             (0.1, 0.1, 0.2, 0.2), 99, 0, 0, num_bins=bins)
        out = f()
        torch.cuda.synchronize()
        report("proposal_target" if bins is None else "proposal_target_balanced, %d bins" % bins, f, 0, args,
               foreground=out[5].tolist(), background=[int((out[1][n] == 0).sum()) for n in range(N)])

    # ---- box-head loss ----
    out = B_.sample_rois(rois_d, num_rois, gt_d, R, 0.25, 0.5, 0.5, 0.0, NC, False, (0.0,) * 4, (0.1, 0.1, 0.2, 0.2), 99, 0, 0)
    labels, tgt, wgt = out[1], out[2], out[3]
    o = (torch.randn((N * R, LD), device=dev) * 2).to(torch.bfloat16)
    g = torch.zeros_like(o)
    loss = torch.zeros((2,), device=dev)
    ws = L_.loss_workspace(N * R, dev)
    nbytes = N * R * ((NC + D) * 2 * 2 + 2 * D * 4 + 4)
    report("rcnn_loss", lambda: L_.rcnn_loss(o, o[:, NC:], labels, tgt, wgt, NC, D, LD, LD, 1.0, 1.0 / (N * R), 1.0, g, g[:, NC:], loss,
                                             ws), nbytes, args)
    report("rcnn_loss_balanced", lambda: L_.rcnn_loss_balanced(o, o[:, NC:], labels, tgt, wgt, NC, D, LD, LD, 0.5, 1.5, 1.0, 1.0,
                                                               1.0 / (N * R), 1.0, g, g[:, NC:], loss, ws), nbytes, args)


if __name__ == "__main__":
    main()
