"""Device times of the OHEM entries on their own, beside the bytes each one has to move, at the benchmark's
shape: N = 2 images, 2000 proposals + 100 ground-truth slots -> a pool of P = 2112 rows per image, R = 512 chosen, 81
classes, the box head's fused bf16 output of 448 columns. The pool is what the model builds: mxdet_proposal_target with
rois_per_image = P and fg_fraction = 1 on jittered ground-truth boxes and random boxes. Each entry is captured `reps` times
into a hipGraph and the replay is timed with device events (no launch gaps in the window); `rounds` repeats show the spread.

    python tools/bench_ohem.py [--reps 20] [--rounds 3]

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
    nbytes = float(nbytes)
    us = [round(graph_time(fn, args.reps), 2) for _ in range(args.rounds)]
    print(json.dumps(dict({"entry": name, "us": us, "bytes": int(nbytes), "GBps": round(nbytes / min(us) / 1e3, 1)}, **extra)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = "cuda"
    N, S, G, R, NC, LD, H, W = 2, 2000, 100, 512, 81, 448, 800, 1344
    D = 4 * NC
    P = B_.ohem_pool_size(S, G)
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
    t = lambda a: torch.from_numpy(a).to(dev)     # noqa: E731
    rois_d, gt_d = t(rois), t(gt)
    num_rois = torch.full((N,), S, dtype=torch.int32, device=dev)
    pool = lambda: B_.sample_rois(rois_d, num_rois, gt_d, P, 1.0, 0.5, 0.5, 0.0, NC, False, (0.0,) * 4, (0.1, 0.1, 0.2, 0.2), 99, 0, 0)  # noqa: E731
    p_rois, p_lab, p_tgt, p_wgt, p_m, p_nfg = pool()
    torch.cuda.synchronize()
    cand = int((p_lab >= 0).sum())
    # zero fill of targets and weights, then the rows
    report("proposal_target at rois_per_image = P (the pool)", pool, N * P * (2 * D * 4 + 5 * 4 + 8) + N * (S * 20 + G * 20), args,
           P=P, candidates=cand, foreground=int(p_nfg.sum()))
    o = (torch.randn((N * P, LD), device=dev) * 2).to(torch.bfloat16)
    score = torch.empty((N * P,), dtype=torch.float32, device=dev)
    head_bytes = cand * (NC + D) * 2
    report("ohem_roi_score smooth_l1", lambda: L_.ohem_roi_score(o, o[:, NC:], p_lab, NC, D, LD, LD, "smooth_l1", bbox_targets=p_tgt,
                                                                 bbox_weights=p_wgt, score=score),
           head_bytes + cand * 2 * D * 4 + N * P * 8, args)
    report("ohem_roi_score giou", lambda: L_.ohem_roi_score(o, o[:, NC:], p_lab, NC, D, LD, LD, "giou", rois=p_rois, matched_gt=p_m,
                                                            gt_boxes=gt_d, reg_weight=10.0, score=score),
           cand * NC * 2 + N * P * (8 + 20 + 4), args)
    L_.ohem_roi_score(o, o[:, NC:], p_lab, NC, D, LD, LD, "smooth_l1", bbox_targets=p_tgt, bbox_weights=p_wgt, score=score)
    sc = score.view(N, P)
    ws = B_.ohem_select_workspace(N, P, dev)
    sel = torch.empty((N, R), dtype=torch.int32, device=dev)
    num_sel, num_fg = torch.empty((N,), dtype=torch.int32, device=dev), torch.empty((N,), dtype=torch.int32, device=dev)
    words = (P + 63) // 64
    for thr in (0.7, 1.0):
        f = lambda thr=thr: B_.ohem_select(sc, p_lab, p_rois, R, thr, workspace=ws, sel=sel, num_sel=num_sel, num_fg=num_fg)  # noqa: E731
        f()
        torch.cuda.synchronize()
        # rank: score, labels, boxes in; order and sorted boxes out. NMS: the upper triangle of the suppression mask, written and read
        nbytes = N * P * (4 + 4 + 20 + 4 + 16) + (N * P * words * 8 if thr < 1.0 else 0) + N * (P * 8 + R * 4)
        report("ohem_select nms %.1f" % thr, f, nbytes, args, chosen=num_sel.tolist(), chosen_fg=num_fg.tolist())
    out = (torch.empty((N, R, 5), device=dev), torch.empty((N, R), dtype=torch.int32, device=dev), torch.empty((N, R, D), device=dev),
           torch.empty((N, R, D), device=dev), torch.empty((N, R), dtype=torch.int32, device=dev))
    report("ohem_gather", lambda: B_.ohem_gather(sel, p_rois, p_lab, p_m, p_tgt, p_wgt, out=out), N * R * (4 * D * 4 + 2 * 28 + 4), args)
    report("ohem_gather without targets / weights", lambda: B_.ohem_gather(sel, p_rois, p_lab, p_m, out=(out[0], out[1], None, None, out[4])),
           N * R * (2 * 28 + 4), args)


if __name__ == "__main__":
    main()
