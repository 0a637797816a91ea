"""Device times of the three Keypoint R-CNN entries on their own, beside the bytes each one has to move, at
the benchmark's shape: R = 256 keypoint rois, S_in = 28, Kpad = 32, K = 17, every (roi, keypoint) valid. Each entry is
captured `reps` times into a hipGraph and the replay is timed with device events (no launch gaps in the window); `rounds`
repeats show the spread. The loss is timed a second time with three rois in four untrained (the usual share of background
rows among the 128 slots per image: those rows write zeros and read nothing).

    python tools/bench_keypoint.py [--reps 20] [--rounds 3]

One JSON line per entry: {"entry", "us" (per call, one value per round), "bytes" (the floor: for the loss the logits read plus
the gradient write), "GBps" (bytes over the best time)}.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxdetection_amd.core import mask as M_   # noqa: E402


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
    N, G, R, S_in, Kpad, K = 2, 16, 256, 28, 32, 17
    rng = np.random.default_rng(0)
    rois = np.zeros((R, 5), np.float32)
    gt_kp = np.zeros((N, G, K, 3), np.float32)
    box = np.zeros((N, G, 4), np.float32)
    for n in range(N):
        for g in range(G):
            bw, bh = np.exp(rng.uniform(np.log(32), np.log(600))), np.exp(rng.uniform(np.log(32), np.log(500)))
            x1, y1 = rng.uniform(0, 1343 - bw), rng.uniform(0, 799 - bh)
            box[n, g] = (x1, y1, x1 + bw, y1 + bh)
            u = rng.uniform(0.1, 0.9, (K, 2))
            gt_kp[n, g, :, 0], gt_kp[n, g, :, 1], gt_kp[n, g, :, 2] = x1 + u[:, 0] * bw, y1 + u[:, 1] * bh, 2
    matched = rng.integers(0, G, R).astype(np.int32)
    for r in range(R):
        n = r * N // R
        rois[r] = (n, *(box[n, matched[r]] + rng.uniform(-2, 2, 4)))
    t = lambda a: torch.from_numpy(a).to(dev)     # noqa: E731
    rois_d, matched_d, kp_d = t(rois), t(matched), t(gt_kp)
    labels = torch.ones((R,), dtype=torch.int32, device=dev)
    tg = torch.empty((R, K), dtype=torch.int32, device=dev)
    report("keypoint_target", lambda: M_.keypoint_target(rois_d, matched_d, labels, kp_d, S_in, out=tg),
           R * (5 * 4 + 8) + R * K * (12 + 4), args)
    valid = int((tg >= 0).sum())
    logits = (torch.randn((R, S_in, S_in, Kpad), device=dev) * 2).to(torch.bfloat16)
    grad = torch.empty_like(logits)
    loss = torch.zeros((1,), device=dev)
    ws = M_.keypoint_loss_workspace(R, dev)
    block = S_in * S_in * Kpad * 2
    report("keypoint_loss", lambda: M_.keypoint_loss(logits, tg, loss, grad, ws), R * 2 * block + R * K * 4, args,
           valid_rows=valid, softmax_elements=valid * 4 * S_in * S_in)
    sparse = tg.clone()
    sparse[torch.arange(R, device=dev) % 4 != 0] = -1
    report("keypoint_loss, 1 roi in 4 trained", lambda: M_.keypoint_loss(logits, sparse, loss, grad, ws),
           (R // 4) * block + R * block + R * K * 4, args, valid_rows=int((sparse >= 0).sum()))
    dets = torch.zeros((R, 6), device=dev)
    dets[:, :4] = rois_d[:, 1:]
    dets[:, 4], dets[:, 5] = 0.9, 1.0
    out = torch.empty((R, K, 3), dtype=torch.float32, device=dev)
    report("keypoint_decode", lambda: M_.keypoint_decode(logits, dets, K, out=out), R * block + R * (24 + K * 12), args)


if __name__ == "__main__":
    main()
