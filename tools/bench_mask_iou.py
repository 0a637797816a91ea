"""Device times of the five Mask Scoring R-CNN entries on their own, beside the bytes each one has to move, at
the benchmark's shape: R = 256 mask rois, S = 28, 128 logit channels, ground-truth masks [2,16,800,1344] u8 (an ellipse in
every box), rois = jittered ground-truth boxes. Each entry is captured `reps` times into a hipGraph and the replay is timed
with device events (no launch gaps in the window); `rounds` repeats show the spread. The target entry is timed twice more:
with every roi a padding row (what is left is the whole-instance area pass: ~1 MB per valid instance) and with rois that
cover the whole frame (the in-box count at its largest).

    python tools/bench_mask_iou.py [--reps 20] [--rounds 3]

One JSON line per entry: {"entry", "us" (per call, one value per round), "bytes", "GBps" (bytes over the best time)}.
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
    N, G, H, W, R, S, Cpad, C = 2, 16, 800, 1344, 256, 28, 128, 256
    h = S // 2
    rng = np.random.default_rng(0)
    gt = np.zeros((N, G, 5), np.float32)
    for n in range(N):
        for g in range(G):
            bw, bh = np.exp(rng.uniform(np.log(32), np.log(600))), np.exp(rng.uniform(np.log(32), np.log(500)))
            x1, y1 = rng.uniform(0, W - 1 - bw), rng.uniform(0, H - 1 - bh)
            gt[n, g] = (x1, y1, x1 + bw, y1 + bh, rng.integers(1, 81))
    b = torch.from_numpy(gt).to(dev)
    yy = torch.arange(H, device=dev).view(1, 1, H, 1).float()
    xx = torch.arange(W, device=dev).view(1, 1, 1, W).float()
    cx, cy = 0.5 * (b[..., 0] + b[..., 2]), 0.5 * (b[..., 1] + b[..., 3])
    rx, ry = 0.5 * (b[..., 2] - b[..., 0]) + 0.5, 0.5 * (b[..., 3] - b[..., 1]) + 0.5
    masks = ((((xx - cx[..., None, None]) / rx[..., None, None]) ** 2 +
              ((yy - cy[..., None, None]) / ry[..., None, None]) ** 2) <= 1.0).to(torch.uint8).contiguous()
    rois = np.zeros((R, 5), np.float32)
    matched = np.zeros((R,), np.int32)
    labels = np.zeros((R,), np.int32)
    for r in range(R):
        n, g = r * N // R, int(rng.integers(0, G))
        rois[r] = (n, *(gt[n, g, :4] + rng.uniform(-8, 8, 4)))
        matched[r], labels[r] = g, int(gt[n, g, 4])
    box_bytes = int(sum((min(W - 1, np.ceil(q[3])) - max(0, np.floor(q[1])) + 1) * (min(H - 1, np.ceil(q[4])) - max(0, np.floor(q[2])) + 1)
                        for q in rois))
    t = lambda a: torch.from_numpy(a).to(dev)     # noqa: E731
    rois_d, matched_d, labels_d = t(rois), t(matched), t(labels)
    tg, cls = M_.mask_target(rois_d, matched_d, labels_d, masks, S)
    logits = (torch.randn((R, S, S, Cpad), device=dev) * 2).to(torch.bfloat16)
    ws = M_.maskiou_target_workspace(N, G, dev)
    out_t = torch.empty((R,), dtype=torch.float32, device=dev)
    roi_bytes = R * (S * S * 2 + S * S + 5 * 4 + 12)
    area_bytes = N * G * H * W
    M_.maskiou_target(rois_d, matched_d, cls, b, masks, logits, tg, out=out_t, workspace=ws)
    report("maskiou_target", lambda: M_.maskiou_target(rois_d, matched_d, cls, b, masks, logits, tg, out=out_t, workspace=ws),
           area_bytes + box_bytes + roi_bytes, args, area_bytes=area_bytes, in_box_bytes=int(box_bytes), valid_instances=N * G,
           mean_target=round(float(out_t.mean()), 4))
    none = torch.full((R,), -1, dtype=torch.int32, device=dev)
    report("maskiou_target, every roi padding (area pass)", lambda: M_.maskiou_target(rois_d, none, none, b, masks, logits, tg,
                                                                                      out=out_t, workspace=ws),
           area_bytes, args, valid_instances=N * G, bytes_per_instance=H * W)
    full = rois_d.clone()
    full[:, 1:] = torch.tensor([0.0, 0.0, W - 1.0, H - 1.0], device=dev)
    report("maskiou_target, whole-frame rois", lambda: M_.maskiou_target(full, matched_d, cls, b, masks, logits, tg, out=out_t,
                                                                         workspace=ws),
           area_bytes + R * H * W + roi_bytes, args)
    mpooled = torch.randn((R, h, h, C), device=dev).to(torch.bfloat16)
    x = torch.empty((R, h, h, M_.MASKIOU_CIN), dtype=torch.bfloat16, device=dev)
    report("maskiou_input", lambda: M_.maskiou_input(mpooled, logits, cls, out=x),
           R * h * h * (C * 2 + M_.MASKIOU_CIN * 2) + R * S * S * 2, args)
    d_in = torch.randn((R, h, h, M_.MASKIOU_CIN), device=dev).to(torch.bfloat16)
    d_mp = torch.zeros((R, h, h, C), dtype=torch.bfloat16, device=dev)
    report("maskiou_input_bwd", lambda: M_.maskiou_input_bwd(d_in, d_mp), R * h * h * C * 2 * 3, args)
    pred = torch.rand((R, Cpad), device=dev).to(torch.bfloat16)
    grad = torch.empty((R, Cpad), dtype=torch.bfloat16, device=dev)
    loss = torch.zeros((1,), device=dev)
    report("maskiou_loss", lambda: M_.maskiou_loss(pred, cls, out_t, loss, grad), R * (2 + 4 + 4) * 2 + R * Cpad * 2, args)
    dets = torch.zeros((R, 6), device=dev)
    dets[:, 4] = torch.rand((R,), device=dev)
    dets[:, 5] = cls.float()
    sc = torch.empty((R,), dtype=torch.float32, device=dev)
    report("maskiou_score", lambda: M_.maskiou_score(dets, pred, out=sc), R * (8 + 2 + 4), args)


if __name__ == "__main__":
    main()
