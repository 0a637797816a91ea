"""Device times of the global context entries on their own at the three stage shapes of the benchmark at batch 2:
C3 100 x 168 x 512, C4 50 x 84 x 1024, C5 25 x 42 x 2048, inner width C / reduction. Each entry stands beside the bytes it must
move (every map operand once; the fp32 chunk partials it writes or reads) and the rate that is of the measured HBM peak
(6.29 TB/s, MI355X_MICROARCH: float4 copy); the summed forward and backward stand beside the same block as an unfused torch
composition on the same GPU (bf16, channels-first, torch's own layout: the logits as a matmul, softmax, matmul, linear, layer_norm, linear,
broadcast add, add, relu, and its autograd backward). The composition's backward measures 12-17 ms beside a 0.15-0.2 ms
forward, with the logits as a conv2d 1x1 or as a matmul alike: some library path of autograd's, not identified, dominates it,
so the backward ratio says little about an unfused composition done well; the forward ratio is the comparison.

The fused entries are captured `reps` times into a hipGraph and the replay is timed with device events (no launch gaps in the
window); the torch composition is timed eagerly with device events around `torch_reps` calls behind a warm-up. Fused and torch
alternate: each of the `rounds` rounds times every fused entry, then the composition; the rounds show the spread.

    python tools/bench_gc.py [--reduction 16] [--reps 20] [--rounds 3] [--torch-reps 5]

One JSON line per entry: {"entry", "shape", "P", "us" (per call, one value per round), "bytes", "GBps" (bytes over the best
time), "of_peak"}, then per shape {"entry": "forward" | "backward", "us" (the entries' best times summed), "torch_us", "speedup"}.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxdetection_amd.ops.context import CHUNK, ContextPlan   # noqa: E402
from tools.bench_carafe import event_time   # noqa: E402
from tools.bench_libra import graph_time   # noqa: E402

HBM_PEAK_GBPS = 6290.0
SHAPES = ((100, 168, 512), (50, 84, 1024), (25, 42, 2048))


def torch_block(t, sc, wk, w1, b1, gamma, beta, w2, b2):
    """t, sc [N, C, H, W] bf16 -> relu(t + add + sc): mmcv's ContextBlock (att pooling, channel_add) in front of the sum."""
    N, C, H, W = t.shape
    x = t.view(N, C, H * W)
    mask = torch.softmax(torch.matmul(wk.view(1, 1, C), x).float(), dim=2).to(t.dtype)
    ctx = torch.matmul(x, mask.transpose(1, 2))[:, :, 0]
    u = torch.relu(F.layer_norm(F.linear(ctx, w1, b1), (w1.shape[0],), gamma, beta, 1e-5))
    add = F.linear(u, w2, b2)
    return torch.relu(t + add[:, :, None, None] + sc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reduction", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev, N = "cuda", 2
    bf, f32 = torch.bfloat16, torch.float32
    gen = torch.Generator().manual_seed(0)
    rnd = lambda s, std=1.0, dt=bf: (torch.randn(s, generator=gen) * std).to(dt).to(dev)     # noqa: E731
    for H, W, C in SHAPES:
        HW, P = H * W, C // args.reduction
        K = -(-HW // CHUNK)
        plan = ContextPlan(N, HW, C, P, dev)
        t, sc, ds = rnd((N, HW, C)), rnd((N, HW, C)).relu_(), rnd((N, HW, C), 0.5)
        wk, w1, w2 = rnd((C,), (2.0 / C) ** 0.5), rnd((P, C), (2.0 / C) ** 0.5), rnd((C, P), (1.0 / P) ** 0.5)
        b1, beta, b2 = rnd((P,), 0.1, f32), rnd((P,), 0.1, f32), rnd((C,), 0.1, f32)
        gamma = torch.ones((P,), dtype=f32, device=dev)
        y, d_t = torch.empty_like(t), torch.empty_like(t)
        bits = torch.empty((N * HW * C // 8,), dtype=torch.uint8, device=dev)
        g = {k: torch.zeros(s, dtype=f32, device=dev) for k, s in (("w1", (P, C)), ("b1", (P,)), ("gamma", (P,)), ("beta", (P,)),
                                                                  ("w2", (C, P)), ("b2", (C,)), ("wk", (C,)))}
        M, part = t.numel() * 2, N * K * C * 4
        small = 2 * (2 * C * P + C) + 4 * (3 * P + C)
        entries = (
            ("gc_pool_fwd", lambda: plan.pool_forward(t, wk), M + part + N * HW * 4, "fwd"),
            ("gc_transform_fwd", lambda: plan.transform_forward(w1, b1, gamma, beta, w2, b2), part + small, "fwd"),
            ("gc_fuse_fwd", lambda: plan.fuse_forward(t, sc, y, bits), 3 * M + M // 16, "fwd"),
            ("gc_reduce_bwd", lambda: plan.reduce_backward(ds), M + part, "bwd"),
            ("gc_transform_bwd", lambda: plan.transform_backward(w1, gamma, beta, w2, g["w1"], g["b1"], g["gamma"], g["beta"],
                                                                  g["w2"], g["b2"]), part + small + 4 * (2 * C * P), "bwd"),
            ("gc_pool_bwd", lambda: plan.pool_backward(t, wk, ds, d_t, g["wk"]), 4 * M + 2 * part + 3 * N * HW * 4, "bwd"),
        )
        for _, fn, _, _ in entries:          # every buffer an entry reads holds a real value before anything is timed
            fn()
        # ---- the unfused composition
        tt = t.view(N, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        st = sc.view(N, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        gt = ds.view(N, H, W, C).permute(0, 3, 1, 2).contiguous()
        params = [p.to(bf).requires_grad_(True) for p in (wk, w1, b1, gamma, beta, w2, b2)]

        def torch_fwd():
            with torch.no_grad():
                torch_block(tt, st, *params)

        def torch_fwd_bwd():
            for p in [tt, st] + params:
                p.grad = None
            torch_block(tt, st, *params).backward(gt)

        us = {name: [] for name, _, _, _ in entries}
        t_fwd, t_both = [], []
        for _ in range(args.rounds):          # fused and torch alternate
            for name, fn, _, _ in entries:
                us[name].append(round(graph_time(fn, args.reps), 2))
            t_fwd.append(round(event_time(torch_fwd, args.torch_reps), 1))
            t_both.append(round(event_time(torch_fwd_bwd, args.torch_reps), 1))
        total = {"fwd": 0.0, "bwd": 0.0}
        for name, _, nbytes, side in entries:
            total[side] += min(us[name])
            rate = float(nbytes) / min(us[name]) / 1e3
            print(json.dumps({"entry": name, "shape": [N, H, W, C], "P": P, "us": us[name], "bytes": int(nbytes),
                              "GBps": round(rate, 1), "of_peak": round(rate / HBM_PEAK_GBPS, 3)}), flush=True)
        t_bwd = [round(b - f, 1) for b, f in zip(t_both, t_fwd)]
        for side, tt_us in (("fwd", t_fwd), ("bwd", t_bwd)):
            print(json.dumps({"entry": "forward" if side == "fwd" else "backward", "shape": [N, H, W, C], "P": P,
                              "us": round(total[side], 2), "torch_us": tt_us, "speedup": round(min(tt_us) / total[side], 1)}),
                  flush=True)


if __name__ == "__main__":
    main()
