"""Device times of the CARAFE entries on their own at the three top-down merges of the benchmark: N = 2 images of
800 x 1344, C = 256, the coarse maps 100 x 168 (-> P2, 200 x 336), 50 x 84 (-> P3) and 25 x 42 (-> P4); k = 5 with the logits
in 128 channels as in the model (and k = 3 in 64). Each entry stands beside the bytes it must move (every operand once) and
beside the same computation as an unfused torch composition on the same GPU: unfold, nearest upsample, pixel shuffle, softmax,
weighted sum, and its autograd backward (bf16, channels-first, torch's own layout).

The fused entries are captured `reps` times into a hipGraph and the replay is timed with device events (no launch gaps in the
window); the torch composition, milliseconds per call, is timed eagerly with device events around `torch_reps` calls behind a
warm-up. `rounds` repeats show the spread.

    python tools/bench_carafe.py [--reps 20] [--rounds 3] [--torch-reps 5]

One JSON line per entry: {"entry", "shape", "k", "us" (per call, one value per round), "bytes", "GBps" (bytes over the best
time), "torch_us", "speedup" (best torch time over best fused time)}.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxdetection_amd.ops.carafe import CarafePlan, logit_channels   # noqa: E402
from tools.bench_libra import graph_time   # noqa: E402


def torch_forward(x, logits, k, out_hw):
    """x [N, C, H, W], logits [N, 4 k^2, H, W] (the real channels) -> [N, C, Hf, Wf]: the published composition."""
    N, C, H, W = x.shape
    cols = F.unfold(x, k, padding=k // 2).view(N, C, k * k, H, W)
    cols = cols.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
    w = torch.softmax(F.pixel_shuffle(logits, 2).float(), dim=1).to(x.dtype)
    return (cols * w[:, None]).sum(dim=2)[:, :, :out_hw[0], :out_hw[1]]


def event_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = "cuda"
    N, C = 2, 256
    gen = torch.Generator().manual_seed(0)
    rnd = lambda s, std=1.0: (torch.randn(s, generator=gen) * std).to(torch.bfloat16).to(dev)     # noqa: E731
    for k in (5, 3):
        real, Cm = logit_channels(k)
        for (H, W), out_hw in (((100, 168), (200, 336)), ((50, 84), (100, 168)), ((25, 42), (50, 84))):
            plan = CarafePlan((N, H, W, C), Cm, k, out_hw)
            x, m, dy = rnd(plan.x_shape), rnd(plan.m_shape, 1.5), rnd(plan.y_shape, 0.5)
            y, dx, dm = torch.empty_like(dy), torch.zeros_like(x), torch.empty_like(m)
            xb, mb, yb = x.numel() * 2, m.numel() * 2, y.numel() * 2
            xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            mt = m[..., :real].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            gt = dy.permute(0, 3, 1, 2).contiguous()

            def torch_fwd_bwd():
                xt.grad = mt.grad = None
                torch_forward(xt, mt, k, out_hw).backward(gt)

            def torch_fwd():
                with torch.no_grad():
                    torch_forward(xt, mt, k, out_hw)

            t_fwd = [round(event_time(torch_fwd, args.torch_reps), 1) for _ in range(args.rounds)]
            t_both = [round(event_time(torch_fwd_bwd, args.torch_reps), 1) for _ in range(args.rounds)]
            t_bwd = [round(b - f, 1) for b, f in zip(t_both, t_fwd)]
            for name, fn, nbytes, t in (
                    ("carafe_fwd", lambda: plan.forward(x, m, y), xb + mb + yb, t_fwd),
                    ("carafe_bwd", lambda: plan.backward(x, m, dy, dx, dm, accumulate=True), 3 * xb + 2 * mb + yb, t_bwd)):
                us = [round(graph_time(fn, args.reps), 2) for _ in range(args.rounds)]
                print(json.dumps({"entry": name, "shape": [N, H, W, C], "k": k, "us": us, "bytes": int(nbytes),
                                  "GBps": round(float(nbytes) / min(us) / 1e3, 1), "torch_us": t,
                                  "speedup": round(min(t) / min(us), 1)}), flush=True)


if __name__ == "__main__":
    main()
