"""Device times of the attention entries on their own at the benchmark's shape: N = 2 images whose refine
level is 50 x 84 = 4,200 positions, d = 64 and 128, on the packed [N, L, 3d] tensor the refine's 1x1 convolution writes.
Beside them torch's unfused composition on the same operands (bmm, softmax, bmm, and its autograd), which materialises the
L x L matrix. Each entry is captured `reps` times into a hipGraph and the replay is timed with device events (no launch gaps
in the window); `rounds` repeats show the spread.

    python tools/bench_attention.py [--reps 10] [--rounds 3] [--L 4200]

One JSON line per entry: {"entry", "d", "us" (per call, one value per round), "flop", "TFLOPs" (flop over the best time)}.
Forward counts 4 N L^2 d; backward counts the products executed: 14 N L^2 d for the two-sweep kernels (seven products) plus
the delta pre-pass, 10 N L^2 d for autograd's five.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxdetection_amd.ops.attention import AttentionPlan   # noqa: E402
from tools.bench_libra import graph_time   # noqa: E402


def report(name, d, fn, flop, args):
    us = [round(graph_time(fn, args.reps), 2) for _ in range(args.rounds)]
    print(json.dumps({"entry": name, "d": d, "us": us, "flop": int(flop), "TFLOPs": round(flop / min(us) / 1e6, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--L", type=int, default=4200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev, N, L = "cuda", 2, args.L
    gen = torch.Generator().manual_seed(0)
    for d in (64, 128):
        scale = 1.0
        qkv = (torch.randn((N, L, 3 * d), generator=gen) * 0.5).to(torch.bfloat16).to(dev)
        d_out = (torch.randn((N, L, d), generator=gen) * 0.5).to(torch.bfloat16).to(dev)
        out = torch.empty((N, L, d), dtype=torch.bfloat16, device=dev)
        d_qkv = torch.empty_like(qkv)
        plan = AttentionPlan(N, L, d, 3 * d, 0, d, 2 * d, scale, dev)
        unit = float(N) * L * L * d
        report("attention_fwd", d, lambda: plan.forward(qkv, out), 4 * unit, args)
        report("attention_bwd", d, lambda: plan.backward(qkv, out, d_out, d_qkv), 14 * unit + 2.0 * N * L * d, args)

        # torch's unfused composition on the same operands (views of the packed tensor)
        q, k, v = (qkv[..., i * d:(i + 1) * d] for i in range(3))

        def compose():
            return torch.bmm(torch.softmax(torch.bmm(q, k.transpose(1, 2)) * scale, dim=2), v)

        o_t = compose()
        err = float((o_t.float() - out.float()).abs().max())
        report("torch bmm/softmax/bmm fwd", d, compose, 4 * unit, args)
        leaves = [t.detach().clone().requires_grad_() for t in (q, k, v)]

        def fwd_bwd():
            o = torch.bmm(torch.softmax(torch.bmm(leaves[0], leaves[1].transpose(1, 2)) * scale, dim=2), leaves[2])
            for t in leaves:
                t.grad = None
            o.backward(d_out)

        report("torch bmm/softmax/bmm fwd + autograd bwd", d, fwd_bwd, 14 * unit, args)
        print(json.dumps({"entry": "max |O - torch|", "d": d, "value": err}), flush=True)


if __name__ == "__main__":
    main()
