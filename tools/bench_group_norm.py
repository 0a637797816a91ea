"""GroupNorm kernel times beside torch's own group_norm (+ ReLU) on the same bf16 channels-last tensors, and the
algorithmic-byte floor. Device events around `iters` back-to-back calls after a warm-up; one JSON line per shape.

    python tools/bench_group_norm.py [--iters 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxdetection_amd.ops import group_norm as GN   # noqa: E402

HBM_BYTES_PER_S = 6.3e12
SHAPES = {"box_head": (1024, 7, 7, 256), "mask_head": (256, 14, 14, 256), "pyramid_tiled": (2, 100, 168, 256)}


def timed(fn, iters, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--groups", type=int, default=32)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    G = args.groups
    for name, shape in SHAPES.items():
        N, H, W, Cc = shape
        g = torch.Generator().manual_seed(0)
        x = (torch.randn(shape, generator=g) + 3.0).to(torch.bfloat16).cuda()
        dy = torch.randn(shape, generator=g).to(torch.bfloat16).cuda()
        gamma, beta = torch.randn(Cc, generator=g).cuda(), torch.randn(Cc, generator=g).cuda()
        y, mean, rstd = GN.group_norm_forward(x, gamma, beta, G, relu=True)
        dx, dg, db = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta)
        ws_f = torch.empty((max(GN.workspace_bytes(shape, G, False), 256),), dtype=torch.uint8, device="cuda")
        ws_b = torch.empty((max(GN.workspace_bytes(shape, G, True), 256),), dtype=torch.uint8, device="cuda")
        fwd = timed(lambda: GN.group_norm_forward(x, gamma, beta, G, relu=True, out=y, mean=mean, rstd=rstd, workspace=ws_f),
                    args.iters, args.warmup)
        bwd_y = timed(lambda: GN.group_norm_backward(x, dy, mean, rstd, gamma, G, dg, db, y=y, relu=True, out=dx,
                                                     workspace=ws_b), args.iters, args.warmup)
        bwd = timed(lambda: GN.group_norm_backward(x, dy, mean, rstd, gamma, G, dg, db, beta=beta, relu=True, out=dx,
                                                   workspace=ws_b), args.iters, args.warmup)
        # torch: the same memory (NHWC) seen as an NCHW channels_last tensor; bf16 parameters as autocast models hold them
        xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)
        gt, bt = gamma.to(torch.bfloat16).requires_grad_(True), beta.to(torch.bfloat16).requires_grad_(True)
        dyt = dy.permute(0, 3, 1, 2)
        F = torch.nn.functional
        t_fwd = timed(lambda: torch.relu(F.group_norm(xt, G, gt, bt, 1e-5)), args.iters, args.warmup)

        def both():
            xt.grad = gt.grad = bt.grad = None
            torch.relu(F.group_norm(xt, G, gt, bt, 1e-5)).backward(dyt)
        t_both = timed(both, args.iters, args.warmup)
        nbytes = x.numel() * 2
        print(json.dumps({
            "shape": name, "dims": list(shape), "groups": G,
            "fwd_us": round(fwd, 2), "bwd_us": round(bwd, 2), "bwd_with_y_us": round(bwd_y, 2),
            "torch_fwd_us": round(t_fwd, 2), "torch_bwd_us": round(t_both - t_fwd, 2),
            "floor_fwd_us": round(2 * nbytes / HBM_BYTES_PER_S * 1e6, 2),      # read x, write y
            "floor_bwd_us": round(3 * nbytes / HBM_BYTES_PER_S * 1e6, 2),      # read x and dy, write dx
        }), flush=True)


if __name__ == "__main__":
    main()
