"""Times of test-time post-processing with greedy NMS and with the two Soft-NMS forms: DetectionPostprocess
at the box head's evaluation shape (N=2 images, R=1000 rois, C=81 classes, score_thresh 0.05, max_per_image 100) on a
clustered input -- most rois are jitters of a few objects, the case in which Soft-NMS has work to do -- and the standalone
entry at B=160 lists of 1000 candidates. Device events around `iters` back-to-back calls after a warm-up; the variants
alternate over `rounds` rounds, so their spread is seen beside their difference. One JSON line per shape; `sha` is a digest of
the hard result, to compare two builds of the library (`--lib` times another build's hard path, e.g. the parent commit's).

    python tools/bench_soft_nms.py [--iters 200] [--warmup 20] [--rounds 3] [--methods hard,linear,gaussian] [--lib PATH]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxdetection_amd import _lib   # noqa: E402


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


def rounds_of(fns, args):
    out = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            out[k].append(round(timed(fn, args.iters, args.warmup), 2))
    return out


def clustered_boxes(rng, n, G):
    """n boxes, each a jitter of one of G objects with probability G/(G+1), else clutter. Returns (boxes [n,4], object or -1)."""
    octr = rng.uniform(150, 1150, (G, 2)) * np.array([1.0, 0.6])
    osz = np.exp(rng.uniform(np.log(48), np.log(320), (G, 2)))
    k = rng.integers(0, G + 1, n)
    kk = np.minimum(k, G - 1)
    sz = osz[kk] * np.exp(rng.uniform(-0.25, 0.25, (n, 2)))
    ctr = octr[kk] + rng.uniform(-0.2, 0.2, (n, 2)) * osz[kk]
    clutter = (k == G)[:, None]
    ctr = np.where(clutter, rng.uniform(40, 1290, (n, 2)) * np.array([1.0, 0.6]), ctr)
    sz = np.where(clutter, np.exp(rng.uniform(np.log(16), np.log(400), (n, 2))), sz)
    return np.concatenate([ctr - sz / 2, ctr + sz / 2], 1).astype(np.float32), np.where(k < G, k, -1)


def bench_postprocess(args, rng):
    from mxdetection_amd.core.evaluation import DetectionPostprocess
    N, R, C, G, ld = 2, 1000, 81, 12, 448
    fused = np.zeros((N * R, ld), np.float32)
    rois = np.zeros((N * R, 5), np.float32)
    rois[:, 0] = np.repeat(np.arange(N), R)
    for n in range(N):
        boxes, obj = clustered_boxes(rng, R, G)
        rois[n * R:(n + 1) * R, 1:] = boxes
        logits = rng.standard_normal((R, C)) * 1.5
        rows = np.flatnonzero(obj >= 0)
        logits[rows, rng.integers(1, C, G)[obj[rows]]] += rng.uniform(3, 7, rows.size)
        fused[n * R:(n + 1) * R, :C] = logits
    fused[:, C:5 * C] = rng.standard_normal((N * R, 4 * C)) * 0.3
    fused = torch.from_numpy(fused).to(torch.bfloat16).cuda()
    rois = torch.from_numpy(rois).cuda()
    num_rois = torch.tensor([R] * N, dtype=torch.int32, device="cuda")
    info = torch.tensor([[800.0, 1333.0, 1.0]] * N, device="cuda")
    fns, res = {}, {}
    for m in args.methods:
        post = DetectionPostprocess(C, score_thresh=0.05, nms_thresh=0.5, max_per_image=100, nms_method=m, soft_sigma=0.5)
        fns[m] = lambda post=post: post(fused[:, :C], fused[:, C:], rois, num_rois, info)
        dets, num = fns[m]()
        torch.cuda.synchronize()
        res[m] = (dets.cpu().numpy().copy(), num.cpu().numpy().copy())
    out = {"shape": "DetectionPostprocess N=%d R=%d C=%d bf16, score_thresh 0.05, max_per_image 100" % (N, R, C),
           "us_per_call": rounds_of(fns, args), "num_dets": {m: r[1].tolist() for m, r in res.items()}}
    if "hard" in res:
        out["sha"] = hashlib.sha256(res["hard"][0].tobytes() + res["hard"][1].tobytes()).hexdigest()[:16]
        for m, (d, _) in res.items():
            if m != "hard":        # how much work Soft-NMS had: output rows that are not rows of the hard result
                cols = [0, 1, 2, 3, 5]
                hard = {tuple(r) for r in res["hard"][0][0][:, cols].tolist()}
                out.setdefault("rows_not_in_hard_image0", {})[m] = sum(tuple(r) not in hard for r in d[0][:, cols].tolist())
    print(json.dumps(out), flush=True)


def bench_standalone(args, rng):
    from mxdetection_amd.ops import soft_nms_batched
    B, n = 160, 1000
    boxes = np.stack([clustered_boxes(rng, n, 12)[0] for _ in range(B)])
    scores = rng.uniform(0.01, 1.0, (B, n)).astype(np.float32)
    boxes, scores = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    counts = torch.from_numpy(rng.integers(n // 2, n + 1, B).astype(np.int32)).cuda()
    fns = {m: (lambda m=m: soft_nms_batched(boxes, scores, counts, m, 0.5, 0.5, 0.001, 100)) for m in args.methods}
    print(json.dumps({"shape": "soft_nms_batched B=%d n_max=%d max_keep 100" % (B, n), "us_per_call": rounds_of(fns, args)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--methods", default="hard,linear,gaussian")
    ap.add_argument("--lib", default="", help="another build of libmxdet_hip.so to time (a build without Soft-NMS: --methods hard)")
    args = ap.parse_args()
    args.methods = args.methods.split(",")
    assert torch.cuda.is_available(), "needs the GPU"
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    lib = _lib.load()
    rng = np.random.default_rng(0)
    bench_postprocess(args, rng)
    if hasattr(lib, "mxdet_soft_nms_batched"):
        bench_standalone(args, rng)


if __name__ == "__main__":
    main()
