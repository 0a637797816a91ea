"""Cost of the gradient-harmonizing losses (GHM-C / GHM-R), modelled on tools/bench_quality_loss.py. Two modes.

entry (default): the GHM step of the head -- histogram pass per level, the weights kernel, loss pass per level, one finalize --
beside mxdet_retina_loss_level on the five RetinaNet levels of the benchmark input (2 x 800 x 1344, 80 classes, 9 anchors per
cell). With --lib PATH the plain side is ALSO taken from that library (the parent commit's build), so the figure shows that
the entry this work did not touch is where it was. The histogram passes and the loss passes are timed on their own too, so
the line says where the time goes. Two logit tables: `init` (every logit near the prior -4.6: every class element in bin 0,
the wave-uniform path of the histogram) and `spread` (logits N(-2, 3): the lanes of a wave disagree on the bin). Device
events around `iters` back-to-back calls after a warm-up; the entries alternate over `rounds` rounds. One JSON line per table.

step: RetinaNet R101-FPN with ghm none against ghm both, bench.py's protocol -- its synthetic batches, capture, warm-up,
timed replays, images/s from the wall clock after a device drain -- both models in one process, alternating over `rounds`
rounds. One JSON line.

    python tools/bench_ghm.py [--mode entry|step] [--lib parent/libmxdet_hip.so] [--ghm both] [--iters 200] [--warmup 20]
                              [--rounds 3] [--steps 20] [--step-warmup 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_iou_loss import RETINA_LEVELS, rounds_of   # noqa: E402
from mxdetection_amd import _lib   # noqa: E402
from mxdetection_amd.core import loss as L   # noqa: E402
from mxdetection_amd._lib import ptr, stream_ptr   # noqa: E402


def other_library(path):
    """mxdet_retina_loss_level and finalize of another build of the library, bound with this tree's signatures."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("mxdet_retina_loss_level", "mxdet_loss_finalize", "mxdet_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def bench_entry(args, g, table):
    N, C, A = 2, 80, 9
    ldc, ldr = (A * C + 63) // 64 * 64, (A * 4 + 63) // 64 * 64
    offs = [0]
    for h, w in RETINA_LEVELS:
        offs.append(offs[-1] + h * w * A)
    At = offs[-1]
    r = torch.rand((N, At), generator=g)
    cls_labels = torch.zeros((N, At), dtype=torch.int32)
    fg = r < 0.002                                                                    # ~400 foreground anchors, as bench_iou_loss
    cls_labels[fg] = torch.randint(1, C + 1, (int(fg.sum()),), generator=g, dtype=torch.int32)
    cls_labels[r > 0.99] = -1
    cls_labels = cls_labels.cuda()
    num_fg = fg.sum().int().view(1).cuda()
    targets = (torch.randn((N, At, 4), generator=g) * 0.3).cuda().contiguous()
    mean, std = (-4.6, 0.01) if table == "init" else (-2.0, 3.0)
    co = [(torch.randn((N, h, w, ldc), generator=g) * std + mean).to(torch.bfloat16).cuda() for h, w in RETINA_LEVELS]
    bo = [(torch.randn((N, h, w, ldr), generator=g) * 0.3).to(torch.bfloat16).cuda() for h, w in RETINA_LEVELS]
    gc, gb = [torch.zeros_like(x) for x in co], [torch.zeros_like(x) for x in bo]
    nparts = [L.retina_loss_num_partials(N, h, w, A) for h, w in RETINA_LEVELS]
    partial, loss = torch.zeros(2 * sum(nparts), device="cuda"), torch.zeros(2, device="cuda")
    c = L.check_ghm(args.ghm)
    nb = c["cls_bins"] + c["reg_bins"]
    counts = torch.zeros((sum(nparts), nb), dtype=torch.int32, device="cuda")
    acc, coef = torch.zeros(nb, device="cuda"), torch.zeros(nb, device="cuda")
    cnt = torch.zeros(nb, dtype=torch.int32, device="cuda")
    other = other_library(args.lib) if args.lib else None

    def plain(lib):
        off = 0
        for l, (h, w) in enumerate(RETINA_LEVELS):
            if lib is None:
                L.retina_loss_level(co[l], bo[l], A, C, cls_labels, targets, offs[l], 0.25, 2.0, 3.0, num_fg, 1.0, gc[l], gb[l],
                                    partial[2 * off:])
            else:
                rc = lib.mxdet_retina_loss_level(ptr(co[l]), ptr(bo[l]), N, h, w, A, C, ldc, ldr, ptr(cls_labels), ptr(targets), At,
                                                 offs[l], 0.25, 2.0, 3.0, ptr(num_fg), 1.0, ptr(gc[l]), ptr(gb[l]),
                                                 ptr(partial[2 * off:]), stream_ptr())
                assert rc == 0, lib.mxdet_last_error()
            off += nparts[l]
        L.loss_finalize(partial, off, 2, loss)

    def hist():
        off = 0
        for l in range(len(RETINA_LEVELS)):
            L.ghm_hist_level(co[l], bo[l], A, C, cls_labels, targets, offs[l], args.ghm, c["cls_bins"], c["reg_bins"], c["reg_mu"],
                             counts[off:])
            off += nparts[l]
        return off

    def weights(rows):
        L.ghm_weights(counts, rows, c["cls_bins"], c["reg_bins"], c["cls_momentum"], c["reg_momentum"], acc, cnt, coef)

    def passes():
        off = 0
        for l in range(len(RETINA_LEVELS)):
            L.retina_loss_level_ghm(co[l], bo[l], A, C, cls_labels, targets, offs[l], args.ghm, 0.25, 2.0, 3.0, coef, c["cls_bins"],
                                    c["reg_bins"], c["cls_weight"], c["reg_mu"], c["reg_weight"], num_fg, 1.0, gc[l], gb[l],
                                    partial[2 * off:])
            off += nparts[l]
        L.loss_finalize(partial, off, 2, loss)

    def ghm():
        weights(hist())
        passes()
    fns = {"plain": lambda: plain(None), "ghm": ghm, "ghm_hist_passes": hist, "ghm_weights": lambda: weights(sum(nparts)),
           "ghm_loss_passes": passes}
    if other is not None:
        fns = {"plain_other_lib": lambda: plain(other), **fns}
    t = rounds_of(fns, args)
    torch.cuda.synchronize()
    best = {k: min(v) for k, v in t.items()}
    base = best["plain_other_lib"] if other is not None else best["plain"]
    print(json.dumps({"shape": "retinanet 5 levels of 2x800x1344, A=%d C=%d, %d anchors" % (A, C, N * At), "table": table,
                      "ghm": args.ghm, "class_bins_in_use": int((cnt[:c["cls_bins"]] > 0).sum()), "us_per_call": t,
                      "ghm_over_plain": round(best["ghm"] / base, 4)}), flush=True)


def bench_step(args):
    import bench
    from mxdetection_amd.models import RetinaNet
    lr = 0.02 * bench.BATCH_PER_GPU / 16.0 / 3.0
    batches = [bench.synth_batch(0, s, "cuda") for s in range(4)]
    models = {}
    for k in ("none", args.ghm):
        m = RetinaNet("cuda", depth=101, seed=7, ghm=k)
        m.enable_wgrad_stream()
        m.enable_branch_stream()
        m.enable_grouped_wgrad()
        m.capture(*batches[0], lr=lr, image_offset=0)
        models[k] = m
    out = {k: [] for k in models}
    losses = {}
    for _ in range(args.rounds):
        for k, m in models.items():
            for i in range(args.step_warmup):
                m.replay(*batches[i % 4], i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                last = m.replay(*batches[(args.step_warmup + i) % 4], args.step_warmup + i)
            torch.cuda.synchronize()
            out[k].append(round(args.steps * bench.BATCH_PER_GPU / (time.perf_counter() - t0), 3))
            losses[k] = [round(float(v), 6) for v in torch.cat(list(last)).cpu().numpy()]
    print(json.dumps({"model": "retinanet r101-fpn, 2 x 800 x 1344", "images_per_sec": out, "losses": losses,
                      "ghm_over_none": round(max(out[args.ghm]) / max(out["none"]), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="entry", choices=("entry", "step"))
    ap.add_argument("--lib", default=None, help="entry mode: another build of libmxdet_hip.so for the plain side (the parent commit's)")
    ap.add_argument("--ghm", default="both", choices=tuple(L.GHM_FLAGS))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    if args.mode == "step":
        bench_step(args)
        return
    g = torch.Generator().manual_seed(0)
    for table in ("init", "spread"):
        bench_entry(args, g, table)


if __name__ == "__main__":
    main()
