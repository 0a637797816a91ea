"""Case tables of the selection / sampling / NMS branch tests (csrc/select.h, proposal.hip, targets.hip, boxes.hip,
postprocess.hip) and the proof -- without a GPU -- that every case reaches the data-dependent branch it is named after.
tests/test_gpu_select_branches.py runs the same tables on the GPU.

Nearly every branch of these kernels is chosen by the data (how many candidates a list holds, whether the cut falls inside
a tie, how long a list is), so a case is only worth its name if the data really has that property. Every builder below is
seeded, deterministic and small and returns plain numpy inputs; every proof derives the branch predicate from the reference
alone and from the constants (kCandCap, kBgKeyCut, kSelChunk, kMaxPre) read out of the .hip sources with a regex, so a
changed constant fails the proof instead of quietly un-targeting the case.

The reference is the C oracle (oracle/mxdet_oracle.c), oracle.sample_key and numpy. The oracle is a legitimate reference for
this family: it selects with qsort on (key, index) and runs greedy NMS in a plain loop, which are different algorithms from
the radix select, the candidate lists, the bitmask scan and the rank merge of the kernels. The two sides share only
include/mxdet_math.h (IoU, Philox key, float key, box transforms), which tests/test_math.py pins independently.

`bg_list_exact` (one image's below-cut background count equals its want_bg): the step is searched on the CPU
(search_bg_list_exact) and committed as a literal. Reading select.h, a list of exactly k candidates still ends in mode 0
(the last non-empty bin satisfies the scan), so this case pins the boundary `n_bg_list >= want_bg` of the list path; the
`rb.mode == 1` rewrite in anchor_sample_kernel is reached with an EMPTY list and want_bg = 0, which `bg_list_empty` builds.
`key_tie_at_cut` holds two background anchors whose 32-bit Philox keys collide (found by search_key_tie, committed as a
literal) with the cut between them: the only input on which the tie index of a candidate list (idxf) decides anything.
"""
import functools
import os
import re

import numpy as np
import pytest

from conftest import synth_boxes, synth_gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mxdetection_amd", "csrc")


def O():
    from oracle import oracle as o
    o.lib()
    return o


@functools.lru_cache(maxsize=None)
def consts():
    """kCandCap, kBgKeyCut (targets.hip), kSelChunk, kMaxPre (proposal.hip), kDetMaxRois (postprocess.hip), and the word
    count at which mxdet_nms_batched switches scan kernels (boxes.hip), read from the sources."""
    tg = open(os.path.join(CSRC, "targets.hip")).read()
    pr = open(os.path.join(CSRC, "proposal.hip")).read()
    pp = open(os.path.join(CSRC, "postprocess.hip")).read()
    bx = open(os.path.join(CSRC, "boxes.hip")).read()

    def one(src, pat):
        m = re.findall(pat, src)
        assert len(m) == 1, (pat, m)
        return int(m[0], 0)
    return {
        "kCandCap": one(tg, r"constexpr int kCandCap = (\d+);"),
        "kBgKeyCut": one(tg, r"constexpr unsigned kBgKeyCut = (0x[0-9a-fA-F]+)u;"),
        "kSelChunk": one(pr, r"constexpr int kSelChunk = (\d+);"),
        "kMaxPre": one(pr, r"constexpr int kMaxPre = (\d+);"),
        "kDetMaxRois": one(pp, r"constexpr int kDetMaxRois = (\d+);"),
        "nms_rows_words": one(bx, r"if \(nwords <= (\d+)\)\s+hipLaunchKernelGGL\(nms_scan_rows_kernel<32>"),
    }


def ids(cases):
    return [c["id"] for c in cases]


def float_key(x):
    """numpy restatement of the order-preserving key of a float32 (larger float -> larger key; -0.0 < +0.0)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# anchor target (anchor_sample_kernel)
# ---------------------------------------------------------------------------------------------------------------------
IM_H, IM_W = 400, 666
PYR3 = ([16, 32, 64], [(25, 42), (13, 21), (7, 11)])
PYR5 = ([4, 8, 16, 32, 64], [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)])


def pyramid_anchors(pyr):
    o = O()
    return np.concatenate([o.grid_anchors(o.base_anchors(s), H, W, s) for s, (H, W) in zip(*pyr)])


def _gt(rows, G):
    g = -np.ones((G, 5), np.float32)
    for k, r in rows.items():
        g[k] = r
    return g


def _big_gt(rng, k, lo=60, hi=220):
    """k boxes of side lo..hi inside the 400x666 image (a +-1.5 px jitter of such a box keeps IoU > 0.9)."""
    w, h = rng.uniform(lo, hi, k), rng.uniform(lo, hi, k)
    x1, y1 = rng.uniform(0, IM_W - 1 - w), rng.uniform(0, IM_H - 1 - h)
    return np.stack([x1, y1, x1 + w, y1 + h, rng.integers(1, 81, k)], 1).astype(np.float32)


def _acase(cid, branch, anchors, gt, im_info=None, batch=256, frac=0.5, fg=0.7, bg=0.3, seed=99, step=7, image_offset=4):
    gt = np.ascontiguousarray(gt, np.float32)
    if im_info is None:
        im_info = np.array([[IM_H, IM_W, 1.0]] * gt.shape[0], np.float32)
    return dict(id=cid, branch=branch, anchors=np.ascontiguousarray(anchors, np.float32), gt=gt,
                im_info=np.ascontiguousarray(im_info, np.float32), batch=batch, frac=frac, fg=fg, bg=bg, seed=seed, step=step,
                image_offset=image_offset)


def _bg_list_short_inputs():
    rng = np.random.default_rng(101)
    anchors = pyramid_anchors(PYR3)
    inside = np.flatnonzero((anchors[:, 0] >= 0) & (anchors[:, 1] >= 0) & (anchors[:, 2] < IM_W) & (anchors[:, 3] < IM_H))
    G = 160
    gt = -np.ones((2, G, 5), np.float32)
    gt[0, :5] = _big_gt(rng, 5)                               # a handful of GT: fewer than max_fg foreground anchors
    inside = inside[anchors[inside, 2] < 330]                 # ... all in the left half: the right half stays background
    pick = rng.choice(inside, G, replace=False)               # 160 GT that ARE anchors: more than max_fg foreground anchors
    gt[1, :, :4] = anchors[pick]
    gt[1, :, 4] = rng.integers(1, 81, G)
    return anchors, gt


def case_bg_list_short():
    anchors, gt = _bg_list_short_inputs()
    return _acase("bg_list_short", "fall-back 2: filtered background list shorter than want_bg", anchors, gt)


BG_LIST_EXACT_STEP = 6            # found by search_bg_list_exact(); the proof re-checks the property


def search_bg_list_exact(lo=0, hi=2000):
    """First step in [lo, hi] at which image 0 of the bg_list_exact inputs has exactly want_bg background anchors with a
    key below the cut. Not run by the suite: it produced BG_LIST_EXACT_STEP."""
    for step in range(lo, hi + 1):
        c = _bg_list_exact_at(step)
        k = anchor_counts(c)
        if k["n_bg_below"][0] == k["want_bg"][0]:
            return step
    return None


def _bg_list_exact_at(step):
    # 4200-anchor pyramid, batch 56: about 1400 background anchors, so about 44 below the cut, around want_bg = 28..56
    rng = np.random.default_rng(102)
    anchors = pyramid_anchors(PYR3)
    gt = -np.ones((2, 8, 5), np.float32)
    gt[0, :4] = _big_gt(rng, 4)
    gt[1, :6] = _big_gt(rng, 6)
    return _acase("bg_list_exact", "list path at its boundary: n_bg_list == want_bg", anchors, gt, batch=56, frac=0.5, step=step)


def case_bg_list_exact():
    return _bg_list_exact_at(BG_LIST_EXACT_STEP)


def case_fg_list_overflow():
    rng = np.random.default_rng(103)
    anchors = pyramid_anchors(PYR5)
    gt = -np.ones((2, 8, 5), np.float32)
    gt[0, :4] = _big_gt(rng, 4)
    gt[1, :5] = synth_gt(rng, 1, 8, IM_H, IM_W, 5, 5)[0, :5]
    copies = gt[0, rng.integers(0, 4, 24000), :4] + rng.uniform(-1.5, 1.5, (24000, 4)).astype(np.float32)
    copies[:, [0, 1]] = np.maximum(copies[:, [0, 1]], 0)
    copies[:, 2] = np.minimum(copies[:, 2], IM_W - 1)
    copies[:, 3] = np.minimum(copies[:, 3], IM_H - 1)
    anchors = np.concatenate([anchors, copies.astype(np.float32)])
    anchors = anchors[rng.permutation(len(anchors))]
    return _acase("fg_list_overflow", "fall-back 1: foreground list above kCandCap (image 0), list path (image 1)", anchors, gt)


def case_bg_list_overflow():
    rng = np.random.default_rng(104)
    anchors = synth_boxes(rng, 700000)
    gt = synth_gt(rng, 1, 8, 800, 1333, 3, 4)
    return _acase("bg_list_overflow", "fall-back 3: filtered background list above kCandCap", anchors, gt,
                  im_info=np.array([[800, 1333, 1.0]], np.float32))


def case_no_fg():
    anchors = pyramid_anchors(PYR5)
    gt = -np.ones((1, 8, 5), np.float32)
    gt[0, 3] = [5000, 5000, 5100, 5100, 7]
    return _acase("no_fg", "empty foreground list (flag_all on n = 0), 256 background", anchors, gt)


def case_fewer_than_batch():
    anchors = pyramid_anchors(PYR3)
    gt = -np.ones((2, 8, 5), np.float32)
    gt[0, 0] = [20, 30, 110, 120, 3]
    gt[1, 0] = [40, 10, 140, 150, 5]
    gt[1, 1] = [200, 30, 260, 170, 9]
    return _acase("fewer_than_batch", "fg + bg < batch: background mode 1 through the full scan", anchors, gt,
                  im_info=np.array([[180, 300, 1.0], [200, 280, 1.0]], np.float32))


def case_max_fg_zero():
    rng = np.random.default_rng(107)
    anchors = pyramid_anchors(PYR5)
    gt = synth_gt(rng, 2, 8, IM_H, IM_W, 3, 6)
    return _acase("max_fg_zero", "fg_fraction 0: foreground select mode 2, want_bg = batch", anchors, gt, frac=0.0)


def case_gt_holes():
    rng = np.random.default_rng(108)
    anchors = pyramid_anchors(PYR5)
    b = _big_gt(rng, 6)
    gt = np.stack([_gt({1: b[0], 2: b[1], 5: b[2]}, 8), _gt({0: b[3], 4: b[4], 7: b[5]}, 8)])
    return _acase("gt_holes", "valid GT at slots {1,2,5} / {0,4,7} of 8", anchors, gt)


BG_LIST_EMPTY_STEP = 1            # found by search_bg_list_empty(); the proof re-checks the property


def _bg_list_empty_at(step):
    # 300 jittered copies of one GT (all foreground) + 24 far-away boxes (all background), fg_fraction 1: want_bg = 0
    rng = np.random.default_rng(109)
    g = np.array([100, 100, 260, 240, 4], np.float32)
    fgs = g[:4] + rng.uniform(-1.5, 1.5, (300, 4)).astype(np.float32)
    x1, y1 = rng.uniform(300, 600, 24), rng.uniform(0, 60, 24)
    bgs = np.stack([x1, y1, x1 + 40, y1 + 30], 1).astype(np.float32)
    anchors = np.concatenate([fgs, bgs]).astype(np.float32)
    anchors = anchors[rng.permutation(len(anchors))]
    gt = _gt({2: g}, 4)[None]
    return _acase("bg_list_empty", "want_bg = 0 on an empty background list: the `mode == 1` rewrite", anchors, gt, frac=1.0,
                  step=step)


def search_bg_list_empty(lo=0, hi=2000):
    for step in range(lo, hi + 1):
        k = anchor_counts(_bg_list_empty_at(step))
        if k["n_bg_below"][0] == 0:
            return step
    return None


def case_bg_list_empty():
    return _bg_list_empty_at(BG_LIST_EMPTY_STEP)


KEY_TIE = dict(step=24, a=40706, b=47818)       # found by search_key_tie(); the proof re-checks the property


def search_key_tie(steps=range(0, 40), n=400000, seed=99, image=4):
    """(step, a, b) with the smallest b such that background-stream keys of anchors a < b collide below kBgKeyCut. 32-bit
    Philox keys collide about n^2 / 2^33 times among n anchors, one in 32 of those below the cut. Not run by the suite."""
    L, cut, best = O().lib(), consts()["kBgKeyCut"], None
    for step in steps:
        keys = np.fromiter((L.oracle_sample_key(seed, step, image, 1, i) for i in range(n)), np.uint32, n)
        idx = np.flatnonzero(keys < cut)
        order = idx[np.argsort(keys[idx], kind="stable")]
        for j in np.flatnonzero(keys[order[1:]] == keys[order[:-1]]):
            a, b = sorted((int(order[j]), int(order[j + 1])))
            if best is None or b < best["b"]:
                best = dict(step=step, a=a, b=b)
    return best


def case_key_tie_at_cut():
    # Two background anchors with the SAME sampling key, and want_bg such that the cut falls between them: only the tie
    # index decides, and in the candidate list that is the anchor index (idxf), not the position in the list.
    L = O().lib()
    seed, image_offset, batch = 99, 4, 8
    a, b, step = KEY_TIE["a"], KEY_TIE["b"], KEY_TIE["step"]
    K = L.oracle_sample_key(seed, step, image_offset, 1, a)
    smaller = []
    i = 0
    while len(smaller) < batch - 1:
        if i not in (a, b) and L.oracle_sample_key(seed, step, image_offset, 1, i) < K:
            smaller.append(i)
        i += 1
    A = b + 182
    anchors = np.tile(np.array([-100, -100, -60, -70], np.float32), (A, 1))       # outside the image: label -1
    bgs = smaller + [a, b]
    for j, i in enumerate(bgs):
        anchors[i] = [300 + 20 * j, 200, 315 + 20 * j, 230]
    gt = _gt({0: [10, 10, 100, 100, 6]}, 4)[None]
    free = next(i for i in range(A) if i not in bgs)
    anchors[free] = gt[0, 0, :4]                                                  # one foreground anchor, never sampled
    return _acase("key_tie_at_cut", "equal keys at the cut of the candidate list: broken by anchor index", anchors, gt,
                  batch=batch, frac=0.0, seed=seed, step=step, image_offset=image_offset)


ANCHOR_BUILDERS = [case_bg_list_short, case_fg_list_overflow, case_bg_list_overflow, case_no_fg, case_fewer_than_batch,
                   case_max_fg_zero, case_gt_holes, case_bg_list_exact, case_bg_list_empty, case_key_tie_at_cut]
ANCHOR_IDS = [f.__name__[5:] for f in ANCHOR_BUILDERS]


@functools.lru_cache(maxsize=None)
def anchor_case(cid):
    return ANCHOR_BUILDERS[ANCHOR_IDS.index(cid)]()


def oracle_anchor(c, batch=None, step=None, image_offset=None, sl=slice(None)):
    return O().anchor_target(c["anchors"], c["gt"][sl], c["im_info"][sl], c["fg"], c["bg"], 0.0,
                             c["batch"] if batch is None else batch, c["frac"], c["seed"], c["step"] if step is None else step,
                             c["image_offset"] if image_offset is None else image_offset)


def anchor_counts(c):
    """Per image, from the oracle run without sampling: foreground / background anchors, background anchors whose key is
    below kBgKeyCut (the length of the kernel's filtered list), and the sampler's arithmetic."""
    o = O()
    cut = consts()["kBgKeyCut"]
    lab = oracle_anchor(c, batch=0)[0]
    N = lab.shape[0]
    out = dict(labels=lab, n_fg=[], n_bg=[], n_bg_below=[], max_fg=int(np.float32(c["frac"]) * np.float32(c["batch"])),
               nfg=[], want_bg=[])
    L = o.lib()
    for n in range(N):
        bgs = np.flatnonzero(lab[n] == 0)
        img = c["image_offset"] + n
        below = sum(1 for a in bgs if L.oracle_sample_key(c["seed"], c["step"], img, 1, int(a)) < cut)
        nf = int((lab[n] == 1).sum())
        out["n_fg"].append(nf)
        out["n_bg"].append(len(bgs))
        out["n_bg_below"].append(below)
        out["nfg"].append(min(nf, out["max_fg"]))
        out["want_bg"].append(c["batch"] - min(nf, out["max_fg"]))
    return out


def test_constants_are_read_from_the_sources():
    k = consts()
    assert k["kCandCap"] > 0 and 0 < k["kBgKeyCut"] < 2 ** 32 and k["kSelChunk"] > 0 and k["kMaxPre"] > 0
    assert k["nms_rows_words"] * 64 == 2048         # the NMS cases sit on both sides of this switch


@pytest.mark.parametrize("cid", ANCHOR_IDS)
def test_anchor_case_reaches_its_branch(cid):
    c = anchor_case(cid)
    k = anchor_counts(c)
    cap = consts()["kCandCap"]
    N = c["gt"].shape[0]
    fg_list = [k["n_fg"][n] <= cap for n in range(N)]
    bg_list = [k["want_bg"][n] <= k["n_bg_below"][n] <= cap for n in range(N)]
    if cid == "bg_list_short":
        assert len(c["anchors"]) == 4200
        assert all(k["n_bg_below"][n] < k["want_bg"][n] <= k["n_bg"][n] for n in range(N))
        assert k["n_fg"][0] < k["max_fg"] < k["n_fg"][1] and k["want_bg"][0] > 128 and k["want_bg"][1] == 128
    elif cid == "fg_list_overflow":
        assert k["n_fg"][0] > cap and 0 < k["n_fg"][1] <= cap and all(bg_list)
    elif cid == "bg_list_overflow":
        assert k["n_bg_below"][0] > cap and fg_list[0]
    elif cid == "no_fg":
        assert k["n_fg"] == [0] and k["n_bg"][0] >= 256 and bg_list[0]
    elif cid == "fewer_than_batch":
        assert all(0 < k["n_fg"][n] and 0 < k["n_bg"][n] and k["nfg"][n] + k["n_bg"][n] < c["batch"] for n in range(N))
    elif cid == "max_fg_zero":
        assert k["max_fg"] == 0 and min(k["n_fg"]) > 0 and k["want_bg"] == [c["batch"]] * N and all(bg_list)
    elif cid == "gt_holes":
        assert [list(np.flatnonzero(g[:, 4] >= 0)) for g in c["gt"]] == [[1, 2, 5], [0, 4, 7]]
        assert min(k["n_fg"]) > 0 and all(bg_list)
        used = [set(oracle_anchor(c, batch=0)[1][n][k["labels"][n] == 1]) for n in range(N)]
        assert used == [{1, 2, 5}, {0, 4, 7}]                 # every valid slot is some anchor's match, no hole is
    elif cid == "bg_list_exact":
        assert k["n_bg_below"][0] == k["want_bg"][0] > 0 and k["n_bg"][0] > k["want_bg"][0]
    elif cid == "bg_list_empty":
        assert k["n_fg"][0] >= c["batch"] == k["max_fg"] and k["want_bg"] == [0] and k["n_bg"][0] > 0
        assert k["n_bg_below"] == [0]
        assert (oracle_anchor(c)[0] == 0).sum() == 0          # no background may be labelled
    elif cid == "key_tie_at_cut":
        L, a, b = O().lib(), KEY_TIE["a"], KEY_TIE["b"]
        ka, kb = (L.oracle_sample_key(c["seed"], c["step"], c["image_offset"], 1, i) for i in (a, b))
        assert a < b and ka == kb < consts()["kBgKeyCut"]
        assert k["n_bg"] == k["n_bg_below"] == [c["batch"] + 1] and k["want_bg"] == [c["batch"]] and bg_list[0]
        bgs = np.flatnonzero(k["labels"][0] == 0)
        keys = np.array([L.oracle_sample_key(c["seed"], c["step"], c["image_offset"], 1, int(i)) for i in bgs])
        assert (keys <= ka).all() and (keys == ka).sum() == 2          # the two largest keys of the list are the equal pair
        lab = oracle_anchor(c)[0][0]
        assert lab[a] == 0 and lab[b] == -1 and (lab == 0).sum() == c["batch"]
    else:
        raise AssertionError(cid)


# ---------------------------------------------------------------------------------------------------------------------
# proposal target (proposal_target_kernel)
# ---------------------------------------------------------------------------------------------------------------------
PT_S, PT_G, PT_R, PT_N = 2500, 12, 512, 3
PT_TRIP = 1024                       # candidates per trip of the ordered compaction (the kernel's workgroup size)
PT_STDS = (0.1, 0.1, 0.2, 0.2)
PT_ROWS = [
    dict(id="default", frac=0.25, bg_lo=0.0, agnostic=False, means=(0, 0, 0, 0)),
    dict(id="bg_lo_agnostic_means", frac=0.25, bg_lo=0.1, agnostic=True, means=(0.01, -0.02, 0.03, 0.0)),
    dict(id="all_fg", frac=1.0, bg_lo=0.0, agnostic=False, means=(0, 0, 0, 0)),
    dict(id="no_rois", frac=0.25, bg_lo=0.0, agnostic=False, means=(0, 0, 0, 0), num_rois=(0, 0, 0)),
    dict(id="no_gt", frac=0.25, bg_lo=0.0, agnostic=False, means=(0, 0, 0, 0), no_gt=True),
]


@functools.lru_cache(maxsize=None)
def pt_inputs():
    rng = np.random.default_rng(201)
    gt = -np.ones((PT_N, PT_G, 5), np.float32)
    slots = [[1, 2, 5, 6, 9], [0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3]]             # image 0: holes
    rois = np.zeros((PT_N, PT_S, 5), np.float32)
    for n in range(PT_N):
        g = _big_gt(rng, len(slots[n]), 50, 200)
        gt[n, slots[n]] = g
        b = synth_boxes(rng, PT_S, IM_H, IM_W)
        where = rng.choice(PT_S, 600, replace=False)                            # scattered: every trip holds some
        b[where] = g[rng.integers(0, len(g), 600), :4] + rng.uniform(-4, 4, (600, 4)).astype(np.float32)
        rois[n, :, 0] = n
        rois[n, :, 1:] = b
    return rois, np.array([PT_S, PT_S + 500, 1100], np.int32), gt


def pt_case(row):
    rois, num_rois, gt = pt_inputs()
    if "num_rois" in row:
        num_rois = np.array(row["num_rois"], np.int32)
    if row.get("no_gt"):
        gt = gt.copy()
        gt[:, :, 4] = -1
    return dict(row, rois=rois, num_rois=num_rois, gt=gt, seed=99, step=3, image_offset=8)


def oracle_pt(c, step=None):
    return O().proposal_target(c["rois"], c["num_rois"], c["gt"], PT_R, c["frac"], 0.5, 0.5, c["bg_lo"], 81, c["agnostic"],
                               c["means"], PT_STDS, c["seed"], c["step"] if step is None else step, c["image_offset"])


def pt_candidate_index(c, out_rois, n):
    """Candidate index (position among the image's rois followed by its valid GT) of every output row of image n."""
    nr = int(min(max(c["num_rois"][n], 0), PT_S))
    valid = np.flatnonzero(c["gt"][n, :, 4] >= 0)
    cand = np.concatenate([c["rois"][n, :nr, 1:], c["gt"][n, valid, :4]])
    table = {}
    for i, b in enumerate(cand):
        table.setdefault(b.tobytes(), i)
    return np.array([table.get(r[1:].tobytes(), -1) for r in out_rois[n]], np.int64), len(cand)


@pytest.mark.parametrize("row", PT_ROWS, ids=ids(PT_ROWS))
def test_proposal_target_case_reaches_its_branch(row):
    c = pt_case(row)
    out_rois, labels, tgt, wgt, matched, nfg = oracle_pt(c)
    npad = (labels < 0).sum(1)
    nbg = PT_R - nfg - npad
    if row["id"] == "default":
        assert list(c["num_rois"]) == [2500, 3000, 1100] and c["num_rois"][1] > PT_S
        assert list(np.flatnonzero(c["gt"][0, :, 4] >= 0)) == [1, 2, 5, 6, 9]
        for n in range(PT_N):
            idx, nc = pt_candidate_index(c, out_rois, n)
            assert nc > PT_TRIP and (idx >= 0).all()
            fg_trips = set(idx[: nfg[n]] // PT_TRIP)
            bg_trips = set(idx[nfg[n]: nfg[n] + nbg[n]] // PT_TRIP)
            assert len(fg_trips) >= 2 and len(bg_trips) >= 2, (n, fg_trips, bg_trips)
            assert nfg[n] == 128 and nbg[n] == 384
        idx, _ = pt_candidate_index(c, out_rois, 0)
        assert len(set(idx[: nfg[0]] // PT_TRIP)) == 3 and len(set(idx[128:] // PT_TRIP)) == 3     # all three trips
    elif row["id"] == "bg_lo_agnostic_means":
        assert tgt.shape[2] == 4 and (npad > 0).sum() >= 2 and (nbg > 0).all(), npad
    elif row["id"] == "all_fg":
        full = [n for n in range(PT_N) if nfg[n] == PT_R]
        mixed = [n for n in range(PT_N) if 0 < nfg[n] < PT_R and nbg[n] == PT_R - nfg[n]]
        assert len(full) == 2 and len(mixed) == 1, (nfg, nbg)
    elif row["id"] == "no_rois":
        nv = (c["gt"][:, :, 4] >= 0).sum(1)
        assert (nfg == nv).all() and (nbg == 0).all() and (npad == PT_R - nv).all()
    elif row["id"] == "no_gt":
        assert (nfg == 0).all() and (nbg[:2] == PT_R).all() and (matched[labels == 0] == -1).all()
    else:
        raise AssertionError(row["id"])


# ---------------------------------------------------------------------------------------------------------------------
# proposal (chip-wide select, tie split, decode, level merge)
# ---------------------------------------------------------------------------------------------------------------------
def _hw(n):
    """(H, W) with H * W == n, as square as possible."""
    h = int(np.sqrt(n))
    while n % h:
        h -= 1
    return h, n // h


QUANT8 = np.array([-1.0, -0.5, -0.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32)      # bf16-exact, both zeros


def _prop(cid, branch, A, sizes, strides, pre, post, logits, N=2, min_size=4.0, thresh=0.7, im_info=None, seed=0, dtypes=("f32",),
          tie_level=None):
    return dict(id=cid, branch=branch, A=A, sizes=sizes, strides=strides, pre=pre, post=post, logits=logits, N=N,
                min_size=min_size, thresh=thresh, im_info=im_info, seed=seed, dtypes=dtypes, tie_level=tie_level)


def _proposal_table():
    k = consts()
    ch, mp = k["kSelChunk"], k["kMaxPre"]
    T = []
    for pre, post in ((512, 400), (600, 500), (mp, 1000)):
        sizes = sorted({2 * ch, ch + 1, ch, pre, pre - 1}, reverse=True)
        st = [4, 8, 8, 16, 32][: len(sizes)]
        T.append(_prop("sizes_pre%d" % pre, "level sizes {2,1 chunk, chunk+1, pre_n, pre_n-1}; pre_n %d" % pre, 1, sizes, st,
                       pre, post, "distinct", seed=300 + pre))
    T.append(_prop("tie_across_chunks", "cut inside a tie that spans chunk boundaries (f32 4-pass split; bf16)", 1,
                   [2 * ch, ch + 1], [8, 16], 600, 500, "quant8", seed=310, dtypes=("f32", "bf16"), tie_level=0))
    T.append(_prop("tie_pre_max", "cut inside a tie, pre_n = kMaxPre", 1, [2 * ch], [8], mp, 1000, "quant8", seed=311,
                   dtypes=("f32", "bf16"), tie_level=0))
    T.append(_prop("constant_level", "one level is a single tie", 3, [3 * 1500, 3 * 400], [8, 16], 600, 500, "const0", seed=312,
                   dtypes=("f32", "bf16"), tie_level=0))
    T.append(_prop("signed_zero", "logits are +0.0 and -0.0 only: the cut splits the +0.0 class", 1, [2 * ch, 900], [8, 16], 600, 500,
                   "zeros", seed=313, dtypes=("f32", "bf16"), tie_level=0))
    T.append(_prop("min_size_empties_level", "min_size leaves level 0 with nothing after decode", 3, [3 * 1200, 3 * 80], [4, 64],
                   600, 500, "distinct", seed=314, min_size=150.0))
    T.append(_prop("post_below_pre", "post_n < pre_n: NMS cap and merge cap", 3, [3 * 1600, 3 * 400, 3 * 100], [8, 16, 32], 600, 100,
                   "distinct", seed=315))
    T.append(_prop("post_above_kept", "post_n above the total kept: padding rows", 3, [3 * 20, 3 * 6], [32, 64], 600, 600,
                   "distinct", seed=316))
    T.append(_prop("single_level", "L = 1", 3, [3 * 1400], [8], 600, 300, "distinct", seed=317))
    T.append(_prop("three_images", "N = 3, a different im_info per image", 3, [3 * 1400, 3 * 350], [8, 16], 600, 500, "distinct",
                   N=3, seed=318, im_info=[[192, 320, 1.0], [180, 300, 1.5], [120, 200, 0.5]]))
    return T


PROPOSAL_CASES = _proposal_table()


@functools.lru_cache(maxsize=None)
def proposal_inputs(cid, dtype="f32"):
    """scores[l] [N, n_l], deltas[l] [N, n_l, 4] (canonical (y,x,a) order), shapes, base anchors, im_info."""
    c = next(x for x in PROPOSAL_CASES if x["id"] == cid)
    o = O()
    rng = np.random.default_rng(c["seed"])
    A, N = c["A"], c["N"]
    shapes = [_hw(n // A) for n in c["sizes"]]
    base = [o.base_anchors(s) if A == 3 else o.base_anchors(s, ratios=(1.0,)) for s in c["strides"]]
    scores, deltas = [], []
    for l, n_l in enumerate(c["sizes"]):
        kind = c["logits"]
        if kind == "const0" and l != 0:
            kind = "distinct"
        if kind == "distinct":
            s = np.stack([(rng.permutation(n_l) - n_l // 2) / np.float32(512) for _ in range(N)]).astype(np.float32)   # no two equal
        elif kind == "quant8":
            s = QUANT8[rng.integers(0, 8, (N, n_l))]
        elif kind == "const0":
            s = np.full((N, n_l), 0.375, np.float32)
        elif kind == "zeros":
            s = np.where(rng.integers(0, 2, (N, n_l)) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        d = (rng.standard_normal((N, n_l, 4)) * 0.3).astype(np.float32)
        if dtype == "bf16":
            s, d = o.round_bf16(s), o.round_bf16(d)
        scores.append(s)
        deltas.append(d)
    if c["im_info"] is not None:
        im_info = np.array(c["im_info"], np.float32)
    else:
        hmax = max(H * s for (H, W), s in zip(shapes, c["strides"]))
        wmax = max(W * s for (H, W), s in zip(shapes, c["strides"]))
        im_info = np.array([[hmax, wmax, 1.0], [hmax - 20, wmax - 33, 1.0]][:N], np.float32)
    return dict(case=c, scores=scores, deltas=deltas, shapes=shapes, base=base, im_info=im_info)


def oracle_proposal(inp):
    c = inp["case"]
    return O().proposal(inp["scores"], inp["deltas"], inp["base"], [s[0] for s in inp["shapes"]], [s[1] for s in inp["shapes"]],
                        c["strides"], inp["im_info"], c["pre"], c["post"], c["thresh"], c["min_size"])


def tie_at_cut(scores_row, pre):
    """For one list: (members of the tie class at rank pre_n, how many of them the cut takes), by numpy sort on the keys."""
    key = float_key(scores_row)
    order = np.lexsort((np.arange(len(key)), ~key))                    # key descending, index ascending
    kcut = key[order[pre - 1]]
    members = np.flatnonzero(key == kcut)
    return members, pre - int((key > kcut).sum())


@pytest.mark.parametrize("c", PROPOSAL_CASES, ids=ids(PROPOSAL_CASES))
def test_proposal_case_reaches_its_branch(c):
    k = consts()
    ch = k["kSelChunk"]
    assert c["pre"] <= k["kMaxPre"] and max(c["sizes"]) <= 2 * ch and 0 < c["post"] <= c["pre"] * len(c["sizes"])
    for dtype in c["dtypes"]:
        inp = proposal_inputs(c["id"], dtype)
        rois, sc, anc, num = oracle_proposal(inp)
        off = np.concatenate([[0], np.cumsum(c["sizes"])])
        assert all(H * W * c["A"] == n for (H, W), n in zip(inp["shapes"], c["sizes"]))
        if c["id"].startswith("sizes_pre"):
            pre = c["pre"]
            assert {2 * ch, ch, ch + 1, pre, pre - 1} == set(c["sizes"])
            assert (pre & (pre - 1) == 0) == (pre != 600)              # 512 and kMaxPre: Kpad == pre_n; 600: Kpad > pre_n
            for s in inp["scores"]:                                    # distinct logits: no tie at any cut
                assert all(len(np.unique(row)) == len(row) for row in s)
        if c["tie_level"] is not None:
            l = c["tie_level"]
            for n in range(c["N"]):
                members, taken = tie_at_cut(inp["scores"][l][n], c["pre"])
                assert 0 < taken < len(members), (taken, len(members))
                if c["sizes"][l] > ch:
                    assert len(set(members // ch)) >= 2                # the tie list is fed by more than one workgroup
                if c["id"] == "constant_level":
                    assert len(members) == c["sizes"][l]
                if c["id"] == "signed_zero":
                    s = inp["scores"][l][n]
                    assert set(s.view(np.uint32)) == {0, 0x80000000} and (s.view(np.uint32)[members] == 0).all()
        if c["id"] == "min_size_empties_level":
            for n in range(c["N"]):
                a = anc[n, : num[n]]
                assert num[n] > 0 and (a >= off[1]).all()              # nothing of level 0 survives ...
            loose = O().proposal(inp["scores"], inp["deltas"], inp["base"], [s[0] for s in inp["shapes"]],
                                 [s[1] for s in inp["shapes"]], c["strides"], inp["im_info"], c["pre"], c["post"], c["thresh"], 4.0)
            assert all((loose[2][n, : loose[3][n]] < off[1]).any() for n in range(c["N"]))      # ... because of min_size
        if c["id"] == "post_below_pre":
            assert c["post"] < c["pre"] and (num == c["post"]).all()
            loose = O().proposal(inp["scores"], inp["deltas"], inp["base"], [s[0] for s in inp["shapes"]],
                                 [s[1] for s in inp["shapes"]], c["strides"], inp["im_info"], c["pre"], c["pre"], c["thresh"],
                                 c["min_size"])
            assert (loose[3] > c["post"]).all()                        # the caps bind: more would have been kept
        if c["id"] == "post_above_kept":
            assert (num < c["post"]).all() and (num > 0).all() and (anc[0, num[0]:] == -1).all()
        if c["id"] == "single_level":
            assert len(c["sizes"]) == 1
        if c["id"] == "three_images":
            assert c["N"] == 3 and len({tuple(r) for r in inp["im_info"]}) == 3 and (num > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# NMS (nms_mask_kernel, nms_scan_rows_kernel<32>, nms_scan_kernel)
# ---------------------------------------------------------------------------------------------------------------------
NMS_NMAX = (2048, 2049, 4096)
NMS_MAX_KEEP = (None, 0, 1, 70)
NMS_THRESH = 0.5


def np_iou_matrix(a, b):
    """float32 IoU of every box of a against every box of b: the restatement of tests/test_math.py (_np_iou), the same
    float32 operations in the same order, on arrays."""
    f = np.float32
    a, b = np.asarray(a, f)[:, None, :], np.asarray(b, f)[None, :, :]
    iw = (np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])) + f(1)
    ih = (np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])) + f(1)
    inter = (iw * ih).astype(f)
    aa = ((a[..., 2] - a[..., 0]) + f(1)) * ((a[..., 3] - a[..., 1]) + f(1))
    ab = ((b[..., 2] - b[..., 0]) + f(1)) * ((b[..., 3] - b[..., 1]) + f(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (inter / ((aa + ab) - inter)).astype(f)
    return np.where((iw <= 0) | (ih <= 0), f(0), v)


def _clustered(rng, n):
    b = synth_boxes(rng, n)
    b[n // 2:] = b[: n - n // 2] + rng.uniform(-6, 6, (n - n // 2, 4)).astype(np.float32)
    return b


@functools.lru_cache(maxsize=None)
def nms_case(kind, n_max):
    """kind 'counts': eight clustered lists of the eight lengths; kind 'shapes': one list per named geometry."""
    rng = np.random.default_rng(400 + n_max)
    if kind == "counts":
        counts = np.array([0, 1, 63, 64, 65, 2047, 2048, n_max], np.int32)
        boxes = np.stack([_clustered(rng, n_max) for _ in counts])
        invalid = (rng.uniform(size=boxes.shape[:2]) < 0.05).astype(np.uint8)
        names = ["count_%d" % v for v in counts]
    else:
        names = ["identical", "disjoint_grid", "chain", "exact_pair", "all_invalid", "short_in_large"]
        boxes = np.zeros((len(names), n_max, 4), np.float32)
        counts = np.full((len(names),), n_max, np.int32)
        invalid = np.zeros((len(names), n_max), np.uint8)
        boxes[0] = [10, 20, 110, 90]
        i = np.arange(n_max)
        boxes[1] = np.stack([(i % 64) * 20, (i // 64) * 20, (i % 64) * 20 + 9, (i // 64) * 20 + 9], 1)
        boxes[2] = np.stack([4 * i, 0 * i, 4 * i + 15, 0 * i + 15], 1)
        boxes[3, :2] = [[0, 0, 9, 9], [0, 0, 9, 4]]
        counts[3] = 2
        boxes[4] = _clustered(rng, n_max)
        invalid[4] = 1
        boxes[5] = _clustered(rng, n_max)
        boxes[5, :100] = _clustered(rng, 100)                          # suppression inside the 100 that count
        counts[5] = 100
    return dict(names=names, boxes=boxes, counts=counts, invalid=invalid, n_max=n_max, thresh=NMS_THRESH)


def oracle_nms_case(c, max_keep=None):
    o = O()
    return [o.nms(c["boxes"][b, : c["counts"][b]], c["thresh"], max_keep, c["invalid"][b, : c["counts"][b]])
            for b in range(len(c["counts"]))]


def check_nms_invariants(boxes, invalid, keep, thresh):
    """Oracle-free: kept indices ascend, no two kept boxes overlap above thresh, every valid dropped box has an earlier kept
    box above thresh. boxes / invalid: the first `count` entries of one list; keep: the untruncated result."""
    keep = np.asarray(keep, np.int64)
    assert (np.diff(keep) > 0).all() and (invalid[keep] == 0).all()
    kb = boxes[keep]
    iou_kk = np_iou_matrix(kb, kb)
    assert not (np.triu(iou_kk, 1) > np.float32(thresh)).any()
    dropped = np.setdiff1d(np.flatnonzero(invalid == 0), keep)
    if len(dropped):
        iou_dk = np_iou_matrix(boxes[dropped], kb)
        earlier = keep[None, :] < dropped[:, None]
        assert ((iou_dk > np.float32(thresh)) & earlier).any(1).all()


@pytest.mark.parametrize("n_max", NMS_NMAX)
def test_nms_cases_are_what_they_are_named(n_max):
    sw = consts()["nms_rows_words"]
    assert ((n_max + 63) // 64 <= sw) == (n_max == 2048)               # 2048: register-row scan; 2049, 4096: LDS scan
    c = nms_case("counts", n_max)
    assert list(c["counts"]) == [0, 1, 63, 64, 65, 2047, 2048, n_max]
    keeps = oracle_nms_case(c)
    for b in range(8):
        n = c["counts"][b]
        assert (len(keeps[b]) == 0) == (n == 0 or bool(c["invalid"][b, :n].all())) and (n < 2047 or len(keeps[b]) < n - 8)
        check_nms_invariants(c["boxes"][b, :n], c["invalid"][b, :n], keeps[b], c["thresh"])
    s = nms_case("shapes", n_max)
    keeps = dict(zip(s["names"], oracle_nms_case(s)))
    assert list(keeps["identical"]) == [0]
    assert np.array_equal(keeps["disjoint_grid"], np.arange(n_max))
    assert np.array_equal(keeps["chain"], np.arange(0, n_max, 2))      # box 64 survives only because box 63 was dropped
    iou = np_iou_matrix(s["boxes"][2, 62:66], s["boxes"][2, 62:66])
    assert iou[1, 2] > 0.5 and iou[0, 1] > 0.5 and iou[0, 2] <= 0.5    # 63 would suppress 64; 62 suppresses 63
    pair = np_iou_matrix(s["boxes"][3, :1], s["boxes"][3, 1:2])[0, 0]
    assert pair.view(np.uint32) == np.float32(0.5).view(np.uint32)     # bit-equal to the threshold ...
    assert list(keeps["exact_pair"]) == [0, 1]                         # ... so not suppressed (strictly greater only)
    assert float(O().box_iou(s["boxes"][3, :1], s["boxes"][3, 1:2])[0, 0]) == 0.5
    assert len(keeps["all_invalid"]) == 0
    assert 0 < len(keeps["short_in_large"]) < 100 and s["counts"][5] * 8 < n_max
    for mk in NMS_MAX_KEEP[1:]:
        cut = oracle_nms_case(s, mk)
        for name, full in keeps.items():
            assert np.array_equal(cut[s["names"].index(name)], full[:mk])


# ---------------------------------------------------------------------------------------------------------------------
# detection postprocess (det_class_sort_kernel, det_merge_kernel)
# ---------------------------------------------------------------------------------------------------------------------
PP_SHAPES = [(64, 3), (1000, 81), (1024, 21), (4096, 2)]
PP_STDS = (0.1, 0.1, 0.2, 0.2)
PP_SCORE_THRESH, PP_NMS_THRESH = 0.02, 0.5
PP_MERGE_LDS = 150 * 1024           # the entry point's limit on (C-1) * (8 * max_per_image + 4) bytes


def pp_ids():
    return ["R%d_C%d" % rc for rc in PP_SHAPES]


def _pp_oracle(c, max_det):
    return O().detection_postprocess(c["cls"], c["reg"], c["rois"], c["num_rois"], c["im_info"], (0, 0, 0, 0), PP_STDS,
                                     PP_SCORE_THRESH, PP_NMS_THRESH, max_det)


@functools.lru_cache(maxsize=None)
def pp_case(R, C):
    """Inputs plus the two max_per_image values whose cut falls inside a tie (same class: broken by roi; other class: broken
    by roi, then class), found on the oracle's untruncated ranking."""
    rng = np.random.default_rng(500 + R + C)
    N = 3
    num_rois = np.array([R, (2 * R) // 3 + 1, 0], np.int32)
    ctr = np.stack([rng.uniform(40, 660, N * R), rng.uniform(40, 600, N * R)], 1).astype(np.float32)
    wh = np.exp(rng.uniform(np.log(16), np.log(120), (N * R, 2))).astype(np.float32)
    rois = np.zeros((N * R, 5), np.float32)
    rois[:, 0] = np.repeat(np.arange(N), R)
    rois[:, 1:3] = ctr - wh / 2
    rois[:, 3:5] = ctr + wh / 2
    nuniq = max(R // 4, 8)
    rows = np.round(rng.standard_normal((nuniq, C)) * 2.5 * 8) / 8
    hot = rng.permutation(nuniq)[: max(nuniq // 3, 4)]
    empty_cls = full_cls = None
    if C >= 5:
        empty_cls, full_cls = 1, 2
        rows[:, 3] = rows[:, 4]                                        # equal logits inside a row: equal scores across classes
        rows[hot[::2], 3:5] += 14.0                                    # ... some of them confident
        rows[hot[1::2], rng.integers(3, C, len(hot[1::2]))] += 8.0     # confident in one class: ties across rois only
        rows[:, empty_cls] = -40.0
        rest = np.delete(rows, full_cls, axis=1)                       # the full class: probability 0.06 in every row
        rows[:, full_cls] = np.log(np.exp(rest).sum(1)) + np.log(0.06 / 0.94)
    elif C == 3:
        rows[::2, 1] = rows[::2, 2]
        rows[hot, rng.integers(1, C, len(hot))] += 8.0
    else:
        rows[:, 1] = rows[:, 0] + np.abs(rows[:, 1]) * 0.25            # C == 2: every roi is a candidate of the one class
    cls = np.tile(rows, (N * R // nuniq + 1, 1))[: N * R].astype(np.float32)      # rows repeat across rois
    reg = (rng.standard_normal((N * R, 4 * C)) * 0.5).astype(np.float32)
    c = dict(id="R%d_C%d" % (R, C), R=R, C=C, N=N, cls=cls, reg=reg, rois=rois, num_rois=num_rois,
             im_info=np.array([[640.0, 704.0, 1.0]] * N, np.float32), empty_cls=empty_cls, full_cls=full_cls)
    cap = min(R, (PP_MERGE_LDS // (C - 1) - 4) // 8)
    dets, num, _, _ = _pp_oracle(c, cap)
    same = other = None
    for k in range(2, int(num[:2].min())):
        for n in (0, 1):
            a, b = dets[n, k - 1], dets[n, k]
            if a[4:5].view(np.uint32) == b[4:5].view(np.uint32):
                if a[5] == b[5] and same is None:
                    same = k
                if a[5] != b[5] and other is None:
                    other = k
    c["cap"], c["cuts"] = cap, [v for v in (same, other) if v is not None]
    c["cut_same"], c["cut_other"] = same, other
    return c


@pytest.mark.parametrize("R,C", PP_SHAPES, ids=pp_ids())
def test_postprocess_case_reaches_its_branch(R, C):
    c = pp_case(R, C)
    k = consts()
    assert R <= k["kDetMaxRois"] and (R == 4096) == (R == k["kDetMaxRois"])
    assert list(c["num_rois"]) == [R, (2 * R) // 3 + 1, 0]
    assert c["cut_same"] is not None and (C == 2 or c["cut_other"] is not None)
    for cut in c["cuts"]:
        assert 0 < cut <= R and (C - 1) * (8 * cut + 4) <= PP_MERGE_LDS
        dets, num, scores, _ = _pp_oracle(c, cut)
        more = _pp_oracle(c, cut + 1)[0]
        hit = [n for n in (0, 1) if num[n] == cut and
               dets[n, cut - 1, 4:5].view(np.uint32) == more[n, cut, 4:5].view(np.uint32)]
        assert hit, cut                                                # last kept and first dropped: bit-equal scores
        assert np.array_equal(dets.view(np.uint32), more[:, :cut].view(np.uint32)) and num[2] == 0
    if c["empty_cls"] is not None:
        _, _, scores, _ = _pp_oracle(c, c["cuts"][0])
        s = scores.reshape(c["N"], R, C)
        for n in (0, 1):
            nr = c["num_rois"][n]
            assert not (s[n, :nr, c["empty_cls"]] > PP_SCORE_THRESH).any()        # a class without a candidate ...
            assert (s[n, :nr, c["full_cls"]] > PP_SCORE_THRESH).all()             # ... next to one where every roi is one
