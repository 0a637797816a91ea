"""GPU run of the case tables of tests/test_select_cases_cpu.py: the data-dependent branches of the selection, sampling and
NMS kernels (csrc/select.h, proposal.hip, targets.hip, boxes.hip, postprocess.hip) through the product's own Python ops,
against the C oracle. Every comparison is exact: integers as integers, floats by their uint32 bits. The CPU module proves
that each case reaches the branch it is named after; this module adds the checks that need no oracle (NMS invariants in
numpy, sampler arithmetic, determinism, image offsets) and the runs on scratch memory that is not fresh.
"""
import numpy as np
import pytest

import test_select_cases_cpu as T

pytestmark = pytest.mark.gpu


def _t(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _np(ts):
    return tuple(t.cpu().numpy() for t in ts)


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(got, want), what


# ---------------------------------------------------------------------------------------------------------------------
# anchor target
# ---------------------------------------------------------------------------------------------------------------------
def run_anchor(c, batch=None, step=None, image_offset=None, sl=slice(None), workspace=None):
    from mxdetection_amd.core.anchor import assign_anchor
    return _np(assign_anchor(_t(c["anchors"]), _t(c["gt"][sl]), _t(c["im_info"][sl]), c["fg"], c["bg"], 0.0,
                             c["batch"] if batch is None else batch, c["frac"], c["seed"], c["step"] if step is None else step,
                             c["image_offset"] if image_offset is None else image_offset, workspace=workspace))


def _anchor_equal(got, want, what):
    lab, mg, tg, mi = got
    w_lab, w_mg, w_tg, w_mi = want
    _same(lab, w_lab, what + ": labels")
    _same(mi, w_mi, what + ": max_iou")
    _same(mg[w_lab == 1], w_mg[w_lab == 1], what + ": matched_gt of the foreground")
    _same(tg, w_tg, what + ": targets")


@pytest.mark.parametrize("cid", T.ANCHOR_IDS)
def test_anchor_target_branches(hip, oracle, cid):
    c = T.anchor_case(cid)
    got = run_anchor(c)
    _anchor_equal(got, T.oracle_anchor(c), cid)
    pre = run_anchor(c, batch=0)
    _anchor_equal(pre, T.oracle_anchor(c, batch=0), cid + " (no sampling)")
    # sampler arithmetic and membership, against the kernel's own labels before sampling
    max_fg = int(np.float32(c["frac"]) * np.float32(c["batch"]))
    lab, lab0 = got[0], pre[0]
    subsampled = False
    for n in range(lab.shape[0]):
        n_fg, n_bg = int((lab0[n] == 1).sum()), int((lab0[n] == 0).sum())
        nfg = min(n_fg, max_fg)
        assert (lab[n] == 1).sum() == nfg and (lab[n] == 0).sum() == min(n_bg, c["batch"] - nfg)
        assert (lab0[n][lab[n] == 1] == 1).all() and (lab0[n][lab[n] == 0] == 0).all()
        subsampled |= n_fg > nfg or n_bg > c["batch"] - nfg > 0
    again = run_anchor(c)
    for a, b in zip(got, again):
        _same(a, b, cid + ": second launch")
    if subsampled:
        other = run_anchor(c, step=c["step"] + 1)
        assert not np.array_equal(other[0], lab)
        _anchor_equal(other, T.oracle_anchor(c, step=c["step"] + 1), cid + " (next step)")


def test_anchor_target_image_offset(hip, oracle):
    """One N=2 launch at image_offset 4 equals two N=1 launches at offsets 4 and 5 (both list paths in one grid)."""
    c = T.anchor_case("fg_list_overflow")
    assert c["image_offset"] == 4
    both = run_anchor(c)
    for n in (0, 1):
        one = run_anchor(c, image_offset=4 + n, sl=slice(n, n + 1))
        for a, b in zip(both, one):
            _same(a[n:n + 1], b, "image %d" % n)


def test_anchor_target_workspace_reuse(hip, oracle):
    """fg_list_overflow, then a launch with short lists, then the first again, all on one workspace: the candidate lists and
    counters of the launch before must not leak into the next."""
    import torch
    from mxdetection_amd.core.anchor import AnchorTargetWorkspace
    c = T.anchor_case("fg_list_overflow")
    N, A, G = c["gt"].shape[0], c["anchors"].shape[0], c["gt"].shape[1]
    ws = AnchorTargetWorkspace(N, A, G, torch.device("cuda"))
    ws.buf.fill_(0xFF)
    first = run_anchor(c, workspace=ws)
    _anchor_equal(first, T.oracle_anchor(c), "first")
    small = dict(c, gt=c["gt"].copy(), im_info=np.array([[150, 200, 1.0], [130, 260, 1.0]], np.float32))
    small["gt"][:, :, 4] = -1
    small["gt"][0, 0] = [20, 20, 90, 100, 3]
    small["gt"][1, 2] = [60, 10, 200, 110, 8]
    k = T.anchor_counts(small)
    assert all(b < w for b, w in zip(k["n_bg_below"], k["want_bg"])) and max(k["n_fg"]) <= T.consts()["kCandCap"]
    second = run_anchor(small, workspace=ws)
    _anchor_equal(second, T.oracle_anchor(small), "second")
    third = run_anchor(c, workspace=ws)
    for a, b in zip(first, third):
        _same(a, b, "third launch")


# ---------------------------------------------------------------------------------------------------------------------
# proposal target
# ---------------------------------------------------------------------------------------------------------------------
def run_pt(c, step=None):
    from mxdetection_amd.core.bbox import sample_rois
    return _np(sample_rois(_t(c["rois"]), _t(c["num_rois"]), _t(c["gt"]), T.PT_R, c["frac"], 0.5, 0.5, c["bg_lo"], 81,
                           c["agnostic"], c["means"], T.PT_STDS, c["seed"], c["step"] if step is None else step,
                           c["image_offset"]))


PT_NAMES = ["rois", "labels", "targets", "weights", "matched", "num_fg"]


@pytest.mark.parametrize("row", T.PT_ROWS, ids=T.ids(T.PT_ROWS))
def test_proposal_target_branches(hip, oracle, row):
    c = T.pt_case(row)
    got = run_pt(c)
    for g, w, nm in zip(got, T.oracle_pt(c), PT_NAMES):
        _same(g, w, row["id"] + ": " + nm)
    rois, labels, tgt, wgt, matched, nfg = got
    max_fg = int(np.float32(c["frac"]) * np.float32(T.PT_R))
    for n in range(T.PT_N):
        k = int(nfg[n])
        assert 0 <= k <= max_fg and (labels[n, :k] > 0).all() and (labels[n, k:] <= 0).all()
        nbg = int((labels[n] == 0).sum())
        assert (labels[n, k:k + nbg] == 0).all() and (labels[n, k + nbg:] == -1).all()      # fg, then bg, then padding
        idx, _ = T.pt_candidate_index(c, rois, n)
        assert (idx[: k + nbg] >= 0).all() and len(set(idx[: k + nbg])) == k + nbg          # each a candidate, none twice
        assert (np.diff(idx[:k]) > 0).all() and (np.diff(idx[k:k + nbg]) > 0).all()          # ascending candidate order
        assert (wgt[n].reshape(T.PT_R, -1).sum(1)[:k] == 4).all() and not wgt[n, k:].any()
    for a, b in zip(got, run_pt(c)):
        _same(a, b, row["id"] + ": second launch")
    if row["id"] in ("default", "bg_lo_agnostic_means", "all_fg"):
        other = run_pt(c, step=c["step"] + 1)
        assert not np.array_equal(other[0], rois)
        for g, w, nm in zip(other, T.oracle_pt(c, step=c["step"] + 1), PT_NAMES):
            _same(g, w, row["id"] + " (next step): " + nm)


# ---------------------------------------------------------------------------------------------------------------------
# proposal
# ---------------------------------------------------------------------------------------------------------------------
def _fused(inp, dtype):
    """One [N,H,W,Cpad] tensor per level: logits in channels 0..A-1, deltas in A..5A-1."""
    import torch
    A, N = inp["case"]["A"], inp["case"]["N"]
    Cp = (5 * A + 7) // 8 * 8
    out = []
    for s, d, (H, W) in zip(inp["scores"], inp["deltas"], inp["shapes"]):
        f = np.zeros((N, H, W, Cp), np.float32)
        f[..., :A] = s.reshape(N, H, W, A)
        f[..., A:5 * A] = d.reshape(N, H, W, 4 * A)
        out.append(_t(f, torch.bfloat16 if dtype == "bf16" else torch.float32))
    return out


def _make_op(inp):
    from mxdetection_amd.ops import PyramidProposal
    c = inp["case"]
    return PyramidProposal([_t(b) for b in inp["base"]], c["strides"], c["pre"], c["post"], c["thresh"], c["min_size"])


def _proposal_equal(got, want, what):
    rois, sc, anc, num = got
    w_rois, w_sc, w_anc, w_num = want
    _same(num, w_num, what + ": num_rois")
    _same(anc, w_anc, what + ": anchor index")
    _same(sc, w_sc, what + ": scores")
    _same(rois, w_rois, what + ": rois")


PROPOSAL_RUNS = [(c["id"], dt) for c in T.PROPOSAL_CASES for dt in c["dtypes"]]


@pytest.mark.parametrize("cid,dtype", PROPOSAL_RUNS, ids=["%s-%s" % r for r in PROPOSAL_RUNS])
def test_proposal_branches(hip, oracle, cid, dtype):
    inp = T.proposal_inputs(cid, dtype)
    op = _make_op(inp)
    f = _fused(inp, dtype)
    got = _np(op(f, f, _t(inp["im_info"])))
    _proposal_equal(got, T.oracle_proposal(inp), "%s %s" % (cid, dtype))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_proposal_workspace_reuse(hip, oracle, dtype):
    """One PyramidProposal object: tie-heavy logits, then distinct logits, then the tie-heavy ones again. Histograms,
    counters and tie lists of the launch before must not leak: both tie-heavy results are bit-identical and the oracle's."""
    X = T.proposal_inputs("tie_across_chunks", dtype)
    rng = np.random.default_rng(77)
    Y = dict(X, scores=[np.stack([(rng.permutation(s.shape[1]) - 100) / np.float32(64) for _ in range(s.shape[0])])
                        .astype(np.float32) for s in X["scores"]])
    if dtype == "bf16":
        Y["scores"] = [oracle.round_bf16(s) for s in Y["scores"]]
    op = _make_op(X)
    info = _t(X["im_info"])
    fx, fy = _fused(X, dtype), _fused(Y, dtype)
    first = _np(op(fx, fx, info))
    ws = op._ws
    second = _np(op(fy, fy, info))
    third = _np(op(fx, fx, info))
    assert op._ws is ws
    _proposal_equal(first, T.oracle_proposal(X), "first")
    _proposal_equal(second, T.oracle_proposal(Y), "second")
    for a, b in zip(first, third):
        _same(a, b, "third launch")


# ---------------------------------------------------------------------------------------------------------------------
# NMS
# ---------------------------------------------------------------------------------------------------------------------
def run_nms(c, max_keep=None):
    from mxdetection_amd.ops import nms_batched
    keep, num = nms_batched(_t(c["boxes"]), _t(c["counts"]), c["thresh"], max_keep=max_keep, invalid=_t(c["invalid"]))
    return keep.cpu().numpy(), num.cpu().numpy()


def _nms_equal(keep, num, want, what):
    for b, w in enumerate(want):
        assert num[b] == len(w), (what, b, num[b], len(w))
        assert np.array_equal(keep[b, : num[b]], w), (what, b)


@pytest.mark.parametrize("kind", ["counts", "shapes"])
@pytest.mark.parametrize("n_max", T.NMS_NMAX)
def test_nms_branches(hip, oracle, n_max, kind):
    c = T.nms_case(kind, n_max)
    keep, num = run_nms(c)
    _nms_equal(keep, num, T.oracle_nms_case(c), "%s %d" % (kind, n_max))
    for b in range(len(c["counts"])):                                  # no oracle: the definition of greedy NMS, in numpy
        n = c["counts"][b]
        T.check_nms_invariants(c["boxes"][b, :n], c["invalid"][b, :n], keep[b, : num[b]], c["thresh"])
    for mk in T.NMS_MAX_KEEP[1:]:
        k2, n2 = run_nms(c, mk)
        _nms_equal(k2, n2, T.oracle_nms_case(c, mk), "%s %d max_keep %d" % (kind, n_max, mk))
        for b in range(len(c["counts"])):
            assert n2[b] == min(mk, num[b]) and np.array_equal(k2[b, : n2[b]], keep[b, : n2[b]])


@pytest.mark.parametrize("n_max", T.NMS_NMAX)
def test_nms_workspace_not_fresh(hip, oracle, n_max):
    """mxdet_nms_batched on a workspace of exactly the reported size, pre-filled with 0xFF and with 0x00: the scan kernels read
    mask words the mask kernel never wrote (lower triangle, words and rows past a list) and must not use them. The 'shapes'
    batch holds full lists and lists much shorter than n_max (2 and 100 boxes)."""
    import torch
    from mxdetection_amd._lib import check, ptr, stream_ptr
    c = T.nms_case("shapes", n_max)
    B = len(c["counts"])
    want = T.oracle_nms_case(c)
    ref_keep, ref_num = run_nms(c)
    _nms_equal(ref_keep, ref_num, want, "wrapper")
    boxes, counts, invalid = _t(c["boxes"]), _t(c["counts"]), _t(c["invalid"])
    nbytes = hip.load().mxdet_nms_batched_workspace_bytes(B, n_max)
    for fill in (0xFF, 0x00):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        keep = torch.full((B, n_max), -1, dtype=torch.int32, device="cuda")
        num = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        check(hip.load().mxdet_nms_batched(ptr(boxes), ptr(counts), ptr(invalid), B, n_max, c["thresh"], n_max, ptr(keep),
                                           ptr(num), ptr(ws), nbytes, stream_ptr()), "nms_batched")
        keep, num = keep.cpu().numpy(), num.cpu().numpy()
        _nms_equal(keep, num, want, "fill %#x" % fill)
        assert np.array_equal(num, ref_num)
        for b in range(B):
            assert (keep[b, num[b]:] == -1).all()                      # nothing written past the kept count


# ---------------------------------------------------------------------------------------------------------------------
# detection postprocess
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", T.PP_SHAPES, ids=T.pp_ids())
def test_detection_postprocess_branches(hip, oracle, R, C):
    import torch
    from mxdetection_amd.core.evaluation import DetectionPostprocess
    c = T.pp_case(R, C)
    ld = (5 * C + 63) // 64 * 64
    fused = torch.zeros((c["N"] * R, ld), dtype=torch.float32, device="cuda")      # fused head layout: cls | reg | padding
    fused[:, :C] = _t(c["cls"])
    fused[:, C:5 * C] = _t(c["reg"])
    rois, num_rois, info = _t(c["rois"]), _t(c["num_rois"]), _t(c["im_info"])
    for cut in c["cuts"] + [min(c["cap"], 100)]:
        post = DetectionPostprocess(C, score_thresh=T.PP_SCORE_THRESH, nms_thresh=T.PP_NMS_THRESH, max_per_image=cut,
                                    stds=T.PP_STDS)
        dets, num = _np(post(fused[:, :C], fused[:, C:], rois, num_rois, info))
        w_dets, w_num, _, _ = T._pp_oracle(c, cut)
        _same(num, w_num, "%s cut %d: num" % (c["id"], cut))
        _same(dets[..., 5], w_dets[..., 5], "%s cut %d: classes" % (c["id"], cut))
        _same(dets, w_dets, "%s cut %d: boxes and scores" % (c["id"], cut))
        for n in range(c["N"]):                                        # no oracle: order and padding
            k = num[n]
            assert (np.diff(dets[n, :k, 4]) <= 0).all() and (dets[n, k:, 5] == -1).all() and (dets[n, :k, 5] >= 1).all()
            if c["empty_cls"] is not None:
                assert not (dets[n, :k, 5] == c["empty_cls"]).any()
