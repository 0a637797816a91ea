"""Float64 definitions of multi-level RoIAlign (Detectron aligned=False), its adjoint, the Mask R-CNN mask target and the
inference mask paste, written from the operations' definitions in plain numpy / torch. They share no code with the HIP
kernels or with oracle/mxdet_oracle.c: tests/test_roi_cases_cpu.py checks that this statement and the C oracle's agree
before any kernel runs, tests/test_gpu_roi_shapes.py measures the kernels against this one.

The roi arithmetic that the operators do on float32 inputs (the scale multiply, the width / height differences, the bin
size and the sample coordinate) is evaluated in float32 here too, so that the reference describes the same sample
points; everything after the sample coordinate (weights, sums, the mean) is float64.
"""
import numpy as np
import torch

F32 = np.float32


def align_coords(start, length, P, g):
    """float32 coordinates of the P*g samples of one RoIAlign axis: sample i of bin b sits at start + b*bin + (i+0.5)*bin/g
    (start / length: float32 scalars, length already clamped to >= 1)."""
    bin_ = F32(length) / F32(P)
    b = np.repeat(np.arange(P), g).astype(F32)
    i = np.tile(np.arange(g), P).astype(F32)
    return (F32(start) + b * bin_) + ((i + F32(0.5)) * bin_) / F32(g)


def axis_taps(v32, L):
    """Per sample coordinate (float32): the coordinate as float64, whether it counts, lo, hi and the weight of hi.
    A sample is dropped iff v < -1 or v > L; otherwise it is clamped at 0 and at L-1 and interpolated between lo and hi."""
    assert v32.dtype == np.float32
    v = v32.astype(np.float64)
    counts = ~((v < -1.0) | (v > float(L)))
    c = np.clip(v, 0.0, float(L - 1))
    lo = np.floor(c).astype(np.int64)
    hi = np.minimum(lo + 1, L - 1)
    return v, counts, lo, hi, c - lo


def roi_geometry(maps, scales, rois, levels, PH, PW, sr, lvl_min, N, r):
    """Everything the definition derives from roi r: level index, image, grid, sample coordinates and taps of both axes."""
    nl = len(maps)
    l = int(np.clip(int(levels[r]) - lvl_min, 0, nl - 1))
    n = int(np.clip(int(np.trunc(float(rois[r, 0]))), 0, N - 1))
    q = np.asarray(rois[r], F32)
    s = F32(scales[l])
    x1, y1, x2, y2 = q[1] * s, q[2] * s, q[3] * s, q[4] * s
    rw, rh = max(F32(x2 - x1), F32(1.0)), max(F32(y2 - y1), F32(1.0))
    if sr > 0:
        gh = gw = sr
    else:
        gh, gw = int(np.ceil(F32(rh) / F32(PH))), int(np.ceil(F32(rw) / F32(PW)))
    H, W = maps[l]
    ys = axis_taps(align_coords(y1, rh, PH, gh), H)
    xs = axis_taps(align_coords(x1, rw, PW, gw), W)
    return dict(l=l, n=n, gh=gh, gw=gw, H=H, W=W, ys=ys, xs=xs, bin_h=float(F32(rh) / F32(PH)), bin_w=float(F32(rw) / F32(PW)))


def _axis_matrix(samples, P, g, L):
    """[P, L] float64: row b holds the summed interpolation weights of bin b's counted samples on each pixel."""
    v, counts, lo, hi, frac = samples
    A = np.zeros((P, L), np.float64)
    b = np.repeat(np.arange(P), g)
    np.add.at(A, (b[counts], lo[counts]), (1.0 - frac)[counts])
    np.add.at(A, (b[counts], hi[counts]), frac[counts])
    return A


def _matrices(maps, scales, rois, levels, PH, PW, sr, lvl_min, N, r):
    g = roi_geometry(maps, scales, rois, levels, PH, PW, sr, lvl_min, N, r)
    Ay = torch.from_numpy(_axis_matrix(g["ys"], PH, g["gh"], g["H"]))
    Ax = torch.from_numpy(_axis_matrix(g["xs"], PW, g["gw"], g["W"]))
    return g, Ay, Ax


def roi_align_ref(feats64, scales, rois, levels, PH, PW, sr, lvl_min, N):
    """feats64[l]: float64 torch [N,H,W,C]; rois [R,5] float32 (numpy); levels [R] -> float64 torch [R,PH,PW,C]: the mean
    over the gh*gw samples of every bin of the bilinear interpolation (dropped samples add 0; the divisor stays gh*gw).
    A sample counts iff both its coordinates do, so the sum over a bin's samples factors into a row and a column part."""
    rois = np.asarray(rois, F32).reshape(-1, 5)
    maps = [(f.shape[1], f.shape[2]) for f in feats64]
    C = feats64[0].shape[3]
    out = []
    for r in range(rois.shape[0]):
        g, Ay, Ax = _matrices(maps, scales, rois, levels, PH, PW, sr, lvl_min, N, r)
        out.append(torch.einsum("ph,hwc,qw->pqc", Ay, feats64[g["l"]][g["n"]], Ax) / float(g["gh"] * g["gw"]))
    return torch.stack(out) if out else torch.zeros((0, PH, PW, C), dtype=torch.float64)


def roi_align_ref_backward(maps, scales, rois, levels, grad64, sr, lvl_min, N):
    """The exact adjoint: grad64 float64 torch [R,PH,PW,C] -> per-level float64 maps [N,H,W,C] (maps: [(H, W)] per level).
    Hand-written; tests/test_roi_cases_cpu.py checks it against autograd of roi_align_ref and <fwd(x), g> = <x, bwd(g)>."""
    rois = np.asarray(rois, F32).reshape(-1, 5)
    R, PH, PW, C = grad64.shape
    d = [torch.zeros((N, H, W, C), dtype=torch.float64) for H, W in maps]
    for r in range(R):
        g, Ay, Ax = _matrices(maps, scales, rois, levels, PH, PW, sr, lvl_min, N, r)
        d[g["l"]][g["n"]] += torch.einsum("ph,pqc,qw->hwc", Ay, grad64[r], Ax) / float(g["gh"] * g["gw"])
    return d


def mask_target_ref(rois, matched, labels, masks, S):
    """rois [R,5] f32 (image, x1, y1, x2, y2 in mask pixels), matched / labels [R], masks [N,G,H,W] {0,1} ->
    (targets u8 [R,S,S], cls i32 [R], value f64 [R,S,S]): value = the bilinear interpolation of the matched instance's mask
    at roi start + (p + 0.5) * bin (width and height clamped to >= 1; a sample with a coordinate < -1 or > L gives 0, the
    others clamp at 0 and L-1); target = value >= 0.5. cls = label iff label > 0 and 0 <= matched < G, else -1, target 0."""
    rois = np.asarray(rois, F32).reshape(-1, 5)
    N, G, H, W = masks.shape
    R = rois.shape[0]
    m64 = masks.astype(np.float64)
    val = np.zeros((R, S, S), np.float64)
    cls = np.full((R,), -1, np.int32)
    for r in range(R):
        lab, mg = int(labels[r]), int(matched[r])
        if not (lab > 0 and 0 <= mg < G):
            continue
        cls[r] = lab
        q = rois[r]
        rw, rh = max(F32(q[3] - q[1]), F32(1.0)), max(F32(q[4] - q[2]), F32(1.0))
        p = np.arange(S).astype(F32) + F32(0.5)
        _, cy, ylo, yhi, fy = axis_taps(q[2] + p * (rh / F32(S)), H)
        _, cx, xlo, xhi, fx = axis_taps(q[1] + p * (rw / F32(S)), W)
        m = m64[int(q[0]), mg]
        top = m[ylo][:, xlo] * (1 - fx)[None, :] + m[ylo][:, xhi] * fx[None, :]
        bot = m[yhi][:, xlo] * (1 - fx)[None, :] + m[yhi][:, xhi] * fx[None, :]
        v = top * (1 - fy)[:, None] + bot * fy[:, None]
        val[r] = np.where(cy[:, None] & cx[None, :], v, 0.0)
    return (val >= 0.5).astype(np.uint8), cls, val


def _paste_axis(first, length, S, L):
    """Destination pixels first .. first+length-1 that lie in [0, L), and per pixel the two source taps and the weight of
    the second: source coordinate (d + 0.5) * S / length - 0.5 (half-pixel centres), clamped at both ends."""
    d = np.arange(length, dtype=np.int64)
    keep = (first + d >= 0) & (first + d < L)
    d = d[keep]
    src = (d + 0.5) * (float(S) / float(length)) - 0.5
    s0 = np.floor(src)
    f = src - s0
    f = np.where((s0 < 0) | (s0 >= S - 1), 0.0, f)
    s0 = np.clip(s0, 0, S - 1).astype(np.int64)
    return first + d, s0, np.minimum(s0 + 1, S - 1), f


def mask_paste_ref(logits, dets, H, W, thresh=0.5):
    """logits [R,S,S,Cpad] (bf16-valued), dets [R,6] f32 (x1, y1, x2, y2, score, class) -> (masks u8 [R,H,W], value f64
    [R,H,W]): the sigmoid of the class channel, resized bilinearly into the inclusive integer box whose corners are the
    detection's rounded half-to-even; mask = value > thresh. Class <= 0, class > Cpad or an inverted box give zeros."""
    logits = np.asarray(logits, np.float64)
    dets = np.asarray(dets, F32).reshape(-1, 6)
    R, S, _, Cpad = logits.shape
    val = np.zeros((R, H, W), np.float64)
    for r in range(R):
        c = int(np.trunc(float(dets[r, 5])))
        bx1, by1, bx2, by2 = (int(v) for v in np.rint(dets[r, :4].astype(np.float64)))
        bw, bh = bx2 - bx1 + 1, by2 - by1 + 1
        if c <= 0 or c > Cpad or bw <= 0 or bh <= 0:
            continue
        p = 1.0 / (1.0 + np.exp(-logits[r, :, :, c - 1]))
        ys, y0, y1, fy = _paste_axis(by1, bh, S, H)
        xs, x0, x1, fx = _paste_axis(bx1, bw, S, W)
        if ys.size == 0 or xs.size == 0:
            continue
        top = p[y0][:, x0] * (1 - fx)[None, :] + p[y0][:, x1] * fx[None, :]
        bot = p[y1][:, x0] * (1 - fx)[None, :] + p[y1][:, x1] * fx[None, :]
        val[r][np.ix_(ys, xs)] = top * (1 - fy)[:, None] + bot * fy[:, None]
    return (val > float(F32(thresh))).astype(np.uint8), val
