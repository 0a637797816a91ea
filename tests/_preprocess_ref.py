"""Independent references for the data-pipeline kernels (csrc/preprocess.hip): numpy and the standard library only, and
none of the kernels' arithmetic -- no 11-bit coefficients, no shifts, no fp32 intersection.

resize_exact        the mathematical bilinear resample in float64
normalise_bits      (v - mean) / std in IEEE float32, rounded to bf16 to nearest even
polygon_mask_exact  even-odd pixel-centre fill in rational arithmetic, with each pixel's distance to the nearest crossing
"""
from fractions import Fraction

import numpy as np


def _axis(dst, inv_scale, slen):
    """Source coordinate of every destination index: half-pixel centres, clamped at both borders; (i0, i1, frac)."""
    s = (np.arange(dst, dtype=np.float64) + 0.5) * float(inv_scale) - 0.5
    s = np.clip(s, 0.0, float(slen - 1))
    i0 = np.minimum(np.floor(s).astype(np.int64), max(slen - 2, 0))
    i1 = np.minimum(i0 + 1, slen - 1)
    return i0, i1, s - i0


def resize_exact(src_u8, dst_h, dst_w, inv_scale, flip):
    """float64 [dst_h, dst_w, 3]: the source (mirrored left-right when `flip`) sampled bilinearly at
    s = (d + 0.5) * inv_scale - 0.5 on both axes."""
    src = np.asarray(src_u8, np.float64)
    if flip:
        src = src[:, ::-1]
    y0, y1, fy = _axis(dst_h, inv_scale, src.shape[0])
    x0, x1, fx = _axis(dst_w, inv_scale, src.shape[1])
    fx = fx[None, :, None]
    top = src[y0][:, x0] * (1.0 - fx) + src[y0][:, x1] * fx
    bot = src[y1][:, x0] * (1.0 - fx) + src[y1][:, x1] * fx
    fy = fy[:, None, None]
    return top * (1.0 - fy) + bot * fy


def f32_to_bf16_bits(x):
    """bf16 bit patterns of finite float32 values, round to nearest even."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_to_f32(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def normalise_bits(v_int, mean, std):
    """bf16 bits of (float32(v) - float32(mean)) / float32(std): two separately rounded float32 operations."""
    v = np.asarray(v_int).astype(np.float32)
    d = np.subtract(v, np.float32(mean), dtype=np.float32)
    return f32_to_bf16_bits(np.divide(d, np.float32(std), dtype=np.float32))


def _frac(x):
    return Fraction(float(x))          # a float32 is a dyadic rational: exact


def polygon_mask_exact(verts, poly_start, inst_first, n_inst, H, W):
    """(mask [n_inst, H, W] u8, margin [n_inst, H, W] f64).

    Per polygon the even-odd rule at the pixel centre (x + 1/2, y + 1/2): an edge a -> b counts for the row when exactly
    one of a.y <= py, b.y <= py holds (half-open in y), and a pixel toggles when its centre is strictly left of the exact
    crossing xi = a.x + (py - a.y) (b.x - a.x) / (b.y - a.y). An instance is the OR of its polygons; polygons of fewer
    than 3 vertices do not count. margin is the smallest |x + 1/2 - xi| over the counted edges of the instance's row (inf
    without one); xi is exact, the distance is its float64 rounding (relative error 2^-52)."""
    verts = np.asarray(verts, np.float32).reshape(-1, 2)
    mask = np.zeros((n_inst, H, W), np.uint8)
    margin = np.full((n_inst, H, W), np.inf)
    centres = np.arange(W, dtype=np.float64) + 0.5
    half = Fraction(1, 2)
    for inst in range(n_inst):
        for p in range(int(inst_first[inst]), int(inst_first[inst + 1])):
            vb, ve = int(poly_start[p]), int(poly_start[p + 1])
            if ve - vb < 3:
                continue
            pts = [(_frac(verts[v, 0]), _frac(verts[v, 1])) for v in range(vb, ve)]
            for y in range(H):
                py = y + half
                par = np.zeros(W, np.uint8)
                for k in range(len(pts)):
                    (ax, ay), (bx, by) = pts[k - 1], pts[k]
                    if (ay <= py) == (by <= py):
                        continue
                    xi = ax + (py - ay) * (bx - ax) / (by - ay)
                    n_left = xi - half                       # centres x + 1/2 < xi  <=>  x < xi - 1/2
                    cnt = -((-n_left.numerator) // n_left.denominator)      # ceil
                    par[:min(max(cnt, 0), W)] ^= 1
                    margin[inst, y] = np.minimum(margin[inst, y], np.abs(centres - float(xi)))
                mask[inst, y] |= par
    return mask, margin
