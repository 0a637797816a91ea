// deform_conv.hip -- deformable convolution (DCN v1 / v2), the parts the MFMA GEMM kernels cannot do.
//
// Slot: models/backbones (reference README.md:27); MXNet role contrib.DeformableConvolution (README.md:37,
// Deformable-ConvNets' deformable_im2col / col2im / col2im_coord). The contraction itself is the existing 1x1
// mxdet_conv2d_fwd / _dgrad / _wgrad on the column tensor col [N,Ho,Wo,9*C] (tap-major, then channel): the [Cout,3,3,C]
// filter IS the [Cout,1,1,9C] filter of that 1x1 convolution. This file supplies
//   im2col       : the bilinear gather x -> col (one 16-B load per corner, a lane owns 8 channels as in roi_align.hip);
//   col2im_coord : d(loss)/d(offset) and, for v2, d(loss)/d(mask logit) from dcol, fixed-order channel reduction;
//   col2im       : d(loss)/d(x) from dcol WITHOUT float atomics -- an inverted index (input pixel -> its (output pixel,
//                  tap, corner, weight) entries in ascending key order) built with integer atomics + a per-list sort,
//                  then a gather that sums every input pixel's entries in fp32 in that order and rounds once to bf16.
//                  Bit-reproducible run to run (the RoIAlign gather backward's store-and-sum form).
// HBM/L2-gather bound: algorithmic bytes of im2col = col written (N*Ho*Wo*9*C*2) + x read once.
#include "common.h"

namespace mxdet {

struct DeformArgs {
  int N, H, W, C, Ho, Wo, stride, pad, G, mod, Coff, acc;
  int CG;      // C / 8: channel groups of 8 (one 16-B load)
  int CGg;     // CG / G: channel groups per deformable group
  long long P; // N * Ho * Wo output pixels
};

// One sample: bilinear corners of (py, px) and their weights; valid = inside the (-1, H) x (-1, W) window.
struct DSample {
  int y0, x0;
  float ly, lx, hy, hx;
  bool valid;
};

__device__ __forceinline__ void deform_pixel(const DeformArgs& a, long long p, int* n, int* ho, int* wo) {
  *wo = (int)(p % a.Wo);
  const long long t = p / a.Wo;
  *ho = (int)(t % a.Ho);
  *n = (int)(t / a.Ho);
}

// offsets (dy, dx) of tap k of deformable group g at output pixel p, and the v2 mask factor sigmoid(logit)
__device__ __forceinline__ DSample deform_sample(const DeformArgs& a, const uint16_t* __restrict__ off, long long p,
                                                 int ho, int wo, int k, int g, float* m) {
  const uint16_t* o = off + p * a.Coff;
  const float dy = bf16_bits_to_f32(o[g * 18 + 2 * k]);
  const float dx = bf16_bits_to_f32(o[g * 18 + 2 * k + 1]);
  *m = 1.0f;
  if (a.mod) *m = 1.0f / (1.0f + expf(-bf16_bits_to_f32(o[18 * a.G + 9 * g + k])));
  // The position is base + offset with an integer base: floor and fraction are taken from the offset alone, so they are
  // those of the real number (base + dy rounds in fp32 -- 2^-15 px at 728 -- and a sample that close to an integer
  // pixel would land on its other side, where d(sample)/d(offset) is another one-sided derivative). The rounded sum
  // only bounds the integer conversion (a NaN or huge offset is not valid).
  const int by = ho * a.stride - a.pad + k / 3, bx = wo * a.stride - a.pad + k % 3;
  const float py = (float)by + dy, px = (float)bx + dx;
  const bool inrange = py > -2.0f && py < (float)a.H + 1.0f && px > -2.0f && px < (float)a.W + 1.0f;
  const float fy = floorf(dy), fx = floorf(dx);
  DSample s;
  s.ly = dy - fy; s.lx = dx - fx;
  s.y0 = inrange ? by + (int)fy : 0;
  s.x0 = inrange ? bx + (int)fx : 0;
  // inside the open window (-1, H) x (-1, W)
  s.valid = inrange && (s.y0 >= 0 || (s.y0 == -1 && s.ly > 0.0f)) && s.y0 < a.H &&
            (s.x0 >= 0 || (s.x0 == -1 && s.lx > 0.0f)) && s.x0 < a.W;
  if (!s.valid) s.y0 = s.x0 = 0;
  s.hy = 1.0f - s.ly; s.hx = 1.0f - s.lx;
  return s;
}

// the four corner rows (8 channels from c0) of a valid sample; corners outside [0,H) x [0,W) read as zero
__device__ __forceinline__ void load_corners(const DeformArgs& a, const uint16_t* __restrict__ xn, const DSample& s,
                                             int c0, float* v1, float* v2, float* v3, float* v4) {
  const int y1 = s.y0 + 1, x1 = s.x0 + 1;
  const bool ty0 = s.y0 >= 0, ty1 = y1 < a.H, tx0 = s.x0 >= 0, tx1 = x1 < a.W;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  const uint4 q1 = (ty0 && tx0) ? *(const uint4*)(xn + ((long long)s.y0 * a.W + s.x0) * a.C + c0) : z;
  const uint4 q2 = (ty0 && tx1) ? *(const uint4*)(xn + ((long long)s.y0 * a.W + x1) * a.C + c0) : z;
  const uint4 q3 = (ty1 && tx0) ? *(const uint4*)(xn + ((long long)y1 * a.W + s.x0) * a.C + c0) : z;
  const uint4 q4 = (ty1 && tx1) ? *(const uint4*)(xn + ((long long)y1 * a.W + x1) * a.C + c0) : z;
  unpack8_bf16(q1, v1); unpack8_bf16(q2, v2); unpack8_bf16(q3, v3); unpack8_bf16(q4, v4);
}

// ---- im2col: work item = (output pixel, tap, 8-channel group), channel group fastest -----------------------------------
__global__ void __launch_bounds__(256)
deform_im2col_kernel(DeformArgs a, const uint16_t* __restrict__ x, const uint16_t* __restrict__ off,
                     uint16_t* __restrict__ col) {
  const long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= a.P * 9 * a.CG) return;
  const int cg = (int)(it % a.CG);
  const long long row = it / a.CG;           // p * 9 + k
  const int k = (int)(row % 9);
  const long long p = row / 9;
  int n, ho, wo;
  deform_pixel(a, p, &n, &ho, &wo);
  float m;
  const DSample s = deform_sample(a, off, p, ho, wo, k, cg / a.CGg, &m);
  float r[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) r[c] = 0.0f;
  if (s.valid) {
    float v1[8], v2[8], v3[8], v4[8];
    load_corners(a, x + (long long)n * a.H * a.W * a.C, s, cg * 8, v1, v2, v3, v4);
    const float w1 = s.hy * s.hx, w2 = s.hy * s.lx, w3 = s.ly * s.hx, w4 = s.ly * s.lx;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float t = w1 * v1[c];
      t = t + w2 * v2[c];
      t = t + w3 * v3[c];
      t = t + w4 * v4[c];
      r[c] = t * m;
    }
  }
  *(uint4*)(col + row * a.C + cg * 8) =
      make_uint4(pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]), pack_bf16x2(r[4], r[5]), pack_bf16x2(r[6], r[7]));
}

// ---- col2im_coord: a segment of L lanes (a power of two <= 8 dividing CGg) per (output pixel, tap, group) -------------
// Lane j of a segment owns the 8-channel groups j, j + L, ... of the group (ascending, channels 0..7 inside each), then
// the segment is folded by a butterfly of fixed shape: the channel reduction order is fixed.
__global__ void __launch_bounds__(256)
deform_col2im_coord_kernel(DeformArgs a, int L, const uint16_t* __restrict__ x, const uint16_t* __restrict__ off,
                           const uint16_t* __restrict__ dcol, uint16_t* __restrict__ doff) {
  const long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = a.P * 9 * a.G * L;
  const bool live = it < total;                 // dead lanes still take part in the shuffles (whole segments)
  const int j = (int)(it % L);
  const long long seg = (live ? it : 0) / L;    // (p * 9 + k) * G + g
  const int g = (int)(seg % a.G);
  const long long row = seg / a.G;
  const int k = (int)(row % 9);
  const long long p = row / 9;
  int n, ho, wo;
  deform_pixel(a, p, &n, &ho, &wo);
  float m;
  const DSample s = deform_sample(a, off, p, ho, wo, k, g, &m);
  float gy = 0.0f, gx = 0.0f, gm = 0.0f;
  if (live && s.valid) {
    const uint16_t* xn = x + (long long)n * a.H * a.W * a.C;
    for (int q = j; q < a.CGg; q += L) {
      const int c0 = (g * a.CGg + q) * 8;
      float v1[8], v2[8], v3[8], v4[8], d[8];
      load_corners(a, xn, s, c0, v1, v2, v3, v4);
      unpack8_bf16(*(const uint4*)(dcol + row * a.C + c0), d);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        // d(sample)/d(py), d(sample)/d(px) with the floor held fixed; the sample itself for the mask gradient
        float ty = s.hx * (v3[c] - v1[c]);
        ty = ty + s.lx * (v4[c] - v2[c]);
        float tx = s.hy * (v2[c] - v1[c]);
        tx = tx + s.ly * (v4[c] - v3[c]);
        float t = s.hy * s.hx * v1[c];
        t = t + s.hy * s.lx * v2[c];
        t = t + s.ly * s.hx * v3[c];
        t = t + s.ly * s.lx * v4[c];
        gy = gy + d[c] * ty;
        gx = gx + d[c] * tx;
        gm = gm + d[c] * t;
      }
    }
  }
  for (int o = L >> 1; o > 0; o >>= 1) {
    gy = gy + __shfl_xor(gy, o, 64);
    gx = gx + __shfl_xor(gx, o, 64);
    gm = gm + __shfl_xor(gm, o, 64);
  }
  if (!live || j != 0) return;
  uint16_t* o = doff + p * a.Coff;
  o[g * 18 + 2 * k] = f32_to_bf16_bits(gy * m);
  o[g * 18 + 2 * k + 1] = f32_to_bf16_bits(gx * m);
  if (a.mod) o[18 * a.G + 9 * g + k] = f32_to_bf16_bits(gm * (m * (1.0f - m)));
  if (k == 0 && g == 0)
    for (int c = (a.mod ? 27 : 18) * a.G; c < a.Coff; ++c) o[c] = 0;
}

// ---- col2im: inverted index + gather ---------------------------------------------------------------------------------
// Lists: one per (group, n, y, x) input pixel, list id ((g * N + n) * H + y) * W + x. Entry = (key, weight) with key =
// (p * 9 + k) * 4 + corner -- the dcol row is key >> 2 -- and weight = bilinear corner weight * v2 mask factor. Only
// corners inside the map of valid samples are entered.
constexpr int kScanThreads = 256;
constexpr int kScanPerThread = 8;
constexpr int kScanBlock = kScanThreads * kScanPerThread;

struct DEntry { unsigned key; float w; };

__device__ __forceinline__ long long deform_list(const DeformArgs& a, int g, int n, int y, int x) {
  return (((long long)g * a.N + n) * a.H + y) * a.W + x;
}

// mode 0: count entries per list (integer atomics); mode 1: place them (slot = --count: positions within a list are in
// atomic order, the sort pass below restores key order)
__global__ void __launch_bounds__(256)
deform_index_kernel(DeformArgs a, int mode, const uint16_t* __restrict__ off, int* __restrict__ cnt,
                    const int* __restrict__ start, DEntry* __restrict__ ent) {
  const long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= a.P * 9 * a.G) return;
  const int g = (int)(it % a.G);
  const long long row = it / a.G;
  const int k = (int)(row % 9);
  const long long p = row / 9;
  int n, ho, wo;
  deform_pixel(a, p, &n, &ho, &wo);
  float m;
  const DSample s = deform_sample(a, off, p, ho, wo, k, g, &m);
  if (!s.valid) return;
  const float w[4] = {s.hy * s.hx, s.hy * s.lx, s.ly * s.hx, s.ly * s.lx};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int y = s.y0 + (c >> 1), xx = s.x0 + (c & 1);
    if (y < 0 || y >= a.H || xx < 0 || xx >= a.W) continue;
    const long long l = deform_list(a, g, n, y, xx);
    if (mode == 0) {
      atomicAdd(cnt + l, 1);
    } else {
      const int slot = atomicSub(cnt + l, 1) - 1;
      DEntry e;
      e.key = (unsigned)(row * 4 + c);
      e.w = w[c] * m;
      ent[start[l] + slot] = e;
    }
  }
}

// scan pass 1: per-block sums of cnt
__global__ void __launch_bounds__(kScanThreads)
deform_scan_sums_kernel(const int* __restrict__ cnt, long long nl, int* __restrict__ bsum) {
  __shared__ int sh[kScanThreads / 64];
  const long long b0 = (long long)blockIdx.x * kScanBlock + threadIdx.x * kScanPerThread;
  int s = 0;
#pragma unroll
  for (int i = 0; i < kScanPerThread; ++i)
    if (b0 + i < nl) s += cnt[b0 + i];
  int tot;
  block_excl_scan(s, sh, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// scan pass 2 (one workgroup): block sums -> block offsets; start[nl] = number of entries
__global__ void __launch_bounds__(kScanThreads)
deform_scan_blocks_kernel(int* __restrict__ bsum, int nb, long long nl, int* __restrict__ start) {
  __shared__ int sh[kScanThreads / 64];
  int carry = 0;
  for (int b = 0; b < nb; b += kScanThreads) {
    const int i = b + threadIdx.x;
    const int v = i < nb ? bsum[i] : 0;
    int tot;
    const int ex = block_excl_scan(v, sh, &tot);
    if (i < nb) bsum[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) start[nl] = carry;
}

// scan pass 3: start[l] = exclusive prefix of cnt
__global__ void __launch_bounds__(kScanThreads)
deform_scan_apply_kernel(const int* __restrict__ cnt, long long nl, const int* __restrict__ bsum, int* __restrict__ start) {
  __shared__ int sh[kScanThreads / 64];
  const long long b0 = (long long)blockIdx.x * kScanBlock + threadIdx.x * kScanPerThread;
  int v[kScanPerThread], s = 0;
#pragma unroll
  for (int i = 0; i < kScanPerThread; ++i) {
    v[i] = b0 + i < nl ? cnt[b0 + i] : 0;
    s += v[i];
  }
  int tot;
  int run = bsum[blockIdx.x] + block_excl_scan(s, sh, &tot);
#pragma unroll
  for (int i = 0; i < kScanPerThread; ++i) {
    if (b0 + i < nl) start[b0 + i] = run;
    run += v[i];
  }
}

// one WAVE per list: a list of up to 64 entries (~36 at stride 1) is one bitonic network over the lanes (coalesced
// 8-byte loads, 21 shuffle stages); longer lists fall back to an insertion sort by lane 0. Keys are unique (< 2^31), the
// padding key 0xffffffff sorts last. (One thread per list with the insertion sort: 150 us per layer, 1.9 ms per step.)
__global__ void __launch_bounds__(256)
deform_sort_kernel(long long nl, const int* __restrict__ start, DEntry* __restrict__ ent) {
  const long long l = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (l >= nl) return;                         // wave-uniform
  const int s = start[l], e = start[l + 1];
  const int n = e - s;
  if (n <= 1) return;
  if (n <= 64) {
    unsigned key = 0xffffffffu;
    float w = 0.0f;
    if (lane < n) {
      const DEntry v = ent[s + lane];
      key = v.key;
      w = v.w;
    }
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) {
        const unsigned ok = __shfl_xor(key, j, 64);
        const float ow = __shfl_xor(w, j, 64);
        const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
        if (keep_min ? ok < key : ok > key) {
          key = ok;
          w = ow;
        }
      }
    }
    if (lane < n) {
      DEntry v;
      v.key = key;
      v.w = w;
      ent[s + lane] = v;
    }
    return;
  }
  if (lane != 0) return;
  for (int i = s + 1; i < e; ++i) {
    const DEntry v = ent[i];
    int j = i - 1;
    while (j >= s && ent[j].key > v.key) {
      ent[j + 1] = ent[j];
      --j;
    }
    ent[j + 1] = v;
  }
}

// gather: work item = (input pixel, 8-channel group), channel group fastest; fp32 sums in list (key) order
__global__ void __launch_bounds__(256)
deform_col2im_gather_kernel(DeformArgs a, const int* __restrict__ start, const DEntry* __restrict__ ent,
                            const uint16_t* __restrict__ dcol, uint16_t* __restrict__ dx) {
  const long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long pix = (long long)a.N * a.H * a.W;
  if (it >= pix * a.CG) return;
  const int cg = (int)(it % a.CG);
  const long long q = it / a.CG;                // (n * H + y) * W + x
  const int g = cg / a.CGg;
  const long long l = (long long)g * pix + q;
  float acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = 0.0f;
  const int e1 = start[l + 1];
  for (int e = start[l]; e < e1; ++e) {
    const DEntry en = ent[e];
    float d[8];
    unpack8_bf16(*(const uint4*)(dcol + (long long)(en.key >> 2) * a.C + cg * 8), d);
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = acc[c] + en.w * d[c];
  }
  uint4* o = (uint4*)(dx + q * a.C + cg * 8);
  if (a.acc) {
    float old[8];
    unpack8_bf16(*o, old);
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = acc[c] + old[c];
  }
  *o = make_uint4(pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3]), pack_bf16x2(acc[4], acc[5]),
                  pack_bf16x2(acc[6], acc[7]));
}

static int deform_check(const mxdet_deform_desc_t* d, DeformArgs* a, const char* who) {
  MXDET_REQUIRE(d != nullptr, MXDET_EINVAL, "%s: null descriptor", who);
  MXDET_REQUIRE(d->KH == 3 && d->KW == 3, MXDET_ESHAPE, "%s: only 3x3 kernels are supported (got %dx%d)", who, d->KH,
                d->KW);
  MXDET_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->stride > 0 && d->pad >= 0 && d->groups > 0,
                MXDET_ESHAPE, "%s: bad shape", who);
  MXDET_REQUIRE(d->C % (8 * d->groups) == 0, MXDET_ESHAPE, "%s: C = %d is not a multiple of 8 * groups", who, d->C);
  MXDET_REQUIRE(d->Ho == (d->H + 2 * d->pad - 3) / d->stride + 1 && d->Wo == (d->W + 2 * d->pad - 3) / d->stride + 1 &&
                    d->Ho > 0 && d->Wo > 0,
                MXDET_ESHAPE, "%s: Ho / Wo do not match H, W, stride, pad", who);
  const int need = (d->modulated ? 27 : 18) * d->groups;
  MXDET_REQUIRE(d->off_channels % 8 == 0 && d->off_channels >= need, MXDET_ESHAPE,
                "%s: off_channels = %d must be a multiple of 8 and at least %d", who, d->off_channels, need);
  const long long P = (long long)d->N * d->Ho * d->Wo;
  MXDET_REQUIRE(P * 36 * d->groups < (1ll << 31) && (long long)d->N * d->H * d->W * d->groups < (1ll << 30) &&
                    (long long)d->N * d->H * d->W * d->C < (1ll << 31) && P * 9 * d->C < (1ll << 31),
                MXDET_ESHAPE, "%s: tensor too large", who);
  a->N = d->N; a->H = d->H; a->W = d->W; a->C = d->C; a->Ho = d->Ho; a->Wo = d->Wo;
  a->stride = d->stride; a->pad = d->pad; a->G = d->groups; a->mod = d->modulated ? 1 : 0;
  a->Coff = d->off_channels; a->acc = d->accumulate ? 1 : 0;
  a->CG = d->C / 8; a->CGg = a->CG / d->groups; a->P = P;
  return MXDET_OK;
}

static unsigned grid_of(long long items) { return (unsigned)((items + 255) / 256); }

struct DeformCarve { size_t cnt, start, bsum, ent, total; long long nl; int nb; long long nent; };

static DeformCarve deform_carve(const DeformArgs& a) {
  DeformCarve c;
  c.nl = (long long)a.G * a.N * a.H * a.W;
  c.nb = (int)ceil_div(c.nl, (long long)kScanBlock);
  c.nent = a.P * 9 * a.G * 4;
  size_t off = 0;
  c.cnt = off; off = align_up(off + (size_t)c.nl * sizeof(int), 256);
  c.start = off; off = align_up(off + (size_t)(c.nl + 1) * sizeof(int), 256);
  c.bsum = off; off = align_up(off + (size_t)c.nb * sizeof(int), 256);
  c.ent = off; off = align_up(off + (size_t)c.nent * sizeof(DEntry), 256);
  c.total = off;
  return c;
}

}  // namespace mxdet

using namespace mxdet;

extern "C" int mxdet_deform_im2col(const mxdet_deform_desc_t* d, const uint16_t* x, const uint16_t* off, uint16_t* col,
                                   mxdet_stream_t stream) {
  clear_error();
  DeformArgs a;
  int rc = deform_check(d, &a, "deform_im2col");
  if (rc) return rc;
  MXDET_REQUIRE(x && off && col, MXDET_EINVAL, "deform_im2col: null pointer");
  hipLaunchKernelGGL(deform_im2col_kernel, dim3(grid_of(a.P * 9 * a.CG)), dim3(256), 0, as_stream(stream), a, x, off,
                     col);
  return check_launch("deform_im2col");
}

extern "C" int mxdet_deform_col2im_coord(const mxdet_deform_desc_t* d, const uint16_t* x, const uint16_t* off,
                                         const uint16_t* dcol, uint16_t* doff, mxdet_stream_t stream) {
  clear_error();
  DeformArgs a;
  int rc = deform_check(d, &a, "deform_col2im_coord");
  if (rc) return rc;
  MXDET_REQUIRE(x && off && dcol && doff, MXDET_EINVAL, "deform_col2im_coord: null pointer");
  int L = 8;
  while (a.CGg % L) L >>= 1;
  hipLaunchKernelGGL(deform_col2im_coord_kernel, dim3(grid_of(a.P * 9 * a.G * L)), dim3(256), 0, as_stream(stream), a, L,
                     x, off, dcol, doff);
  return check_launch("deform_col2im_coord");
}

extern "C" size_t mxdet_deform_col2im_workspace_bytes(const mxdet_deform_desc_t* d) {
  DeformArgs a;
  if (deform_check(d, &a, "deform_col2im_workspace_bytes") != MXDET_OK) return 0;
  return deform_carve(a).total;
}

extern "C" int mxdet_deform_col2im(const mxdet_deform_desc_t* d, const uint16_t* off, const uint16_t* dcol, uint16_t* dx,
                                   void* workspace, size_t workspace_bytes, mxdet_stream_t stream) {
  clear_error();
  DeformArgs a;
  int rc = deform_check(d, &a, "deform_col2im");
  if (rc) return rc;
  MXDET_REQUIRE(off && dcol && dx, MXDET_EINVAL, "deform_col2im: null pointer");
  const DeformCarve c = deform_carve(a);
  MXDET_REQUIRE(workspace && workspace_bytes >= c.total, MXDET_EWORKSPACE, "deform_col2im: workspace %zu < %zu",
                workspace_bytes, c.total);
  hipStream_t s = as_stream(stream);
  char* ws = (char*)workspace;
  int* cnt = (int*)(ws + c.cnt);
  int* start = (int*)(ws + c.start);
  int* bsum = (int*)(ws + c.bsum);
  DEntry* ent = (DEntry*)(ws + c.ent);
  if (zero_async(cnt, (size_t)c.nl * sizeof(int), s) != hipSuccess) return check_launch("deform_col2im");
  const long long items = a.P * 9 * a.G;
  hipLaunchKernelGGL(deform_index_kernel, dim3(grid_of(items)), dim3(256), 0, s, a, 0, off, cnt, (const int*)start, ent);
  hipLaunchKernelGGL(deform_scan_sums_kernel, dim3((unsigned)c.nb), dim3(kScanThreads), 0, s, (const int*)cnt, c.nl, bsum);
  hipLaunchKernelGGL(deform_scan_blocks_kernel, dim3(1), dim3(kScanThreads), 0, s, bsum, c.nb, c.nl, start);
  hipLaunchKernelGGL(deform_scan_apply_kernel, dim3((unsigned)c.nb), dim3(kScanThreads), 0, s, (const int*)cnt, c.nl,
                     (const int*)bsum, start);
  hipLaunchKernelGGL(deform_index_kernel, dim3(grid_of(items)), dim3(256), 0, s, a, 1, off, cnt, (const int*)start, ent);
  hipLaunchKernelGGL(deform_sort_kernel, dim3(grid_of(c.nl * 64)), dim3(256), 0, s, c.nl, (const int*)start, ent);
  hipLaunchKernelGGL(deform_col2im_gather_kernel, dim3(grid_of((long long)a.N * a.H * a.W * a.CG)), dim3(256), 0, s, a,
                     (const int*)start, (const DEntry*)ent, dcol, dx);
  return check_launch("deform_col2im");
}
