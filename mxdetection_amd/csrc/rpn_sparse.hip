// rpn_sparse.hip -- backward of the RPN head over the sampled anchors' cells only ("Sparse RPN-head
// backward").
//
// The RPN loss samples at most batch_size anchors per image, so d(loss)/d(head) has at most Smax = N * batch_size non-zero
// rows out of every pyramid cell. The dense head backward multiplies the zero rows as well; here
//   list:   the ACTIVE cells (a cell with a label >= 0 among its A anchors) in ascending cell order, their count S and
//           a cell -> slot map (-1 = inactive);
//   dt:     the rpn.out data gradient of the S active rows only, compact: dts [Smax, C];
//   wgrad:  both layers' weight / bias gradients as GEMMs whose reduction runs over the S slots;
//   dgrad:  the rpn.conv data gradient of the <= 9 S pixels that have an active cell in their 3x3 neighbourhood.
// Every grid is derived from Smax; the kernels read S from device memory, so a captured step follows its batch. No waits,
// no floating-point atomics (one integer atomic appends to the list). The data gradients reproduce the dense kernels' bits:
// the same v_mfma_f32_16x16x32_bf16 chain per output element in the dense K order (64-channel slice, tap, 32-channel half),
// minus the steps whose A operand is all zero -- adding exact zeros does not change an fp32 sum.
//
// Cell ids: g = n * CT + coff[l] + h * W_l + w with CT the cells of one image over all levels (the anchor index of
// mxdet_anchor_target divided by A). Operand fragments follow conv.hip: lane (frow = lane & 15, fq = lane >> 4) holds
// row frow, k = 8 fq .. 8 fq + 7; accumulator register r is row 4 fq + r, column frow.
//
// Ordered weight gradients (WGRAD_ORDERED): the same sums with the BITS of the dense grouped weight gradient. The dense
// kernels (wgrad.hip) reduce one level of one filter over its pixels in a fixed tree: 32-pixel MFMA half-steps in pixel
// order (real pixels m = (n H + h) W + w for the one-tap tile, virtual pixels v = (n H + h)(W + 1) + w for the three-tap
// tile), pixel p at reduction position p mod 32, one accumulator chain per split-K slab starting at +0, then the slabs of
// the filter's run (levels in item order, splits ascending) added in index order. A half-step without an active pixel
// adds +-0 to an accumulator that is never -0, an empty slab is +0: both are skipped. The bias sums follow wgrad_tile.h's
// bias workgroups the same way (16 row-interleaved partial sums per split, added in row order, splits in index order).
#include "common.h"
#include "wgrad3_tile.h"

namespace mxdet {

constexpr int kSpLevels = MXDET_RPN_SPARSE_MAX_LEVELS;
constexpr int kSpMaxSlots = 8192;       // the one-workgroup sort keeps its keys in LDS

struct SpGeo {
  int L, N, A, C, Ch, smax, CT;
  int H[kSpLevels], W[kSpLevels], coff[kSpLevels + 1];
  const uint16_t* P[kSpLevels];
  const uint16_t* t[kSpLevels];
  const unsigned char* tbits[kSpLevels];
  const uint16_t* gh[kSpLevels];
  uint16_t* dP[kSpLevels];
  uint16_t* dt[kSpLevels];   // dense dt maps (or null): the listed rows are scattered into them for the dense weight gradient
  int acc[kSpLevels];
  const int* list;     // [2 * smax]: sorted list, then the unordered append area
  const int* state;    // [0] = S, [1] = append counter
  const int* map;      // [N * CT]
  const uint16_t* wt_out;    // rpn.out transposed filter  [C][Ch]
  const uint16_t* wt_conv;   // rpn.conv transposed filter [C][9][C]
  uint16_t* dts;       // [smax][C]
  uint16_t* ghs;       // [smax][Ch]
  float* dw_out;       // [Ch][C]
  float* db_out;       // [Ch]
  float* dw_conv;      // [C][9][C]
  float* db_conv;      // [C]
};

struct SpCell { int n, l, h, w, pix; };   // pix = (n * H + h) * W + w: row of the level's tensors

__device__ __forceinline__ SpCell sp_decode(const SpGeo& g, int cell) {
  SpCell c;
  c.n = cell / g.CT;
  const int gc = cell - c.n * g.CT;
  int l = 0;
#pragma unroll
  for (int i = 1; i < kSpLevels; ++i)
    if (i < g.L && gc >= g.coff[i]) l = i;
  c.l = l;
  const int local = gc - g.coff[l];
  c.h = local / g.W[l];
  c.w = local - c.h * g.W[l];
  c.pix = c.n * g.H[l] * g.W[l] + local;
  return c;
}

__device__ __forceinline__ uint16_t sp_bf16(float v) { return (uint16_t)(pack_bf16x2(v, 0.0f) & 0xffffu); }

// ---- 1. active-cell list ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
rpn_sparse_mark_kernel(const int32_t* __restrict__ labels, int cells, int A, int smax, int* __restrict__ list,
                       int* __restrict__ state, int* __restrict__ map) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= cells) return;
  bool act = false;
  for (int a = 0; a < A; ++a) act = act || labels[(long long)g * A + a] >= 0;
  map[g] = -1;
  if (act) {
    const int pos = atomicAdd(&state[1], 1);
    if (pos < smax) list[smax + pos] = g;
  }
}

// one workgroup: rank of every appended key among the (distinct) keys = its slot
__global__ void __launch_bounds__(1024)
rpn_sparse_sort_kernel(int smax, int* __restrict__ list, int* __restrict__ state, int* __restrict__ map) {
  __shared__ int keys[kSpMaxSlots];
  int cnt = state[1];
  cnt = cnt < smax ? cnt : smax;
  for (int i = threadIdx.x; i < cnt; i += 1024) keys[i] = list[smax + i];
  __syncthreads();
  for (int i = threadIdx.x; i < smax; i += 1024) {
    if (i < cnt) {
      const int k = keys[i];
      int rank = 0;
      for (int j = 0; j < cnt; ++j) rank += keys[j] < k ? 1 : 0;
      list[rank] = k;
      map[k] = rank;
    } else {
      list[i] = -1;       // (ranks are < cnt: these writes never meet the ones above)
    }
  }
  if (threadIdx.x == 0) state[0] = cnt;
}

// ---- zero fill, 16 bytes per thread ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rpn_sparse_zero_kernel(uint4* __restrict__ p, long long n16) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- 2. compact dt rows: one wave per 16 slots -----------------------------------------------------------------------
// dts[s][ci] = bf16(mask(sum_co gh[cell(s)][co] * wt_out[ci][co])): the K = 64 reduction as the dense 1x1 data gradient
// runs it (half 0, then half 1, into one accumulator), the dense epilogue's mask and rounding. Rows past S are zero.
__global__ void __launch_bounds__(64) rpn_sparse_dt_kernel(const SpGeo g) {
  const int lane = threadIdx.x, frow = lane & 15, fq = lane >> 4;
  const int S = g.state[0];
  const int s = blockIdx.x * 16 + frow;
  const bool ok = s < S;
  SpCell c = {0, 0, 0, 0, 0};
  if (ok) c = sp_decode(g, g.list[s]);
  const bf16x8_t zero = __builtin_bit_cast(bf16x8_t, make_uint4(0u, 0u, 0u, 0u));
  bf16x8_t a0 = zero, a1 = zero;
  if (ok) {
    const uint16_t* row = g.gh[c.l] + (size_t)c.pix * g.Ch;
    a0 = *(const bf16x8_t*)(row + fq * 8);
    a1 = *(const bf16x8_t*)(row + 32 + fq * 8);
  }
  if (s < g.smax) {
    *(bf16x8_t*)(g.ghs + (size_t)s * g.Ch + fq * 8) = a0;
    *(bf16x8_t*)(g.ghs + (size_t)s * g.Ch + 32 + fq * 8) = a1;
  }
  for (int j = 0; j < g.C / 16; ++j) {
    const uint16_t* wr = g.wt_out + (size_t)(j * 16 + frow) * g.Ch;
    const bf16x8_t b0 = *(const bf16x8_t*)(wr + fq * 8), b1 = *(const bf16x8_t*)(wr + 32 + fq * 8);
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc, 0, 0, 0);
    const int ci = j * 16 + frow;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = fq * 4 + r;
      const int rok = __shfl((int)ok, row), rl = __shfl(c.l, row), rpix = __shfl(c.pix, row);
      float v = acc[r] + 0.0f;
      if (rok) {
        bool on;
        const size_t e = (size_t)rpix * g.C + ci;
        if (g.tbits[rl]) on = (g.tbits[rl][e >> 3] >> (ci & 7)) & 1u;
        else { const unsigned m = g.t[rl][e]; on = m != 0u && m < 0x8000u; }
        if (!on) v = 0.0f;
      }
      const int srow = blockIdx.x * 16 + row;
      const uint16_t o = sp_bf16(v);
      if (srow < g.smax) g.dts[(size_t)srow * g.C + ci] = o;
      if (rok && g.dt[rl]) g.dt[rl][(size_t)rpix * g.C + ci] = o;
    }
  }
}

// ---- 3. weight gradients and biases ----------------------------------------------------------------------------------
// One workgroup (4 waves) per 64 x 64 output tile; the reduction runs over the slots, 32 per step in slot order:
// dW[co][ci] = sum_s X[s][co] * Y[row(s)][ci], X compact (dts / ghs), Y gathered (P at the tap's offset / t). Both tiles of
// a step sit in LDS slot-major; a fragment is 8 slots of one column. The bias is the column sum of X, by the tile's first
// 64 threads in slot order.
__global__ void __launch_bounds__(256) rpn_sparse_wgrad_kernel(const SpGeo g) {
  constexpr int LD = 68;                          // LDS row stride (bf16): fragment reads of the 4 lane groups miss each other
  __shared__ __attribute__((aligned(16))) uint16_t Xs[32 * LD];
  __shared__ __attribute__((aligned(16))) uint16_t Ys[32 * LD];
  const int tid = threadIdx.x, lane = tid & 63, frow = lane & 15, fq = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ct = g.C / 64;
  const int nconv = 9 * ct * ct;
  int b = blockIdx.x;
  const uint16_t* X;
  const bool conv = b < nconv;                      // Y = P (rpn.conv) or t (rpn.out)
  int ldx, x0, y0, dh, dw, ldw;
  float* out;
  float* bias = nullptr;
  if (conv) {
    const int tap = b / (ct * ct), r = b - tap * ct * ct, cot = r / ct, cit = r - cot * ct;
    X = g.dts; ldx = g.C; x0 = cot * 64; y0 = cit * 64; dh = tap / 3 - 1; dw = tap % 3 - 1;
    ldw = 9 * g.C;
    out = g.dw_conv + (size_t)x0 * ldw + tap * g.C + y0;
    if (tap == 0 && cit == 0) bias = g.db_conv + x0;
  } else {
    b -= nconv;
    const int cit = b;                              // Ch == 64: one tile of output channels
    X = g.ghs; ldx = g.Ch; x0 = 0; y0 = cit * 64; dh = 0; dw = 0;
    ldw = g.C;
    out = g.dw_out + y0;
    if (cit == 0) bias = g.db_out;
  }
  const int S = g.state[0];
  const int lr = tid >> 3, lc = tid & 7;            // this thread's row and 16-byte chunk of the step's tiles
  f32x4_t acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.0f;
  for (int k0 = 0; k0 < S; k0 += 32) {
    const int s = k0 + lr;
    uint4 xv = make_uint4(0u, 0u, 0u, 0u), yv = xv;
    if (s < S) {
      xv = *(const uint4*)(X + (size_t)s * ldx + x0 + lc * 8);
      const SpCell c = sp_decode(g, g.list[s]);
      const int hh = c.h + dh, ww = c.w + dw;
      const uint16_t* y = conv ? g.P[c.l] : g.t[c.l];
      if (hh >= 0 && hh < g.H[c.l] && ww >= 0 && ww < g.W[c.l])
        yv = *(const uint4*)(y + ((size_t)(c.n * g.H[c.l] + hh) * g.W[c.l] + ww) * g.C + y0 + lc * 8);
    }
    __syncthreads();                                // the previous step's fragments have been read
    *(uint2*)(Xs + lr * LD + lc * 8) = make_uint2(xv.x, xv.y);
    *(uint2*)(Xs + lr * LD + lc * 8 + 4) = make_uint2(xv.z, xv.w);
    *(uint2*)(Ys + lr * LD + lc * 8) = make_uint2(yv.x, yv.y);
    *(uint2*)(Ys + lr * LD + lc * 8 + 4) = make_uint2(yv.z, yv.w);
    __syncthreads();
    unsigned af[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      af[e] = (unsigned)Xs[(fq * 8 + 2 * e) * LD + wid * 16 + frow] |
              ((unsigned)Xs[(fq * 8 + 2 * e + 1) * LD + wid * 16 + frow] << 16);
    const bf16x8_t a = __builtin_bit_cast(bf16x8_t, make_uint4(af[0], af[1], af[2], af[3]));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned bf[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        bf[e] = (unsigned)Ys[(fq * 8 + 2 * e) * LD + j * 16 + frow] |
                ((unsigned)Ys[(fq * 8 + 2 * e + 1) * LD + j * 16 + frow] << 16);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(bf16x8_t, make_uint4(bf[0], bf[1], bf[2], bf[3])),
                                                       acc[j], 0, 0, 0);
    }
    if (bias != nullptr && tid < 64) {
      for (int r = 0; r < 32; ++r) bsum += bf16_bits_to_f32(Xs[r * LD + tid]);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      out[(size_t)(wid * 16 + fq * 4 + r) * ldw + j * 16 + frow] = acc[j][r];
  if (bias != nullptr && tid < 64) bias[tid] = bsum;
}

// ---- 4. rpn.conv data gradient of the touched pixels -------------------------------------------------------------------
// Candidate row m = tap * Smax + s is the pixel whose tap `tap` reads cell(s): d = cell(s) - pad + (kh, kw). It is produced
// here iff it lies inside the map and no EARLIER tap of d reads an active cell (the first active tap owns the pixel: every
// touched pixel exactly once). One wave per 16 candidate rows x 64 input channels; an owned row sums all nine taps in the
// dense order with zero A fragments where the tap's source cell is inactive; a tap no row of the wave needs is skipped.
__global__ void __launch_bounds__(256) rpn_sparse_dgrad_kernel(const SpGeo g) {
  const int lane = threadIdx.x & 63, frow = lane & 15, fq = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = g.state[0];
  const int m = blockIdx.x * 16 + frow;
  const int tap_m = m / g.smax, s = m - tap_m * g.smax;
  int src[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) src[t] = -1;
  int dl = 0, dpix = -1;
  if (tap_m < 9 && s < S) {
    const int cell = g.list[s];
    const SpCell c = sp_decode(g, cell);
    const int H = g.H[c.l], W = g.W[c.l];
    const int hd = c.h - 1 + tap_m / 3, wd = c.w - 1 + tap_m % 3;
    if (hd >= 0 && hd < H && wd >= 0 && wd < W) {
      bool owner = true;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int hs = hd + 1 - t / 3, ws = wd + 1 - t % 3;
        int sl = -1;
        if (hs >= 0 && hs < H && ws >= 0 && ws < W) sl = g.map[cell + (hs - c.h) * W + (ws - c.w)];
        if (t < tap_m && sl >= 0) owner = false;
        src[t] = sl;
      }
      if (owner) { dl = c.l; dpix = (c.n * H + hd) * W + wd; }
    }
  }
  if (dpix < 0) {
#pragma unroll
    for (int t = 0; t < 9; ++t) src[t] = -1;
  }
  if (__ballot(dpix >= 0) == 0ull) return;          // wave-uniform: no owned row here
  const bf16x8_t zero = __builtin_bit_cast(bf16x8_t, make_uint4(0u, 0u, 0u, 0u));
  const int K9 = 9 * g.C;
  for (int cit = wid; cit < g.C / 64; cit += 4) {
    f32x4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const uint16_t* wbase = g.wt_conv + (size_t)(cit * 64 + frow) * K9 + fq * 8;
    for (int c0 = 0; c0 < g.C; c0 += 64) {
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        if (__ballot(src[t] >= 0) == 0ull) continue;   // wave-uniform: this step's A operand is all zero
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int k = c0 + hf * 32;
          bf16x8_t a = zero;
          if (src[t] >= 0) a = *(const bf16x8_t*)(g.dts + (size_t)src[t] * g.C + k + fq * 8);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bf16x8_t bw = *(const bf16x8_t*)(wbase + (size_t)j * 16 * K9 + t * g.C + k);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bw, acc[j], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = fq * 4 + r;
      const int rl = __shfl(dl, row), rpix = __shfl(dpix, row);
      if (rpix < 0) continue;
      uint16_t* drow = g.dP[rl] + (size_t)rpix * g.C + cit * 64 + frow;
      const bool accum = g.acc[rl] != 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = acc[j][r] + 0.0f;                    // (the dense epilogue's "+ bias" with no bias)
        if (accum) v += bf16_bits_to_f32(drow[j * 16]);
        drow[j * 16] = sp_bf16(v);
      }
    }
  }
}

// ---- 5. ordered weight gradients -----------------------------------------------------------------------------------------
// Layer q = 0 is rpn.out (dy = gh rows, x = t rows), q = 1 rpn.conv (dy = dt rows, x = P rows at the tap's offset).
struct SpOrd {
  int kind[2][kSpLevels];    // 1: the reduction runs over virtual pixels (row width W + 1)
  int hps[2][kSpLevels];     // 32-pixel half-steps per slab
  int bpix[2][kSpLevels];    // real pixels per bias split
  int* work;                 // [16] header (nh[q] = non-empty half-steps), ent[2][smax] int4, hsf[2][smax + 1]
};
// An entry (one active cell in the dense order of its layer): x = slot | level << 16, y = pixel row of the level's
// tensors, z = h | w << 16, w = position in the half-step | flags << 5 | index of its non-empty half-step << 8.
constexpr int kOrdNewHalf = 1, kOrdNewSlab = 2, kOrdNewBias = 4;
constexpr int kOrdHalves = 8;                       // half-steps per round of the main kernel
constexpr int kOrdImg = 32 * 128;                   // one operand image of a half-step: [32 positions][64 channels] bf16

__device__ __forceinline__ int4* sp_ord_ent(const SpGeo& g, const SpOrd& o, int q) { return (int4*)(o.work + 16) + (size_t)q * g.smax; }
__device__ __forceinline__ int* sp_ord_hsf(const SpGeo& g, const SpOrd& o, int q) {
  return o.work + 16 + 8 * (size_t)g.smax + (size_t)q * (g.smax + 1);
}

// One workgroup: ranks the slots level-major (the list is image-major), then keys every entry by (item, slab, half-step,
// position) for both layers and numbers the non-empty half-steps.
__global__ void __launch_bounds__(1024) rpn_sparse_order_kernel(const SpGeo g, const SpOrd o) {
  __shared__ int keys[kSpMaxSlots];
  __shared__ unsigned short ordv[kSpMaxSlots];
  __shared__ __attribute__((aligned(16))) unsigned char nhalf[2][kSpMaxSlots];
  const int tid = threadIdx.x;
  const int S = g.state[0];
  for (int i = tid; i < S; i += 1024) {
    const SpCell c = sp_decode(g, g.list[i]);
    keys[i] = g.N * g.coff[c.l] + c.pix;            // level-major pixel number: distinct, below N * CT
  }
  __syncthreads();
  for (int i = tid; i < S; i += 1024) {
    const int k = keys[i];
    int rank = 0;
    for (int j = 0; j < S; ++j) rank += keys[j] < k ? 1 : 0;
    ordv[rank] = (unsigned short)i;
  }
  __syncthreads();
  for (int r = tid; r < S; r += 1024) {
    const int s = ordv[r];
    const SpCell c = sp_decode(g, g.list[s]);
    SpCell cp = c;
    if (r > 0) cp = sp_decode(g, g.list[ordv[r - 1]]);
    const int H = g.H[c.l], W = g.W[c.l], Hp = g.H[cp.l], Wp = g.W[cp.l];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int v = o.kind[q][c.l] ? (c.n * H + c.h) * (W + 1) + c.w : c.pix;
      const int vp = o.kind[q][cp.l] ? (cp.n * Hp + cp.h) * (Wp + 1) + cp.w : cp.pix;
      const int hs = v >> 5, hsp = vp >> 5;
      const bool first = r == 0 || cp.l != c.l;
      int fl = 0;
      if (first || hsp != hs) fl |= kOrdNewHalf;
      if (first || hsp / o.hps[q][cp.l] != hs / o.hps[q][c.l]) fl |= kOrdNewSlab;
      if (first || cp.pix / o.bpix[q][cp.l] != c.pix / o.bpix[q][c.l]) fl |= kOrdNewBias;
      nhalf[q][r] = (unsigned char)(fl & kOrdNewHalf);
      sp_ord_ent(g, o, q)[r] = make_int4(s | (c.l << 16), c.pix, c.h | (c.w << 16), (v & 31) | (fl << 5));
    }
  }
  __syncthreads();
  for (int r = tid; r < S; r += 1024) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const unsigned* w32 = (const unsigned*)nhalf[q];
      int cnt = 0;
      const int words = (r + 1) >> 2;
      for (int j = 0; j < words; ++j) cnt += __popc(w32[j]);
      for (int j = words * 4; j <= r; ++j) cnt += nhalf[q][j];
      int* wq = (int*)&sp_ord_ent(g, o, q)[r];
      wq[3] |= (cnt - 1) << 8;                      // (this thread wrote the entry above)
      int* hsf = sp_ord_hsf(g, o, q);
      if (nhalf[q][r]) hsf[cnt - 1] = r;
      if (r == S - 1) { o.work[q] = cnt; hsf[cnt] = S; }
    }
  }
  if (S == 0 && tid < 2) { o.work[tid] = 0; sp_ord_hsf(g, o, tid)[0] = 0; }
}

// granule (16 channels, 32 B) swizzle of a [32][64] image row: the rows a 32-lane half of the transposing read touches fall
// on different bank slots (wgrad3_tile.h's x image)
__device__ __forceinline__ int sp_ord_g2(int row) { return ((row >> 1) & 1) | (((row >> 3) & 1) << 1); }

// Main kernel. Workgroups [0, 9 ct^2) are the 64 x 64 tiles of the rpn.conv taps, the next ct the tiles of rpn.out, the
// rest sum the biases (16 channels each). A tile walks its layer's non-empty half-steps in order, kOrdHalves per round: the
// round's active rows are gathered to zero-padded [32 positions][64 channels] images in LDS (16 entries x 2 operands x 8
// chunks per pass of the 256 threads), the fragments are transposing reads as in the dense tiles, `acc` is the current
// slab's chain and `fold` the sum of the finished slabs. The entries of round i + 3 and the rows of rounds i + 1, i + 2 are
// in flight while round i is multiplied; the rows a round wrote are cleared behind it (two image sets alternate).
__global__ void __launch_bounds__(256) rpn_sparse_wgrad_ordered_kernel(const SpGeo g, const SpOrd o) {
  __shared__ __attribute__((aligned(1024))) unsigned char img[2 * kOrdHalves * 2 * kOrdImg];
  __shared__ int rb[kSpMaxSlots / kOrdHalves + 2];
  __shared__ int rflag[2][kOrdHalves];
  const int tid = threadIdx.x, lane = tid & 63, frow = lane & 15, fq = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ct = g.C / 64;
  const int nconv = 9 * ct * ct;
  const int S = g.state[0];
  int b = blockIdx.x;
  if (b >= nconv + ct) {
    // ---- bias sums: 16 channels per workgroup; thread (channel c, partial r0) adds the rows m = r0 mod 16 of a split
    b -= nconv + ct;
    const int nb_conv = g.C / 16;
    const int q = b < nb_conv ? 1 : 0;
    const int c0 = (q ? b : b - nb_conv) * 16;
    const uint16_t* X = q ? g.dts : g.ghs;
    const int ldx = q ? g.C : g.Ch;
    float* db = q ? g.db_conv : g.db_out;
    const int4* ent = sp_ord_ent(g, o, q);
    uint16_t* xv = (uint16_t*)img;                  // [256 entries][16 channels]
    int* xm = (int*)(img + 256 * 32);               // [256] pixel row | new-split flag << 31
    const int c = tid >> 4, r0 = tid & 15;
    float part = 0.0f, fold = 0.0f;
    for (int e0 = 0; e0 < S; e0 += 256) {
      __syncthreads();
      if (e0 + tid < S) {
        const int4 en = ent[e0 + tid];
        const uint16_t* row = X + (size_t)(en.x & 0xffff) * ldx + c0;
        *(uint4*)(xv + tid * 16) = *(const uint4*)row;
        *(uint4*)(xv + tid * 16 + 8) = *(const uint4*)(row + 8);
        xm[tid] = (en.y & 15) | (((en.w >> 5) & kOrdNewBias) ? (1 << 31) : 0);
      }
      __syncthreads();
      const int n = S - e0 < 256 ? S - e0 : 256;
      for (int i = 0; i < n; ++i) {
        const int m = xm[i];
        if (m < 0) {                                // a new split: close the previous one (the first closes an empty one)
          float t = __shfl(part, lane & 48);
          for (int r = 1; r < 16; ++r) t += __shfl(part, (lane & 48) + r);
          fold += t;
          part = 0.0f;
        }
        if ((m & 15) == r0) part += bf16_bits_to_f32(xv[i * 16 + c]);
      }
    }
    float t = __shfl(part, lane & 48);
    for (int r = 1; r < 16; ++r) t += __shfl(part, (lane & 48) + r);
    fold += t;
    if (r0 == 0) db[c0 + c] = fold;
    return;
  }
  const bool conv = b < nconv;
  const int q = conv ? 1 : 0;
  const uint16_t* X;
  int ldx, x0, y0, dh, dw, ldw;
  float* out;
  if (conv) {
    const int tap = b / (ct * ct), r = b - tap * ct * ct, cot = r / ct, cit = r - cot * ct;
    X = g.dts; ldx = g.C; x0 = cot * 64; y0 = cit * 64; dh = tap / 3 - 1; dw = tap % 3 - 1;
    ldw = 9 * g.C;
    out = g.dw_conv + (size_t)x0 * ldw + tap * g.C + y0;
  } else {
    b -= nconv;
    X = g.ghs; ldx = g.Ch; x0 = 0; y0 = b * 64; dh = 0; dw = 0;
    ldw = g.C;
    out = g.dw_out + y0;
  }
  const int4* ent = sp_ord_ent(g, o, q);
  const int* hsf = sp_ord_hsf(g, o, q);
  const int nh = o.work[q];
  const int nr = (nh + kOrdHalves - 1) / kOrdHalves;
  for (int i = tid; i <= nr; i += 256) rb[i] = hsf[i * kOrdHalves < nh ? i * kOrdHalves : nh];
  for (int i = tid; i < (int)sizeof(img) / 16; i += 256) ((uint4*)img)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  const int eidx = tid >> 4, op = (tid >> 3) & 1, c8 = tid & 7;
  // the row an entry gives this thread: LDS byte offset (or -1) and the 16 bytes
  auto locate = [&](const int4& en, int rd) -> int {
    const int k = en.w & 31, hi = (en.w >> 8) - rd * kOrdHalves;
    return (((rd & 1) * kOrdHalves + hi) * 2 + op) * kOrdImg + k * 128 + ((((c8 >> 1) ^ sp_ord_g2(k))) << 5) + ((c8 & 1) << 4);
  };
  auto fetch = [&](const int4& en) -> uint4 {
    if (op == 0) return *(const uint4*)(X + (size_t)(en.x & 0xffff) * ldx + x0 + c8 * 8);
    const int l = en.x >> 16, hh = (en.z & 0xffff) + dh, ww = (en.z >> 16) + dw;
    const uint16_t* y = conv ? g.P[l] : g.t[l];
    if (hh < 0 || hh >= g.H[l] || ww < 0 || ww >= g.W[l]) return make_uint4(0u, 0u, 0u, 0u);
    return *(const uint4*)(y + (size_t)(en.y + dh * g.W[l] + dw) * g.C + y0 + c8 * 8);
  };
  auto flag = [&](const int4& en, int rd) {
    if (op == 0 && c8 == 0 && ((en.w >> 5) & kOrdNewHalf))
      rflag[rd & 1][(en.w >> 8) - rd * kOrdHalves] = (en.w >> 5) & kOrdNewSlab;
  };
  const int4 none = make_int4(-1, 0, 0, 0);
  auto load_ent = [&](int rd, int4 (&en)[2]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      en[p] = none;
      if (rd < nr) {
        const int e = rb[rd] + p * 16 + eidx;
        if (e < rb[rd + 1]) en[p] = ent[e];
      }
    }
  };
  struct Stage { int4 enw[2]; uint4 dat[2]; int woff[2]; };   // a round's rows on their way to LDS
  int4 en[2];
  Stage st0, st1;                                     // rounds rd + 1 and rd + 2 while round rd is multiplied
  auto load_dat = [&](int rd, Stage& st) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      st.enw[p] = en[p];
      st.woff[p] = -1;
      if (en[p].x >= 0) { st.woff[p] = locate(en[p], rd); st.dat[p] = fetch(en[p]); }
    }
  };
  f32x4_t acc[4], fold[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f}; fold[j] = acc[j]; }
  // transposing reads: lane 16 fq + 4 qq + pp addresses position 8 fq + qq (second read: + 4), channels 4 pp .. 4 pp + 3 of
  // a granule, and receives channel frow of positions 8 fq .. 8 fq + 3: reduction position = pixel mod 32 as in the dense tiles
  const int qq = (lane >> 2) & 3, pp = lane & 3;
  const int rowa = 8 * fq + qq, g2a = sp_ord_g2(rowa);
  const int offa = rowa * 128 + ((wid ^ g2a) << 5) + pp * 8;
  int offb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) offb[j] = kOrdImg + rowa * 128 + ((j ^ g2a) << 5) + pp * 8;
  typedef __attribute__((ext_vector_type(8))) short s16x8_t;
  auto frag = [&](const unsigned char* base, int off) -> bf16x8_t {
    const s16x4_t lo = tr_read(base, off), hi = tr_read(base, off + 512);
    return __builtin_bit_cast(bf16x8_t, (s16x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
  };
  load_ent(0, en);
  load_dat(0, st0);
  load_ent(1, en);
  load_dat(1, st1);
  load_ent(2, en);
  for (int rd = 0; rd < nr; ++rd) {
    const int e0 = rb[rd], e1 = rb[rd + 1];
    int zoff[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      zoff[p] = st0.woff[p];
      if (st0.woff[p] >= 0) { *(uint4*)(img + st0.woff[p]) = st0.dat[p]; flag(st0.enw[p], rd); }
    }
    // A round with more than 32 entries (every cell of a small level active): the rest is fetched load -> wait -> store,
    // and read once more for the clear below -- the form the prefetch above avoids for the common case (about one entry
    // per half-step at the benchmark's 512 of 179,046 cells). Correct (S = Smax tests), its cost is not measured.
    for (int e = e0 + 32 + eidx; e < e1; e += 16) {
      const int4 x = ent[e];
      *(uint4*)(img + locate(x, rd)) = fetch(x);
      flag(x, rd);
    }
    __syncthreads();
    st0 = st1;
    load_dat(rd + 2, st1);
    load_ent(rd + 3, en);
    const unsigned char* set = img + (rd & 1) * kOrdHalves * 2 * kOrdImg;
    const int nhere = nh - rd * kOrdHalves < kOrdHalves ? nh - rd * kOrdHalves : kOrdHalves;
    int fl[kOrdHalves];                                // (read together: one LDS round trip per round, not per half-step)
#pragma unroll
    for (int hh = 0; hh < kOrdHalves; ++hh) fl[hh] = rflag[rd & 1][hh];
#pragma unroll
    for (int hh = 0; hh < kOrdHalves; ++hh) {
      if (hh >= nhere) break;
      const unsigned char* base = set + hh * 2 * kOrdImg;
      if (__builtin_amdgcn_readfirstlane(fl[hh])) {     // a dense slab boundary: fold the finished slab
#pragma unroll
        for (int j = 0; j < 4; ++j) { fold[j] += acc[j]; acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
      }
      const bf16x8_t a = frag(base, offa);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, frag(base, offb[j]), acc[j], 0, 0, 0);
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p)
      if (zoff[p] >= 0) *(uint4*)(img + zoff[p]) = make_uint4(0u, 0u, 0u, 0u);
    for (int e = e0 + 32 + eidx; e < e1; e += 16) *(uint4*)(img + locate(ent[e], rd)) = make_uint4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) fold[j] += acc[j];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      out[(size_t)(wid * 16 + fq * 4 + r) * ldw + j * 16 + frow] = fold[j][r];
}

// zero the levels of `ptr` selected by `skip[l] == 0`: one launch per run of adjacent levels (flat buffers: one launch)
static int sp_zero_levels(const SpGeo& g, uint16_t* const* ptr, const int* skip, hipStream_t s) {
  for (int l = 0; l < g.L;) {
    if (skip && skip[l]) { ++l; continue; }
    MXDET_REQUIRE(ptr[l] != nullptr && ((uintptr_t)ptr[l] & 15) == 0, MXDET_EINVAL, "rpn_sparse_backward: level %d null / unaligned", l);
    char* p0 = (char*)ptr[l];
    char* p1 = p0;
    while (l < g.L && !(skip && skip[l]) && (char*)ptr[l] == p1) {
      p1 += (size_t)g.N * g.H[l] * g.W[l] * g.C * 2;
      ++l;
    }
    const long long n16 = (long long)(p1 - p0) / 16;           // C % 64 == 0: a level is a multiple of 128 bytes
    hipLaunchKernelGGL(rpn_sparse_zero_kernel, dim3((unsigned)ceil_div<long long>(n16, 256)), dim3(256), 0, s, (uint4*)p0, n16);
  }
  return MXDET_OK;
}

static int sp_fill(SpGeo& g, const mxdet_rpn_sparse_t* d, const char* who) {
  MXDET_REQUIRE(d != nullptr, MXDET_EINVAL, "%s: null descriptor", who);
  MXDET_REQUIRE(d->num_levels > 0 && d->num_levels <= kSpLevels && d->N > 0 && d->A > 0, MXDET_ESHAPE,
                "%s: 1..%d levels, N > 0, A > 0", who, kSpLevels);
  MXDET_REQUIRE(d->C > 0 && d->C % 64 == 0 && d->Ch == 64, MXDET_ESHAPE, "%s: C %d must be a multiple of 64 and Ch %d must be 64",
                who, d->C, d->Ch);
  MXDET_REQUIRE(d->smax > 0 && d->smax <= kSpMaxSlots, MXDET_ESHAPE, "%s: smax %d must be in 1..%d", who, d->smax, kSpMaxSlots);
  memset(&g, 0, sizeof(g));
  g.L = d->num_levels; g.N = d->N; g.A = d->A; g.C = d->C; g.Ch = d->Ch; g.smax = d->smax;
  long long ct = 0;
  for (int l = 0; l < g.L; ++l) {
    MXDET_REQUIRE(d->H[l] > 0 && d->W[l] > 0, MXDET_ESHAPE, "%s: level %d is empty", who, l);
    g.H[l] = d->H[l]; g.W[l] = d->W[l]; g.coff[l] = (int)ct;
    ct += (long long)d->H[l] * d->W[l];
    MXDET_REQUIRE((long long)d->N * d->H[l] * d->W[l] * d->C < (1ll << 31), MXDET_ESHAPE, "%s: level %d exceeds 2^31 elements", who, l);
  }
  MXDET_REQUIRE((long long)d->N * ct * d->A < (1ll << 31), MXDET_ESHAPE, "%s: more than 2^31 anchors", who);
  g.coff[g.L] = (int)ct;
  g.CT = (int)ct;
  return MXDET_OK;
}

}  // namespace mxdet

using namespace mxdet;

extern "C" int mxdet_rpn_sparse_list(const mxdet_rpn_sparse_t* d, const int32_t* labels, int32_t* list, int32_t* state,
                                     int32_t* map, mxdet_stream_t stream) {
  clear_error();
  SpGeo g;
  int rc = sp_fill(g, d, "rpn_sparse_list");
  if (rc) return rc;
  MXDET_REQUIRE(labels && list && state && map, MXDET_EINVAL, "rpn_sparse_list: null pointer");
  hipStream_t s = as_stream(stream);
  const int cells = g.N * g.CT;
  if (zero_async(state + 1, sizeof(int32_t), s) != hipSuccess) return check_launch("rpn_sparse_list");
  hipLaunchKernelGGL(rpn_sparse_mark_kernel, dim3((unsigned)ceil_div(cells, 256)), dim3(256), 0, s, labels, cells, g.A, g.smax,
                     list, state, map);
  hipLaunchKernelGGL(rpn_sparse_sort_kernel, dim3(1), dim3(1024), 0, s, g.smax, list, state, map);
  return check_launch("rpn_sparse_list");
}

extern "C" int mxdet_rpn_sparse_backward(const mxdet_rpn_sparse_t* d, const int32_t* list, const int32_t* state,
                                         const int32_t* map, const uint16_t* wt_out, const uint16_t* wt_conv, uint16_t* dts,
                                         uint16_t* ghs, float* dw_out, float* db_out, float* dw_conv, float* db_conv,
                                         int32_t parts, mxdet_stream_t stream) {
  clear_error();
  SpGeo g;
  int rc = sp_fill(g, d, "rpn_sparse_backward");
  if (rc) return rc;
  MXDET_REQUIRE(list && state && map && dts && ghs, MXDET_EINVAL, "rpn_sparse_backward: null pointer");
  g.list = list; g.state = state; g.map = map; g.wt_out = wt_out; g.wt_conv = wt_conv; g.dts = dts; g.ghs = ghs;
  g.dw_out = dw_out; g.db_out = db_out; g.dw_conv = dw_conv; g.db_conv = db_conv;
  for (int l = 0; l < g.L; ++l) {
    g.P[l] = (const uint16_t*)d->P[l]; g.t[l] = (const uint16_t*)d->t[l]; g.tbits[l] = (const unsigned char*)d->tbits[l];
    g.gh[l] = (const uint16_t*)d->gh[l]; g.dP[l] = (uint16_t*)d->dP[l]; g.acc[l] = d->accumulate[l];
  }
  hipStream_t s = as_stream(stream);
  if (parts & MXDET_RPN_SPARSE_ZERO) {
    rc = sp_zero_levels(g, g.dP, g.acc, s);
    if (rc) return rc;
  }
  if (parts & MXDET_RPN_SPARSE_DTMAP) {
    MXDET_REQUIRE(parts & MXDET_RPN_SPARSE_DT, MXDET_EINVAL, "rpn_sparse_backward: DTMAP needs DT");
    for (int l = 0; l < g.L; ++l) g.dt[l] = (uint16_t*)d->dt[l];
    rc = sp_zero_levels(g, g.dt, nullptr, s);
    if (rc) return rc;
  }
  if (parts & MXDET_RPN_SPARSE_DT) {
    MXDET_REQUIRE(wt_out, MXDET_EINVAL, "rpn_sparse_backward: null wt_out");
    for (int l = 0; l < g.L; ++l)
      MXDET_REQUIRE(g.gh[l] && (g.tbits[l] || g.t[l]), MXDET_EINVAL, "rpn_sparse_backward: level %d: null gh / mask", l);
    hipLaunchKernelGGL(rpn_sparse_dt_kernel, dim3((unsigned)ceil_div(g.smax, 16)), dim3(64), 0, s, g);
  }
  if (parts & MXDET_RPN_SPARSE_WGRAD) {
    MXDET_REQUIRE(dw_out && db_out && dw_conv && db_conv, MXDET_EINVAL, "rpn_sparse_backward: null weight-gradient pointer");
    for (int l = 0; l < g.L; ++l)
      MXDET_REQUIRE(g.P[l] && g.t[l], MXDET_EINVAL, "rpn_sparse_backward: level %d: null P / t", l);
    const int ct = g.C / 64;
    hipLaunchKernelGGL(rpn_sparse_wgrad_kernel, dim3((unsigned)(9 * ct * ct + ct)), dim3(256), 0, s, g);
  }
  if (parts & MXDET_RPN_SPARSE_DGRAD) {
    MXDET_REQUIRE(wt_conv, MXDET_EINVAL, "rpn_sparse_backward: null wt_conv");
    for (int l = 0; l < g.L; ++l)
      MXDET_REQUIRE(g.dP[l], MXDET_EINVAL, "rpn_sparse_backward: level %d: null dP", l);
    hipLaunchKernelGGL(rpn_sparse_dgrad_kernel, dim3((unsigned)ceil_div(9 * g.smax, 16)), dim3(256), 0, s, g);
  }
  if (parts & MXDET_RPN_SPARSE_WGRAD_ORDERED) {
    MXDET_REQUIRE(!(parts & MXDET_RPN_SPARSE_WGRAD), MXDET_EINVAL, "rpn_sparse_backward: WGRAD and WGRAD_ORDERED write the same gradients");
    MXDET_REQUIRE(dw_out && db_out && dw_conv && db_conv, MXDET_EINVAL, "rpn_sparse_backward: null weight-gradient pointer");
    MXDET_REQUIRE(d->ordered && d->ordered_work && ((uintptr_t)d->ordered_work & 15) == 0, MXDET_EINVAL,
                  "rpn_sparse_backward: WGRAD_ORDERED needs the schedule and 16-byte aligned scratch");
    SpOrd o;
    memset(&o, 0, sizeof(o));
    o.work = (int*)d->ordered_work;
    for (int q = 0; q < 2; ++q)
      for (int l = 0; l < g.L; ++l) {
        const mxdet_rpn_ordered_item_t& it = d->ordered[q * g.L + l];
        MXDET_REQUIRE((it.kind == 0 || it.kind == 1) && it.H == g.H[l] && it.W == g.W[l] && it.halves_per_slab > 0 &&
                          it.bias_pixels > 0 && it.bias_pixels % 16 == 0,
                      MXDET_EINVAL, "rpn_sparse_backward: schedule record %d does not describe level %d", q * g.L + l, l);
        MXDET_REQUIRE((long long)g.N * g.H[l] * (g.W[l] + 1) < (1ll << 31), MXDET_ESHAPE, "rpn_sparse_backward: level %d too large", l);
        // the kernel folds the slabs in item order: the recorded run must be laid out that way
        const int prev = l == 0 ? -1 : d->ordered[q * g.L + l - 1].slab0;
        MXDET_REQUIRE((l == 0 ? it.slab0 == 0 : it.slab0 > prev) && it.slab0 < it.fold_ksplit &&
                          it.fold_ksplit == d->ordered[q * g.L].fold_ksplit && it.bias_splits >= 1,
                      MXDET_EINVAL, "rpn_sparse_backward: schedule record %d: slabs out of item order", q * g.L + l);
        o.kind[q][l] = it.kind; o.hps[q][l] = it.halves_per_slab; o.bpix[q][l] = it.bias_pixels;
      }
    for (int l = 0; l < g.L; ++l)
      MXDET_REQUIRE(g.P[l] && g.t[l], MXDET_EINVAL, "rpn_sparse_backward: level %d: null P / t", l);
    const int ct = g.C / 64;
    hipLaunchKernelGGL(rpn_sparse_order_kernel, dim3(1), dim3(1024), 0, s, g, o);
    hipLaunchKernelGGL(rpn_sparse_wgrad_ordered_kernel, dim3((unsigned)(9 * ct * ct + ct + g.C / 16 + g.Ch / 16)), dim3(256), 0, s, g, o);
  }
  return check_launch("rpn_sparse_backward");
}

extern "C" int mxdet_rpn_ordered_schedule(const void* table_host, int32_t n, int32_t num_levels, mxdet_rpn_ordered_item_t* items) {
  clear_error();
  MXDET_REQUIRE(table_host && items && num_levels > 0 && num_levels <= kSpLevels && n == 2 * num_levels, MXDET_EINVAL,
                "rpn_ordered_schedule: a table of 2 * num_levels items");
  const WgradG* t = (const WgradG*)table_host;
  for (int q = 0; q < 2; ++q) {
    const WgradG& own = t[q * num_levels];           // the first item of a filter owns its run of slabs and folds it
    int next = 0;
    for (int l = 0; l < num_levels; ++l) {
      const int i = q * num_levels + l;
      const WgradP& p = t[i].p;
      MXDET_REQUIRE(p.dw == own.p.dw && p.db == own.p.db && p.db != nullptr && !p.accumulate && t[i].nparams == own.nparams,
                    MXDET_EINVAL, "rpn_ordered_schedule: item %d is not a level of filter %d (with a bias, no accumulate)", i, q);
      MXDET_REQUIRE(p.stride == 1 && p.Ho == p.H && p.Wo == p.W && (q ? (p.KH == 3 && p.KW == 3 && p.pad == 1)
                                                                      : (p.KH == 1 && p.KW == 1 && p.pad == 0)),
                    MXDET_EINVAL, "rpn_ordered_schedule: item %d is not the head's %s convolution", i, q ? "3x3" : "1x1");
      const size_t slab_bytes = (size_t)own.nparams * sizeof(float);
      const size_t doff = (size_t)p.slab - (size_t)own.p.slab, boff = (size_t)p.bslab - (size_t)own.p.bslab;
      mxdet_rpn_ordered_item_t& it = items[i];
      it.kind = p.t3_nwg > 0 ? 1 : 0;
      it.H = p.H; it.W = p.W;
      it.halves_per_slab = it.kind ? p.t3_steps * (kT3Px / 32) : p.steps_per_split * (kWgradBKP / 32);
      it.slab0 = (int32_t)(doff / slab_bytes);
      it.fold_ksplit = own.fold_ksplit;
      it.bias_pixels = p.steps_per_split * kWgradBKP;
      it.bias_splits = p.ksplit;
      // the kernel adds the slabs in item order: the run must be laid out that way, weights and biases alike
      MXDET_REQUIRE(doff % slab_bytes == 0 && it.slab0 == next && boff == (size_t)next * p.Cout * sizeof(float), MXDET_EINVAL,
                    "rpn_ordered_schedule: item %d: its slabs do not follow item %d's", i, i - 1);
      next += it.kind ? p.t3_ksplit : p.ksplit;
    }
    MXDET_REQUIRE(next == own.fold_ksplit, MXDET_EINVAL, "rpn_ordered_schedule: filter %d folds %d slabs, its levels write %d", q,
                  own.fold_ksplit, next);
  }
  return MXDET_OK;
}
