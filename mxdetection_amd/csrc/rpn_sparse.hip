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
#include "common.h"

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
  return check_launch("rpn_sparse_backward");
}
