// wgrad.hip -- bf16 weight-gradient convolution on MFMA for gfx950 (deterministic split-K).
//
// Slots: backbones / necks / rpn_heads / bbox_heads / mask_heads (/root/reference/README.md:27-31);
// MXNet role: Convolution / FullyConnected backward-weights (README.md:37).
//
//   dW[co][kh][kw][ci] = sum over output pixels m of dY[m][co] * X[src(m,kh,kw)][ci]
//
// GEMM view per tap: rows = co, cols = ci, reduction = pixels. Both operands are channels-last, i.e.
// the reduction index is the *strided* one, so the MFMA fragments (8 consecutive k per lane) are
// columns of the LDS image: they are fetched with ds_read_b64_tr_b16 (the CDNA4 transposing LDS
// read), two per fragment. LDS images are [pixel][128 ch] with the 32-B granule index XOR-swizzled
// by (row&3)|((row>>3)&1)<<2, which makes every transposed read conflict-free.
// The pixel range is split over `ksplit` workgroups per tile; each writes an fp32 slab and a second kernel adds
// the slabs in index order (bit-reproducible, no float atomics) and optionally accumulates into dw (filters
// shared across pyramid levels: RPN head); with one split the tile goes straight to dw. The bias gradient
// (column sums of dy) rides along as co_tiles*ksplit extra workgroups appended to the same grid (a ones-vector
// MFMA inside the main loop was measured first: +16 accumulators took the kernel from 120 to 176 registers and
// halved its occupancy) and is folded over the splits by the same second kernel.
// (A "last workgroup of the tile folds the slabs" epilogue was measured and dropped: the device-scope fence it
// needs is buffer_wbl2 + buffer_inv of the whole XCD L2 per workgroup, which destroys the tap-sharing L2 reuse
// -- 2.3 -> 8.9 ms per step.)
//
// Layout of this file: the kernels (wgrad_item() fetches a grouped table item, wgrad_fold() is the one fold body); then
// the host side: validate_wgrad_desc(), fill_wgrad() (descriptor -> WgradP), tile_one_tap() / tile_three_tap() (one
// item's tiling over equal_ranges()), the two split rules single_split() (plan_wgrad(), one call) and grouped_split() /
// group_three_tap_steps() (mxdet_conv2d_wgrad_grouped_plan), place_slabs() and for_ring_depth() at the launch sites.
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "wgrad_tile.h"
#include "wgrad3_tile.h"

namespace mxdet {

template <int BKP, int NS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
wgrad_kernel(WgradP p) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * 2 * BKP * 256];
  if (wgrad_plain(p)) wgrad_tile<BKP, NS, true>(p, (int)blockIdx.x, smem);
  else wgrad_tile<BKP, NS, false>(p, (int)blockIdx.x, smem);
}

// the three-tap tiles: 256 threads, NS * 25 KiB of LDS, two workgroups per CU
template <int NS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
wgrad3_kernel(WgradP p) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * kT3Stage];
  wgrad3_tile<NS>(p, (int)blockIdx.x, smem);
}

// ---- grouped form: the weight gradients of MANY layers in one launch ----------------------------------------------
// A ResNet stage at batch 2 is 10-20 layers whose own grids (one or two workgroups per CU, 17-step K loops, a slab
// fold each) leave the chip latency-bound; issued as one grid of a few thousand workgroups they run at the
// occupancy the big P2-level layers get, need 3-4x less split-K (slab traffic) and two launches instead of 40.
// The table lives in device memory (built once per group by mxdet_conv2d_wgrad_grouped_plan, pointers are static
// under hipGraph replay); slab addresses are offsets from the workspace passed at launch.

// The two tile kinds as the grouped kernels see them: the tile function, and the members of a table entry that number
// the kind's workgroups
template <int BKP, int NS>
struct OneTap {      // + the bias workgroups
  static constexpr int WgradG::*First = &WgradG::block0;
  static constexpr int WgradG::*Count = &WgradG::nblocks;
  static __device__ __forceinline__ void run(const WgradP& p, int b, unsigned char* smem) {
    if (wgrad_plain(p)) wgrad_tile<BKP, NS, true>(p, b, smem);
    else wgrad_tile<BKP, NS, false>(p, b, smem);
  }
};
template <int NS>
struct ThreeTap {    // wgrad3_tile.h
  static constexpr int WgradG::*First = &WgradG::bblock0;
  static constexpr int WgradG::*Count = &WgradG::bnblocks;
  static __device__ __forceinline__ void run(const WgradP& p, int b, unsigned char* smem) { wgrad3_tile<NS>(p, b, smem); }
};

// Workgroup `bid` of a group's tiles of kind Tile: fetches the item that owns it -- its parameters, slab / bslab rebased
// onto the workspace (the three-tap tiles never read bslab) -- and runs that item's tile `bid - First`.
template <typename Tile>
__device__ __forceinline__ void wgrad_item(const WgradG* table, int n, unsigned char* workspace, int bid, unsigned char* smem) {
  const int i = table_lookup<WgradG, Tile::First>(table, n, bid);
  const int b = bid - table[i].*Tile::First;
  if (b >= table[i].*Tile::Count) return;            // alignment padding between layers
  WgradP p = table[i].p;
  p.slab = (float*)(workspace + (size_t)p.slab);
  p.bslab = (float*)(workspace + (size_t)p.bslab);
  Tile::run(p, b, smem);
}

template <int BKP, int NS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NS == 2 ? 4 : (NS == 3 ? 3 : 2), 4)))
wgrad_grouped_kernel(const WgradG* __restrict__ table, int n, unsigned char* __restrict__ workspace) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * 2 * BKP * 256];
  wgrad_item<OneTap<BKP, NS>>(table, n, workspace, (int)blockIdx.x, smem);
}

template <int NS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
wgrad3_grouped_kernel(const WgradG* __restrict__ table, int n, unsigned char* __restrict__ workspace) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * kT3Stage];
  wgrad_item<ThreeTap<NS>>(table, n, workspace, (int)blockIdx.x, smem);
}

// Both tile kinds of a group in ONE grid. The 3x3 tiles are MFMA-bound, the 1x1 / strided tiles mostly HBM-bound (a 1x1
// layer reads x and dy once for Cin*Cout/(Cin+Cout) flop per byte): as two launches in a row each phase leaves the other
// resource idle (measured: the three-tap kernel at 1.24 PFLOP/s in the step, the one-tap kernel behind it at 0.4), mixed
// in one grid a CU holds one workgroup of each kind. Groups of 8 workgroups (one per XCD) alternate between the two lists
// in proportion to their lengths (n3g : n1g groups), so that both lists run out together.
template <int NS3, int NS1>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
wgrad_mixed_grouped_kernel(const WgradG* __restrict__ table, int n, unsigned char* __restrict__ workspace, int n3g, int n1g) {
  constexpr int kLds = NS3 * kT3Stage > NS1 * 2 * kWgradBKP * 256 ? NS3 * kT3Stage : NS1 * 2 * kWgradBKP * 256;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[kLds];
  const int G = (int)blockIdx.x >> 3, x8 = (int)blockIdx.x & 7, T = n3g + n1g;
  const int a = (int)(((long long)G * n3g) / T), a2 = (int)(((long long)(G + 1) * n3g) / T);
  if (a2 > a) wgrad_item<ThreeTap<NS3>>(table, n, workspace, a * 8 + x8, smem);                // the a-th group of three-tap tiles
  else wgrad_item<OneTap<kWgradBKP, NS1>>(table, n, workspace, (G - a) * 8 + x8, smem);      // the (G - a)-th group of one-tap tiles
}

// dw[i] (+)= sum_ks slab[ks][i] in index order, by workgroup `b` of the fold; workgroups wblocks and up fold the bias
// partials the same way. Four independent 16-B loads in flight per thread (the slabs are read exactly once: latency, not
// bandwidth, bounds a small grid).
__device__ __forceinline__ void wgrad_fold(const float* __restrict__ slab, const float* __restrict__ bslab, int ksplit,
                                           long long n, int Cout, int wblocks, int accumulate, float* __restrict__ dw,
                                           float* __restrict__ db, int b) {
  if (b >= wblocks) {
    int c = (b - wblocks) * 256 + threadIdx.x;
    if (c >= Cout) return;
    float s = bslab[c];
    for (int k = 1; k < ksplit; ++k) s += bslab[(size_t)k * Cout + c];
    db[c] = accumulate ? db[c] + s : s;
    return;
  }
  long long i = ((long long)b * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  const float* sp = slab + i;
  float4 s = *(const float4*)sp;
  int k = 1;
  for (; k + 3 < ksplit; k += 4) {
    float4 v0 = *(const float4*)(sp + (long long)k * n);
    float4 v1 = *(const float4*)(sp + (long long)(k + 1) * n);
    float4 v2 = *(const float4*)(sp + (long long)(k + 2) * n);
    float4 v3 = *(const float4*)(sp + (long long)(k + 3) * n);
    s.x += v0.x; s.y += v0.y; s.z += v0.z; s.w += v0.w;
    s.x += v1.x; s.y += v1.y; s.z += v1.z; s.w += v1.w;
    s.x += v2.x; s.y += v2.y; s.z += v2.z; s.w += v2.w;
    s.x += v3.x; s.y += v3.y; s.z += v3.z; s.w += v3.w;
  }
  for (; k < ksplit; ++k) {
    float4 v = *(const float4*)(sp + (long long)k * n);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  if (accumulate) {
    float4 o = *(const float4*)(dw + i);
    s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
  }
  *(float4*)(dw + i) = s;
}

__global__ void __launch_bounds__(256)
wgrad_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bslab, int ksplit, long long n,
                    int Cout, int wblocks, int accumulate, float* __restrict__ dw, float* __restrict__ db) {
  wgrad_fold(slab, bslab, ksplit, n, Cout, wblocks, accumulate, dw, db, (int)blockIdx.x);
}

// fold kernel of the grouped form: one launch for every layer of the group
__global__ void __launch_bounds__(256)
wgrad_reduce_grouped_kernel(const WgradG* __restrict__ table, int n, const unsigned char* __restrict__ workspace) {
  const int bid = (int)blockIdx.x;
  const WgradG& g = table[table_lookup<WgradG, &WgradG::rblock0>(table, n, bid)];
  const int b = bid - g.rblock0;
  if (b >= g.wblocks + g.bblocks) return;      // nothing to fold (single split: dw / db written directly; or not the owner)
  wgrad_fold((const float*)(workspace + (size_t)g.p.slab), (const float*)(workspace + (size_t)g.p.bslab), g.fold_ksplit,
             g.nparams, g.p.Cout, g.wblocks, g.p.accumulate, g.p.dw, g.p.db, b);
}

// w [Cout][taps][Cin] -> wt [Cin][taps][Cout]
__global__ void filter_transpose_kernel(const uint16_t* __restrict__ w, int Cout, int taps, int Cin,
                                        uint16_t* __restrict__ wt) {
  __shared__ uint16_t tile[32][33];
  const int tap = blockIdx.z;
  const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
  for (int r = threadIdx.y; r < 32; r += blockDim.y) {
    int co = co0 + r, ci = ci0 + threadIdx.x;
    uint16_t v = 0;
    if (co < Cout && ci < Cin) v = w[((size_t)co * taps + tap) * Cin + ci];
    tile[r][threadIdx.x] = v;
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += blockDim.y) {
    int ci = ci0 + r, co = co0 + threadIdx.x;
    if (co < Cout && ci < Cin) wt[((size_t)ci * taps + tap) * Cout + co] = tile[threadIdx.x][r];
  }
}

// batched form: one launch for every filter of the model (descriptor table in device memory)
struct TransposeDesc { const uint16_t* w; uint16_t* wt; int Cout, taps, Cin, tile0; };
__global__ void __launch_bounds__(256)
filter_transpose_batched_kernel(const TransposeDesc* __restrict__ descs, int ndesc) {
  // 64 (co) x 64 (ci) tile per workgroup: 16-byte global loads along ci, 16-byte global stores along co. LDS pitch 66
  // halfwords: the column gathers of the store phase (lanes = 8 ci x 8 co-groups) fall on 32 distinct banks, two lanes
  // per bank reading the same dword.
  __shared__ uint32_t tile32[64 * 33];
  uint16_t* tile = (uint16_t*)tile32;
  const int b = blockIdx.x;
  const TransposeDesc d = descs[table_lookup<TransposeDesc, &TransposeDesc::tile0>(descs, ndesc, b)];
  int t = b - d.tile0;
  const int tiles_ci = (d.Cin + 63) >> 6, tiles_co = (d.Cout + 63) >> 6;
  const int tci = t % tiles_ci; t /= tiles_ci;
  const int tco = t % tiles_co; t /= tiles_co;
  const int tap = t;
  const int ci0 = tci * 64, co0 = tco * 64;
  const bool vec = ((d.Cin | d.Cout) & 7) == 0 && ((((uintptr_t)d.w) | ((uintptr_t)d.wt)) & 15) == 0;
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = tid; c < 512; c += 256) {
    const int r = c >> 3, k = (c & 7) * 8;
    const int co = co0 + r, ci = ci0 + k;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (co < d.Cout && ci < d.Cin) {
      const uint16_t* src = d.w + ((size_t)co * d.taps + tap) * d.Cin + ci;
      if (vec) {
        const uint4 q = *(const uint4*)src;
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        for (int j = 0; j < 8; ++j)
          if (ci + j < d.Cin) v[j >> 1] |= (uint32_t)src[j] << (16 * (j & 1));
      }
    }
    uint32_t* dst = tile32 + r * 33 + (k >> 1);
    dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
  }
  __syncthreads();
#pragma unroll
  for (int c = tid; c < 512; c += 256) {
    const int r = c >> 3, k = (c & 7) * 8;        // r: ci within the tile, k: first of 8 co
    const int ci = ci0 + r, co = co0 + k;
    if (ci >= d.Cin || co >= d.Cout) continue;
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      v[j] = (uint32_t)tile[(k + 2 * j) * 66 + r] | ((uint32_t)tile[(k + 2 * j + 1) * 66 + r] << 16);
    uint16_t* dst = d.wt + ((size_t)ci * d.taps + tap) * d.Cout + co;
    if (vec) {
      *(uint4*)dst = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
      for (int j = 0; j < 8; ++j)
        if (co + j < d.Cout) dst[j] = (uint16_t)(v[j >> 1] >> (16 * (j & 1)));
    }
  }
}

// ---- host side: descriptor -> WgradP, the split rules, the launches ---------------------------------------------------
static thread_local int g_force_ksplit = 0;   // tuning hook (mxdet_debug_force_wgrad_ksplit), 0 = heuristic

static int validate_wgrad_desc(const mxdet_conv_desc_t* d, const char* who) {
  MXDET_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0 && d->KH > 0 && d->KW > 0 &&
                    d->stride > 0 && d->pad >= 0,
                MXDET_ESHAPE, "%s: non-positive dimension", who);
  MXDET_REQUIRE(d->Ho == (d->H + 2 * d->pad - d->KH) / d->stride + 1 &&
                    d->Wo == (d->W + 2 * d->pad - d->KW) / d->stride + 1,
                MXDET_ESHAPE, "%s: Ho/Wo do not match the convolution arithmetic", who);
  MXDET_REQUIRE(d->Cin % 8 == 0 && d->Cout % 8 == 0, MXDET_ESHAPE, "%s: Cin and Cout must be multiples of 8", who);
  MXDET_REQUIRE((long long)d->N * d->H * d->W * d->Cin < (1ll << 31) &&
                    (long long)d->N * d->Ho * d->Wo * d->Cout < (1ll << 31),
                MXDET_ESHAPE, "%s: tensor exceeds 2^31 elements", who);
  return MXDET_OK;
}

// 3x3 / stride 1 / pad 1 layers go to the three-tap kernel (wgrad3_tile.h), everything else to the one-tap kernel
static bool three_tap(const mxdet_conv_desc_t& d) {
  return tuning(MXDET_TUNE_T3_ENABLE) != 0 && wgrad3_eligible(d.KH, d.KW, d.stride, d.pad, d.H, d.W);
}
// K-loop steps over all pixels of a layer, and tiles per split, for either kernel
static int one_tap_steps(const mxdet_conv_desc_t& d) {
  return (int)ceil_div<long long>((long long)d.N * d.Ho * d.Wo, kWgradBKP);
}
static int three_tap_steps(const mxdet_conv_desc_t& d) {       // virtual pixels (one pad pixel per image row)
  return (int)ceil_div<long long>(wgrad3_vpixels(d.N, d.H, d.W), kT3Px);
}
static long long one_tap_tiles(const mxdet_conv_desc_t& d) {
  return (long long)ceil_div(d.Cout, 128) * ceil_div(d.Cin, 128) * d.KH * d.KW;
}
static long long three_tap_tiles(const mxdet_conv_desc_t& d) {
  return (long long)ceil_div(d.Cout, 128) * ceil_div(d.Cin, 64) * 3;
}
static size_t wgrad_params(const mxdet_conv_desc_t& d) { return (size_t)d.Cout * d.KH * d.KW * d.Cin; }

// `steps` cut into at most `ks` equal ranges (the last one may be shorter): the length of a range; *n = how many are not empty
static int equal_ranges(int steps, int ks, int* n) {
  const int per = ceil_div(steps, ks);
  *n = ceil_div(steps, per);
  return per;
}
static int clamp_split(long long ks) { return ks < 1 ? 1 : (ks > 64 ? 64 : (int)ks); }
// the most splits that leave every range at least min_steps long
static int max_split(int steps, int min_steps) { return steps / min_steps > 0 ? steps / min_steps : 1; }

// Everything of WgradP that the descriptor and the pointers decide (slab / bslab and the tiling: below)
static void fill_wgrad(WgradP& p, const mxdet_conv_desc_t& d, const void* x, const void* dy, float* dw, float* db) {
  memset(&p, 0, sizeof(p));
  p.x = (const uint16_t*)x; p.dy = (const uint16_t*)dy; p.dw = dw; p.db = db; p.accumulate = d.accumulate;
  p.N = d.N; p.H = d.H; p.W = d.W; p.Cin = d.Cin; p.Cout = d.Cout; p.KH = d.KH; p.KW = d.KW;
  p.stride = d.stride; p.pad = d.pad; p.Ho = d.Ho; p.Wo = d.Wo;
  p.M = (int)((long long)d.N * d.Ho * d.Wo);
  p.co_tiles = ceil_div(d.Cout, 128); p.ci_tiles = ceil_div(d.Cin, 128);
}
// One item's tiling, the pixels cut into at most `ks` ranges: by the one-tap kernel ...
static void tile_one_tap(WgradP& p, const mxdet_conv_desc_t& d, int ks) {
  p.steps_per_split = equal_ranges(one_tap_steps(d), ks, &p.ksplit);
  p.nwg_main = (int)(one_tap_tiles(d) * p.ksplit);
}
// ... or by the three-tap kernel; the one-tap kernel keeps only the bias workgroups, over the same number of ranges
static void tile_three_tap(WgradP& p, const mxdet_conv_desc_t& d, int ks) {
  p.t3_steps = equal_ranges(three_tap_steps(d), ks, &p.t3_ksplit);
  p.t3_ci_tiles = ceil_div(d.Cin, 64);
  p.t3_nwg = (int)(three_tap_tiles(d) * p.t3_ksplit);
  p.ksplit = p.t3_ksplit;
  p.steps_per_split = ceil_div(one_tap_steps(d), p.ksplit);   // any partition of the pixels into ksplit ranges
}
// `ks` weight slabs, then `ks` bias slabs, appended to a workspace of *off bytes: the byte offsets at which they start
static void place_slabs(size_t ks, size_t params, size_t cout, size_t* off, size_t* slab0, size_t* bslab0) {
  *slab0 = *off;
  *off += align_up(ks * params * sizeof(float), 256);
  *bslab0 = *off;
  *off += align_up(ks * cout * sizeof(float), 256);
}

// The split of a single call: one round of the `resident` workgroups the chip holds at once (one-tap: 4 per CU with 32 KiB
// of LDS and <= 128 registers; three-tap: 2 per CU) -- one more would run alone in a second round, so the split rounds
// DOWN -- and at least 512 pixels (min_steps) per split.
static int single_split(int steps, long long tiles, int resident, int min_steps) {
  if (g_force_ksplit > 0) return g_force_ksplit < steps ? g_force_ksplit : steps;
  const int want = resident / tiles > 0 ? (int)(resident / tiles) : 1, most = max_split(steps, min_steps);
  return clamp_split(want < most ? want : most);
}

struct WgradPlan {
  WgradP p;         // slab / bslab hold byte offsets into the workspace
  size_t total;     // workspace bytes
};
static WgradPlan plan_wgrad(const mxdet_conv_desc_t& d, const void* x, const void* dy, float* dw, float* db) {
  WgradPlan w;
  fill_wgrad(w.p, d, x, dy, dw, db);
  if (three_tap(d)) tile_three_tap(w.p, d, single_split(three_tap_steps(d), three_tap_tiles(d), 512, 512 / kT3Px));
  else tile_one_tap(w.p, d, single_split(one_tap_steps(d), one_tap_tiles(d), 1024, 512 / kWgradBKP));
  size_t slab0, bslab0;
  w.total = 0;
  place_slabs((size_t)w.p.ksplit, wgrad_params(d), (size_t)d.Cout, &w.total, &slab0, &bslab0);
  w.p.slab = (float*)slab0;
  w.p.bslab = (float*)bslab0;
  return w;
}

// calls launch(std::integral_constant<int, D>) for the ring depth D of the list that equals ns (0 = nothing to launch)
template <int... D, typename F>
static void for_ring_depth(int ns, F launch) {
  ((ns == D ? launch(std::integral_constant<int, D>()) : (void)0), ...);
}

}  // namespace mxdet

using namespace mxdet;

extern "C" int mxdet_debug_force_wgrad_ksplit(int32_t ks) {
  g_force_ksplit = ks;
  return MXDET_OK;
}

extern "C" size_t mxdet_conv2d_wgrad_workspace_bytes(const mxdet_conv_desc_t* d) {
  if (!d || d->N <= 0 || d->Cout <= 0 || d->Cin <= 0 || d->KH <= 0 || d->KW <= 0 || d->Ho <= 0 || d->Wo <= 0)
    return 0;
  return plan_wgrad(*d, nullptr, nullptr, nullptr, nullptr).total;
}

extern "C" int mxdet_conv2d_wgrad(const mxdet_conv_desc_t* d, const uint16_t* x, const uint16_t* dy,
                                  float* dw, float* db, void* workspace,
                                  size_t workspace_bytes, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(d != nullptr, MXDET_EINVAL, "conv2d_wgrad: null descriptor");
  if (int rc = validate_wgrad_desc(d, "conv2d_wgrad")) return rc;
  MXDET_REQUIRE(x && dy && dw, MXDET_EINVAL, "conv2d_wgrad: null pointer");
  WgradPlan w = plan_wgrad(*d, x, dy, dw, db);
  MXDET_REQUIRE(workspace && workspace_bytes >= w.total, MXDET_EWORKSPACE,
                "conv2d_wgrad: workspace %zu < %zu", workspace_bytes, w.total);
  hipStream_t s = as_stream(stream);
  WgradP& p = w.p;
  p.slab = (float*)((char*)workspace + (size_t)p.slab);
  p.bslab = (float*)((char*)workspace + (size_t)p.bslab);
  // the launches this call makes, decided once: the route probe and the launch code below read the same values
  const int t3 = p.t3_nwg > 0;          // three-tap tiles: the one-tap kernel keeps only the bias workgroups (same pixel ranges)
  const int t3_ns = t3 ? (tuning(MXDET_TUNE_T3_NS) == 3 ? 3 : 2) : 0;                   // ring depth of the three-tap kernel (0 = not launched)
  const long long n1_grid = p.nwg_main + (db ? (long long)p.co_tiles * p.ksplit : 0);
  // few workgroups per CU: a deeper ring hides the load latency that co-resident workgroups would otherwise hide
  const int n1_ns = n1_grid > 0 ? (n1_grid <= 2 * 256 ? 4 : 2) : 0;                     // ... of the one-tap kernel
  const bool fold = p.ksplit > 1;
  if (route_probe_on()) {   // mxdet_debug_route_probe: say what would run, touch nothing
    const int32_t rec[kRouteWords] = {MXDET_ROUTE_WGRAD, t3, p.ksplit, p.steps_per_split, p.t3_steps, t3_ns, n1_ns, fold,
                                      (int32_t)n1_grid, p.t3_nwg, d->accumulate, one_tap_steps(*d),
                                      t3 ? three_tap_steps(*d) : 0, 0, 0, 0};
    route_record(rec);
    return MXDET_OK;
  }
  for_ring_depth<2, 3>(t3_ns, [&](auto ns) {
    hipLaunchKernelGGL((wgrad3_kernel<decltype(ns)::value>), dim3((unsigned)p.t3_nwg), dim3(256), 0, s, p);
  });
  for_ring_depth<2, 4>(n1_ns, [&](auto ns) {
    hipLaunchKernelGGL((wgrad_kernel<kWgradBKP, decltype(ns)::value>), dim3((unsigned)n1_grid), dim3(256), 0, s, p);
  });
  if (fold) {
    const long long params = (long long)wgrad_params(*d);
    int wblocks = (int)ceil_div<long long>(params / 4, 256);
    int bblocks = db ? ceil_div(d->Cout, 256) : 0;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)(wblocks + bblocks)), dim3(256), 0, s,
                       (const float*)p.slab, (const float*)p.bslab, p.ksplit, params, d->Cout, wblocks,
                       d->accumulate, dw, db);
  }
  return check_launch("conv2d_wgrad");
}

// ---- grouped weight gradients -----------------------------------------------------------------------------------------
// The plan, step by step. All three-tap items get the same step count S per workgroup (64-pixel steps), the smallest S >=
// the minimum for which the group has at most the target number of workgroups: equal-length workgroups pack the rounds of
// the 512 resident ones evenly, whatever the map size.
static int group_three_tap_steps(const mxdet_wgrad_item_t* items, int n) {
  // workgroups aimed for: the tuned total for a large group (the two groups of the single-GPU step hold 9-10 such layers),
  // proportionally fewer for a small one (the per-stage groups of the exchange schedule hold 2-5: split as deep as the
  // large groups, they paid more in slabs and folds than the extra workgroups gave back)
  int n_t3 = 0;
  for (int i = 0; i < n; ++i) n_t3 += three_tap(items[i].desc) ? 1 : 0;
  long long target = tuning(MXDET_TUNE_T3_TARGET);
  const long long per_item = tuning(MXDET_TUNE_T3_PER_ITEM);
  if (per_item > 0 && per_item * n_t3 < target) target = per_item * n_t3;
  const int smin = (int)tuning(MXDET_TUNE_T3_MINSTEPS);
  auto count = [&](int S) {
    long long c = 0;
    for (int i = 0; i < n; ++i)
      if (three_tap(items[i].desc))
        c += three_tap_tiles(items[i].desc) * clamp_split(ceil_div(three_tap_steps(items[i].desc), S));
    return c;
  };
  int lo = smin < 1 ? 1 : smin, hi = 1 << 16;
  if (count(lo) <= target) hi = lo;
  while (lo < hi) {                         // count() is non-increasing in S
    const int mid = (lo + hi) >> 1;
    if (count(mid) <= target) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The split of a one-tap item of a group with `tiles_total` one-tap tiles per split. Pixels per workgroup: long enough K
// loops to amortise the 64-KiB slab a workgroup writes, short enough that the group has a few thousand workgroups.
// Measured sweep (profiles/r01_h_grouped_wgrad_sweep.txt): ~3072 workgroups per group (3 rounds of the 1024 resident
// ones), 64..128 steps each (mxdet_debug_set_tuning overrides for whole-step sweeps, e.g. shorter workgroups for the
// fused backward launch).
static int grouped_split(int steps, long long tiles_total) {
  const long long target = tuning(MXDET_TUNE_WG_TARGET);
  const int min_steps = (int)tuning(MXDET_TUNE_WG_MINSTEPS) * 32 / kWgradBKP;      // the tunings count 32-pixel steps
  const int max_steps = (int)tuning(MXDET_TUNE_WG_MAXSTEPS) * 32 / kWgradBKP;
  int ks = (int)(tiles_total > 0 ? (target + tiles_total - 1) / tiles_total : 1);
  const int most = max_split(steps, min_steps), least = ceil_div(steps, max_steps);
  ks = ks > most ? most : ks;
  ks = ks < least ? least : ks;
  return clamp_split(ks);
}

// Slabs: items that share dw (one filter applied at several pyramid levels) write into one run of slabs that the first of
// them (the owner) folds, all of it; everything else owns its run. Sets slab / bslab / force_slab of every item and the
// fold fields of the owners; *off = workspace bytes.
static int place_group_slabs(const mxdet_wgrad_item_t* items, int n, WgradG* t, size_t* off) {
  for (int i = 0; i < n; ++i) {
    int owner = i;
    for (int j = 0; j < i; ++j)
      if (items[j].dw == items[i].dw) { owner = j; break; }
    if (owner != i) continue;
    int total_ks = 0, members = 0;
    for (int j = i; j < n; ++j)
      if (items[j].dw == items[i].dw) { total_ks += t[j].p.ksplit; ++members; }
    const size_t params = (size_t)t[i].nparams, cout = (size_t)t[i].p.Cout;
    size_t slab0, bslab0;
    place_slabs((size_t)total_ks, params, cout, off, &slab0, &bslab0);
    int ks0 = 0;
    for (int j = i; j < n; ++j) {
      if (items[j].dw != items[i].dw) continue;
      MXDET_REQUIRE((size_t)t[j].nparams == params && items[j].db == items[i].db, MXDET_ESHAPE,
                    "wgrad_grouped_plan: items %d and %d share dw but differ in shape or db", i, j);
      t[j].p.slab = (float*)(slab0 + (size_t)ks0 * params * sizeof(float));
      t[j].p.bslab = (float*)(bslab0 + (size_t)ks0 * cout * sizeof(float));
      t[j].p.force_slab = members > 1 ? 1 : 0;
      ks0 += t[j].p.ksplit;
    }
    WgradG& g = t[i];
    g.fold_ksplit = total_ks;
    const bool fold = members > 1 || g.p.ksplit > 1;
    g.wblocks = fold ? (int)ceil_div<long long>((long long)params / 4, 256) : 0;
    g.bblocks = (fold && g.p.db) ? ceil_div((int)cout, 256) : 0;
  }
  return MXDET_OK;
}

extern "C" size_t mxdet_conv2d_wgrad_grouped_table_bytes(int32_t n) {
  return n > 0 ? (size_t)n * sizeof(WgradG) : 0;
}

extern "C" int mxdet_conv2d_wgrad_grouped_plan(const mxdet_wgrad_item_t* items, int32_t n, void* table_host,
                                               size_t table_bytes, size_t* workspace_bytes, int32_t* grid_wgrad,
                                               int32_t* grid_big, int32_t* grid_reduce) {
  clear_error();
  MXDET_REQUIRE(items && n > 0 && table_host && workspace_bytes && grid_wgrad && grid_big && grid_reduce, MXDET_EINVAL,
                "wgrad_grouped_plan: null pointer or empty group");
  MXDET_REQUIRE(table_bytes >= (size_t)n * sizeof(WgradG), MXDET_EWORKSPACE, "wgrad_grouped_plan: table too small");
  WgradG* t = (WgradG*)table_host;
  const int S3 = group_three_tap_steps(items, n);
  long long tiles_total = 0;
  for (int i = 0; i < n; ++i)
    if (!three_tap(items[i].desc)) tiles_total += one_tap_tiles(items[i].desc);
  // per item: its tiling and its workgroups in the two numberings, each item's first one a multiple of 8
  long long blocks = 0, bblocks = 0, rblocks = 0;
  for (int i = 0; i < n; ++i) {
    const mxdet_conv_desc_t& d = items[i].desc;
    if (int rc = validate_wgrad_desc(&d, "wgrad_grouped_plan")) return rc;
    MXDET_REQUIRE(items[i].x && items[i].dy && items[i].dw, MXDET_EINVAL, "wgrad_grouped_plan: item %d: null pointer", i);
    WgradG& g = t[i];
    memset(&g, 0, sizeof(g));
    fill_wgrad(g.p, d, items[i].x, items[i].dy, items[i].dw, items[i].db);
    if (three_tap(d)) tile_three_tap(g.p, d, clamp_split(ceil_div(three_tap_steps(d), S3)));
    else tile_one_tap(g.p, d, grouped_split(one_tap_steps(d), tiles_total));
    g.nparams = (long long)wgrad_params(d);
    g.nblocks = g.p.nwg_main + (g.p.db ? g.p.co_tiles * g.p.ksplit : 0);   // one-tap tiles (if any), then the bias workgroups
    g.block0 = (int)blocks;
    blocks += align_up((size_t)g.nblocks, 8);
    g.bnblocks = g.p.t3_nwg;             // no three-tap tiles: an empty range keeps the table sorted for the search
    g.bblock0 = (int)bblocks;
    bblocks += align_up((size_t)g.bnblocks, 8);
    MXDET_REQUIRE(blocks < (1ll << 30) && bblocks < (1ll << 30), MXDET_ESHAPE, "wgrad_grouped_plan: group too large");
  }
  size_t off = 0;
  if (int rc = place_group_slabs(items, n, t, &off)) return rc;
  for (int i = 0; i < n; ++i) {          // fold numbering: only owners that have something to fold hold workgroups
    t[i].rblock0 = (int)rblocks;
    rblocks += t[i].wblocks + t[i].bblocks;
    MXDET_REQUIRE(rblocks < (1ll << 30), MXDET_ESHAPE, "wgrad_grouped_plan: group too large");
  }
  *workspace_bytes = off;
  *grid_wgrad = (int32_t)blocks;
  *grid_big = (int32_t)bblocks;
  *grid_reduce = (int32_t)rblocks;
  return MXDET_OK;
}

extern "C" int mxdet_conv2d_wgrad_grouped(const void* table_dev, int32_t n, int32_t grid_wgrad, int32_t grid_big,
                                          int32_t grid_reduce, void* workspace, size_t workspace_bytes,
                                          size_t workspace_needed, mxdet_stream_t stream) {
  return mxdet_conv2d_wgrad_grouped_parts(table_dev, n, grid_wgrad, grid_big, grid_reduce, 7, workspace, workspace_bytes,
                                          workspace_needed, stream);
}

// parts: bit 0 = the three-tap kernel, bit 1 = the one-tap kernel (+ bias workgroups), bit 2 = the fold. The two tile
// kernels are independent of each other (a caller may issue them on two streams: the 3x3 tiles are MFMA-bound, the 1x1
// tiles HBM-bound); the fold needs both.
extern "C" int mxdet_conv2d_wgrad_grouped_parts(const void* table_dev, int32_t n, int32_t grid_wgrad, int32_t grid_big,
                                                int32_t grid_reduce, int32_t parts, void* workspace, size_t workspace_bytes,
                                                size_t workspace_needed, mxdet_stream_t stream) {
  clear_error();
  if (!(parts & 1)) grid_big = 0;
  if (!(parts & 4)) grid_reduce = 0;
  if (!(parts & 2)) {
    if (grid_big == 0 && grid_reduce == 0) return MXDET_OK;
    grid_wgrad = 0;
  } else if (grid_wgrad == 0 && grid_big == 0 && grid_reduce == 0) {
    return MXDET_OK;
  }
  MXDET_REQUIRE(table_dev && n > 0 && grid_wgrad >= 0 && grid_big >= 0 && grid_wgrad + grid_big + grid_reduce > 0, MXDET_EINVAL,
                "wgrad_grouped: empty group");
  MXDET_REQUIRE(workspace_needed == 0 || (workspace && workspace_bytes >= workspace_needed), MXDET_EWORKSPACE,
                "wgrad_grouped: workspace %zu < %zu", workspace_bytes, workspace_needed);
  hipStream_t s = as_stream(stream);
  // the launches this call makes, decided once: the route probe and the launch code below read the same values
  const int mix = (grid_big > 0 && grid_wgrad > 0 && tuning(MXDET_TUNE_T3_MIX) != 0 && (grid_big & 7) == 0 && (grid_wgrad & 7) == 0)
                      ? (tuning(MXDET_TUNE_T3_MIX) == 2 ? 2 : 1) : 0;            // both tile kinds in one grid (one-tap ring of 3 / of 2)
  const int wg_ns = (int)tuning(MXDET_TUNE_WG_NS);
  const int ns3 = grid_big > 0 ? (mix ? 2 : (tuning(MXDET_TUNE_T3_NS) == 3 ? 3 : 2)) : 0;                    // ring depth, three-tap tiles
  // one-tap tiles: 2 stages (32 KiB, 4 workgroups per CU), 3 (48 KiB, 3 per CU) or 4 (64 KiB, 2 per CU)
  const int ns1 = grid_wgrad > 0 ? (mix ? (mix == 2 ? 2 : 3) : (wg_ns == 3 || wg_ns == 4 ? wg_ns : 2)) : 0;
  if (route_probe_on()) {
    const int32_t rec[kRouteWords] = {MXDET_ROUTE_WGRAD_GROUPED, mix, ns3, ns1, grid_big, grid_wgrad, grid_reduce, parts,
                                      0, 0, 0, 0, 0, 0, 0, 0};
    route_record(rec);
    return MXDET_OK;
  }
  const WgradG* table = (const WgradG*)table_dev;
  unsigned char* ws = (unsigned char*)workspace;
  if (mix) {
    for_ring_depth<2, 3>(ns1, [&](auto ns) {
      hipLaunchKernelGGL((wgrad_mixed_grouped_kernel<2, decltype(ns)::value>), dim3((unsigned)(grid_big + grid_wgrad)),
                         dim3(256), 0, s, table, n, ws, grid_big >> 3, grid_wgrad >> 3);
    });
  } else {
    for_ring_depth<2, 3>(ns3, [&](auto ns) {
      hipLaunchKernelGGL((wgrad3_grouped_kernel<decltype(ns)::value>), dim3((unsigned)grid_big), dim3(256), 0, s, table, n, ws);
    });
    for_ring_depth<2, 3, 4>(ns1, [&](auto ns) {
      hipLaunchKernelGGL((wgrad_grouped_kernel<kWgradBKP, decltype(ns)::value>), dim3((unsigned)grid_wgrad), dim3(256), 0, s,
                         table, n, ws);
    });
  }
  if (grid_reduce > 0)
    hipLaunchKernelGGL(wgrad_reduce_grouped_kernel, dim3((unsigned)grid_reduce), dim3(256), 0, s, table, n,
                       (const unsigned char*)ws);
  return check_launch("conv2d_wgrad_grouped");
}

extern "C" int mxdet_filter_transpose_batched(const void* descs_dev, int32_t ndesc, int32_t total_tiles,
                                              mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(ndesc > 0 && total_tiles > 0, MXDET_ESHAPE, "filter_transpose_batched: empty table");
  MXDET_REQUIRE(descs_dev != nullptr, MXDET_EINVAL, "filter_transpose_batched: null pointer");
  hipLaunchKernelGGL(filter_transpose_batched_kernel, dim3(total_tiles), dim3(256), 0, as_stream(stream),
                     (const TransposeDesc*)descs_dev, ndesc);
  return check_launch("filter_transpose_batched");
}

extern "C" int mxdet_filter_transpose(const uint16_t* w, int32_t Cout, int32_t KH, int32_t KW,
                                      int32_t Cin, uint16_t* wt, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(Cout > 0 && KH > 0 && KW > 0 && Cin > 0, MXDET_ESHAPE, "filter_transpose: bad shape");
  MXDET_REQUIRE(w && wt, MXDET_EINVAL, "filter_transpose: null pointer");
  dim3 grid(ceil_div(Cin, 32), ceil_div(Cout, 32), KH * KW);
  hipLaunchKernelGGL(filter_transpose_kernel, grid, dim3(32, 8), 0, as_stream(stream), w, Cout, KH * KW,
                     Cin, wt);
  return check_launch("filter_transpose");
}
