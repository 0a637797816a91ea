// roi_gather.h -- what roi_align.hip and deform_roi_pool.hip share: the feature pyramid as a kernel argument, the roi
// header clamp, packed pixel spans, and the skeleton of the tile gather that both feature-gradient kernels are built on
// (workgroup -> pyramid level, the ascending LDS roi list, the bf16 row write-out).
//
// The tile gather: a workgroup of kSegWaves waves owns kSegWaves consecutive kSegW-pixel row segments (one WAVE per
// segment, a lane owns 4 channels). Per round of kSegChunk rois it compacts, in ascending roi order, the rois whose
// pixel box meets its tile into LDS (block_compact_ascending), every wave walks that list, and seg_store4 writes the
// sums. What a hit stores and how the walk weighs it is the caller's.
#pragma once
#include "common.h"

namespace mxdet {

struct FeatPyr {
  int num_levels, lvl_min, N;
  int H[8], W[8];
  float scale[8];
  void* feat[8];
};

// the copy only: every caller checks the level count, sizes and maps first, with its own messages
static inline void pyr_copy(FeatPyr& d, const mxdet_feat_pyramid_t& f, int N) {
  memset(&d, 0, sizeof(d));
  d.num_levels = f.num_levels;
  d.lvl_min = f.lvl_min;
  d.N = N;
  for (int l = 0; l < f.num_levels; ++l) {
    d.H[l] = f.H[l]; d.W[l] = f.W[l]; d.scale[l] = f.spatial_scale[l]; d.feat[l] = f.feat[l];
  }
}

// level index of roi r clamped into the pyramid, image index clamped into [0, N): never index outside either
__device__ __forceinline__ void roi_image_level(const FeatPyr& f, const float* __restrict__ rois,
                                                const int32_t* __restrict__ levels, long long r, int* lvl, int* n) {
  int l = levels[r] - f.lvl_min;
  *lvl = l < 0 ? 0 : (l >= f.num_levels ? f.num_levels - 1 : l);
  const int b = (int)rois[r * 5];
  *n = b < 0 ? 0 : (b >= f.N ? f.N - 1 : b);
}

// block0[l] = first workgroup (or row) of level l, block0[num_levels] = their number
static inline int layout_block0(int* block0, const int* per_level, int num_levels) {
  int blocks = 0;
  for (int l = 0; l < num_levels; ++l) {
    block0[l] = blocks;
    blocks += per_level[l];
  }
  block0[num_levels] = blocks;
  return blocks;
}

__device__ __forceinline__ int level_of_block(const int* block0, int num_levels, int bid) {
  int l = 0;
  while (l + 1 < num_levels && bid >= block0[l + 1]) ++l;
  return l;
}

// ---- pixel spans [lo, hi] packed as lo | hi << 16 (sizes < 32768; the records of both workspaces hold them) ----
constexpr unsigned kSpanEmpty = 0xffffu;                 // lo 0xffff > hi 0
__device__ __forceinline__ unsigned span_pack(int lo, int hi) { return (unsigned)lo | ((unsigned)hi << 16); }
__device__ __forceinline__ int span_lo(unsigned packed) { return (int)(packed & 0xffffu); }
__device__ __forceinline__ int span_hi(unsigned packed) { return (int)(packed >> 16); }
__device__ __forceinline__ bool span_hits(unsigned packed, int lo, int hi) {   // [plo, phi] meets [lo, hi]
  return span_hi(packed) >= lo && span_lo(packed) <= hi;
}

constexpr int kSegW = 8;          // pixels per wave
constexpr int kSegWaves = 4;      // waves (segment columns) per workgroup
constexpr int kSegChunk = 1024;   // rois per list round

// One iteration of the list builder, for all WAVES * 64 threads of the workgroup: `hit` threads get consecutive slots
// from *s_cnt on in thread order (so ascending roi order) and run store(slot); *s_cnt then grows by the hit count.
// All three barriers are reached by every thread. A round starts with `__syncthreads(); if (tid == 0) s_cnt = 0;
// __syncthreads();` at the caller, and the list is complete (and *s_cnt its length) when the last call returns.
template <int WAVES, class Store>
__device__ __forceinline__ void block_compact_ascending(bool hit, int lane, int wid, int* wcnt, int* s_cnt, Store store) {
  const unsigned long long m = __ballot(hit);
  if (lane == 0) wcnt[wid] = __popcll(m);
  __syncthreads();
  int base = *s_cnt;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) base += (w < wid) ? wcnt[w] : 0;
  if (hit) store(base + __popcll(m & ((1ull << lane) - 1ull)));
  __syncthreads();
  if (threadIdx.x == 0) {
    int tt = *s_cnt;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) tt += wcnt[w];
    *s_cnt = tt;
  }
  __syncthreads();
}

__device__ __forceinline__ float readlane_f(float v, int lane) {
  return __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(v), lane));
}

// four channels of one pixel to the bf16 map at o, optionally added to what is there (new + old). EXACT packs with the
// shared bit-exact f32_to_bf16_bits (RoIAlign), otherwise with the hardware conversion (deformable pool); the two
// differ in NaN payloads only. (The half-vector unpack stays spelled out: with unpack4_bf16 hipcc emits different
// code for RoIAlign's table and segment kernels.)
template <bool EXACT>
__device__ __forceinline__ void seg_store4(uint16_t* o, const float (&v)[4], bool add) {
  float s[4] = {v[0], v[1], v[2], v[3]};
  if (add) {
    const uint2 e = *(const uint2*)o;
    s[0] = s[0] + __uint_as_float(e.x << 16); s[1] = s[1] + __uint_as_float(e.x & 0xffff0000u);
    s[2] = s[2] + __uint_as_float(e.y << 16); s[3] = s[3] + __uint_as_float(e.y & 0xffff0000u);
  }
  uint2 w;
  if (EXACT) {
    w.x = (unsigned)f32_to_bf16_bits(s[0]) | ((unsigned)f32_to_bf16_bits(s[1]) << 16);
    w.y = (unsigned)f32_to_bf16_bits(s[2]) | ((unsigned)f32_to_bf16_bits(s[3]) << 16);
  } else {
    w = make_uint2(pack_bf16x2(s[0], s[1]), pack_bf16x2(s[2], s[3]));
  }
  *(uint2*)o = w;
}

}  // namespace mxdet
