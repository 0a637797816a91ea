// wave.h -- the one set of cross-lane / cross-wave reduce and scan primitives (wave = 64 lanes); common.h includes it. Each
// choice below decides result bits or the safety of a kernel: pick a form here, write no new loop (users: DESIGN.md 5w).
//
// Deliberately NOT expressed through these: the sequential 16-lane sums of rpn_sparse.hip (the dense split-K order); the
// (value, index) argmax exchange of keypoint_decode_kernel; the sort exchange of deform_conv.hip; the lane reads
// __shfl(x, q0 + k) of the distribution box part (loss_elem.h, losses.hip, retina_loss.hip); the __shfl(.., src) broadcasts
// of select.h and rpn_sparse.hip; the __shfl_down partial prefix sums of RoIAlign's sample weights; row16_max / dpp_mov of
// attention.hip; the Chan merge of gn_merge_stats_kernel (three values combined as one record); the wgrad* and conv tiles.
// Left hand-written as well, because a helper changed their kernels' device code and no test pins their fp32 order bit for
// bit: the 16-lane row sums of attn_fwd_kernel, the 4-lane fold of carafe_bwd_m_kernel, the run-time-width butterfly of
// deform_col2im_coord_kernel.
#pragma once
#include <hip/hip_runtime.h>

namespace mxdet {

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// Op::f(own value, other lane's value). MaxSel / MinSel are comparison-selects: a NaN never wins. FMax is fmaxf: the non-NaN
// operand wins, so it is not MaxSel where NaNs can occur. fold4: how block4_reduce combines the four wave results (MaxSel
// and MinSel have none: no block fold uses them; add one with the first).
struct Sum {
  template <class T> __device__ static __forceinline__ T f(T a, T b) { return a + b; }
  template <class T> __device__ static __forceinline__ T fold4(T a, T b, T c, T d) { return ((a + b) + c) + d; }
};
struct MaxSel { template <class T> __device__ static __forceinline__ T f(T a, T b) { return b > a ? b : a; } };
struct MinSel { template <class T> __device__ static __forceinline__ T f(T a, T b) { return b < a ? b : a; } };
struct FMax {
  __device__ static __forceinline__ float f(float a, float b) { return fmaxf(a, b); }
  __device__ static __forceinline__ float fold4(float a, float b, float c, float d) { return fmaxf(fmaxf(a, b), fmaxf(c, d)); }
};
enum WaveSteps { kDescend, kAscend };
enum WaveLanes { kEveryLane, kLane0 };
enum BlockScratch { kScratchReused, kScratchOnce };

// WAVE REDUCTION over aligned segments of W lanes (a power of two <= 64). No barrier, no LDS; every lane of the wave must
// arrive (a shuffle reads whatever an inactive lane's register holds).
//   Steps  kDescend: lane distances W/2, W/4 .. 1.  kAscend: 1, 2 .. W/2. Level d combines the partial results of lanes l and
//          l ^ d, so for a float Sum the two round differently: a site keeps the order it was written with.
//   Lanes  kEveryLane: the __shfl_xor butterfly; every lane of the segment ends with the same bits.
//          kLane0: the __shfl_down tree (64 lanes, kDescend only); lane 0 holds the result, the other lanes rubbish. On
//          lane 0 it pairs the same operands at every level as the kDescend butterfly and fp32 addition is commutative: the
//          lane-0 bits are equal. Both forms are kept: with the tree the device code of the lane-0 sites stays as it was.
// wave_reduce_each reduces several values in place, level by level in argument order; each gets the bits of its own call.
template <class Op = Sum, int W = 64, WaveSteps S = kDescend, WaveLanes L = kEveryLane, class... T>
__device__ __forceinline__ void wave_reduce_each(T&... v) {
  static_assert(W <= 64 && (W & (W - 1)) == 0 && (L == kEveryLane || (W == 64 && S == kDescend)), "see the forms above");
  if (L == kLane0) {
    for (int o = 32; o > 0; o >>= 1) ((v = Op::f(v, __shfl_down(v, o))), ...);
  } else if (S == kDescend) {
    for (int o = W >> 1; o > 0; o >>= 1) ((v = Op::f(v, __shfl_xor(v, o))), ...);
  } else {
    for (int o = 1; o < W; o <<= 1) ((v = Op::f(v, __shfl_xor(v, o))), ...);
  }
}
template <class Op = Sum, int W = 64, WaveSteps S = kDescend, WaveLanes L = kEveryLane, class T>
__device__ __forceinline__ T wave_reduce(T v) { wave_reduce_each<Op, W, S, L>(v); return v; }
template <class T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce<Sum>(v); }
template <class T> __device__ __forceinline__ T wave_sum_lane0(T v) { return wave_reduce<Sum, 64, kDescend, kLane0>(v); }

// WAVE SCAN of ints, the __shfl_up ladder 1, 2 .. 32: lane l returns v_0 + .. + v_l. `lane` is the caller's lane_id().
// Callers derive the exclusive value (incl - v) and the total (__shfl(incl, 63)).
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    int t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

__device__ __forceinline__ int wave_excl_count(bool pred, int* total) {
  unsigned long long m = __ballot(pred);
  int lane = lane_id();
  unsigned long long below = (lane == 0) ? 0ull : (m & (~0ull >> (64 - lane)));
  *total = __popcll(m);
  return __popcll(below);
}

// BLOCK FOLD for workgroups of exactly 4 waves: the wave step (64 lanes, kDescend), lane 0 of wave w writes s4[w],
// __syncthreads, and EVERY thread returns Op::fold4(s4[0..3]): ((r0 + r1) + r2) + r3 for Sum (wave order, no start value: a
// -0.0f of wave 0 survives), the pair tree for FMax (associative). Scratch is the caller's promise about s4:
//   kScratchReused  s4 may still be read from an earlier call: a __syncthreads stands in front of the write (two in all).
//   kScratchOnce    no leading barrier: correct ONLY if nothing else in the kernel writes or has read s4.
// Other folds on the same wave step, not to be merged with this one: block_sum_fixed (loss_elem.h: run-time wave count,
// starts from 0.0f, valid on thread 0) and kp_block_max / kp_block_sum (keypoint.hip: 16 waves, pair tree of float4 reads).
template <class Op, WaveLanes L, BlockScratch P, class T>
__device__ __forceinline__ T block4_reduce(T v, T* s4) {
  v = wave_reduce<Op, 64, kDescend, L>(v);
  if (P == kScratchReused) __syncthreads();
  if (lane_id() == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return Op::fold4(s4[0], s4[1], s4[2], s4[3]);
}

// BLOCK SCAN of ints in thread order, any whole number of waves; `sh` holds blockDim.x / 64 ints. No barrier in front of the
// write of sh, one behind the last read: a second call may follow at once, but the caller must not have sh in use before
// the first. (block_excl_count below, the ballot form for predicates, has its barrier in FRONT of the write instead.)
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int* total) {
  const int wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int incl = wave_incl_scan(v, lane_id());
  if (lane_id() == 63) sh[wid] = incl;
  __syncthreads();
  int base = 0, all = 0;
  for (int i = 0; i < nw; ++i) {
    const int s = sh[i];
    if (i < wid) base += s;
    all += s;
  }
  __syncthreads();
  *total = all;
  return base + incl - v;
}

// Block-wide exclusive prefix count of a predicate in thread order; returns this thread's rank and
// the block total. `scratch` must hold (blockDim.x/64 + 1) ints. Contains __syncthreads.
__device__ inline int block_excl_count(bool pred, int* scratch, int* total) {
  int wtot;
  int r = wave_excl_count(pred, &wtot);
  int wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();  // protect scratch reuse
  if (lane_id() == 0) scratch[wid] = wtot;
  __syncthreads();
  int base = 0, all = 0;
  for (int i = 0; i < nw; ++i) {
    int v = scratch[i];
    if (i < wid) base += v;
    all += v;
  }
  *total = all;
  return base + r;
}

}  // namespace mxdet
