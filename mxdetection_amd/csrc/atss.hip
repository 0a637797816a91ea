// atss.hip -- Adaptive Training Sample Selection (Zhang et al., CVPR 2020) for the dense head on gfx950.
//
// The anchor<->GT assignment of RetinaNet + ATSS: per ground-truth box the k nearest anchors of every pyramid level, an
// IoU threshold per box from their mean and (unbiased) variance, the candidates above it whose centre lies inside the
// box. Like every other target op (targets.hip) it stays on the device, inside the captured step; the semantics are
// frozen in include/mxdet.h and restated in numpy by tests/_atss_ref.py, compared bit for bit.
//
//   zero_u32_kernel         the per-(image, anchor) 64-bit word of the workspace := 0 (0 = unassigned)
//   atss_candidates_kernel  grid (G_max, N), 1024 threads: one workgroup owns one ground-truth box.
//                           per level: the k smallest (distance bits, anchor index) by select.h's radix select (a pure
//                           predicate), the chosen indices appended to an LDS list (<= L*k <= 128);
//                           rank sort of the list (ascending anchor index: the order of the sums is part of the
//                           definition); IoUs in parallel; ONE lane walks them for s, mean, ss, var;
//                           the lanes test (threshold, centre inside) and post atomicMax(iou_bits << 32 | ~g) on the
//                           anchor's word: integer, order independent, hence deterministic; at most L*k per box.
//   atss_encode_kernel      one thread per (image, anchor): word -> labels, matched_gt, bbox_targets, matched_iou.
//
// All arithmetic is one fp32 operation per step in the header's order; this file is built without FMA contraction.
#include "common.h"
#include "select.h"

namespace mxdet {

constexpr int kAtssThreads = 1024;
constexpr int kAtssMaxLevels = 8;
constexpr int kAtssMaxTopk = 16;
constexpr int kAtssMaxCand = kAtssMaxLevels * kAtssMaxTopk;   // 128

struct AtssLevels { int off[kAtssMaxLevels + 1]; };   // by value: the host array is read at call time only

// squared centre distance of anchor b to the point (gx, gy): product, product, one add. Non-negative (never -0), so
// its bit pattern orders like the value.
__device__ __forceinline__ unsigned atss_dist_bits(const float4 b, float gx, float gy) {
  const float cx = 0.5f * (b.x + b.z);
  const float cy = 0.5f * (b.y + b.w);
  const float dx = cx - gx;
  const float dy = cy - gy;
  const float dxx = dx * dx;
  const float dyy = dy * dy;
  return __float_as_uint(dxx + dyy);
}

__global__ void __launch_bounds__(kAtssThreads)
atss_candidates_kernel(const float4* __restrict__ anchors, long long A_total, AtssLevels lv, int L,
                       const float* __restrict__ gt, int G_max, int topk, unsigned long long* __restrict__ words) {
  __shared__ SelectSmem sm;
  __shared__ int s_raw[kAtssMaxCand], s_idx[kAtssMaxCand];
  __shared__ float s_iou[kAtssMaxCand];
  __shared__ int s_count;
  __shared__ float s_mean, s_var;
  const int g = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const float* q = gt + ((long long)n * G_max + g) * 5;
  if (q[4] < 0.0f) return;   // padding row: block-uniform
  const float gx1 = q[0], gy1 = q[1], gx2 = q[2], gy2 = q[3];
  const float gx = 0.5f * (gx1 + gx2);
  const float gy = 0.5f * (gy1 + gy2);
  if (tid == 0) s_count = 0;
  // the first barrier inside block_select_threshold orders this store before the first append

  for (int l = 0; l < L; ++l) {
    const int base = lv.off[l], nl = lv.off[l + 1] - base;
    auto keyf = [&](int i, unsigned& kv) -> bool { kv = atss_dist_bits(anchors[base + i], gx, gy); return true; };
    // position in the level as the tie-break index: the same order as the global anchor index
    const SelectResult r = block_select_threshold(nl, topk, 32, keyf, sm);
    for (int i = tid; i < nl; i += kAtssThreads) {
      unsigned kv;
      keyf(i, kv);
      if (r.chosen(kv, (unsigned)i)) {
        const int slot = atomicAdd(&s_count, 1);          // exactly min(topk, nl) per level: slot < kAtssMaxCand
        if (slot < kAtssMaxCand) s_raw[slot] = base + i;
      }
    }
    // the next level's select starts with a barrier after its histogram clear; s_raw / s_count are not touched by it
  }
  __syncthreads();
  const int cnt = s_count < kAtssMaxCand ? s_count : kAtssMaxCand;

  // ascending anchor index by rank (indices are distinct), then the IoU of every candidate
  if (tid < cnt) {
    const int mine = s_raw[tid];
    int rank = 0;
    for (int j = 0; j < cnt; ++j) rank += (s_raw[j] < mine) ? 1 : 0;
    s_idx[rank] = mine;
  }
  __syncthreads();
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  float v = 0.0f;
  int a = 0;
  if (tid < cnt) {
    a = s_idx[tid];
    b = anchors[a];
    v = mxdet_iou(b.x, b.y, b.z, b.w, gx1, gy1, gx2, gy2);
    s_iou[tid] = v;
  }
  __syncthreads();
  if (tid == 0) {   // the order of both sums is part of the definition
    float s = 0.0f;   // 0 + v_0 = v_0 exactly
    for (int i = 0; i < cnt; ++i) s = s + s_iou[i];
    const float mean = s / (float)cnt;
    float ss = 0.0f;
    for (int i = 0; i < cnt; ++i) {
      const float t = s_iou[i] - mean;
      const float tt = t * t;
      ss = ss + tt;
    }
    s_mean = mean;
    s_var = cnt > 1 ? ss / (float)(cnt - 1) : 0.0f;
  }
  __syncthreads();
  if (tid < cnt) {
    const float mean = s_mean, var = s_var;
    const float t = v - mean;
    const float tt = t * t;
    const bool above = (v >= mean) && (tt >= var);
    const float cx = 0.5f * (b.x + b.z);
    const float cy = 0.5f * (b.y + b.w);
    float m = cx - gx1;
    const float m1 = cy - gy1, m2 = gx2 - cx, m3 = gy2 - cy;
    m = m1 < m ? m1 : m;
    m = m2 < m ? m2 : m;
    m = m3 < m ? m3 : m;
    if (above && m > 0.01f) {
      const unsigned long long w = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(~(unsigned)g);
      atomicMax(&words[(long long)n * A_total + a], w);
    }
  }
}

__global__ void __launch_bounds__(256)
atss_encode_kernel(const float4* __restrict__ anchors, long long A_total, const float* __restrict__ gt, int G_max,
                   const unsigned long long* __restrict__ words, int32_t* __restrict__ labels,
                   int32_t* __restrict__ matched_gt, float4* __restrict__ targets, float* __restrict__ matched_iou) {
  const int n = blockIdx.y;
  const long long a = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= A_total) return;
  const long long idx = (long long)n * A_total + a;
  const unsigned long long w = words[idx];
  int lab = 0, mg = -1;
  float iou = 0.0f;
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  if (w != 0ull) {   // a posted word is never 0: its low half is ~g with g < 2^31
    lab = 1;
    mg = (int)(~(unsigned)w);
    iou = __uint_as_float((unsigned)(w >> 32));
    const float4 b = anchors[a];
    const float* q = gt + ((long long)n * G_max + mg) * 5;
    float o[4];
    mxdet_encode(b.x, b.y, b.z, b.w, q[0], q[1], q[2], q[3], o);
    t = make_float4(o[0], o[1], o[2], o[3]);
  }
  labels[idx] = lab;
  matched_gt[idx] = mg;
  targets[idx] = t;
  if (matched_iou) matched_iou[idx] = iou;
}

}  // namespace mxdet

using namespace mxdet;

extern "C" size_t mxdet_atss_assign_workspace_bytes(int32_t N, int64_t A_total, int32_t G_max) {
  if (N <= 0 || A_total <= 0 || G_max <= 0) return 0;
  return align_up((size_t)N * (size_t)A_total * sizeof(unsigned long long), 256);
}

extern "C" int mxdet_atss_assign(const float* anchors, int64_t A_total, const int64_t* level_offsets, int32_t L,
                                 const float* gt_boxes, int32_t N, int32_t G_max, int32_t topk, int32_t* labels,
                                 int32_t* matched_gt, float* bbox_targets, float* matched_iou, void* workspace,
                                 size_t workspace_bytes, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(N > 0 && A_total > 0 && G_max > 0, MXDET_ESHAPE, "atss_assign: bad sizes (N, A_total, G_max)");
  MXDET_REQUIRE(A_total < (1ll << 30) && G_max <= 1024, MXDET_ESHAPE, "atss_assign: A_total / G_max too large");
  MXDET_REQUIRE(L >= 1 && L <= kAtssMaxLevels, MXDET_ESHAPE, "atss_assign: L %d not in 1..%d", L, kAtssMaxLevels);
  MXDET_REQUIRE(topk >= 1 && topk <= kAtssMaxTopk, MXDET_EINVAL, "atss_assign: topk %d not in 1..%d", topk, kAtssMaxTopk);
  MXDET_REQUIRE(level_offsets, MXDET_EINVAL, "atss_assign: level_offsets is null");
  MXDET_REQUIRE(anchors && gt_boxes, MXDET_EINVAL, "atss_assign: null input (anchors / gt_boxes)");
  MXDET_REQUIRE(labels && matched_gt && bbox_targets, MXDET_EINVAL,
                "atss_assign: null output (labels / matched_gt / bbox_targets)");
  AtssLevels lv;
  MXDET_REQUIRE(level_offsets[0] == 0, MXDET_ESHAPE, "atss_assign: level_offsets[0] = %lld, not 0",
                (long long)level_offsets[0]);
  for (int l = 0; l < L; ++l)
    MXDET_REQUIRE(level_offsets[l + 1] > level_offsets[l], MXDET_ESHAPE,
                  "atss_assign: level_offsets not ascending at level %d (an empty level)", l);
  MXDET_REQUIRE(level_offsets[L] == A_total, MXDET_ESHAPE, "atss_assign: level_offsets[L] = %lld != A_total = %lld",
                (long long)level_offsets[L], (long long)A_total);
  for (int l = 0; l <= kAtssMaxLevels; ++l) lv.off[l] = (int)level_offsets[l < L ? l : L];
  const size_t need = mxdet_atss_assign_workspace_bytes(N, A_total, G_max);
  MXDET_REQUIRE(workspace && workspace_bytes >= need, MXDET_EWORKSPACE, "atss_assign: workspace %zu < %zu",
                workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  unsigned long long* words = (unsigned long long*)workspace;
  hipError_t e = zero_async(words, (size_t)N * (size_t)A_total * sizeof(unsigned long long), s);
  MXDET_REQUIRE(e == hipSuccess, MXDET_EHIP, "atss_assign: zero fill failed");
  hipLaunchKernelGGL(atss_candidates_kernel, dim3(G_max, N), dim3(kAtssThreads), 0, s, (const float4*)anchors,
                     (long long)A_total, lv, (int)L, gt_boxes, (int)G_max, (int)topk, words);
  hipLaunchKernelGGL(atss_encode_kernel, dim3((unsigned)ceil_div<long long>(A_total, 256), N), dim3(256), 0, s,
                     (const float4*)anchors, (long long)A_total, gt_boxes, (int)G_max,
                     (const unsigned long long*)words, labels, matched_gt, (float4*)bbox_targets, matched_iou);
  return check_launch("atss_assign");
}
