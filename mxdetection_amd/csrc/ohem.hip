// ohem.hip -- online hard example mining for the R-CNN box head (Shrivastava et al., CVPR 2016):
// the per-roi loss of a read-only forward pass, a total order of an image's candidates by that loss, NMS dedup
// over the order (the mask + keep scan of boxes.hip), the choice of the first R survivors and the gather of their
// proposal-target rows. Definitions in include/mxdet.h. Integer selection, no float atomics, no host round trip.
#include "common.h"
#include "loss_elem.h"

namespace mxdet {

constexpr int kOhemMaxPool = 16384 + 1024;   // rois_stride + G_max of mxdet_proposal_target
constexpr int kOhemNmsMaxPool = 4096;        // n_max of mxdet_nms_batched
constexpr int kRankTile = 8192;              // keys staged in LDS per pass (32 KB)

// score[r] = cls_r + reg_r, the two sums mxdet_rcnn_loss / mxdet_rcnn_loss_iou report for row r alone (norm = 1): the
// walks of loss_elem.h with kGrad = false. One wave per row.
__global__ void __launch_bounds__(256)
ohem_score_kernel(const void* __restrict__ cls, const void* __restrict__ reg, int dtype, int ld_cls, int ld_reg,
                  const int32_t* __restrict__ labels, const float* __restrict__ tgt, const float* __restrict__ wgt,
                  const float* __restrict__ rois, const int32_t* __restrict__ matched, const float* __restrict__ gt, int N,
                  int G_max, long long R, int num_classes, int reg_dim, int kind, float sigma2, BoxStds sd, float reg_weight,
                  float* __restrict__ score) {
  const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r >= R) return;
  const int lane = lane_id();
  const int lab = labels[r];
  if (lab < 0) {                                         // wave-uniform
    if (lane == 0) score[r] = -1.0f;
    return;
  }
  const float lcls = rcnn_softmax_ce<false>(cls, dtype, ld_cls, r, lab, lane, num_classes, 1.0f, 1.0f, nullptr);
  float lreg;
  if (kind < 0)
    lreg = rcnn_reg_smooth_l1<false>(reg, dtype, ld_reg, r, lab, lane, tgt, wgt, reg_dim, sigma2, 1.0f, 1.0f, nullptr);
  else
    lreg = rcnn_reg_iou<false>(reg, dtype, ld_reg, r, lab, lane, rois, matched, gt, N, G_max, num_classes, reg_dim, kind, sd,
                               reg_weight, 1.0f, 1.0f, nullptr);
  // the entries report sum(partial) with partial = l * norm, summed from 0.0f: the same two steps here
  const float c = 0.0f + lcls * 1.0f, g = 0.0f + lreg * 1.0f;
  if (lane == 0) score[r] = c + g;
}

// Rank of every candidate (label >= 0) of image blockIdx.y in the order (score bits descending, pool slot ascending): the
// number of candidates that beat it. The order is total, so the ranks are a permutation of [0, count): order[rank] = slot
// and sorted[rank] = the slot's box are written without atomics. Every workgroup walks all P keys, staged in LDS a tile
// at a time. kRankLanes lanes share a candidate: lane `sub` takes the keys j = sub (mod kRankLanes), so the lanes of a
// wave read kRankLanes consecutive LDS words (each a broadcast to the wave's candidates), and three xor steps add their
// counts. One thread per candidate walked 2,112 words in 18 workgroups: most of the 82 us the selection took without NMS.
// Workgroup x = 0 also writes the candidate count.
constexpr int kRankLanes = 8;
constexpr int kRankPerBlock = 256 / kRankLanes;
__global__ void __launch_bounds__(256)
ohem_rank_kernel(const float* __restrict__ score, const int32_t* __restrict__ labels, const float* __restrict__ rois, int P,
                 int32_t* __restrict__ order, float4* __restrict__ sorted, int32_t* __restrict__ counts) {
  __shared__ unsigned keys[kRankTile];
  __shared__ unsigned vmask[kRankTile / 32];
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, sub = tid & (kRankLanes - 1);
  const long long row0 = (long long)n * P;
  const int i = blockIdx.x * kRankPerBlock + tid / kRankLanes;
  const bool mine = i < P && labels[row0 + i] >= 0;
  const unsigned k = mine ? __float_as_uint(score[row0 + i]) : 0u;
  int rank = 0, total = 0;
  for (int base = 0; base < P; base += kRankTile) {
    const int len = (P - base) < kRankTile ? (P - base) : kRankTile;
    __syncthreads();                                     // the previous tile has been read
    for (int j0 = tid & ~63; j0 < len; j0 += blockDim.x) {
      const int j = j0 + lane, idx = base + j;           // j < kRankTile: len rounds up to at most the tile
      const bool v = idx < P && labels[row0 + idx] >= 0;
      keys[j] = v ? __float_as_uint(score[row0 + idx]) : 0u;
      const unsigned long long m = __ballot(v);
      if (lane == 0) {
        vmask[(j0 >> 5) + 0] = (unsigned)m;
        vmask[(j0 >> 5) + 1] = (unsigned)(m >> 32);
      }
    }
    __syncthreads();
    const int nw = (len + 31) >> 5;                      // keys and mask are staged up to the next multiple of 64
    for (int w = 0; w < nw; ++w) {
      const unsigned m = vmask[w];
      if (m == 0u) continue;                             // workgroup-uniform
      total += __popc(m);
#pragma unroll
      for (int u = 0; u < 32 / kRankLanes; ++u) {
        const int b = u * kRankLanes + sub;
        const unsigned kj = keys[w * 32 + b];
        const int g = base + w * 32 + b;
        const bool beats = kj > k || (kj == k && g < i);
        rank += (int)((m >> b) & 1u) & (int)beats;
      }
    }
  }
  wave_reduce_each<Sum, kRankLanes, kAscend>(rank);
  if (mine && sub == 0) {
    const float* ro = rois + (row0 + i) * 5;
    order[row0 + rank] = i;
    sorted[row0 + rank] = make_float4(ro[1], ro[2], ro[3], ro[4]);
  }
  if (blockIdx.x == 0 && tid == 0) counts[n] = total;
}

// The first min(R, kept) survivors of image blockIdx.x in rank order (keep_idx: ranks the keep scan kept, already cut at R;
// NULL: no dedup, the ranks themselves), written as pool slots: chosen foreground in ascending slot, then chosen
// background in ascending slot, then -1. Ordered compaction by block prefix counts, as proposal_target_kernel.
__global__ void __launch_bounds__(1024)
ohem_choose_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ order, const int32_t* __restrict__ counts,
                   const int32_t* __restrict__ keep_idx, const int32_t* __restrict__ num_keep, int P, int R,
                   int32_t* __restrict__ sel, int32_t* __restrict__ num_sel, int32_t* __restrict__ num_fg) {
  extern __shared__ unsigned char flag[];                // [P]: 1 = chosen
  __shared__ int scratch[32];
  __shared__ int s_nfg;
  const int n = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const long long row0 = (long long)n * P;
  for (int i = tid; i < P; i += nt) flag[i] = 0;
  if (tid == 0) s_nfg = 0;
  int cnt = counts[n];
  cnt = cnt < 0 ? 0 : (cnt > P ? P : cnt);
  int nch = keep_idx ? num_keep[n] : cnt;
  nch = nch < 0 ? 0 : (nch > cnt ? cnt : nch);
  nch = nch > R ? R : nch;
  __syncthreads();
  for (int t = tid; t < nch; t += nt) {
    const int rank = keep_idx ? keep_idx[row0 + t] : t;
    if (rank >= 0 && rank < cnt) {
      const int slot = order[row0 + rank];
      if (slot >= 0 && slot < P) flag[slot] = 1;
    }
  }
  __syncthreads();
  int local = 0;
  for (int i = tid; i < P; i += nt) local += (flag[i] && labels[row0 + i] > 0) ? 1 : 0;
  local = wave_sum(local);
  if ((tid & 63) == 0 && local) atomicAdd(&s_nfg, local);     // integer: any order gives the same sum
  __syncthreads();
  const int nfg = s_nfg;
  int32_t* osel = sel + (long long)n * R;
  int base_fg = 0, base_bg = 0;
  for (int base = 0; base < P; base += nt) {
    const int i = base + tid;
    int st = 0;
    if (i < P && flag[i]) st = labels[row0 + i] > 0 ? 1 : 2;
    int tf, tb;
    const int rf = block_excl_count(st == 1, scratch, &tf);
    const int rb = block_excl_count(st == 2, scratch, &tb);
    if (st) {
      const int pos = st == 1 ? base_fg + rf : nfg + base_bg + rb;
      if (pos < R) osel[pos] = i;
    }
    base_fg += tf;
    base_bg += tb;
  }
  const int chosen = base_fg + base_bg;                  // <= nch <= R
  for (int s = chosen + tid; s < R; s += nt) osel[s] = -1;
  if (tid == 0) {
    num_sel[n] = chosen;
    num_fg[n] = nfg;
  }
}

// One wave per output row (n, s): the pool row sel[n, s] of image n, or the padding row of proposal_target_kernel for
// sel < 0. Target / weight rows move as 16-byte words (reg_dim % 4 == 0); tgt == NULL skips them.
__global__ void __launch_bounds__(256)
ohem_gather_kernel(const int32_t* __restrict__ sel, const float* __restrict__ rois, const int32_t* __restrict__ labels,
                   const int32_t* __restrict__ matched, const float4* __restrict__ tgt, const float4* __restrict__ wgt, int N,
                   int P, int R, int reg4, float* __restrict__ out_rois, int32_t* __restrict__ out_labels,
                   int32_t* __restrict__ out_matched, float4* __restrict__ out_tgt, float4* __restrict__ out_wgt) {
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= (long long)N * R) return;
  const int lane = lane_id();
  const int n = (int)(row / R);
  int s = sel[row];
  if (s >= P) s = -1;                                    // never an index outside the pool
  const long long src = (long long)n * P + s;
  if (lane == 0) {
    float* o = out_rois + row * 5;
    o[0] = (float)n;
    if (s >= 0) {
      const float* ro = rois + src * 5;
      o[1] = ro[1]; o[2] = ro[2]; o[3] = ro[3]; o[4] = ro[4];
      out_labels[row] = labels[src];
      out_matched[row] = matched[src];
    } else {
      o[1] = 0.f; o[2] = 0.f; o[3] = 0.f; o[4] = 0.f;
      out_labels[row] = -1;
      out_matched[row] = -1;
    }
  }
  if (tgt == nullptr) return;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = lane; c < reg4; c += 64) {
    out_tgt[row * reg4 + c] = s >= 0 ? tgt[src * reg4 + c] : z;
    out_wgt[row * reg4 + c] = s >= 0 ? wgt[src * reg4 + c] : z;
  }
}

struct OhemWs {
  float4* sorted;
  int32_t *order, *counts, *keep_idx, *num_keep;
  void* nms;
  size_t nms_bytes, total;
};
static OhemWs carve_ohem(void* base, int N, int P) {
  OhemWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    void* p = base ? (char*)base + off : nullptr;
    off += align_up(bytes, 256);
    return p;
  };
  const size_t rows = (size_t)N * P;
  w.sorted = (float4*)take(rows * sizeof(float4));
  w.order = (int32_t*)take(rows * sizeof(int32_t));
  w.keep_idx = (int32_t*)take(rows * sizeof(int32_t));
  w.counts = (int32_t*)take((size_t)N * sizeof(int32_t));
  w.num_keep = (int32_t*)take((size_t)N * sizeof(int32_t));
  w.nms_bytes = P <= kOhemNmsMaxPool ? mxdet_nms_batched_workspace_bytes(N, P) : 0;
  w.nms = take(w.nms_bytes);
  w.total = off;
  return w;
}

}  // namespace mxdet

using namespace mxdet;

extern "C" int mxdet_ohem_roi_score(const void* cls_logits, const void* bbox_pred, int32_t dtype, int32_t ld_cls,
                                    int32_t ld_reg, const int32_t* labels, const float* bbox_targets,
                                    const float* bbox_weights, const float* rois, const int32_t* matched_gt,
                                    const float* gt_boxes, int32_t N, int32_t G_max, int64_t R, int32_t num_classes,
                                    int32_t reg_dim, int32_t kind, float sigma, float std_x, float std_y, float std_w,
                                    float std_h, float reg_weight, float* score, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(R > 0 && num_classes > 0 && reg_dim > 0 && ld_cls >= num_classes && ld_reg >= reg_dim, MXDET_ESHAPE,
                "ohem_roi_score: bad shape (R, num_classes, reg_dim must be positive, ld_cls >= num_classes, ld_reg >= reg_dim)");
  MXDET_REQUIRE(dtype == MXDET_DTYPE_F32 || dtype == MXDET_DTYPE_BF16, MXDET_EINVAL, "ohem_roi_score: dtype");
  MXDET_REQUIRE(kind == -1 || iou_kind_ok(kind), MXDET_EINVAL,
                "ohem_roi_score: kind must be -1 (smooth-L1) or MXDET_IOU_LOSS_IOU, _GIOU or _DIOU");
  MXDET_REQUIRE(cls_logits && bbox_pred && labels && score, MXDET_EINVAL,
                "ohem_roi_score: null pointer (cls_logits, bbox_pred, labels, score)");
  if (kind < 0) {
    MXDET_REQUIRE(bbox_targets && bbox_weights, MXDET_EINVAL,
                  "ohem_roi_score: bbox_targets and bbox_weights are needed for kind -1 (smooth-L1)");
  } else {
    MXDET_REQUIRE(reg_dim == 4 * num_classes && N > 0 && G_max > 0, MXDET_ESHAPE,
                  "ohem_roi_score: an IoU kind needs reg_dim == 4 * num_classes and N, G_max > 0");
    MXDET_REQUIRE(stds_ok(std_x, std_y, std_w, std_h) && reg_weight > 0.0f, MXDET_EINVAL,
                  "ohem_roi_score: stds and reg_weight must be positive");
    MXDET_REQUIRE(rois && matched_gt && gt_boxes, MXDET_EINVAL,
                  "ohem_roi_score: rois, matched_gt and gt_boxes are needed for an IoU kind");
  }
  const BoxStds sd = {std_x, std_y, std_w, std_h};
  hipLaunchKernelGGL(ohem_score_kernel, dim3((unsigned)ceil_div<int64_t>(R, 4)), dim3(256), 0, as_stream(stream), cls_logits,
                     bbox_pred, dtype, ld_cls, ld_reg, labels, bbox_targets, bbox_weights, rois, matched_gt, gt_boxes, N, G_max,
                     (long long)R, num_classes, reg_dim, kind, sigma * sigma, sd, reg_weight, score);
  return check_launch("ohem_roi_score");
}

extern "C" size_t mxdet_ohem_select_workspace_bytes(int32_t N, int32_t P) {
  if (N <= 0 || P <= 0 || P > kOhemMaxPool) return 0;
  return carve_ohem(nullptr, N, P).total;
}

extern "C" int mxdet_ohem_select(const float* score, const int32_t* labels, const float* rois, int32_t N, int32_t P,
                                 int32_t R, float nms_thresh, int32_t* sel, int32_t* num_sel, int32_t* num_fg,
                                 void* workspace, size_t workspace_bytes, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(N > 0 && P > 0, MXDET_ESHAPE, "ohem_select: N and P must be positive");
  MXDET_REQUIRE(P <= kOhemMaxPool, MXDET_ESHAPE, "ohem_select: P %d > %d unsupported", P, kOhemMaxPool);
  MXDET_REQUIRE(R >= 1, MXDET_ESHAPE, "ohem_select: R must be >= 1");
  MXDET_REQUIRE(nms_thresh > 0.0f, MXDET_EINVAL, "ohem_select: nms_thresh must be positive (>= 1: no dedup)");
  const bool nms = nms_thresh < 1.0f;
  MXDET_REQUIRE(!nms || P <= kOhemNmsMaxPool, MXDET_ESHAPE,
                "ohem_select: P %d > %d needs nms_thresh >= 1 (the keep scan's limit)", P, kOhemNmsMaxPool);
  MXDET_REQUIRE(score && labels && rois && sel && num_sel && num_fg, MXDET_EINVAL, "ohem_select: null pointer");
  const OhemWs w = carve_ohem(workspace, N, P);
  MXDET_REQUIRE(workspace && workspace_bytes >= w.total, MXDET_EWORKSPACE, "ohem_select: workspace %zu < %zu",
                workspace_bytes, w.total);
  MXDET_REQUIRE(((uintptr_t)workspace % 16) == 0, MXDET_EINVAL, "ohem_select: workspace must be 16-byte aligned");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(ohem_rank_kernel, dim3((unsigned)ceil_div(P, kRankPerBlock), (unsigned)N), dim3(256), 0, s, score, labels, rois,
                     P, w.order, w.sorted, w.counts);
  if (nms) {
    int rc = check_launch("ohem_select");
    if (rc != MXDET_OK) return rc;
    rc = mxdet_nms_batched((const float*)w.sorted, w.counts, nullptr, N, P, nms_thresh, R, w.keep_idx, w.num_keep, w.nms,
                           w.nms_bytes, stream);
    if (rc != MXDET_OK) return rc;
  }
  hipLaunchKernelGGL(ohem_choose_kernel, dim3((unsigned)N), dim3(1024), (size_t)align_up((size_t)P, 16), s, labels, w.order,
                     w.counts, nms ? w.keep_idx : nullptr, nms ? w.num_keep : nullptr, P, R, sel, num_sel, num_fg);
  return check_launch("ohem_select");
}

extern "C" int mxdet_ohem_gather(const int32_t* sel, const float* pool_rois, const int32_t* pool_labels,
                                 const int32_t* pool_matched_gt, const float* pool_bbox_targets,
                                 const float* pool_bbox_weights, int32_t N, int32_t P, int32_t R, int32_t reg_dim,
                                 float* out_rois, int32_t* labels, float* bbox_targets, float* bbox_weights,
                                 int32_t* matched_gt, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(N > 0 && P > 0 && R >= 1, MXDET_ESHAPE, "ohem_gather: N, P and R must be positive");
  MXDET_REQUIRE(P <= kOhemMaxPool, MXDET_ESHAPE, "ohem_gather: P %d > %d unsupported", P, kOhemMaxPool);
  MXDET_REQUIRE(sel && pool_rois && pool_labels && pool_matched_gt && out_rois && labels && matched_gt, MXDET_EINVAL,
                "ohem_gather: null pointer");
  const int nset = (pool_bbox_targets != nullptr) + (pool_bbox_weights != nullptr) + (bbox_targets != nullptr) +
                   (bbox_weights != nullptr);
  MXDET_REQUIRE(nset == 0 || nset == 4, MXDET_EINVAL,
                "ohem_gather: pool_bbox_targets, pool_bbox_weights, bbox_targets and bbox_weights must be NULL together");
  if (nset) {
    MXDET_REQUIRE(reg_dim > 0 && reg_dim % 4 == 0, MXDET_ESHAPE, "ohem_gather: reg_dim must be a positive multiple of 4");
    MXDET_REQUIRE((((uintptr_t)pool_bbox_targets | (uintptr_t)pool_bbox_weights | (uintptr_t)bbox_targets |
                    (uintptr_t)bbox_weights) % 16) == 0,
                  MXDET_EINVAL, "ohem_gather: targets and weights must be 16-byte aligned");
  }
  const int64_t rows = (int64_t)N * R;
  hipLaunchKernelGGL(ohem_gather_kernel, dim3((unsigned)ceil_div<int64_t>(rows, 4)), dim3(256), 0, as_stream(stream), sel,
                     pool_rois, pool_labels, pool_matched_gt, (const float4*)pool_bbox_targets,
                     (const float4*)pool_bbox_weights, N, P, R, reg_dim / 4, out_rois, labels, matched_gt, (float4*)bbox_targets,
                     (float4*)bbox_weights);
  return check_launch("ohem_gather");
}
