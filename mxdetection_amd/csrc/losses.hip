// losses.hip -- fused forward+backward detection losses for gfx950.
//
// Slot: core/loss (/root/reference/README.md:19); MXNet roles smooth_l1(scalar=sigma), SoftmaxOutput
// (use_ignore, normalization='valid') and the RetinaNet sigmoid focal loss (README.md:37). Each loss
// reads its logits once and writes the gradient in the same pass (HBM-bound: 2 B read + 2 B written
// per bf16 logit). Scalar losses are reduced in a fixed order (per-block tree, then an index-ordered
// single-workgroup pass), so repeated runs give identical bits.
#include "common.h"
#include "loss_elem.h"

namespace mxdet {

// ---------------------------------------------------------------------------------------------
__global__ void smooth_l1_fwd_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                     const float* __restrict__ w, long long n, float sigma2,
                                     float* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float d = p[i] - t[i];
  if (w) d = d * w[i];
  out[i] = mxdet_smooth_l1(d, sigma2);
}
__global__ void smooth_l1_bwd_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                     const float* __restrict__ w, const float* __restrict__ go,
                                     long long n, float sigma2, int accumulate, float* __restrict__ gp) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float ww = w ? w[i] : 1.0f;
  float d = (p[i] - t[i]) * ww;
  float g = mxdet_smooth_l1_grad(d, sigma2) * ww;
  if (go) g = g * go[i];
  gp[i] = accumulate ? gp[i] + g : g;
}

// ---------------------------------------------------------------------------------------------
// focal loss
__global__ void count_fg_kernel(const int32_t* __restrict__ labels, long long n, int* __restrict__ cnt) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool fg = (i < n) && labels[i] > 0;
  unsigned long long m = __ballot(fg);
  if (lane_id() == 0 && m) atomicAdd(cnt, __popcll(m));
}

// The unfused class loss over [n, C] logits: sigmoid focal (FocalElem; quality is not read) or QFL / VFL (QualityElem) with a
// per-row quality as the target of the row's own class column. Grid-stride, gradient in the logits' dtype.
template <class Elem>
__global__ void __launch_bounds__(256)
cls_loss_kernel(const void* __restrict__ logits, int dtype, const int32_t* __restrict__ labels,
                const float* __restrict__ quality, long long n, int C, const Elem elem, float grad_scale,
                const int* __restrict__ num_fg, void* __restrict__ grad, float* __restrict__ partial) {
  __shared__ float red[8];
  const long long total = n * C;
  int nf = *num_fg;
  float inv_norm = 1.0f / (float)(nf > 1 ? nf : 1);
  float acc = 0.0f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    long long r = i / C;
    int c = (int)(i - r * C);
    int lab = labels[r];
    float g = 0.0f;
    if (lab >= 0) {
      const bool positive = lab == c + 1;
      acc += elem(load_as_f32(logits, i, dtype), positive, (Elem::kQuality && positive) ? quality[r] : 0.0f, g);
    }
    store_from_f32(grad, i, dtype, g * inv_norm * grad_scale);
  }
  store_block_partials<1>({acc}, inv_norm, red, partial);
}

// out[j] = sum_i partial[i*ncomp + j], index-ordered, one workgroup
__global__ void __launch_bounds__(256)
finalize_kernel(const float* __restrict__ partial, int count, int ncomp, float* __restrict__ out) {
  __shared__ float red[8];
  for (int j = 0; j < ncomp; ++j) {
    float acc = 0.0f;
    for (int i = threadIdx.x; i < count; i += blockDim.x) acc += partial[(long long)i * ncomp + j];
    float s = block_sum_fixed(acc, red);
    if (threadIdx.x == 0) out[j] = s;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// RPN losses over one level's head output [N,H,W,Cpad]; one thread per cell.
__global__ void __launch_bounds__(256)
rpn_loss_kernel(const uint16_t* __restrict__ head, int N, int H, int W, int A, int Cpad,
                const int32_t* __restrict__ labels, const float4* __restrict__ targets,
                long long A_total, long long level_offset, float sigma2, float norm, float loss_scale,
                uint16_t* __restrict__ grad, float* __restrict__ partial) {
  __shared__ float red[8];
  long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long cells = (long long)N * H * W;
  float lc = 0.0f, lr = 0.0f;
  if (cell < cells) {
    int n = (int)(cell / ((long long)H * W));
    long long local = cell - (long long)n * H * W;
    const uint16_t* h = head + cell * Cpad;
    uint16_t* g = grad + cell * Cpad;
    for (int c = 5 * A; c < Cpad; ++c) g[c] = 0;
    for (int a = 0; a < A; ++a) {
      long long gi = (long long)n * A_total + level_offset + local * A + a;
      int lab = labels[gi];
      float gz = 0.0f;
      if (lab >= 0) {
        float z = bf16_bits_to_f32(h[a]);
        float sp = softplus_neg_abs(z);
        float l = (z > 0.0f ? z : 0.0f) - z * (float)lab + sp;
        lc += l;
        gz = (sigmoidf_det(z) - (float)lab) * norm * loss_scale;
      }
      g[a] = f32_to_bf16_bits(gz);
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lab == 1) t = targets[gi];
      float tt[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float gd = 0.0f;
        if (lab == 1) {
          float d = bf16_bits_to_f32(h[A + 4 * a + k]) - tt[k];
          lr += mxdet_smooth_l1(d, sigma2);
          gd = mxdet_smooth_l1_grad(d, sigma2) * norm * loss_scale;
        }
        g[A + 4 * a + k] = f32_to_bf16_bits(gd);
      }
    }
  }
  store_block_partials<2>({lc, lr}, norm, red, partial);
}

// ---------------------------------------------------------------------------------------------
// (rcnn_softmax_ce / rcnn_reg_smooth_l1 / rcnn_reg_iou, the per-roi walks of the two kernels below, live in loss_elem.h:
// ohem.hip scores rows with the same code.)
// Box-head losses: one wave per roi. Elem: the regression element (SmoothL1Elem: reg_weight is 1, an exact factor;
// BalancedL1Elem).
template <class Elem>
__global__ void __launch_bounds__(256)
rcnn_loss_kernel(const void* __restrict__ cls, const void* __restrict__ reg, int dtype, int ld_cls,
                 int ld_reg, const int32_t* __restrict__ labels, const float* __restrict__ tgt,
                 const float* __restrict__ wgt, long long R, int num_classes, int reg_dim,
                 const Elem elem, float reg_weight, float norm, float loss_scale, void* __restrict__ gcls,
                 void* __restrict__ greg, float* __restrict__ partial) {
  long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r >= R) return;
  const int lane = lane_id();
  int lab = labels[r];
  const float lcls = rcnn_softmax_ce<true>(cls, dtype, ld_cls, r, lab, lane, num_classes, norm, loss_scale, gcls);
  const float lreg = reg_weight * rcnn_reg_elem<true>(reg, dtype, ld_reg, r, lab, lane, tgt, wgt, reg_dim, elem, norm, loss_scale, greg);
  if (lane == 0) {
    partial[2 * r + 0] = lcls * norm;
    partial[2 * r + 1] = lreg * norm;
  }
}

// the unfused primitive: one thread per box
__global__ void __launch_bounds__(256)
box_iou_loss_kernel(const float4* __restrict__ boxes, const float4* __restrict__ gt, const void* __restrict__ deltas,
                    int dtype, int ld, const float* __restrict__ weight, long long n, int kind, BoxStds sd,
                    float grad_scale, float* __restrict__ loss, void* __restrict__ grad) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float d[4], gd[4];
  load_deltas4(deltas, i * ld, dtype, d);
  const float w = weight ? weight[i] : 1.0f;
  const float L = box_iou_loss_elem(boxes[i], gt[i], d, sd, kind, gd);
  loss[i] = w * L;
#pragma unroll
  for (int k = 0; k < 4; ++k) store_from_f32(grad, i * ld + k, dtype, gd[k] * w * grad_scale);
}

// Box-head losses with an IoU-family regression term: one wave per roi, the softmax-CE half of rcnn_loss_kernel.
__global__ void __launch_bounds__(256)
rcnn_loss_iou_kernel(const void* __restrict__ cls, const void* __restrict__ reg, int dtype, int ld_cls, int ld_reg,
                     const int32_t* __restrict__ labels, const float* __restrict__ rois,
                     const int32_t* __restrict__ matched, const float* __restrict__ gt, int N, int G_max, long long R,
                     int num_classes, int reg_dim, int kind, BoxStds sd, float reg_weight, float norm, float loss_scale,
                     void* __restrict__ gcls, void* __restrict__ greg, float* __restrict__ partial) {
  long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r >= R) return;
  const int lane = lane_id();
  int lab = labels[r];
  const float lcls = rcnn_softmax_ce<true>(cls, dtype, ld_cls, r, lab, lane, num_classes, norm, loss_scale, gcls);
  const float lreg = rcnn_reg_iou<true>(reg, dtype, ld_reg, r, lab, lane, rois, matched, gt, N, G_max, num_classes, reg_dim, kind, sd,
                                        reg_weight, norm, loss_scale, greg);
  if (lane == 0) {
    partial[2 * r + 0] = lcls * norm;
    partial[2 * r + 1] = lreg * norm;
  }
}

// the unfused primitive: four lanes per row
__global__ void __launch_bounds__(256)
box_dist_loss_kernel(const float4* __restrict__ boxes, const float4* __restrict__ gt, const void* __restrict__ logits,
                     int dtype, int ld, long long n, int R, float stride, int kind, float reg_weight, float dfl_weight,
                     float grad_scale, float* __restrict__ loss_box, float* __restrict__ loss_dfl,
                     float* __restrict__ quality, void* __restrict__ grad) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long i = t >> 2;
  const int side = (int)(t & 3);
  if (i >= n) return;                                     // whole quads leave together
  float dfl, q;
  const float L = dist_box_quad(logits, i * ld + side * (R + 1), dtype, R, side, boxes[i], gt[i], stride, kind, reg_weight,
                                dfl_weight, grad_scale, grad, dfl, q);
  const int q0 = lane_id() & ~3;
  const float dsum = ((__shfl(dfl, q0 + 0) + __shfl(dfl, q0 + 1)) + __shfl(dfl, q0 + 2)) + __shfl(dfl, q0 + 3);
  if (side == 0) {
    loss_box[i] = reg_weight * L;
    loss_dfl[i] = dfl_weight * 0.25f * dsum;
    if (quality) quality[i] = q;
  }
}

}  // namespace mxdet

using namespace mxdet;

extern "C" int mxdet_smooth_l1_fwd(const float* pred, const float* target, const float* weight,
                                   int64_t n, float sigma, float* out, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(n >= 0 && sigma > 0.0f, MXDET_ESHAPE, "smooth_l1_fwd: bad arguments");
  if (n == 0) return MXDET_OK;
  MXDET_REQUIRE(pred && target && out, MXDET_EINVAL, "smooth_l1_fwd: null pointer");
  hipLaunchKernelGGL(smooth_l1_fwd_kernel, dim3((unsigned)ceil_div<int64_t>(n, 256)), dim3(256), 0,
                     as_stream(stream), pred, target, weight, (long long)n, sigma * sigma, out);
  return check_launch("smooth_l1_fwd");
}

extern "C" int mxdet_smooth_l1_bwd(const float* pred, const float* target, const float* weight,
                                   const float* grad_out, int64_t n, float sigma, int32_t accumulate,
                                   float* grad_pred, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(n >= 0 && sigma > 0.0f, MXDET_ESHAPE, "smooth_l1_bwd: bad arguments");
  if (n == 0) return MXDET_OK;
  MXDET_REQUIRE(pred && target && grad_pred, MXDET_EINVAL, "smooth_l1_bwd: null pointer");
  hipLaunchKernelGGL(smooth_l1_bwd_kernel, dim3((unsigned)ceil_div<int64_t>(n, 256)), dim3(256), 0,
                     as_stream(stream), pred, target, weight, grad_out, (long long)n, sigma * sigma,
                     accumulate, grad_pred);
  return check_launch("smooth_l1_bwd");
}

extern "C" size_t mxdet_loss_workspace_bytes(int64_t n) {
  size_t a = (size_t)(n > 0 ? n : 0) * 2 * sizeof(float);
  size_t b = 4096 * sizeof(float);
  return (a > b ? a : b) + 256;
}

// count the foreground rows, run cls_loss_kernel<Elem>, finalize: the two unfused class-loss entries after their checks
template <class Elem>
static int cls_loss_launch(const char* entry, const void* logits, int32_t dtype, const int32_t* labels, const float* quality,
                           int64_t n, int32_t C, const Elem elem, float grad_scale, float* loss_out, void* grad_logits,
                           void* workspace, hipStream_t s) {
  int* cnt = (int*)workspace;
  float* partial = (float*)((char*)workspace + 256);
  hipError_t e = zero_async(cnt, 256, s);
  MXDET_REQUIRE(e == hipSuccess, MXDET_EHIP, "%s: memset failed", entry);
  hipLaunchKernelGGL(count_fg_kernel, dim3((unsigned)ceil_div<int64_t>(n, 256)), dim3(256), 0, s, labels, (long long)n, cnt);
  long long total = (long long)n * C;
  int blocks = (int)(ceil_div<long long>(total, 256) < 2048 ? ceil_div<long long>(total, 256) : 2048);
  hipLaunchKernelGGL(cls_loss_kernel<Elem>, dim3(blocks), dim3(256), 0, s, logits, dtype, labels, quality, (long long)n, C, elem,
                     grad_scale, cnt, grad_logits, partial);
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, 1, loss_out);
  return check_launch(entry);
}

extern "C" int mxdet_focal_loss(const void* logits, int32_t dtype, const int32_t* labels, int64_t n,
                                int32_t C, float alpha, float gamma, float grad_scale,
                                float* loss_out, void* grad_logits, void* workspace,
                                size_t workspace_bytes, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(n > 0 && C > 0, MXDET_ESHAPE, "focal_loss: bad shape");
  MXDET_REQUIRE(dtype == MXDET_DTYPE_F32 || dtype == MXDET_DTYPE_BF16, MXDET_EINVAL, "focal_loss: dtype");
  MXDET_REQUIRE(logits && labels && loss_out && grad_logits, MXDET_EINVAL, "focal_loss: null pointer");
  MXDET_REQUIRE(workspace && workspace_bytes >= mxdet_loss_workspace_bytes(n), MXDET_EWORKSPACE,
                "focal_loss: workspace too small");
  return cls_loss_launch("focal_loss", logits, dtype, labels, nullptr, n, C, FocalElem{alpha, gamma}, grad_scale, loss_out,
                         grad_logits, workspace, as_stream(stream));
}

extern "C" int mxdet_quality_focal_loss(const void* logits, int32_t dtype, const int32_t* labels, const float* quality,
                                        int64_t n, int32_t C, int32_t cls_kind, float alpha, float gamma, float grad_scale,
                                        float* loss_out, void* grad_logits, void* workspace, size_t workspace_bytes,
                                        mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(n >= 0 && C > 0, MXDET_ESHAPE, "quality_focal_loss: bad shape");
  MXDET_REQUIRE(dtype == MXDET_DTYPE_F32 || dtype == MXDET_DTYPE_BF16, MXDET_EINVAL, "quality_focal_loss: dtype");
  MXDET_REQUIRE(cls_kind_ok(cls_kind), MXDET_EINVAL, "quality_focal_loss: cls_kind must be MXDET_CLS_LOSS_QFL or _VFL");
  MXDET_REQUIRE(gamma > 0.0f, MXDET_EINVAL, "quality_focal_loss: gamma must be positive");
  MXDET_REQUIRE(loss_out, MXDET_EINVAL, "quality_focal_loss: null pointer");
  hipStream_t s = as_stream(stream);
  if (n == 0) {                                             // nothing to read or write but the loss word
    hipError_t e0 = zero_async(loss_out, sizeof(float), s);
    MXDET_REQUIRE(e0 == hipSuccess, MXDET_EHIP, "quality_focal_loss: memset failed");
    return MXDET_OK;
  }
  MXDET_REQUIRE(logits && labels && quality && grad_logits, MXDET_EINVAL, "quality_focal_loss: null pointer");
  MXDET_REQUIRE(workspace && workspace_bytes >= mxdet_loss_workspace_bytes(n), MXDET_EWORKSPACE,
                "quality_focal_loss: workspace too small");
  return cls_loss_launch("quality_focal_loss", logits, dtype, labels, quality, n, C, QualityElem{cls_kind, alpha, gamma},
                         grad_scale, loss_out, grad_logits, workspace, s);
}

extern "C" int32_t mxdet_rpn_loss_num_partials(int32_t N, int32_t H, int32_t W) {
  long long cells = (long long)N * H * W;
  return (int32_t)((cells + 255) / 256);
}

extern "C" int mxdet_rpn_loss_level(const uint16_t* head, int32_t N, int32_t H, int32_t W, int32_t A,
                                    int32_t Cpad, const int32_t* labels, const float* bbox_targets,
                                    int64_t A_total, int64_t level_offset, float sigma, float norm,
                                    float loss_scale, uint16_t* grad_head, float* partial,
                                    mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(N > 0 && H > 0 && W > 0 && A > 0 && Cpad >= 5 * A, MXDET_ESHAPE,
                "rpn_loss_level: bad shape (Cpad must be >= 5*A)");
  MXDET_REQUIRE(head && labels && bbox_targets && grad_head && partial, MXDET_EINVAL,
                "rpn_loss_level: null pointer");
  MXDET_REQUIRE(level_offset >= 0 && level_offset + (int64_t)H * W * A <= A_total, MXDET_ESHAPE,
                "rpn_loss_level: level outside the anchor range");
  int blocks = mxdet_rpn_loss_num_partials(N, H, W);
  hipLaunchKernelGGL(rpn_loss_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), head, N, H, W, A,
                     Cpad, labels, (const float4*)bbox_targets, (long long)A_total,
                     (long long)level_offset, sigma * sigma, norm, loss_scale, grad_head, partial);
  return check_launch("rpn_loss_level");
}

extern "C" int mxdet_loss_finalize(const float* partial, int32_t count, int32_t ncomp, float* out,
                                   mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(count >= 0 && ncomp > 0 && ncomp <= 8, MXDET_ESHAPE, "loss_finalize: bad arguments");
  MXDET_REQUIRE(partial && out, MXDET_EINVAL, "loss_finalize: null pointer");
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, as_stream(stream), partial, count, ncomp,
                     out);
  return check_launch("loss_finalize");
}

// the shared checks and the two launches of mxdet_rcnn_loss / mxdet_rcnn_loss_balanced
template <class Elem>
static int rcnn_loss_launch(const char* entry, const void* cls_logits, const void* bbox_pred, int32_t dtype, int32_t ld_cls,
                            int32_t ld_reg, const int32_t* labels, const float* bbox_targets, const float* bbox_weights,
                            int64_t R, int32_t num_classes, int32_t reg_dim, const Elem elem, float reg_weight, float norm,
                            float loss_scale, float* loss_out, void* grad_cls, void* grad_reg, void* workspace,
                            size_t workspace_bytes, mxdet_stream_t stream) {
  MXDET_REQUIRE(R > 0 && num_classes > 0 && reg_dim > 0 && ld_cls >= num_classes && ld_reg >= reg_dim,
                MXDET_ESHAPE, "%s: bad shape", entry);
  MXDET_REQUIRE(dtype == MXDET_DTYPE_F32 || dtype == MXDET_DTYPE_BF16, MXDET_EINVAL, "%s: dtype", entry);
  MXDET_REQUIRE(cls_logits && bbox_pred && labels && bbox_targets && bbox_weights && loss_out &&
                    grad_cls && grad_reg,
                MXDET_EINVAL, "%s: null pointer", entry);
  MXDET_REQUIRE(workspace && workspace_bytes >= mxdet_loss_workspace_bytes(R), MXDET_EWORKSPACE,
                "%s: workspace too small", entry);
  float* partial = (float*)((char*)workspace + 256);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(rcnn_loss_kernel<Elem>, dim3((unsigned)ceil_div<int64_t>(R, 4)), dim3(256), 0, s,
                     cls_logits, bbox_pred, dtype, ld_cls, ld_reg, labels, bbox_targets, bbox_weights,
                     (long long)R, num_classes, reg_dim, elem, reg_weight, norm, loss_scale, grad_cls,
                     grad_reg, partial);
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, s, partial, (int)R, 2, loss_out);
  return check_launch(entry);
}

extern "C" int mxdet_rcnn_loss(const void* cls_logits, const void* bbox_pred, int32_t dtype,
                               int32_t ld_cls, int32_t ld_reg, const int32_t* labels,
                               const float* bbox_targets, const float* bbox_weights, int64_t R,
                               int32_t num_classes, int32_t reg_dim, float sigma, float norm,
                               float loss_scale, float* loss_out, void* grad_cls, void* grad_reg,
                               void* workspace, size_t workspace_bytes, mxdet_stream_t stream) {
  clear_error();
  return rcnn_loss_launch("rcnn_loss", cls_logits, bbox_pred, dtype, ld_cls, ld_reg, labels, bbox_targets, bbox_weights, R,
                          num_classes, reg_dim, SmoothL1Elem{sigma * sigma}, 1.0f, norm, loss_scale, loss_out, grad_cls,
                          grad_reg, workspace, workspace_bytes, stream);
}

extern "C" int mxdet_rcnn_loss_balanced(const void* cls_logits, const void* bbox_pred, int32_t dtype, int32_t ld_cls,
                                        int32_t ld_reg, const int32_t* labels, const float* bbox_targets,
                                        const float* bbox_weights, int64_t R, int32_t num_classes, int32_t reg_dim,
                                        float alpha, float gamma, float beta, float b, float reg_weight, float norm,
                                        float loss_scale, float* loss_out, void* grad_cls, void* grad_reg, void* workspace,
                                        size_t workspace_bytes, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(alpha > 0.0f && gamma > 0.0f && beta > 0.0f && b > 0.0f && reg_weight > 0.0f, MXDET_EINVAL,
                "rcnn_loss_balanced: alpha, gamma, beta, b and reg_weight must be positive");
  return rcnn_loss_launch("rcnn_loss_balanced", cls_logits, bbox_pred, dtype, ld_cls, ld_reg, labels, bbox_targets,
                          bbox_weights, R, num_classes, reg_dim, BalancedL1Elem{alpha, gamma, beta, b, reg_weight}, reg_weight,
                          norm, loss_scale, loss_out, grad_cls, grad_reg, workspace, workspace_bytes, stream);
}

extern "C" int mxdet_box_iou_loss(const float* boxes, const float* gt, const void* deltas, int32_t dtype, int32_t ld,
                                  const float* weight, int64_t n, int32_t kind, float std_x, float std_y, float std_w,
                                  float std_h, float grad_scale, float* loss, void* grad_deltas, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(n >= 0 && ld >= 4, MXDET_ESHAPE, "box_iou_loss: bad shape (ld must be >= 4)");
  MXDET_REQUIRE(dtype == MXDET_DTYPE_F32 || dtype == MXDET_DTYPE_BF16, MXDET_EINVAL, "box_iou_loss: dtype");
  MXDET_REQUIRE(iou_kind_ok(kind), MXDET_EINVAL, "box_iou_loss: kind must be MXDET_IOU_LOSS_IOU, _GIOU or _DIOU");
  MXDET_REQUIRE(stds_ok(std_x, std_y, std_w, std_h), MXDET_EINVAL, "box_iou_loss: stds must be positive");
  if (n == 0) return MXDET_OK;
  MXDET_REQUIRE(boxes && gt && deltas && loss && grad_deltas, MXDET_EINVAL, "box_iou_loss: null pointer");
  MXDET_REQUIRE((((uintptr_t)boxes | (uintptr_t)gt) % 16) == 0, MXDET_EINVAL,
                "box_iou_loss: boxes and gt must be 16-byte aligned");
  const BoxStds sd = {std_x, std_y, std_w, std_h};
  hipLaunchKernelGGL(box_iou_loss_kernel, dim3((unsigned)ceil_div<int64_t>(n, 256)), dim3(256), 0, as_stream(stream),
                     (const float4*)boxes, (const float4*)gt, deltas, dtype, ld, weight, (long long)n, kind, sd, grad_scale,
                     loss, grad_deltas);
  return check_launch("box_iou_loss");
}

extern "C" int mxdet_rcnn_loss_iou(const void* cls_logits, const void* bbox_pred, int32_t dtype, int32_t ld_cls,
                                   int32_t ld_reg, const int32_t* labels, const float* rois, const int32_t* matched_gt,
                                   const float* gt_boxes, int32_t N, int32_t G_max, int64_t R, int32_t num_classes,
                                   int32_t reg_dim, int32_t kind, float std_x, float std_y, float std_w, float std_h,
                                   float reg_weight, float norm, float loss_scale, float* loss_out, void* grad_cls,
                                   void* grad_reg, void* workspace, size_t workspace_bytes, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(R > 0 && num_classes > 0 && reg_dim == 4 * num_classes && ld_cls >= num_classes && ld_reg >= reg_dim &&
                    N > 0 && G_max > 0,
                MXDET_ESHAPE, "rcnn_loss_iou: bad shape (reg_dim must be 4 * num_classes)");
  MXDET_REQUIRE(dtype == MXDET_DTYPE_F32 || dtype == MXDET_DTYPE_BF16, MXDET_EINVAL, "rcnn_loss_iou: dtype");
  MXDET_REQUIRE(iou_kind_ok(kind), MXDET_EINVAL, "rcnn_loss_iou: kind must be MXDET_IOU_LOSS_IOU, _GIOU or _DIOU");
  MXDET_REQUIRE(stds_ok(std_x, std_y, std_w, std_h) && reg_weight > 0.0f, MXDET_EINVAL,
                "rcnn_loss_iou: stds and reg_weight must be positive");
  MXDET_REQUIRE(cls_logits && bbox_pred && labels && rois && matched_gt && gt_boxes && loss_out && grad_cls && grad_reg,
                MXDET_EINVAL, "rcnn_loss_iou: null pointer");
  MXDET_REQUIRE(workspace && workspace_bytes >= mxdet_loss_workspace_bytes(R), MXDET_EWORKSPACE,
                "rcnn_loss_iou: workspace too small");
  float* partial = (float*)((char*)workspace + 256);
  hipStream_t s = as_stream(stream);
  const BoxStds sd = {std_x, std_y, std_w, std_h};
  hipLaunchKernelGGL(rcnn_loss_iou_kernel, dim3((unsigned)ceil_div<int64_t>(R, 4)), dim3(256), 0, s, cls_logits, bbox_pred,
                     dtype, ld_cls, ld_reg, labels, rois, matched_gt, gt_boxes, N, G_max, (long long)R, num_classes, reg_dim,
                     kind, sd, reg_weight, norm, loss_scale, grad_cls, grad_reg, partial);
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, s, partial, (int)R, 2, loss_out);
  return check_launch("rcnn_loss_iou");
}

extern "C" int mxdet_box_dist_loss(const float* boxes, const float* gt, const void* logits, int32_t dtype, int32_t ld,
                                   int64_t n, int32_t reg_max, float stride, int32_t kind, float reg_weight,
                                   float dfl_weight, float grad_scale, float* loss_box, float* loss_dfl, float* quality,
                                   void* grad_logits, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(reg_max >= 1 && reg_max <= MXDET_REG_MAX_LIMIT, MXDET_EINVAL, "box_dist_loss: reg_max %d not in 1..%d", reg_max,
                MXDET_REG_MAX_LIMIT);
  MXDET_REQUIRE(n >= 0 && n <= (int64_t)1 << 28 && ld >= 4 * (reg_max + 1), MXDET_ESHAPE,
                "box_dist_loss: bad shape (ld must be >= 4 * (reg_max + 1))");
  MXDET_REQUIRE(dtype == MXDET_DTYPE_F32 || dtype == MXDET_DTYPE_BF16, MXDET_EINVAL, "box_dist_loss: dtype");
  MXDET_REQUIRE(iou_kind_ok(kind), MXDET_EINVAL, "box_dist_loss: kind must be MXDET_IOU_LOSS_IOU, _GIOU or _DIOU");
  MXDET_REQUIRE(stride > 0.0f && reg_weight > 0.0f && dfl_weight > 0.0f, MXDET_EINVAL,
                "box_dist_loss: stride, reg_weight and dfl_weight must be positive");
  if (n == 0) return MXDET_OK;
  MXDET_REQUIRE(boxes && gt && logits && loss_box && loss_dfl && grad_logits, MXDET_EINVAL, "box_dist_loss: null pointer");
  MXDET_REQUIRE((((uintptr_t)boxes | (uintptr_t)gt) % 16) == 0, MXDET_EINVAL,
                "box_dist_loss: boxes and gt must be 16-byte aligned");
  hipLaunchKernelGGL(box_dist_loss_kernel, dim3((unsigned)ceil_div<int64_t>(4 * n, 256)), dim3(256), 0, as_stream(stream),
                     (const float4*)boxes, (const float4*)gt, logits, dtype, ld, (long long)n, reg_max, stride, kind,
                     reg_weight, dfl_weight, grad_scale, loss_box, loss_dfl, quality, grad_logits);
  return check_launch("box_dist_loss");
}
