// mask_iou.hip -- Mask Scoring R-CNN (Huang et al., CVPR 2019) operators for gfx950: the MaskIoU regression target, the
// MaskIoU head's input (mask RoI features + the 2x2 max-pooled mask probability), the adjoint of that concatenation, the
// L2 MaskIoU loss and the test-time mask rescoring.
//
// Slots: core/mask (/root/reference/README.md:18) and models/mask_heads (README.md:30). The head's convolutions and FCs run
// on the MFMA kernels of conv.hip / wgrad.hip; this file holds what nothing there provides. Compiled without FMA
// contraction: every product, quotient and sum below is one IEEE operation in the order written, so the
// numpy-float32 restatement of tests/_mask_iou_ref.py is bit-identical.
#include "common.h"

namespace mxdet {

constexpr int kAreaChunks = 16;   // workgroups per instance of the whole-instance area pass (partials, summed in order)

__device__ __forceinline__ int nonzero_bytes(unsigned w) {
  // one bit per non-zero byte: (b | b>>1 | ... ) folded into bit 0 of each byte
  w |= w >> 4; w |= w >> 2; w |= w >> 1;
  return __popc(w & 0x01010101u);
}

// Non-zero bytes of p[0, n), walked by `nthr` cooperating threads of which this one is `tid`: scalar bytes up to the
// first 16-byte boundary, 16-byte loads over the aligned body, scalar bytes behind it. Returns this thread's share.
__device__ __forceinline__ int count_span(const uint8_t* __restrict__ p, long long n, int tid, int nthr) {
  int cnt = 0;
  long long head = (long long)((16u - (unsigned)((unsigned long long)p & 15u)) & 15u);
  if (head > n) head = n;
  for (long long i = tid; i < head; i += nthr) cnt += p[i] != 0;
  const long long body = (n - head) >> 4;
  const uint4* q = (const uint4*)(p + head);
  for (long long i = tid; i < body; i += nthr) {
    const uint4 v = q[i];
    cnt += nonzero_bytes(v.x) + nonzero_bytes(v.y) + nonzero_bytes(v.z) + nonzero_bytes(v.w);
  }
  const long long done = head + (body << 4);
  for (long long i = done + tid; i < n; i += nthr) cnt += p[i] != 0;
  return cnt;
}

// ---- whole-instance areas: partial[(n*G+g)*kAreaChunks + chunk] = set pixels of that chunk of gt_masks[n,g] --------------
// Padding instances (gt_boxes class < 0) are not read: their partials are zero.
__global__ void __launch_bounds__(256)
maskiou_area_kernel(const uint8_t* __restrict__ gt_masks, const float* __restrict__ gt_boxes, int G, int G_boxes,
                    long long HW, int* __restrict__ partial) {
  __shared__ int red[4];
  const int inst = blockIdx.y, chunk = blockIdx.x;
  int total = 0;
  const int n = inst / G, g = inst - n * G;
  if (gt_boxes[((long long)n * G_boxes + g) * 5 + 4] >= 0.0f) {   // block-uniform
    // chunk bounds on 16-byte multiples of the instance's own offset range: [lo, hi) of HW bytes
    const long long per = ((HW + kAreaChunks - 1) / kAreaChunks + 15) & ~15ll;
    const long long lo = (long long)chunk * per;
    const long long hi = lo + per < HW ? lo + per : HW;
    int cnt = 0;
    if (lo < hi) cnt = count_span(gt_masks + (long long)inst * HW + lo, hi - lo, threadIdx.x, 256);
    total = block4_reduce<Sum, kLane0, kScratchReused>(cnt, red);
  }
  if (threadIdx.x == 0) partial[inst * kAreaChunks + chunk] = total;
}

// ---- per-roi counts and the target: one workgroup per roi ---------------------------------------------------------------
__global__ void __launch_bounds__(256)
maskiou_target_kernel(const float* __restrict__ rois, const int32_t* __restrict__ matched_gt,
                      const int32_t* __restrict__ cls, const uint8_t* __restrict__ gt_masks,
                      const uint16_t* __restrict__ logits, const uint8_t* __restrict__ targets,
                      const int* __restrict__ partial, int N, int G, int H, int W, int SS, int Cpad,
                      float* __restrict__ out) {
  __shared__ int red[4];
  const int r = blockIdx.x;
  const float* q = rois + (long long)r * 5;
  const int c = cls[r], g = matched_gt[r];
  const int n = (int)q[0];
  // rows that read no mask memory (block-uniform): not foreground, unmatched, or indices outside the tensors
  if (c <= 0 || c > Cpad || g < 0 || g >= G || n < 0 || n >= N) {
    if (threadIdx.x == 0) out[r] = 0.0f;
    return;
  }
  const long long inst = (long long)n * G + g;
  // the box in pixels, clipped to the frame (the float clamps keep the casts in range for any input)
  const int ix1 = (int)fminf(fmaxf(floorf(q[1]), 0.0f), (float)W);
  const int iy1 = (int)fminf(fmaxf(floorf(q[2]), 0.0f), (float)H);
  const int ix2 = (int)fmaxf(fminf(ceilf(q[3]), (float)(W - 1)), -1.0f);
  const int iy2 = (int)fmaxf(fminf(ceilf(q[4]), (float)(H - 1)), -1.0f);
  int cnt_in = 0;
  if (ix1 <= ix2 && iy1 <= iy2) {
    const uint8_t* m = gt_masks + inst * H * W;
    // sixteen lanes per row of the box, sixteen rows in flight: a typical row is a few hundred bytes (a dozen 16-byte
    // loads), and a whole wave per row left the pass bound by the latency of ~rows/4 dependent round trips (120 us
    // for 12 MB at the benchmark shape)
    const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
    for (int y = iy1 + grp; y <= iy2; y += 16)
      cnt_in += count_span(m + (long long)y * W + ix1, (long long)(ix2 - ix1 + 1), gl, 16);
  }
  int cnt_pred = 0, cnt_tgt = 0, cnt_ovr = 0;
  const uint16_t* lg = logits + (long long)r * SS * Cpad + (c - 1);
  const uint8_t* tg = targets + (long long)r * SS;
  for (int i = threadIdx.x; i < SS; i += 256) {
    const int p = bf16_bits_to_f32(lg[(long long)i * Cpad]) > 0.0f;
    const int t = tg[i] != 0;
    cnt_pred += p; cnt_tgt += t; cnt_ovr += p & t;
  }
  const int a_in = block4_reduce<Sum, kLane0, kScratchReused>(cnt_in, red);
  const int a_pred = block4_reduce<Sum, kLane0, kScratchReused>(cnt_pred, red);
  const int a_tgt = block4_reduce<Sum, kLane0, kScratchReused>(cnt_tgt, red);
  const int a_ovr = block4_reduce<Sum, kLane0, kScratchReused>(cnt_ovr, red);
  if (threadIdx.x == 0) {
    int a_full = 0;
    for (int k = 0; k < kAreaChunks; ++k) a_full += partial[inst * kAreaChunks + k];
    float t = 0.0f;
    if (a_in > 0) {
      const float gt_s = ((float)a_tgt * (float)a_full) / (float)a_in;
      const float uni = ((float)a_pred + gt_s) - (float)a_ovr;
      t = (float)a_ovr / fmaxf(uni, 1e-7f);
    }
    out[r] = t;
  }
}

// ---- head input: [R,h,h,Ct] = mpooled channels | sigmoid(max of the 2x2 logits of the class channel) | zeros -------------
// one lane = one 16-byte chunk (8 channels) of the output
__global__ void __launch_bounds__(256)
maskiou_input_kernel(const uint4* __restrict__ mpooled, const uint16_t* __restrict__ logits,
                     const int32_t* __restrict__ cls, long long total, int h, int C8, int Ct8, int Cpad,
                     uint4* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % Ct8);
  const long long pix = idx / Ct8;   // (r*h + y)*h + x
  uint4 o = make_uint4(0u, 0u, 0u, 0u);
  if (k < C8) {
    o = mpooled[pix * C8 + k];
  } else if (k == C8) {
    const int x = (int)(pix % h);
    const long long t = pix / h;
    const int y = (int)(t % h);
    const int r = (int)(t / h);
    const int c = cls[r];
    if (c > 0 && c <= Cpad) {
      const int S = 2 * h;
      const uint16_t* lg = logits + (((long long)r * S + 2 * y) * S + 2 * x) * Cpad + (c - 1);
      const float z00 = bf16_bits_to_f32(lg[0]), z01 = bf16_bits_to_f32(lg[Cpad]);
      const float z10 = bf16_bits_to_f32(lg[(long long)S * Cpad]), z11 = bf16_bits_to_f32(lg[(long long)S * Cpad + Cpad]);
      const float z = fmaxf(fmaxf(z00, z01), fmaxf(z10, z11));
      const float p = z >= 0.0f ? 1.0f / (1.0f + mxdet_expf(-z)) : mxdet_expf(z) / (1.0f + mxdet_expf(z));
      o.x = (unsigned)f32_to_bf16_bits(p);
    }
  }
  out[idx] = o;
}

// ---- adjoint of the concatenation: d_mpooled[., c] = bf16(d_mpooled + d_in[., c]) for c < C --------------------------------
__global__ void __launch_bounds__(256)
maskiou_input_bwd_kernel(const uint4* __restrict__ d_in, long long total, int C8, int Ct8, uint4* __restrict__ d_mpooled) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % C8);
  const long long pix = idx / C8;
  float a[8], b[8];
  unpack8_bf16(d_mpooled[idx], a);
  unpack8_bf16(d_in[pix * Ct8 + k], b);
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = a[j] + b[j];
  d_mpooled[idx] = pack8_bf16_exact(a);
}

// ---- L2 loss on the class column, forward + gradient: one workgroup, fixed-order sum ----------------------------------
__global__ void __launch_bounds__(256)
maskiou_loss_kernel(const uint16_t* __restrict__ pred, const int32_t* __restrict__ cls, const float* __restrict__ tgt, int R,
                    int ld, float scale, float* __restrict__ loss_out, uint16_t* __restrict__ grad) {
  __shared__ int red[4];
  __shared__ float redf[4];
  int np = 0;
  for (int r = threadIdx.x; r < R; r += 256) {
    const int c = cls[r];
    np += (c > 0 && c <= ld && tgt[r] > 0.0f);
  }
  const int n_pos = block4_reduce<Sum, kLane0, kScratchReused>(np, red);
  const float k = scale / (float)(n_pos > 1 ? n_pos : 1);
  float l = 0.0f;
  for (int r = threadIdx.x; r < R; r += 256) {   // rows in ascending order per lane
    const int c = cls[r];
    const float t = tgt[r];
    if (c > 0 && c <= ld && t > 0.0f) {
      const float d = bf16_bits_to_f32(pred[(long long)r * ld + (c - 1)]) - t;
      l += 0.5f * (d * d);
    }
  }
  l = block4_reduce<Sum, kLane0, kScratchOnce>(l, redf);
  if (threadIdx.x == 0) loss_out[0] = k * l;
  // the gradient, written completely: consecutive lanes on consecutive 16-byte chunks
  const int CH = ld >> 3;
  for (int it = threadIdx.x; it < R * CH; it += 256) {
    const int r = it / CH, ck = it - r * CH;
    const int c = cls[r];
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    if (c > 0 && c <= ld && ((c - 1) >> 3) == ck) {
      const float t = tgt[r];
      if (t > 0.0f) {
        const float p = bf16_bits_to_f32(pred[(long long)r * ld + (c - 1)]);
        const unsigned gb = (unsigned)f32_to_bf16_bits((p - t) * k) << (16 * ((c - 1) & 1));
        const int w = ((c - 1) & 7) >> 1;
        o.x = w == 0 ? gb : 0u; o.y = w == 1 ? gb : 0u; o.z = w == 2 ? gb : 0u; o.w = w == 3 ? gb : 0u;
      }
    }
    *(uint4*)(grad + (long long)it * 8) = o;
  }
}

// ---- test time: mask score = detection score * predicted IoU of the detection's class ------------------------------------
__global__ void maskiou_score_kernel(const float* __restrict__ dets, const uint16_t* __restrict__ pred, int R, int ld,
                                     float* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int c = (int)dets[(long long)r * 6 + 5];
  float s = 0.0f;
  if (c > 0 && c <= ld) s = dets[(long long)r * 6 + 4] * bf16_bits_to_f32(pred[(long long)r * ld + (c - 1)]);
  out[r] = s;
}

}  // namespace mxdet

using namespace mxdet;

extern "C" size_t mxdet_maskiou_target_workspace_bytes(int32_t N, int32_t G) {
  return (size_t)(N > 0 ? N : 0) * (size_t)(G > 0 ? G : 0) * kAreaChunks * sizeof(int) + 256;
}

extern "C" int mxdet_maskiou_target(const float* rois, const int32_t* matched_gt, const int32_t* cls,
                                    const float* gt_boxes, const uint8_t* gt_masks, const uint16_t* logits,
                                    const uint8_t* targets, int64_t R, int32_t N, int32_t G, int32_t G_boxes, int32_t H,
                                    int32_t W, int32_t S, int32_t Cpad, float* out, void* workspace, size_t workspace_bytes,
                                    mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(R >= 0 && N > 0 && G > 0 && G_boxes >= G && H > 0 && W > 0 && S > 0 && Cpad > 0, MXDET_ESHAPE,
                "maskiou_target: bad shape (G_boxes >= G)");
  MXDET_REQUIRE((long long)N * G <= 65535, MXDET_ESHAPE, "maskiou_target: N*G = %lld exceeds the grid", (long long)N * G);
  if (R == 0) return MXDET_OK;
  MXDET_REQUIRE(rois && matched_gt && cls && gt_boxes && gt_masks && logits && targets && out, MXDET_EINVAL,
                "maskiou_target: null pointer");
  MXDET_REQUIRE(workspace && workspace_bytes >= mxdet_maskiou_target_workspace_bytes(N, G), MXDET_EWORKSPACE,
                "maskiou_target: workspace too small");
  hipStream_t s = as_stream(stream);
  int* partial = (int*)workspace;
  hipLaunchKernelGGL(maskiou_area_kernel, dim3(kAreaChunks, (unsigned)(N * G)), dim3(256), 0, s, gt_masks, gt_boxes,
                     G, G_boxes, (long long)H * W, partial);
  hipLaunchKernelGGL(maskiou_target_kernel, dim3((unsigned)R), dim3(256), 0, s, rois, matched_gt, cls, gt_masks, logits,
                     targets, (const int*)partial, N, G, H, W, S * S, Cpad, out);
  return check_launch("maskiou_target");
}

extern "C" int mxdet_maskiou_input(const uint16_t* mpooled, const uint16_t* logits, const int32_t* cls, int64_t R,
                                   int32_t S, int32_t C, int32_t Cpad, int32_t Ctot, uint16_t* out,
                                   mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(R >= 0 && S > 0 && S % 2 == 0 && C > 0 && C % 8 == 0 && Cpad > 0 && Ctot % 8 == 0 && Ctot > C, MXDET_ESHAPE,
                "maskiou_input: bad shape (S even, C %% 8, Ctot %% 8, Ctot > C)");
  if (R == 0) return MXDET_OK;
  MXDET_REQUIRE(mpooled && logits && cls && out, MXDET_EINVAL, "maskiou_input: null pointer");
  const int h = S / 2;
  const long long total = (long long)R * h * h * (Ctot / 8);
  MXDET_REQUIRE(total < (1ll << 31) * 256, MXDET_ESHAPE, "maskiou_input: tensor exceeds the grid");
  hipLaunchKernelGGL(maskiou_input_kernel, dim3((unsigned)ceil_div<long long>(total, 256)), dim3(256), 0, as_stream(stream),
                     (const uint4*)mpooled, logits, cls, total, h, C / 8, Ctot / 8, Cpad, (uint4*)out);
  return check_launch("maskiou_input");
}

extern "C" int mxdet_maskiou_input_bwd(const uint16_t* d_in, int64_t pixels, int32_t C, int32_t Ctot, uint16_t* d_mpooled,
                                       mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(pixels >= 0 && C > 0 && C % 8 == 0 && Ctot % 8 == 0 && Ctot >= C, MXDET_ESHAPE,
                "maskiou_input_bwd: bad shape (C %% 8, Ctot %% 8, Ctot >= C)");
  if (pixels == 0) return MXDET_OK;
  MXDET_REQUIRE(d_in && d_mpooled, MXDET_EINVAL, "maskiou_input_bwd: null pointer");
  const long long total = (long long)pixels * (C / 8);
  MXDET_REQUIRE(total < (1ll << 31) * 256, MXDET_ESHAPE, "maskiou_input_bwd: tensor exceeds the grid");
  hipLaunchKernelGGL(maskiou_input_bwd_kernel, dim3((unsigned)ceil_div<long long>(total, 256)), dim3(256), 0,
                     as_stream(stream), (const uint4*)d_in, total, C / 8, Ctot / 8, (uint4*)d_mpooled);
  return check_launch("maskiou_input_bwd");
}

extern "C" int mxdet_maskiou_loss(const uint16_t* pred, const int32_t* cls, const float* targets, int64_t R, int32_t ld,
                                  float loss_scale, float weight, float* loss_out, uint16_t* grad,
                                  mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(R > 0 && R <= (1 << 20) && ld > 0 && ld <= 4096 && ld % 8 == 0, MXDET_ESHAPE,
                "maskiou_loss: bad shape (ld %% 8, ld <= 4096, R <= 2^20)");
  MXDET_REQUIRE(pred && cls && targets && loss_out && grad, MXDET_EINVAL, "maskiou_loss: null pointer");
  hipLaunchKernelGGL(maskiou_loss_kernel, dim3(1), dim3(256), 0, as_stream(stream), pred, cls, targets, (int)R, ld,
                     loss_scale * weight, loss_out, grad);
  return check_launch("maskiou_loss");
}

extern "C" int mxdet_maskiou_score(const float* dets, const uint16_t* pred, int64_t R, int32_t ld, float* scores,
                                   mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(R >= 0 && R < (1ll << 31) && ld > 0, MXDET_ESHAPE, "maskiou_score: bad shape");
  if (R == 0) return MXDET_OK;
  MXDET_REQUIRE(dets && pred && scores, MXDET_EINVAL, "maskiou_score: null pointer");
  hipLaunchKernelGGL(maskiou_score_kernel, dim3((unsigned)ceil_div<long long>(R, 256)), dim3(256), 0, as_stream(stream),
                     dets, pred, (int)R, ld, scores);
  return check_launch("maskiou_score");
}
