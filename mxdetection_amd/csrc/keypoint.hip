// keypoint.hip -- Keypoint R-CNN (He et al., Mask R-CNN, ICCV 2017, section 5) operators for gfx950: the one-hot heatmap
// target, the spatial-softmax cross-entropy over the x2 bilinearly upsampled heatmap with its gradient, and the test-time
// argmax decode.
//
// Slots: core/mask (/root/reference/README.md:18) and models/mask_heads (README.md:30). The head's convolutions run on the
// MFMA kernels of conv.hip / wgrad.hip; this file holds what nothing there provides. The 2S_in x 2S_in map the loss and
// the decode see is never stored in HBM: a workgroup stages its roi's [S_in,S_in,Kpad] logits in LDS (channel-major) and
// forms the upsampled values from there. Compiled without FMA contraction: every product, quotient and sum below is one
// IEEE operation in the order written, so target and decode match the numpy-float32 restatement of
// tests/_keypoint_ref.py bit for bit.
#include "common.h"

namespace mxdet {

constexpr int kKpLossThreads = 1024;    // loss workgroup: 16 waves (4 per SIMD), all on one channel at a time, one thread
                                        // per input pixel: S_in <= 32
constexpr int kKpDecodeThreads = 1024;  // decode workgroup: 16 waves, one channel per wave at a time
constexpr size_t kKpLdsLimit = 64 * 1024;

__host__ __device__ inline int kp_pad4(int k) { return (k + 3) & ~3; }

// bytes of dynamic LDS of the loss kernel: q [S*S] f32 | red [32] f32 | tg [pad4(K)] i32 | lse [2][pad4(K)] f32 | sh [K * S_in^2] u16
static inline size_t kp_loss_lds(int S_in, int K) {
  const size_t P = (size_t)S_in * S_in;
  return 4 * P * 4 + 32 * 4 + (size_t)kp_pad4(K) * 12 + (((size_t)K * P * 2 + 15) & ~(size_t)15);
}
static inline size_t kp_decode_lds(int S_in, int K) { return (((size_t)K * S_in * S_in * 2 + 15) & ~(size_t)15); }

__device__ __forceinline__ int kp_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Stage one roi's [P,Kpad] bf16 block (channels last, 16-byte chunks on consecutive lanes) into LDS as sh[c*P + pix] for
// the channels c < K. Chunks that hold padding channels only are not read.
__device__ __forceinline__ void kp_stage(const uint16_t* __restrict__ blk, int P, int Kpad, int K, uint16_t* sh, int tid,
                                         int nthr) {
  const int CH = Kpad >> 3;
  const float rcp = 1.0f / (float)CH;
  const uint4* src = (const uint4*)blk;
  for (int i = tid; i < P * CH; i += nthr) {
    int ck;
    const int pix = fast_divmod(i, CH, rcp, &ck);
    if (ck * 8 >= K) continue;
    const uint4 v = src[i];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = ck * 8 + j;
      if (c < K) sh[c * P + pix] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
    }
  }
}

// Value (Y, X) of the x2 upsampled map of one channel ch[S_in*S_in]: half-pixel centres, edge replication, horizontal
// first: h = 0.75f*in[j] + 0.25f*in[clamp(j-1+2p)] at X = 2j+p, then the same vertically on h.
__device__ __forceinline__ float kp_up(const uint16_t* ch, int S_in, int Y, int X) {
  const int j = X >> 1, jn = kp_clamp(j - 1 + 2 * (X & 1), S_in - 1);
  const int i = Y >> 1, in = kp_clamp(i - 1 + 2 * (Y & 1), S_in - 1);
  const float a = 0.75f * bf16_bits_to_f32(ch[i * S_in + j]) + 0.25f * bf16_bits_to_f32(ch[i * S_in + jn]);
  const float b = 0.75f * bf16_bits_to_f32(ch[in * S_in + j]) + 0.25f * bf16_bits_to_f32(ch[in * S_in + jn]);
  return 0.75f * a + 0.25f * b;
}

// block-wide max / fixed-order sum over the loss workgroup's 16 waves (red: 16 floats, 16-byte aligned, read back as four
// 16-byte loads); every thread gets the result. Contain __syncthreads.
__device__ __forceinline__ float kp_block_max(float v, float* red) {
  v = wave_reduce<FMax>(v);
  __syncthreads();   // protect reuse of red
  if (lane_id() == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float4 a = ((const float4*)red)[0], b = ((const float4*)red)[1], c = ((const float4*)red)[2], d = ((const float4*)red)[3];
  return fmaxf(fmaxf(fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)), fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w))),
               fmaxf(fmaxf(fmaxf(c.x, c.y), fmaxf(c.z, c.w)), fmaxf(fmaxf(d.x, d.y), fmaxf(d.z, d.w))));
}
__device__ __forceinline__ float kp_block_sum(float v, float* red) {
  v = wave_sum_lane0(v);
  __syncthreads();
  if (lane_id() == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float4 a = ((const float4*)red)[0], b = ((const float4*)red)[1], c = ((const float4*)red)[2], d = ((const float4*)red)[3];
  return ((((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w))) + (((c.x + c.y) + (c.z + c.w)) + ((d.x + d.y) + (d.z + d.w))));
}

// ---- target: one thread per (roi, keypoint) -------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
keypoint_target_kernel(const float* __restrict__ rois, const int32_t* __restrict__ matched_gt,
                       const int32_t* __restrict__ labels, const float* __restrict__ gt_kp, long long total, int N, int G,
                       int K, int S, int32_t* __restrict__ targets) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long long r = idx / K;
  const int j = (int)(idx - r * K);
  const float* q = rois + r * 5;
  const int g = matched_gt[r];
  const float nf = q[0];
  int t = -1;
  // rows that read no keypoint memory: not foreground, unmatched, or indices outside the tensors
  if (labels[r] > 0 && g >= 0 && g < G && nf > -1.0f && nf < (float)N) {
    const int n = (int)nf;
    const float* kp = gt_kp + (((long long)n * G + g) * K + j) * 3;
    const float kx = kp[0], ky = kp[1], v = kp[2];
    if (v > 0.0f) {
      const float x1 = q[1], y1 = q[2], x2 = q[3], y2 = q[4];
      const float rw = fmaxf(x2 - x1, 1.0f), rh = fmaxf(y2 - y1, 1.0f);
      const float fx = (kx == x2) ? (float)(S - 1) : floorf((kx - x1) * ((float)S / rw));
      const float fy = (ky == y2) ? (float)(S - 1) : floorf((ky - y1) * ((float)S / rh));
      // the range test in float keeps the casts in range for any input (NaN fails every comparison)
      if (fx >= 0.0f && fx < (float)S && fy >= 0.0f && fy < (float)S) t = (int)fy * S + (int)fx;
    }
  }
  targets[idx] = t;
}

// ---- n_valid = #{targets in [0, SS)}: one workgroup, integer count -------------------------------------------------------
__global__ void __launch_bounds__(256)
keypoint_count_kernel(const int32_t* __restrict__ targets, long long total, int SS, int* __restrict__ n_valid) {
  __shared__ int red[4];
  int cnt = 0;
  for (long long i = threadIdx.x; i < total; i += 256) {
    const int t = targets[i];
    cnt += (t >= 0 && t < SS);
  }
  cnt = block4_reduce<Sum, kLane0, kScratchOnce>(cnt, red);
  if (threadIdx.x == 0) n_valid[0] = cnt;
}

// ---- loss + gradient: one workgroup per roi -------------------------------------------------------------------------------
// The roi's block is read once into LDS; the valid channels are processed one after the other by the whole workgroup, one
// thread per INPUT pixel: its 2x2 upsampled values from the clamped 3x3 neighbourhood, in registers -> max -> e = exp(u - max)
// -> sum -> q = (e / sum - onehot) * k into LDS -> the adjoint of the upsample in gather form for the same pixel (four taps
// per direction on clamped indices, fixed order) -> bf16 into the channel's own LDS slot, whose logits nobody needs any
// more. The block leaves LDS once, channels last, padding channels as zeros.
__global__ void __launch_bounds__(kKpLossThreads)
keypoint_loss_kernel(const uint16_t* __restrict__ logits, const int32_t* __restrict__ targets,
                     const int* __restrict__ n_valid, float scale, int S_in, int Kpad, int K,
                     uint16_t* __restrict__ grad, float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kp_smem[];
  const int P = S_in * S_in, S = 2 * S_in, SS = S * S;
  float* q = (float*)kp_smem;                   // [SS]
  float* red = q + SS;                          // [0,16): reductions; [24]: the upsampled logit at the target
  int* tg = (int*)(red + 32);                   // [K]
  float* lse = (float*)(tg + kp_pad4(K));       // [K] softmax sums | [K] upsampled logit at the target minus the maximum
  uint16_t* sh = (uint16_t*)(lse + 2 * kp_pad4(K));   // [K][P]
  const int tid = threadIdx.x;
  const long long r = blockIdx.x;
  const int CH = Kpad >> 3;
  for (int c = tid; c < K; c += kKpLossThreads) {
    const int t = targets[r * K + c];
    tg[c] = (t >= 0 && t < SS) ? t : -1;
  }
  __syncthreads();
  int any = 0;
  for (int c = 0; c < K; ++c) any |= tg[c] >= 0;
  uint4* gout = (uint4*)(grad + r * P * Kpad);
  if (!any) {   // block-uniform: nothing to train on this roi, its logits are not read
    for (int i = tid; i < P * CH; i += kKpLossThreads) gout[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) partial[r] = 0.0f;
    return;
  }
  kp_stage(logits + r * P * Kpad, P, Kpad, K, sh, tid, kKpLossThreads);
  __syncthreads();
  const int nv = n_valid[0];
  const float k = scale / (float)(nv > 1 ? nv : 1);
  // thread tid < P owns input pixel (i, j): its 2x2 upsampled values in the forward half, its gradient in the backward half
  const bool own = tid < P;
  int j = 0;
  const int i = own ? fast_divmod(tid, S_in, 1.0f / (float)S_in, &j) : 0;
  const int im = kp_clamp(i - 1, S_in - 1) * S_in, ic = i * S_in, ip = kp_clamp(i + 1, S_in - 1) * S_in;
  const int jm = kp_clamp(j - 1, S_in - 1), jp = kp_clamp(j + 1, S_in - 1);
  const int o00 = (2 * i) * S + 2 * j, o10 = o00 + S;   // linear indices of the quad: o00, o00+1, o10, o10+1
  const int X0 = kp_clamp(2 * j - 1, S - 1), X1 = 2 * j, X2 = 2 * j + 1, X3 = kp_clamp(2 * j + 2, S - 1);
  const float* r0 = q + kp_clamp(2 * i - 1, S - 1) * S;
  const float* r1 = q + (2 * i) * S;
  const float* r2 = q + (2 * i + 1) * S;
  const float* r3 = q + kp_clamp(2 * i + 2, S - 1) * S;
  for (int c = 0; c < K; ++c) {
    uint16_t* ch = sh + c * P;
    const int t = tg[c];
    if (t < 0) {   // block-uniform
      if (own) ch[tid] = 0;
      continue;
    }
    float u00 = 0.0f, u01 = 0.0f, u10 = 0.0f, u11 = 0.0f;
    float m = -3.402823466e+38f;
    if (own) {
      // the 3x3 neighbourhood (clamped), horizontal pass on its three rows, vertical pass: the operands of kp_up
      const float a00 = bf16_bits_to_f32(ch[im + jm]), a01 = bf16_bits_to_f32(ch[im + j]), a02 = bf16_bits_to_f32(ch[im + jp]);
      const float a10 = bf16_bits_to_f32(ch[ic + jm]), a11 = bf16_bits_to_f32(ch[ic + j]), a12 = bf16_bits_to_f32(ch[ic + jp]);
      const float a20 = bf16_bits_to_f32(ch[ip + jm]), a21 = bf16_bits_to_f32(ch[ip + j]), a22 = bf16_bits_to_f32(ch[ip + jp]);
      const float h00 = 0.75f * a01 + 0.25f * a00, h01 = 0.75f * a01 + 0.25f * a02;
      const float h10 = 0.75f * a11 + 0.25f * a10, h11 = 0.75f * a11 + 0.25f * a12;
      const float h20 = 0.75f * a21 + 0.25f * a20, h21 = 0.75f * a21 + 0.25f * a22;
      u00 = 0.75f * h10 + 0.25f * h00; u01 = 0.75f * h11 + 0.25f * h01;
      u10 = 0.75f * h10 + 0.25f * h20; u11 = 0.75f * h11 + 0.25f * h21;
      m = fmaxf(fmaxf(u00, u01), fmaxf(u10, u11));
      const int d = t - o00;   // the target inside this quad?
      if (d == 0) red[24] = u00;
      if (d == 1) red[24] = u01;
      if (d == S) red[24] = u10;
      if (d == S + 1) red[24] = u11;
    }
    m = kp_block_max(m, red);
    float s = 0.0f;
    if (own) {
      u00 = mxdet_expf(u00 - m); u01 = mxdet_expf(u01 - m); u10 = mxdet_expf(u10 - m); u11 = mxdet_expf(u11 - m);
      s = ((u00 + u01) + u10) + u11;
    }
    s = kp_block_sum(s, red);
    if (tid == 0) {   // the logarithms are taken behind the loop, all channels at once
      lse[c] = s;
      lse[kp_pad4(K) + c] = red[24] - m;
    }
    if (own) {
      const int d = t - o00;
      const float inv = 1.0f / s;   // one quotient per thread and channel: p = e * (1 / sum)
      *(float2*)(q + o00) = make_float2((u00 * inv - (d == 0 ? 1.0f : 0.0f)) * k, (u01 * inv - (d == 1 ? 1.0f : 0.0f)) * k);
      *(float2*)(q + o10) = make_float2((u10 * inv - (d == S ? 1.0f : 0.0f)) * k, (u11 * inv - (d == S + 1 ? 1.0f : 0.0f)) * k);
    }
    __syncthreads();   // q complete (and red[24] read) before anyone gathers / the next channel writes
    if (own) {
      const float c0 = ((0.25f * r0[X0] + 0.75f * r1[X0]) + 0.75f * r2[X0]) + 0.25f * r3[X0];
      const float c1 = ((0.25f * r0[X1] + 0.75f * r1[X1]) + 0.75f * r2[X1]) + 0.25f * r3[X1];
      const float c2 = ((0.25f * r0[X2] + 0.75f * r1[X2]) + 0.75f * r2[X2]) + 0.25f * r3[X2];
      const float c3 = ((0.25f * r0[X3] + 0.75f * r1[X3]) + 0.75f * r2[X3]) + 0.25f * r3[X3];
      ch[tid] = f32_to_bf16_bits(((0.25f * c0 + 0.75f * c1) + 0.75f * c2) + 0.25f * c3);
    }
    // no barrier here: the next channel reads its own logits, and q is rewritten only behind the two reductions' barriers
  }
  __syncthreads();
  const float rcpCH = 1.0f / (float)CH;
  for (int i = tid; i < P * CH; i += kKpLossThreads) {
    int ck;
    const int pix = fast_divmod(i, CH, rcpCH, &ck);
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = ck * 8 + j;
      if (c < K) w[j >> 1] |= (unsigned)sh[c * P + pix] << (16 * (j & 1));
    }
    gout[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  // cross-entropy of channel c = log(sum) - (u_target - max); one thread per channel, thread 0 adds them in channel order
  float* ce = q;   // nobody reads q any more (the barrier in front of the write-out)
  if (tid < K) ce[tid] = tg[tid] >= 0 ? mxdet_logf(lse[tid]) - lse[kp_pad4(K) + tid] : 0.0f;
  __syncthreads();
  if (tid == 0) {
    float acc = 0.0f;
    for (int c = 0; c < K; ++c) acc = acc + ce[c];
    partial[r] = acc;
  }
}

// ---- loss value: k * (partials summed in a fixed order), one workgroup; R = 0 writes 0 ------------------------------------
__global__ void __launch_bounds__(256)
keypoint_loss_final_kernel(const float* __restrict__ partial, const int* __restrict__ n_valid, int R, float scale,
                           float* __restrict__ loss_out) {
  __shared__ float redf[4];
  if (R == 0) {
    if (threadIdx.x == 0) loss_out[0] = 0.0f;
    return;
  }
  float l = 0.0f;
  for (int r = threadIdx.x; r < R; r += 256) l = l + partial[r];   // rows in ascending order per lane
  l = block4_reduce<Sum, kLane0, kScratchOnce>(l, redf);
  if (threadIdx.x == 0) {
    const int nv = n_valid[0];
    const float k = scale / (float)(nv > 1 ? nv : 1);
    loss_out[0] = k * l;
  }
}

// ---- decode: one workgroup per detection, one wave per channel at a time --------------------------------------------------
__global__ void __launch_bounds__(kKpDecodeThreads)
keypoint_decode_kernel(const uint16_t* __restrict__ logits, const float* __restrict__ dets, int S_in, int Kpad, int K,
                       float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kp_smem[];
  uint16_t* sh = (uint16_t*)kp_smem;   // [K][P]
  const int P = S_in * S_in, S = 2 * S_in, SS = S * S;
  const int tid = threadIdx.x;
  const long long r = blockIdx.x;
  const float* d = dets + r * 6;
  float* o = out + r * K * 3;
  if (!(d[5] > 0.0f) || (int)fminf(d[5], 1e9f) <= 0) {   // block-uniform: padding rows give zeros and read no logits
    for (int i = tid; i < K * 3; i += kKpDecodeThreads) o[i] = 0.0f;
    return;
  }
  kp_stage(logits + r * P * Kpad, P, Kpad, K, sh, tid, kKpDecodeThreads);
  __syncthreads();
  const float x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3];
  const float rw = fmaxf(x2 - x1, 1.0f), rh = fmaxf(y2 - y1, 1.0f);
  const float rcpS = 1.0f / (float)S;
  const int lane = lane_id();
  for (int c = tid >> 6; c < K; c += kKpDecodeThreads >> 6) {
    const uint16_t* ch = sh + c * P;
    float best = -__builtin_inff();
    int bi = 0;
    for (int idx = lane; idx < SS; idx += 64) {   // ascending per lane: a strict > keeps the lowest index
      int X;
      const int Y = fast_divmod(idx, S, rcpS, &X);
      const float u = kp_up(ch, S_in, Y, X);
      if (u > best || idx == lane) { best = u; bi = idx; }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off);
      const int oi = __shfl_xor(bi, off);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) {
      int bx;
      const int by = fast_divmod(bi, S, rcpS, &bx);
      o[c * 3 + 0] = x1 + ((float)bx + 0.5f) * (rw / (float)S);
      o[c * 3 + 1] = y1 + ((float)by + 0.5f) * (rh / (float)S);
      o[c * 3 + 2] = best;
    }
  }
}

}  // namespace mxdet

using namespace mxdet;

extern "C" int mxdet_keypoint_target(const float* rois, const int32_t* matched_gt, const int32_t* labels,
                                     const float* gt_keypoints, int64_t R, int32_t N, int32_t G, int32_t K, int32_t S_in,
                                     int32_t* targets, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(R >= 0 && N > 0 && G > 0 && K > 0 && S_in > 0 && S_in <= 16384, MXDET_ESHAPE, "keypoint_target: bad shape");
  if (R == 0) return MXDET_OK;
  MXDET_REQUIRE(rois && matched_gt && labels && gt_keypoints && targets, MXDET_EINVAL, "keypoint_target: null pointer");
  const long long total = (long long)R * K;
  MXDET_REQUIRE(total < (1ll << 31) * 256, MXDET_ESHAPE, "keypoint_target: tensor exceeds the grid");
  hipLaunchKernelGGL(keypoint_target_kernel, dim3((unsigned)ceil_div<long long>(total, 256)), dim3(256), 0,
                     as_stream(stream), rois, matched_gt, labels, gt_keypoints, total, N, G, K, 2 * S_in, targets);
  return check_launch("keypoint_target");
}

extern "C" size_t mxdet_keypoint_loss_workspace_bytes(int64_t R) {
  return 256 + (size_t)(R > 0 ? R : 0) * sizeof(float);   // n_valid | one partial sum per roi
}

extern "C" int mxdet_keypoint_loss(const uint16_t* logits, const int32_t* targets, int64_t R, int32_t S_in, int32_t Kpad,
                                   int32_t K, float loss_scale, float weight, float* loss_out, uint16_t* grad,
                                   void* workspace, size_t workspace_bytes, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(R >= 0 && R < (1ll << 31) && S_in > 0 && Kpad > 0 && Kpad % 8 == 0 && K > 0 && K <= Kpad, MXDET_ESHAPE,
                "keypoint_loss: bad shape (Kpad %% 8, 0 < K <= Kpad)");
  MXDET_REQUIRE(S_in <= 1024 && Kpad <= 4096 && S_in * S_in <= kKpLossThreads &&
                    kp_loss_lds(S_in, K) <= kKpLdsLimit,
                MXDET_ESHAPE, "keypoint_loss: S_in = %d, K = %d do not fit one workgroup (S_in <= 32, 64 KiB of LDS)", S_in, K);
  MXDET_REQUIRE(loss_out, MXDET_EINVAL, "keypoint_loss: null pointer");
  hipStream_t s = as_stream(stream);
  if (R == 0) {
    hipLaunchKernelGGL(keypoint_loss_final_kernel, dim3(1), dim3(256), 0, s, (const float*)nullptr, (const int*)nullptr, 0,
                       0.0f, loss_out);
    return check_launch("keypoint_loss");
  }
  MXDET_REQUIRE(logits && targets && grad, MXDET_EINVAL, "keypoint_loss: null pointer");
  MXDET_REQUIRE((long long)R * K < (1ll << 31), MXDET_ESHAPE, "keypoint_loss: R * K exceeds 2^31");
  MXDET_REQUIRE(workspace && workspace_bytes >= mxdet_keypoint_loss_workspace_bytes(R), MXDET_EWORKSPACE,
                "keypoint_loss: workspace too small");
  int* n_valid = (int*)workspace;
  float* partial = (float*)((char*)workspace + 256);
  const float scale = loss_scale * weight;
  hipLaunchKernelGGL(keypoint_count_kernel, dim3(1), dim3(256), 0, s, targets, (long long)R * K, 4 * S_in * S_in, n_valid);
  hipLaunchKernelGGL(keypoint_loss_kernel, dim3((unsigned)R), dim3(kKpLossThreads), kp_loss_lds(S_in, K), s, logits, targets,
                     (const int*)n_valid, scale, S_in, Kpad, K, grad, partial);
  hipLaunchKernelGGL(keypoint_loss_final_kernel, dim3(1), dim3(256), 0, s, (const float*)partial, (const int*)n_valid,
                     (int)R, scale, loss_out);
  return check_launch("keypoint_loss");
}

extern "C" int mxdet_keypoint_decode(const uint16_t* logits, const float* dets, int64_t R, int32_t S_in, int32_t Kpad,
                                     int32_t K, float* out, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(R >= 0 && R < (1ll << 31) && S_in > 0 && Kpad > 0 && Kpad % 8 == 0 && K > 0 && K <= Kpad, MXDET_ESHAPE,
                "keypoint_decode: bad shape (Kpad %% 8, 0 < K <= Kpad)");
  MXDET_REQUIRE(S_in <= 1024 && Kpad <= 4096 && kp_decode_lds(S_in, K) <= kKpLdsLimit, MXDET_ESHAPE,
                "keypoint_decode: S_in = %d, K = %d need more than 64 KiB of LDS", S_in, K);
  if (R == 0) return MXDET_OK;
  MXDET_REQUIRE(logits && dets && out, MXDET_EINVAL, "keypoint_decode: null pointer");
  hipLaunchKernelGGL(keypoint_decode_kernel, dim3((unsigned)R), dim3(kKpDecodeThreads), kp_decode_lds(S_in, K),
                     as_stream(stream), logits, dets, S_in, Kpad, K, out);
  return check_launch("keypoint_decode");
}
