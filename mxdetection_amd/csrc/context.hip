// context.hip -- the global context block of GCNet (Cao et al., "GCNet: Non-local Networks Meet Squeeze-Excitation Networks and
// Beyond", ICCVW 2019): attention pooling over the whole map, a bottleneck transform with LayerNorm, and the broadcast add in
// front of a bottleneck's residual sum, forward and backward (include/mxdet.h).
//
// Slot: models/backbones (/root/reference/README.md:27). t is bf16 [N,HW,C] channels-last. All arithmetic is fp32; every
// summation order is a function of the shape alone; no float atomics: the same bits on every run.
//
// The map kernels (pool_fwd, reduce_bwd, the two sweeps of pool_bwd) share one decomposition: a workgroup of four waves owns a
// CHUNK of kGcChunk = 64 consecutive positions of one image; wave w takes the positions w, w + 4, ... of the chunk, one position
// at a time, lane l the 16-byte vectors l, l + 64, ... of its row (NV = ceil(C / 512) of them, four rows in flight per lane).
// A dot over C is the lane's fma chain (vector order, then element order), then a 64-lane butterfly; a per-chunk sum is each
// wave's chain over its positions in order, then the four waves in wave order through LDS; the chunks of an image are folded
// by the small kernel behind (transform_fwd, transform_bwd, the d_wk fold) in runs whose bounds depend on the shape alone
// (gc_fold_chunks, block4_reduce of wave.h, gc_fold_wk_kernel). Rows past HW and vectors past C / 8 are
// predicates: no address outside a tensor is formed.
#include <initializer_list>

#include "common.h"

namespace mxdet {

constexpr int kGcChunk = 64;            // positions per workgroup of the map kernels
constexpr int kGcThreads = 256;
constexpr int kGcWaves = kGcThreads / kWave;
constexpr float kGcLowest = -3.402823466e+38f;

// the kernels' view of the descriptor and of the workspace (every region a multiple of 16 bytes)
struct GcK {
  int N, HW, C, C8, P, P8, K;            // K = chunks per image
  float eps;
  float* ms;                             // [N*K][2]   per chunk: maximum logit, sum of exp(logit - maximum)
  float* part;                           // [N*K][C]   per chunk column sums: pooled t (fwd), ds (reduce_bwd), dl * t (pool_bwd)
  float* u;                              // [N][P]     relu(LayerNorm(h)), recomputed by transform_bwd
  float* gz;                             // [N][P]     gradient at the LayerNorm's affine output, masked
  float* dh;                             // [N][P]
  float* e;                              // [N][HW]    d_ctx . t
  float* sp;                             // [N*K]      per chunk sum of att * e
};

static size_t gc_layout(const mxdet_gc_desc_t* d, GcK* k, void* base) {
  const size_t N = (size_t)d->N, K = (size_t)ceil_div(d->HW, kGcChunk), C = (size_t)d->C, P = (size_t)d->P;
  size_t off = 0;
  auto take = [&](size_t floats) {
    float* p = base ? (float*)((char*)base + off) : nullptr;
    off += align_up(floats * sizeof(float), 16);
    return p;
  };
  float* ms = take(N * K * 2);
  float* part = take(N * K * C);
  float* u = take(N * P);
  float* gz = take(N * P);
  float* dh = take(N * P);
  float* e = take(N * (size_t)d->HW);
  float* sp = take(N * K);
  if (k) { k->ms = ms; k->part = part; k->u = u; k->gz = gz; k->dh = dh; k->e = e; k->sp = sp; }
  return off;
}

// eight fp32 of a row -> registers; eight bf16 likewise (zeros past the row's end)
__device__ __forceinline__ void gc_load8_f32(const float* __restrict__ p, int v, int nv, float* f) {
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  if (v < nv) {
    a = *(const float4*)(p + 8 * v);
    b = *(const float4*)(p + 8 * v + 4);
  }
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
__device__ __forceinline__ uint4 gc_load8_bf16(const uint4* __restrict__ row, int v, int nv) {
  return v < nv ? row[v] : make_uint4(0u, 0u, 0u, 0u);
}

struct GcChunk { int n, p0, p1, wave, lane; };
__device__ __forceinline__ GcChunk gc_chunk(const GcK& k) {
  GcChunk c;
  c.n = (int)blockIdx.x / k.K;
  c.p0 = ((int)blockIdx.x % k.K) * kGcChunk;
  c.p1 = min(c.p0 + kGcChunk, k.HW);
  c.wave = (int)threadIdx.x >> 6;
  c.lane = (int)threadIdx.x & 63;
  return c;
}

// The four waves' column sums -> part[block][c] = ((a_0 + a_1) + a_2) + a_3, each a_w scaled by f[w] first if f is given.
template <int NV>
__device__ __forceinline__ void gc_merge_columns(const GcK& k, float (*s_acc)[NV * 512], const float (&acc)[NV][8], const GcChunk& c,
                                                 const float* f) {
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) s_acc[c.wave][(i * 64 + c.lane) * 8 + j] = acc[i][j];
  __syncthreads();
  float* out = k.part + (size_t)blockIdx.x * k.C;
  for (int col = (int)threadIdx.x; col < k.C; col += kGcThreads) {
    float a = f ? s_acc[0][col] * f[0] : s_acc[0][col];
#pragma unroll
    for (int w = 1; w < kGcWaves; ++w) a += f ? s_acc[w][col] * f[w] : s_acc[w][col];
    out[col] = a;
  }
}

// ---- forward --------------------------------------------------------------------------------------------------------------------
// logits[n,p] = sum_c t[n,p,c] wk[c]; per chunk the online softmax (maximum, sum, weighted column sums) into the workspace
template <int NV>
__global__ void __launch_bounds__(kGcThreads)
gc_pool_fwd_kernel(const GcK k, const uint4* __restrict__ t, const uint4* __restrict__ wk, float* __restrict__ logits) {
  constexpr int UN = 4 / NV;
  __shared__ float s_acc[kGcWaves][NV * 512];
  __shared__ float s_m[kGcWaves], s_s[kGcWaves], s_f[kGcWaves];
  const GcChunk c = gc_chunk(k);
  float w[NV][8], acc[NV][8];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    unpack8_bf16(gc_load8_bf16(wk, c.lane + 64 * i, k.C8), w[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  }
  float m = kGcLowest, s = 0.f;
  for (int p = c.p0 + c.wave; p < c.p1; p += kGcWaves * UN) {
    uint4 raw[UN][NV];
#pragma unroll
    for (int q = 0; q < UN; ++q) {
      const int pp = p + kGcWaves * q;
      const uint4* row = t + ((long long)c.n * k.HW + min(pp, c.p1 - 1)) * k.C8;
#pragma unroll
      for (int i = 0; i < NV; ++i) raw[q][i] = gc_load8_bf16(row, c.lane + 64 * i, k.C8);
    }
#pragma unroll
    for (int q = 0; q < UN; ++q) {
      const int pp = p + kGcWaves * q;
      if (pp >= c.p1) break;             // wave-uniform
      float x[NV][8], dot = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        unpack8_bf16(raw[q][i], x[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) dot += x[i][j] * w[i][j];
      }
      dot = wave_sum(dot);
      if (c.lane == 0) logits[(long long)c.n * k.HW + pp] = dot;
      const float mn = fmaxf(m, dot), f = __expf(m - mn), pe = __expf(dot - mn);
      s = s * f + pe;
#pragma unroll
      for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = acc[i][j] * f + pe * x[i][j];
      m = mn;
    }
  }
  if (c.lane == 0) { s_m[c.wave] = m; s_s[c.wave] = s; }
  __syncthreads();
  float M = s_m[0];
#pragma unroll
  for (int w2 = 1; w2 < kGcWaves; ++w2) M = fmaxf(M, s_m[w2]);
  if ((int)threadIdx.x < kGcWaves) s_f[threadIdx.x] = __expf(s_m[threadIdx.x] - M);    // 0 for a wave without positions
  __syncthreads();
  if (threadIdx.x == 0) {
    float S = s_s[0] * s_f[0];
#pragma unroll
    for (int w2 = 1; w2 < kGcWaves; ++w2) S += s_s[w2] * s_f[w2];
    k.ms[2 * (size_t)blockIdx.x] = M;
    k.ms[2 * (size_t)blockIdx.x + 1] = S;
  }
  gc_merge_columns<NV>(k, s_acc, acc, c, s_f);
}

// Fold the K chunk partials of image n into s_part[w][c]: wave w takes the chunks [w Kq, (w + 1) Kq), Kq = ceil(K / 4), in
// order; lane l the 8-column groups l, l + 64, ... (four chunks' loads in flight). SCALE: each chunk times exp(m_q - M).
// The caller adds the four waves in wave order.
template <bool SCALE>
__device__ __forceinline__ void gc_fold_chunks(const GcK& k, int n, float M, float (*s_part)[2048]) {
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int Kq = ceil_div(k.K, kGcWaves), q0 = wave * Kq, q1 = min(q0 + Kq, k.K);
  const float* ms = k.ms + 2 * (size_t)n * k.K;
  for (int cg = lane; cg < k.C8; cg += 64) {
    const float* part = k.part + (size_t)n * k.K * k.C + 8 * cg;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int q = q0; q < q1; q += 4) {
      float4 lo[4], hi[4];
      float f[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int qq = min(q + i, q1 - 1);
        lo[i] = *(const float4*)(part + (size_t)qq * k.C);
        hi[i] = *(const float4*)(part + (size_t)qq * k.C + 4);
        f[i] = SCALE ? __expf(ms[2 * qq] - M) : 1.0f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (q + i >= q1) break;
        if (SCALE) {
          a[0] += lo[i].x * f[i]; a[1] += lo[i].y * f[i]; a[2] += lo[i].z * f[i]; a[3] += lo[i].w * f[i];
          a[4] += hi[i].x * f[i]; a[5] += hi[i].y * f[i]; a[6] += hi[i].z * f[i]; a[7] += hi[i].w * f[i];
        } else {
          a[0] += lo[i].x; a[1] += lo[i].y; a[2] += lo[i].z; a[3] += lo[i].w;
          a[4] += hi[i].x; a[5] += hi[i].y; a[6] += hi[i].z; a[7] += hi[i].w;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s_part[wave][8 * cg + j] = a[j];
  }
}

// per image: chunks -> lse, ctx; h = W1 ctx + b1; LayerNorm + ReLU; add = W2 u + b2. grid = N
__global__ void __launch_bounds__(kGcThreads)
gc_transform_fwd_kernel(const GcK k, const uint4* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ gamma,
                        const float* __restrict__ beta, const uint4* __restrict__ W2, const float* __restrict__ b2,
                        float* __restrict__ lse, float* __restrict__ ctx, float* __restrict__ h, float* __restrict__ mean,
                        float* __restrict__ rstd, float* __restrict__ add) {
  __shared__ float s_part[kGcWaves][2048];
  __shared__ float s_ctx[2048], s_h[512], s_u[512], s_4[kGcWaves];
  const int n = (int)blockIdx.x, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* ms = k.ms + 2 * (size_t)n * k.K;
  // maximum and sum over the chunks: thread t the chunks t, t + 256, ... in order, then the block fold
  float M = kGcLowest;
  for (int q = tid; q < k.K; q += kGcThreads) M = fmaxf(M, ms[2 * q]);
  M = block4_reduce<FMax, kEveryLane, kScratchReused>(M, s_4);
  float S = 0.f;
  for (int q = tid; q < k.K; q += kGcThreads) S += ms[2 * q + 1] * __expf(ms[2 * q] - M);
  S = block4_reduce<Sum, kEveryLane, kScratchReused>(S, s_4);
  if (tid == 0) lse[n] = M + logf(S);
  const float inv = 1.0f / S;
  gc_fold_chunks<true>(k, n, M, s_part);
  __syncthreads();
  for (int col = tid; col < k.C; col += kGcThreads) {
    const float a = (((s_part[0][col] + s_part[1][col]) + s_part[2][col]) + s_part[3][col]) * inv;
    s_ctx[col] = a;
    ctx[(size_t)n * k.C + col] = a;
  }
  __syncthreads();
  // h[j] = W1[j] . ctx + b1[j]: a wave takes four rows at a time (16 loads in flight per lane), lane l the vectors l, l + 64, ...
  // of each; the dot is the lane's chain (vector order, element order), then the 64-lane butterfly
  for (int j0 = 4 * wave; j0 < k.P; j0 += 4 * kGcWaves) {
    uint4 raw[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        raw[r][i] = gc_load8_bf16(W1 + (size_t)min(j0 + r, k.P - 1) * k.C8, lane + 64 * i, k.C8);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (64 * i >= k.C8) break;
        float x[8];
        unpack8_bf16(raw[r][i], x);
        const int v = min(lane + 64 * i, k.C8 - 1);          // (a vector past the row is zeros: any finite ctx will do)
#pragma unroll
        for (int j = 0; j < 8; ++j) dot += x[j] * s_ctx[8 * v + j];
      }
      dot = wave_sum(dot);
      if (lane == 0 && j0 + r < k.P) {
        const float v = dot + b1[j0 + r];
        s_h[j0 + r] = v;
        h[(size_t)n * k.P + j0 + r] = v;
      }
    }
  }
  __syncthreads();
  // LayerNorm over the P values: every thread sums them in order (the same bits everywhere)
  float mu = 0.f;
  for (int j = 0; j < k.P; ++j) mu += s_h[j];
  mu /= (float)k.P;
  float var = 0.f;
  for (int j = 0; j < k.P; ++j) var += (s_h[j] - mu) * (s_h[j] - mu);
  const float rs = 1.0f / sqrtf(var / (float)k.P + k.eps);
  if (tid == 0) { mean[n] = mu; rstd[n] = rs; }
  for (int j = tid; j < k.P; j += kGcThreads) s_u[j] = fmaxf(gamma[j] * ((s_h[j] - mu) * rs) + beta[j], 0.f);
  __syncthreads();
  // add[c] = W2[c] . u + b2[c]: a thread per row, its P values in order (four vectors in flight). A row per group of lanes
  // (lane g the row's vector g, a butterfly over the group, sixteen rows in flight) reads W2 coalesced but measured twice
  // as slow at every shape (C5: 83 against 48 us at P = 128, 391 against 193 us at P = 512): the kernel is one workgroup per
  // image and waits on dependent shuffles, not on bytes.
  for (int col = tid; col < k.C; col += kGcThreads) {
    const uint4* row = W2 + (size_t)col * k.P8;
    float dot = 0.f;
    for (int v0 = 0; v0 < k.P8; v0 += 4) {
      uint4 raw[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) raw[i] = gc_load8_bf16(row, v0 + i, k.P8);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (v0 + i >= k.P8) break;
        float x[8];
        unpack8_bf16(raw[i], x);
#pragma unroll
        for (int j = 0; j < 8; ++j) dot += x[j] * s_u[8 * (v0 + i) + j];
      }
    }
    add[(size_t)n * k.C + col] = dot + b2[col];
  }
}

// y = bf16(relu((t + add[n,c]) + sc)) and the 1-bit mask of the stored values (conv.hip's layout: byte [pixel][c / 8])
__global__ void __launch_bounds__(kGcThreads)
gc_fuse_fwd_kernel(const GcK k, const uint4* __restrict__ t, const float* __restrict__ add, const uint4* __restrict__ sc,
                   uint4* __restrict__ y, unsigned char* __restrict__ bits, const long long total) {
  const long long i = (long long)blockIdx.x * kGcThreads + threadIdx.x;
  if (i >= total) return;
  const int c8 = (int)(i % k.C8);
  const int n = (int)(i / ((long long)k.HW * k.C8));
  float a[8], b[8], r[8];
  unpack8_bf16(t[i], a);
  unpack8_bf16(sc[i], b);
  gc_load8_f32(add + (size_t)n * k.C, c8, k.C8, r);
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = fmaxf((a[j] + r[j]) + b[j], 0.f);
  const uint4 o = pack8_bf16_hw(a);
  y[i] = o;
  if (bits) {
    // bf16 > 0 <=> sign clear and magnitude non-zero
    const unsigned w4[4] = {o.x, o.y, o.z, o.w};
    unsigned mb = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned lo = w4[q] & 0xffffu, hi = w4[q] >> 16;
      mb |= ((lo != 0u && lo < 0x8000u) ? 1u : 0u) << (2 * q);
      mb |= ((hi != 0u && hi < 0x8000u) ? 1u : 0u) << (2 * q + 1);
    }
    bits[i] = (unsigned char)mb;
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
// per chunk column sums of ds
template <int NV>
__global__ void __launch_bounds__(kGcThreads)
gc_reduce_bwd_kernel(const GcK k, const uint4* __restrict__ ds) {
  constexpr int UN = 4 / NV;
  __shared__ float s_acc[kGcWaves][NV * 512];
  const GcChunk c = gc_chunk(k);
  float acc[NV][8];
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  for (int p = c.p0 + c.wave; p < c.p1; p += kGcWaves * UN) {
    uint4 raw[UN][NV];
#pragma unroll
    for (int q = 0; q < UN; ++q) {
      const int pp = p + kGcWaves * q;
      const uint4* row = ds + ((long long)c.n * k.HW + min(pp, c.p1 - 1)) * k.C8;
#pragma unroll
      for (int i = 0; i < NV; ++i) raw[q][i] = gc_load8_bf16(row, pp < c.p1 ? c.lane + 64 * i : k.C8, k.C8);   // zeros past the chunk
    }
#pragma unroll
    for (int q = 0; q < UN; ++q)
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        float x[8];
        unpack8_bf16(raw[q][i], x);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] += x[j];
      }
  }
  gc_merge_columns<NV>(k, s_acc, acc, c, nullptr);
}

// per image: d_add from the chunks; LayerNorm and MLP backward down to dh and d_ctx; u, gz, dh into the workspace. grid = N
__global__ void __launch_bounds__(kGcThreads)
gc_transform_bwd_kernel(const GcK k, const uint4* __restrict__ W1, const float* __restrict__ gamma, const float* __restrict__ beta,
                        const uint4* __restrict__ W2, const float* __restrict__ h, const float* __restrict__ mean,
                        const float* __restrict__ rstd, float* __restrict__ d_add, float* __restrict__ d_ctx) {
  __shared__ float s_part[kGcWaves][2048];             // the chunk fold; then the row slices of du ([slice][P], 2048 floats)
  __shared__ float s_dadd[2048], s_xh[512], s_gg[512], s_dh[512], s_pos[512];
  const int n = (int)blockIdx.x, tid = (int)threadIdx.x;
  gc_fold_chunks<false>(k, n, 0.f, s_part);
  __syncthreads();
  for (int col = tid; col < k.C; col += kGcThreads) {
    const float a = ((s_part[0][col] + s_part[1][col]) + s_part[2][col]) + s_part[3][col];
    s_dadd[col] = a;
    d_add[(size_t)n * k.C + col] = a;
  }
  const float mu = mean[n], rs = rstd[n];
  for (int j = tid; j < k.P; j += kGcThreads) {
    const float xh = (h[(size_t)n * k.P + j] - mu) * rs, z = gamma[j] * xh + beta[j];
    s_xh[j] = xh;
    s_pos[j] = z > 0.f ? 1.f : 0.f;
    k.u[(size_t)n * k.P + j] = fmaxf(z, 0.f);
  }
  __syncthreads();
  // du[j] = sum_c d_add[c] W2[c, j]: thread = (row slice s, vector jv of eight j), ns = 256 / (P / 8) slices; slice s takes
  // the rows s, s + ns, ... in order (eight loads in flight), then thread j adds the slices in order
  const int ns = kGcThreads / k.P8;
  float* s_du = &s_part[0][0];
  {
    const int jv = tid % k.P8, slice = tid / k.P8;
    if (slice < ns) {
      float du[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int c0 = slice; c0 < k.C; c0 += 8 * ns) {
        uint4 raw[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) raw[i] = W2[(size_t)min(c0 + i * ns, k.C - 1) * k.P8 + jv];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (c0 + i * ns >= k.C) break;
          float x[8];
          unpack8_bf16(raw[i], x);
          const float a = s_dadd[c0 + i * ns];
#pragma unroll
          for (int j = 0; j < 8; ++j) du[j] += a * x[j];
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s_du[slice * k.P + jv * 8 + j] = du[j];
    }
  }
  __syncthreads();
  for (int j = tid; j < k.P; j += kGcThreads) {
    float du = s_du[j];
    for (int sl = 1; sl < ns; ++sl) du += s_du[sl * k.P + j];
    const float gz = du * s_pos[j];
    k.gz[(size_t)n * k.P + j] = gz;
    s_gg[j] = gz * gamma[j];
  }
  __syncthreads();
  float m1 = 0.f, m2 = 0.f;
  for (int j = 0; j < k.P; ++j) {
    m1 += s_gg[j];
    m2 += s_gg[j] * s_xh[j];
  }
  m1 /= (float)k.P;
  m2 /= (float)k.P;
  for (int j = tid; j < k.P; j += kGcThreads) {
    const float v = rs * ((s_gg[j] - m1) - s_xh[j] * m2);
    s_dh[j] = v;
    k.dh[(size_t)n * k.P + j] = v;
  }
  __syncthreads();
  // d_ctx[c] = sum_j dh[j] W1[j, c]: thread = a vector of eight c, j in order (eight loads in flight)
  for (int cv = tid; cv < k.C8; cv += kGcThreads) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < k.P; j0 += 8) {              // P is a multiple of 8
      uint4 raw[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) raw[i] = W1[(size_t)(j0 + i) * k.C8 + cv];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float x[8];
        unpack8_bf16(raw[i], x);
        const float v = s_dh[j0 + i];
#pragma unroll
        for (int q = 0; q < 8; ++q) a[q] += v * x[q];
      }
    }
    float* out = d_ctx + (size_t)n * k.C + 8 * cv;
    *(float4*)out = make_float4(a[0], a[1], a[2], a[3]);
    *(float4*)(out + 4) = make_float4(a[4], a[5], a[6], a[7]);
  }
}

// the six parameter gradients: one thread per element, the images summed in order. Elements: dW2 [C,P], dW1 [P,C], db2 [C],
// db1 [P], dgamma [P], dbeta [P]
__global__ void __launch_bounds__(kGcThreads)
gc_param_grad_kernel(const GcK k, const float* __restrict__ ctx, const float* __restrict__ h, const float* __restrict__ mean,
                     const float* __restrict__ rstd, const float* __restrict__ d_add, float* __restrict__ dW1,
                     float* __restrict__ db1, float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dW2,
                     float* __restrict__ db2, const int accumulate) {
  const long long CP = (long long)k.C * k.P;
  long long i = (long long)blockIdx.x * kGcThreads + threadIdx.x;
  float a = 0.f;
  float* out;
  if (i < CP) {
    const int col = (int)(i / k.P), j = (int)(i % k.P);
    for (int n = 0; n < k.N; ++n) a += d_add[(size_t)n * k.C + col] * k.u[(size_t)n * k.P + j];
    out = dW2 + i;
  } else if ((i -= CP) < CP) {
    const int j = (int)(i / k.C), col = (int)(i % k.C);
    for (int n = 0; n < k.N; ++n) a += k.dh[(size_t)n * k.P + j] * ctx[(size_t)n * k.C + col];
    out = dW1 + i;
  } else if ((i -= CP) < k.C) {
    for (int n = 0; n < k.N; ++n) a += d_add[(size_t)n * k.C + i];
    out = db2 + i;
  } else if ((i -= k.C) < k.P) {
    for (int n = 0; n < k.N; ++n) a += k.dh[(size_t)n * k.P + i];
    out = db1 + i;
  } else if ((i -= k.P) < k.P) {
    for (int n = 0; n < k.N; ++n) a += k.gz[(size_t)n * k.P + i] * ((h[(size_t)n * k.P + i] - mean[n]) * rstd[n]);
    out = dgamma + i;
  } else if ((i -= k.P) < k.P) {
    for (int n = 0; n < k.N; ++n) a += k.gz[(size_t)n * k.P + i];
    out = dbeta + i;
  } else {
    return;
  }
  *out = accumulate ? *out + a : a;
}

// sweep 1: e[n,p] = d_ctx[n] . t[n,p]; per chunk sum of att * e
template <int NV>
__global__ void __launch_bounds__(kGcThreads)
gc_pool_bwd_e_kernel(const GcK k, const uint4* __restrict__ t, const float* __restrict__ logits, const float* __restrict__ lse,
                     const float* __restrict__ d_ctx) {
  constexpr int UN = 4 / NV;
  __shared__ float s_s[kGcWaves];
  const GcChunk c = gc_chunk(k);
  float w[NV][8];
#pragma unroll
  for (int i = 0; i < NV; ++i) gc_load8_f32(d_ctx + (size_t)c.n * k.C, c.lane + 64 * i, k.C8, w[i]);
  const float L = lse[c.n];
  float s = 0.f;
  for (int p = c.p0 + c.wave; p < c.p1; p += kGcWaves * UN) {
    uint4 raw[UN][NV];
#pragma unroll
    for (int q = 0; q < UN; ++q) {
      const int pp = p + kGcWaves * q;
      const uint4* row = t + ((long long)c.n * k.HW + min(pp, c.p1 - 1)) * k.C8;
#pragma unroll
      for (int i = 0; i < NV; ++i) raw[q][i] = gc_load8_bf16(row, c.lane + 64 * i, k.C8);
    }
#pragma unroll
    for (int q = 0; q < UN; ++q) {
      const int pp = p + kGcWaves * q;
      if (pp >= c.p1) break;             // wave-uniform
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        float x[8];
        unpack8_bf16(raw[q][i], x);
#pragma unroll
        for (int j = 0; j < 8; ++j) dot += x[j] * w[i][j];
      }
      dot = wave_sum(dot);
      const long long o = (long long)c.n * k.HW + pp;
      if (c.lane == 0) k.e[o] = dot;
      s += __expf(logits[o] - L) * dot;
    }
  }
  if (c.lane == 0) s_s[c.wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) k.sp[blockIdx.x] = ((s_s[0] + s_s[1]) + s_s[2]) + s_s[3];
}

// sweep 2: d_t = bf16((ds + att * d_ctx[c]) + dl * wk[c]), dl = att * (e - S); per chunk column sums of dl * t
template <int NV>
__global__ void __launch_bounds__(kGcThreads)
gc_pool_bwd_dt_kernel(const GcK k, const uint4* __restrict__ t, const uint4* __restrict__ wk, const uint4* __restrict__ ds,
                      const float* __restrict__ logits, const float* __restrict__ lse, const float* __restrict__ d_ctx,
                      uint4* __restrict__ d_t) {
  constexpr int UN = NV >= 2 ? 1 : 2;
  __shared__ float s_acc[kGcWaves][NV * 512];
  __shared__ float s_4[kGcWaves];
  const GcChunk c = gc_chunk(k);
  float w[NV][8], dc[NV][8], acc[NV][8];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    unpack8_bf16(gc_load8_bf16(wk, c.lane + 64 * i, k.C8), w[i]);
    gc_load8_f32(d_ctx + (size_t)c.n * k.C, c.lane + 64 * i, k.C8, dc[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  }
  const float L = lse[c.n];
  // S[n]: thread t adds the chunks t, t + 256, ... in order, then the block fold (the same bits in every workgroup)
  float S = 0.f;
  for (int q = (int)threadIdx.x; q < k.K; q += kGcThreads) S += k.sp[(size_t)c.n * k.K + q];
  S = block4_reduce<Sum, kEveryLane, kScratchReused>(S, s_4);
  for (int p = c.p0 + c.wave; p < c.p1; p += kGcWaves * UN) {
    uint4 rt[UN][NV], rg[UN][NV];
#pragma unroll
    for (int q = 0; q < UN; ++q) {
      const long long r = ((long long)c.n * k.HW + min(p + kGcWaves * q, c.p1 - 1)) * k.C8;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        rt[q][i] = gc_load8_bf16(t + r, c.lane + 64 * i, k.C8);
        rg[q][i] = gc_load8_bf16(ds + r, c.lane + 64 * i, k.C8);
      }
    }
#pragma unroll
    for (int q = 0; q < UN; ++q) {
      const int pp = p + kGcWaves * q;
      if (pp >= c.p1) break;             // wave-uniform
      const long long o = (long long)c.n * k.HW + pp;
      const float att = __expf(logits[o] - L), dl = att * (k.e[o] - S);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        float x[8], g[8];
        unpack8_bf16(rt[q][i], x);
        unpack8_bf16(rg[q][i], g);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          g[j] = (g[j] + att * dc[i][j]) + dl * w[i][j];
          acc[i][j] += dl * x[j];
        }
        const int v = c.lane + 64 * i;
        if (v < k.C8) d_t[o * k.C8 + v] = pack8_bf16_hw(g);
      }
    }
  }
  gc_merge_columns<NV>(k, s_acc, acc, c, nullptr);
}

// d_wk[c] (+)= the N K chunk partials: a workgroup owns 16 columns; slice s of 16 takes the partials [s B, (s + 1) B),
// B = ceil(N K / 16), in order (eight loads in flight); then the 16 slices in order
constexpr int kGcFoldCols = 16;
__global__ void __launch_bounds__(kGcThreads)
gc_fold_wk_kernel(const GcK k, float* __restrict__ d_wk, const int accumulate) {
  __shared__ float s_p[kGcThreads / kGcFoldCols][kGcFoldCols];
  const int ci = (int)threadIdx.x % kGcFoldCols, slice = (int)threadIdx.x / kGcFoldCols;
  const int col = (int)blockIdx.x * kGcFoldCols + ci;
  const long long nb = (long long)k.N * k.K, B = ceil_div(nb, (long long)(kGcThreads / kGcFoldCols));
  const long long b0 = slice * B, b1 = min(b0 + B, nb);
  float a = 0.f;
  if (col < k.C)
    for (long long b = b0; b < b1; b += 8) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = k.part[min(b + i, b1 - 1) * k.C + col];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (b + i < b1) a += v[i];
    }
  s_p[slice][ci] = a;
  __syncthreads();
  if (slice == 0 && col < k.C) {
    float r = s_p[0][ci];
#pragma unroll
    for (int sl = 1; sl < kGcThreads / kGcFoldCols; ++sl) r += s_p[sl][ci];
    d_wk[col] = accumulate ? d_wk[col] + r : r;
  }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

static int gc_check_desc(const char* entry, const mxdet_gc_desc_t* d) {
  MXDET_REQUIRE(d != nullptr, MXDET_EINVAL, "%s: null descriptor", entry);
  MXDET_REQUIRE(d->C >= 8 && d->C <= 2048 && d->C % 8 == 0, MXDET_ESHAPE, "%s: C %d must be a multiple of 8 in [8, 2048]", entry,
                d->C);
  MXDET_REQUIRE(d->P >= 8 && d->P <= 512 && d->P % 8 == 0, MXDET_ESHAPE, "%s: P %d must be a multiple of 8 in [8, 512]", entry,
                d->P);
  MXDET_REQUIRE(d->HW >= 1 && d->HW < (1 << 20), MXDET_ESHAPE, "%s: HW %d must be in [1, 2^20)", entry, d->HW);
  MXDET_REQUIRE(d->N >= 1 && d->N <= 65535, MXDET_ESHAPE, "%s: N %d must be in [1, 65535]", entry, d->N);
  MXDET_REQUIRE((long long)d->N * d->HW * d->C < (1ll << 31), MXDET_ESHAPE, "%s: tensors too large", entry);
  MXDET_REQUIRE(d->eps > 0.f && d->eps < 1.f, MXDET_EINVAL, "%s: eps %g must be in (0, 1)", entry, (double)d->eps);
  return MXDET_OK;
}

// The descriptor's and the workspace's checks and the kernels' view of both.
static int gc_prepare(const char* entry, const mxdet_gc_desc_t* d, void* workspace, size_t workspace_bytes, bool need_ws, GcK* k) {
  const int rc = gc_check_desc(entry, d);
  if (rc != MXDET_OK) return rc;
  k->N = d->N; k->HW = d->HW; k->C = d->C; k->C8 = d->C / 8; k->P = d->P; k->P8 = d->P / 8;
  k->K = ceil_div(d->HW, kGcChunk);
  k->eps = d->eps;
  if (need_ws) {
    MXDET_REQUIRE(workspace != nullptr && aligned16(workspace), MXDET_EINVAL, "%s: workspace null or not 16-byte aligned", entry);
    const size_t need = gc_layout(d, k, workspace);
    MXDET_REQUIRE(workspace_bytes >= need, MXDET_EWORKSPACE, "%s: workspace %zu bytes, need %zu", entry, workspace_bytes, need);
  }
  return MXDET_OK;
}

static bool gc_all_aligned(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (p == nullptr || !aligned16(p)) return false;
  return true;
}

// NV of the map kernels: vectors per lane, 1 (C <= 512), 2 (<= 1024) or 4
#define GC_LAUNCH_NV(kernel, k, stream, ...)                                                                     \
  do {                                                                                                           \
    const dim3 grid((unsigned)((k).N * (k).K));                                                                  \
    if ((k).C8 <= 64)                                                                                            \
      hipLaunchKernelGGL(kernel<1>, grid, dim3(kGcThreads), 0, as_stream(stream), k, __VA_ARGS__);               \
    else if ((k).C8 <= 128)                                                                                      \
      hipLaunchKernelGGL(kernel<2>, grid, dim3(kGcThreads), 0, as_stream(stream), k, __VA_ARGS__);               \
    else                                                                                                         \
      hipLaunchKernelGGL(kernel<4>, grid, dim3(kGcThreads), 0, as_stream(stream), k, __VA_ARGS__);               \
  } while (0)

}  // namespace mxdet

using namespace mxdet;

extern "C" size_t mxdet_gc_workspace_bytes(const mxdet_gc_desc_t* d) {
  clear_error();
  if (gc_check_desc("gc_workspace_bytes", d) != MXDET_OK) return 0;
  return gc_layout(d, nullptr, nullptr);
}

extern "C" int mxdet_gc_pool_fwd(const mxdet_gc_desc_t* d, const uint16_t* t, const uint16_t* wk, float* logits, void* workspace,
                                 size_t workspace_bytes, mxdet_stream_t stream) {
  clear_error();
  GcK k;
  const int rc = gc_prepare("gc_pool_fwd", d, workspace, workspace_bytes, true, &k);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(gc_all_aligned({t, wk, logits}), MXDET_EINVAL, "gc_pool_fwd: null or not 16-byte aligned pointer");
  GC_LAUNCH_NV(gc_pool_fwd_kernel, k, stream, (const uint4*)t, (const uint4*)wk, logits);
  return check_launch("gc_pool_fwd");
}

extern "C" int mxdet_gc_transform_fwd(const mxdet_gc_desc_t* d, const uint16_t* W1, const float* b1, const float* gamma,
                                      const float* beta, const uint16_t* W2, const float* b2, float* lse, float* ctx, float* h,
                                      float* mean, float* rstd, float* add, const void* workspace, size_t workspace_bytes,
                                      mxdet_stream_t stream) {
  clear_error();
  GcK k;
  const int rc = gc_prepare("gc_transform_fwd", d, (void*)workspace, workspace_bytes, true, &k);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(gc_all_aligned({W1, b1, gamma, beta, W2, b2, lse, ctx, h, mean, rstd, add}), MXDET_EINVAL,
                "gc_transform_fwd: null or not 16-byte aligned pointer");
  hipLaunchKernelGGL(gc_transform_fwd_kernel, dim3((unsigned)k.N), dim3(kGcThreads), 0, as_stream(stream), k, (const uint4*)W1, b1,
                     gamma, beta, (const uint4*)W2, b2, lse, ctx, h, mean, rstd, add);
  return check_launch("gc_transform_fwd");
}

extern "C" int mxdet_gc_fuse_fwd(const mxdet_gc_desc_t* d, const uint16_t* t, const float* add, const uint16_t* sc, uint16_t* y,
                                 uint8_t* y_bits, mxdet_stream_t stream) {
  clear_error();
  GcK k;
  const int rc = gc_prepare("gc_fuse_fwd", d, nullptr, 0, false, &k);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(gc_all_aligned({t, add, sc, y}) && aligned16(y_bits), MXDET_EINVAL,
                "gc_fuse_fwd: null or not 16-byte aligned pointer (y_bits may be null)");
  const long long total = (long long)k.N * k.HW * k.C8;
  hipLaunchKernelGGL(gc_fuse_fwd_kernel, dim3((unsigned)ceil_div(total, (long long)kGcThreads)), dim3(kGcThreads), 0,
                     as_stream(stream), k, (const uint4*)t, add, (const uint4*)sc, (uint4*)y, y_bits, total);
  return check_launch("gc_fuse_fwd");
}

extern "C" int mxdet_gc_reduce_bwd(const mxdet_gc_desc_t* d, const uint16_t* ds, void* workspace, size_t workspace_bytes,
                                   mxdet_stream_t stream) {
  clear_error();
  GcK k;
  const int rc = gc_prepare("gc_reduce_bwd", d, workspace, workspace_bytes, true, &k);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(gc_all_aligned({ds}), MXDET_EINVAL, "gc_reduce_bwd: null or not 16-byte aligned pointer");
  GC_LAUNCH_NV(gc_reduce_bwd_kernel, k, stream, (const uint4*)ds);
  return check_launch("gc_reduce_bwd");
}

extern "C" int mxdet_gc_transform_bwd(const mxdet_gc_desc_t* d, const uint16_t* W1, const float* gamma, const float* beta,
                                      const uint16_t* W2, const float* ctx, const float* h, const float* mean, const float* rstd,
                                      float* d_add, float* d_ctx, float* dW1, float* db1, float* dgamma, float* dbeta, float* dW2,
                                      float* db2, int32_t accumulate, void* workspace, size_t workspace_bytes,
                                      mxdet_stream_t stream) {
  clear_error();
  GcK k;
  const int rc = gc_prepare("gc_transform_bwd", d, workspace, workspace_bytes, true, &k);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(gc_all_aligned({W1, gamma, beta, W2, ctx, h, mean, rstd, d_add, d_ctx, dW1, db1, dgamma, dbeta, dW2, db2}),
                MXDET_EINVAL, "gc_transform_bwd: null or not 16-byte aligned pointer");
  hipLaunchKernelGGL(gc_transform_bwd_kernel, dim3((unsigned)k.N), dim3(kGcThreads), 0, as_stream(stream), k, (const uint4*)W1,
                     gamma, beta, (const uint4*)W2, h, mean, rstd, d_add, d_ctx);
  const long long outs = 2ll * k.C * k.P + k.C + 3ll * k.P;
  hipLaunchKernelGGL(gc_param_grad_kernel, dim3((unsigned)ceil_div(outs, (long long)kGcThreads)), dim3(kGcThreads), 0,
                     as_stream(stream), k, ctx, h, mean, rstd, (const float*)d_add, dW1, db1, dgamma, dbeta, dW2, db2,
                     accumulate ? 1 : 0);
  return check_launch("gc_transform_bwd");
}

extern "C" int mxdet_gc_pool_bwd(const mxdet_gc_desc_t* d, const uint16_t* t, const uint16_t* wk, const uint16_t* ds,
                                 const float* logits, const float* lse, const float* d_ctx, uint16_t* d_t, float* d_wk,
                                 int32_t accumulate, void* workspace, size_t workspace_bytes, mxdet_stream_t stream) {
  clear_error();
  GcK k;
  const int rc = gc_prepare("gc_pool_bwd", d, workspace, workspace_bytes, true, &k);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(gc_all_aligned({t, wk, ds, logits, lse, d_ctx, d_t, d_wk}), MXDET_EINVAL,
                "gc_pool_bwd: null or not 16-byte aligned pointer");
  GC_LAUNCH_NV(gc_pool_bwd_e_kernel, k, stream, (const uint4*)t, logits, lse, d_ctx);
  GC_LAUNCH_NV(gc_pool_bwd_dt_kernel, k, stream, (const uint4*)t, (const uint4*)wk, (const uint4*)ds, logits, lse, d_ctx,
               (uint4*)d_t);
  hipLaunchKernelGGL(gc_fold_wk_kernel, dim3((unsigned)ceil_div(k.C, kGcFoldCols)), dim3(kGcThreads), 0, as_stream(stream), k, d_wk,
                     accumulate ? 1 : 0);
  return check_launch("gc_pool_bwd");
}
