// group_norm.hip -- GroupNorm (+ fused ReLU) forward / backward over channels-last bf16 [N, HW, C] (include/mxdet.h,
// mxdet_gn_desc_t). Bandwidth-bound: every kernel moves 16 bytes per lane per access and reduces in fp32.
//
// Thread layout (both routes). A lane owns one 8-channel vector (16 B); C / 8 = CV vectors make a pixel, and since
// (C / G) % 8 == 0 a vector lies inside one group. The first Teff = PR * CV threads of a workgroup (PR = T / CV pixel
// rows) are laid over PR consecutive pixels, thread t at (row t / CV, vector t % CV) -- consecutive threads read
// consecutive 16-byte words -- and thread t's i-th vector is the same channel vector PR * i pixels further on. So a
// thread's channels, group, gamma and beta are fixed, and its VPT vectors stay in registers between the passes.
//
// Resident route (one sample <= 8 vectors per thread of a 1024-thread workgroup: the RoI heads): one workgroup per sample;
// x (backward: x and dy) is read from HBM once, mean, variance about the mean, normalisation and store all come from the
// register copy. Nothing a sample's workgroup does depends on N or on the sample's index.
// Tiled route (larger samples: pyramid maps): a sample is cut into chunks of PR * 8 pixels, one workgroup each. Forward:
// per-chunk (mean, M2) about the chunk's own mean -> workspace -> Chan merge of (count, mean, M2) in chunk order (one
// wave per (sample, group), fixed butterfly) -> apply kernel. Backward: per-chunk partial sums -> merged in chunk order
// -> apply kernel.
// dgamma / dbeta: every workgroup writes its fp32 per-channel partial row to the workspace; a fold kernel sums the rows
// in a fixed order (no float atomics anywhere).
#include "common.h"

namespace mxdet {
namespace {

constexpr int kGnMaxVpt = 8;          // vectors a thread keeps in registers
constexpr int kGnBigBlock = 1024;     // resident route: workgroup size of the larger samples
constexpr int kGnBlock = 256;         // resident route (small samples) and tiled route
constexpr int kGnGridY = 65535;       // samples per grid.y; the rest of N goes to grid.z
constexpr int kGnFoldRows = 16;       // fold kernel: row lanes per 64 columns

struct GnGeom {
  int N, HW, C, G;
  int CV;       // vectors per pixel
  int gv;       // vectors per group
  int PR;       // pixel rows per workgroup pass
  int Teff;     // PR * CV active threads
  int chunks;   // workgroups per sample (1 = resident)
  int pc;       // pixels per chunk
  float eps;
  float inv_m;  // 1 / (HW * C / G)
  int relu;
};

// Keeps a register-resident vector packed between two passes: without it hipcc carries the 8 unpacked floats of every
// vector (and values derived from them) across the block reduction and spills; re-unpacking is two ALU ops per value.
__device__ __forceinline__ void keep_packed(uint4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
// two packed bf16 -> 0xffff in the half whose value is > 0 (sign clear, not zero)
__device__ __forceinline__ unsigned positive_mask(unsigned w) {
  const unsigned lo = w & 0xffffu, hi = w >> 16;
  return ((lo != 0u && lo < 0x8000u) ? 0xffffu : 0u) | ((hi != 0u && hi < 0x8000u) ? 0xffff0000u : 0u);
}
// the one place the normalised value is computed: forward, and backward's recomputed ReLU mask, agree bit for bit
__device__ __forceinline__ float gn_affine(float xh, float ga, float be) { return xh * ga + be; }

// Per-group sums of K per-thread values over the workgroup, in a fixed order: rows of a column first (ascending),
// then the columns of a group (ascending). sh: K * Teff + K * CV floats. Every active thread gets its group's sums.
template <int K>
__device__ __forceinline__ void group_sums(const GnGeom& a, float* sh, int t, int cv, bool active, const float (&v)[K],
                                           float (&out)[K]) {
  float* col = sh + K * a.Teff;
  __syncthreads();   // the previous use of sh is over
  if (active) {
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k * a.Teff + t] = v[k];
  }
  __syncthreads();
  for (int o = t; o < K * a.CV; o += blockDim.x) {
    const int k = o / a.CV, c = o - k * a.CV;
    float s = 0.f;
    for (int r = 0; r < a.PR; ++r) s += sh[k * a.Teff + r * a.CV + c];
    col[o] = s;
  }
  __syncthreads();
  const int g0 = (cv / a.gv) * a.gv;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float s = 0.f;
    if (active)
      for (int j = 0; j < a.gv; ++j) s += col[k * a.CV + g0 + j];
    out[k] = s;
  }
}

// Per-channel sums of a thread's 8 values over the pixel rows of the workgroup -> row[(cv * 8 + k)] of the partials.
__device__ __forceinline__ void channel_sums(const GnGeom& a, float* sh, int t, bool active, const float (&v)[8],
                                             float* __restrict__ row) {
  __syncthreads();
  if (active) {
#pragma unroll
    for (int k = 0; k < 8; ++k) sh[k * a.Teff + t] = v[k];
  }
  __syncthreads();
  for (int o = t; o < 8 * a.CV; o += blockDim.x) {
    const int k = o / a.CV, c = o - k * a.CV;
    float s = 0.f;
    for (int r = 0; r < a.PR; ++r) s += sh[k * a.Teff + r * a.CV + c];
    row[c * 8 + k] = s;
  }
}

// Element offset of (pixel p, this thread's vector) from the chunk's first element, with p clamped into the chunk: loads
// are issued unconditionally (no branch per vector, all of a thread's loads in flight together) and padding vectors are
// zeroed afterwards. Needs `pend`, `ch`, `cv` and `a` in scope.
#define GN_VOFF(p) ((unsigned)((min((p), pend - 1) - ch * a.pc) * a.C + cv * 8))

// ---- forward ------------------------------------------------------------------------------------------------------
// grid (chunks, N). STATS_ONLY (tiled route): writes the chunk's (mean, M2) per group to part[((n*chunks+ch)*G+g)*2].
template <int VPT, bool STATS_ONLY, int TB>
__global__ void __launch_bounds__(TB) gn_fwd_kernel(GnGeom a, const uint16_t* __restrict__ x,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, uint16_t* __restrict__ y,
                                                             float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                             float* __restrict__ part) {
  extern __shared__ float sh[];
  const int t = threadIdx.x, n = blockIdx.y + blockIdx.z * kGnGridY, ch = blockIdx.x;
  if (n >= a.N) return;   // uniform per workgroup
  const bool active = t < a.Teff;
  const int pr = t / a.CV, cv = t - pr * a.CV;
  const int p0 = ch * a.pc + pr;
  const int pend = min(a.HW, (ch + 1) * a.pc);
  const long long sbase = ((long long)n * a.HW + (long long)ch * a.pc) * a.C;
  uint4 xv[VPT];
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int p = p0 + i * a.PR;
    xv[i] = *reinterpret_cast<const uint4*>(x + sbase + GN_VOFF(p));
    if (!(active && p < pend)) xv[i] = make_uint4(0, 0, 0, 0);
  }
  const float inv_cnt = STATS_ONLY ? 1.f / ((float)(pend - ch * a.pc) * (float)(a.gv * 8)) : a.inv_m;
  // mean
  float s[1] = {0.f}, r[1];
#pragma unroll
  for (int i = 0; i < VPT; ++i) {   // padding vectors are zero: they add nothing
    float f[8];
    unpack8_bf16(xv[i], f);
    s[0] += ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
  }
  group_sums<1>(a, sh, t, cv, active, s, r);
#pragma unroll
  for (int i = 0; i < VPT; ++i) keep_packed(xv[i]);
  const float mean = r[0] * inv_cnt;
  // M2 about the mean, from the register copy
  s[0] = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    if (p0 + i * a.PR < pend) {
      float f[8];
      unpack8_bf16(xv[i], f);
      float q = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) { const float d = f[k] - mean; q += d * d; }
      s[0] += q;
    }
  }
  group_sums<1>(a, sh, t, cv, active, s, r);
#pragma unroll
  for (int i = 0; i < VPT; ++i) keep_packed(xv[i]);
  const int g = cv / a.gv;
  if (STATS_ONLY) {
    if (active && pr == 0 && cv == g * a.gv) {
      float* o = part + (((long long)n * a.chunks + ch) * a.G + g) * 2;
      o[0] = mean;
      o[1] = r[0];
    }
    return;
  }
  const float rstd = 1.0f / sqrtf(r[0] * a.inv_m + a.eps);
  if (!active) return;
  if (pr == 0 && cv == g * a.gv) {
    mean_out[(long long)n * a.G + g] = mean;
    rstd_out[(long long)n * a.G + g] = rstd;
  }
  float ga[8], be[8];
  {
    const float4 g0 = *reinterpret_cast<const float4*>(gamma + cv * 8), g1 = *reinterpret_cast<const float4*>(gamma + cv * 8 + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(beta + cv * 8), b1 = *reinterpret_cast<const float4*>(beta + cv * 8 + 4);
    ga[0] = g0.x; ga[1] = g0.y; ga[2] = g0.z; ga[3] = g0.w; ga[4] = g1.x; ga[5] = g1.y; ga[6] = g1.z; ga[7] = g1.w;
    be[0] = b0.x; be[1] = b0.y; be[2] = b0.z; be[3] = b0.w; be[4] = b1.x; be[5] = b1.y; be[6] = b1.z; be[7] = b1.w;
  }
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int p = p0 + i * a.PR;
    if (p < pend) {
      float f[8];
      unpack8_bf16(xv[i], f);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float v = gn_affine((f[k] - mean) * rstd, ga[k], be[k]);
        f[k] = a.relu ? fmaxf(v, 0.f) : v;
      }
      *reinterpret_cast<uint4*>(y + sbase + GN_VOFF(p)) = pack8_bf16_hw(f);
    }
  }
}

// Chan merge of the chunks' (count, mean, M2) of one (sample, group), one wave each: lane l folds chunks l, l + 64, ...
// in ascending order, then the lanes are folded by a fixed butterfly (lane l takes lane l + off, off = 32 ... 1).
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& qa, float nb, float mb, float qb) {
  if (nb == 0.f) return;
  if (na == 0.f) { na = nb; ma = mb; qa = qb; return; }
  const float nn = na + nb, d = mb - ma;
  ma = ma + d * (nb / nn);
  qa = qa + qb + d * d * (na * (nb / nn));
  na = nn;
}
__global__ void __launch_bounds__(kGnBlock) gn_merge_stats_kernel(GnGeom a, const float* __restrict__ part,
                                                                  float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  const int wave = blockIdx.x * (kGnBlock / kWave) + (threadIdx.x >> 6), lane = lane_id();
  if (wave >= a.N * a.G) return;
  const int n = wave / a.G, g = wave - n * a.G;
  float cn = 0.f, cm = 0.f, cq = 0.f;
  for (int ch = lane; ch < a.chunks; ch += kWave) {
    const float* o = part + (((long long)n * a.chunks + ch) * a.G + g) * 2;
    const int pix = min(a.HW, (ch + 1) * a.pc) - ch * a.pc;
    chan_merge(cn, cm, cq, (float)pix * (float)(a.gv * 8), o[0], o[1]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float nb = __shfl_down(cn, off), mb = __shfl_down(cm, off), qb = __shfl_down(cq, off);
    chan_merge(cn, cm, cq, nb, mb, qb);
  }
  if (lane == 0) {
    mean_out[wave] = cm;
    rstd_out[wave] = 1.0f / sqrtf(cq * a.inv_m + a.eps);
  }
}

// tiled route: y from the merged statistics, same chunk geometry
__global__ void __launch_bounds__(kGnBlock) gn_apply_kernel(GnGeom a, const uint16_t* __restrict__ x,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                            uint16_t* __restrict__ y) {
  const int t = threadIdx.x, n = blockIdx.y + blockIdx.z * kGnGridY, ch = blockIdx.x;
  if (n >= a.N) return;   // uniform per workgroup
  if (t >= a.Teff) return;
  const int pr = t / a.CV, cv = t - pr * a.CV, g = cv / a.gv;
  const int pend = min(a.HW, (ch + 1) * a.pc);
  const long long sbase = ((long long)n * a.HW + (long long)ch * a.pc) * a.C;
  const float mean = mean_in[(long long)n * a.G + g], rstd = rstd_in[(long long)n * a.G + g];
  float ga[8], be[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { ga[k] = gamma[cv * 8 + k]; be[k] = beta[cv * 8 + k]; }
  const int p0 = ch * a.pc + pr;
  uint4 xv[kGnMaxVpt];
#pragma unroll
  for (int i = 0; i < kGnMaxVpt; ++i) xv[i] = *reinterpret_cast<const uint4*>(x + sbase + GN_VOFF(p0 + i * a.PR));
#pragma unroll
  for (int i = 0; i < kGnMaxVpt; ++i) {
    const int p = p0 + i * a.PR;
    if (p < pend) {
      float f[8];
      unpack8_bf16(xv[i], f);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float v = gn_affine((f[k] - mean) * rstd, ga[k], be[k]);
        f[k] = a.relu ? fmaxf(v, 0.f) : v;
      }
      *reinterpret_cast<uint4*>(y + sbase + GN_VOFF(p)) = pack8_bf16_hw(f);
    }
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------
// xh = (x - mean) * rstd, g = dy (where y > 0 under relu), m = HW * C / G:
//   dgamma_c = sum g * xh, dbeta_c = sum g, s1 = sum_group g * gamma * xh, s2 = sum_group g * gamma,
//   dx = rstd * (g * gamma - (s2 + xh * s1) / m).
// grid (chunks, N). PHASE 0: resident (everything). PHASE 1: tiled, partial sums only (s1, s2 per chunk ->
// gpart[((n*chunks+ch)*G+g)*2], channel rows -> rows). PHASE 2: tiled, dx from the merged sums gsum[(n*G+g)*2].
template <int VPT, int PHASE, int TB>
__global__ void __launch_bounds__(TB) gn_bwd_kernel(GnGeom a, const uint16_t* __restrict__ x,
                                                             const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
                                                             const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             uint16_t* __restrict__ dx, float* __restrict__ rows,
                                                             float* __restrict__ gpart, const float* __restrict__ gsum) {
  extern __shared__ float sh[];
  const int t = threadIdx.x, n = blockIdx.y + blockIdx.z * kGnGridY, ch = blockIdx.x;
  if (n >= a.N) return;   // uniform per workgroup
  const bool active = t < a.Teff;
  const int pr = t / a.CV, cv = active ? t - pr * a.CV : 0, g = cv / a.gv;
  const int p0 = ch * a.pc + pr;
  const int pend = min(a.HW, (ch + 1) * a.pc);
  const long long sbase = ((long long)n * a.HW + (long long)ch * a.pc) * a.C;
  const float mean = mean_in[(long long)n * a.G + g], rstd = rstd_in[(long long)n * a.G + g];
  float ga[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) ga[k] = gamma[cv * 8 + k];
  uint4 xv[VPT], gv_[VPT];
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int p = p0 + i * a.PR;
    xv[i] = *reinterpret_cast<const uint4*>(x + sbase + GN_VOFF(p));
    gv_[i] = *reinterpret_cast<const uint4*>(dy + sbase + GN_VOFF(p));
    if (!(active && p < pend)) xv[i] = gv_[i] = make_uint4(0, 0, 0, 0);
  }
  if (a.relu) {   // dy counts where the stored bf16 y is > 0; from here on gv_ holds the masked dy
    if (y != nullptr) {
#pragma unroll
      for (int i = 0; i < VPT; ++i) {
        const int p = p0 + i * a.PR;
        const uint4 yv = *reinterpret_cast<const uint4*>(y + sbase + GN_VOFF(p));   // padding vectors: dy is zero already
        gv_[i].x &= positive_mask(yv.x); gv_[i].y &= positive_mask(yv.y);
        gv_[i].z &= positive_mask(yv.z); gv_[i].w &= positive_mask(yv.w);
        if (i % 4 == 3) __builtin_amdgcn_sched_barrier(0);   // at most four y vectors in flight beside x and dy
      }
    } else {      // no y: the bits forward stored, recomputed
      float be[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) be[k] = beta[cv * 8 + k];
#pragma unroll
      for (int i = 0; i < VPT; ++i) {
        float f[8];
        unpack8_bf16(xv[i], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = gn_affine((f[k] - mean) * rstd, ga[k], be[k]);
        const uint4 yv = pack8_bf16_hw(f);
        gv_[i].x &= positive_mask(yv.x); gv_[i].y &= positive_mask(yv.y);
        gv_[i].z &= positive_mask(yv.z); gv_[i].w &= positive_mask(yv.w);
      }
    }
#pragma unroll
    for (int i = 0; i < VPT; ++i) keep_packed(gv_[i]);
  }
  float s[2] = {0.f, 0.f}, dg[8], db[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) dg[k] = db[k] = 0.f;
  if (PHASE != 2) {
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      float f[8], d[8];
      unpack8_bf16(xv[i], f);
      unpack8_bf16(gv_[i], d);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float xh = (f[k] - mean) * rstd;
        const float dg_ = d[k] * ga[k];
        s[0] += dg_ * xh;
        s[1] += dg_;
        dg[k] += d[k] * xh;
        db[k] += d[k];
      }
      __builtin_amdgcn_sched_barrier(0);   // one vector's unpacked floats at a time: the packed copies are what stays live
    }
  }
  float r[2];
  if (PHASE != 2) {
    group_sums<2>(a, sh, t, cv, active, s, r);
    float* row = rows + ((long long)n * a.chunks + ch) * 2 * a.C;
    channel_sums(a, sh, t, active, dg, row);     // before the dx pass: their 16 registers are free in it
    channel_sums(a, sh, t, active, db, row + a.C);
#pragma unroll
    for (int i = 0; i < VPT; ++i) { keep_packed(xv[i]); keep_packed(gv_[i]); }
  }
  if (PHASE == 1) {
    if (active && pr == 0 && cv == g * a.gv) {
      float* o = gpart + (((long long)n * a.chunks + ch) * a.G + g) * 2;
      o[0] = r[0];
      o[1] = r[1];
    }
  } else {
    if (PHASE == 2) {
      r[0] = gsum[((long long)n * a.G + g) * 2];
      r[1] = gsum[((long long)n * a.G + g) * 2 + 1];
    }
    const float c1 = r[0] * a.inv_m, c2 = r[1] * a.inv_m;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int p = p0 + i * a.PR;
      if (active && p < pend) {
        float f[8], d[8];
        unpack8_bf16(xv[i], f);
        unpack8_bf16(gv_[i], d);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float xh = (f[k] - mean) * rstd;
          f[k] = rstd * (d[k] * ga[k] - (c2 + xh * c1));
        }
        *reinterpret_cast<uint4*>(dx + sbase + GN_VOFF(p)) = pack8_bf16_hw(f);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// sums of the chunks' (s1, s2) per (sample, group): same wave layout as gn_merge_stats_kernel, plain fp32 sums
__global__ void __launch_bounds__(kGnBlock) gn_merge_sums_kernel(GnGeom a, const float* __restrict__ gpart,
                                                                 float* __restrict__ gsum) {
  const int wave = blockIdx.x * (kGnBlock / kWave) + (threadIdx.x >> 6), lane = lane_id();
  if (wave >= a.N * a.G) return;
  const int n = wave / a.G, g = wave - n * a.G;
  float s1 = 0.f, s2 = 0.f;
  for (int ch = lane; ch < a.chunks; ch += kWave) {
    const float* o = gpart + (((long long)n * a.chunks + ch) * a.G + g) * 2;
    s1 += o[0];
    s2 += o[1];
  }
  wave_reduce_each<Sum, 64, kDescend, kLane0>(s1, s2);
  if (lane == 0) {
    gsum[(long long)wave * 2] = s1;
    gsum[(long long)wave * 2 + 1] = s2;
  }
}

// out[j] (+)= sum over the P partial rows of rows[p][j], j < 2C (dgamma | dbeta): row lane q sums rows q, q + 16, ...
// ascending, then the 16 lanes are summed ascending.
__global__ void __launch_bounds__(kGnFoldRows * 64) gn_fold_kernel(const float* __restrict__ rows, long long P, int C,
                                                                   int accumulate, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta) {
  __shared__ float sh[kGnFoldRows][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (j < 2 * C)
    for (long long p = q; p < P; p += kGnFoldRows) s += rows[p * 2 * C + j];
  sh[q][lane] = s;
  __syncthreads();
  if (q == 0 && j < 2 * C) {
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < kGnFoldRows; ++i) tot += sh[i][lane];
    float* o = j < C ? dgamma + j : dbeta + (j - C);
    *o = accumulate ? *o + tot : tot;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
struct GnPlan {
  GnGeom a;
  int block, vpt;       // resident: workgroup size and register vectors (1, 2, 4, 8); tiled: kGnBlock, 8
  int resident;
};

int gn_plan(const mxdet_gn_desc_t* d, const char* who, GnPlan* out) {
  MXDET_REQUIRE(d != nullptr, MXDET_EINVAL, "%s: null descriptor", who);
  MXDET_REQUIRE(d->N > 0 && d->HW > 0 && d->C > 0 && d->G > 0, MXDET_ESHAPE, "%s: N, HW, C, G must be positive (got %d, %d, %d, %d)",
                who, d->N, d->HW, d->C, d->G);
  MXDET_REQUIRE(d->C <= 1024, MXDET_ESHAPE, "%s: C = %d exceeds 1024", who, d->C);
  MXDET_REQUIRE(d->C % d->G == 0, MXDET_ESHAPE, "%s: C = %d is not a multiple of G = %d (C %% G != 0)", who, d->C, d->G);
  MXDET_REQUIRE((d->C / d->G) % 8 == 0, MXDET_ESHAPE, "%s: C / G = %d is not a multiple of 8", who, d->C / d->G);
  MXDET_REQUIRE((long long)d->HW * d->C < (1ll << 30) && (long long)d->N * d->G < (1ll << 31), MXDET_ESHAPE,
                "%s: tensor too large (one sample must stay under 2^30 elements, N * G under 2^31)", who);
  MXDET_REQUIRE(d->eps > 0.f, MXDET_EINVAL, "%s: eps must be positive", who);
  GnGeom& a = out->a;
  a.N = d->N; a.HW = d->HW; a.C = d->C; a.G = d->G;
  a.CV = d->C / 8;
  a.gv = d->C / d->G / 8;
  a.eps = d->eps;
  a.inv_m = 1.0f / ((float)d->HW * (float)(d->C / d->G));
  a.relu = d->relu ? 1 : 0;
  const int pr_small = kGnBlock / a.CV, pr_big = kGnBigBlock / a.CV;
  out->resident = ceil_div(d->HW, pr_big) <= kGnMaxVpt;
  int need;
  if (out->resident) {
    out->block = ceil_div(d->HW, pr_small) <= kGnMaxVpt ? kGnBlock : kGnBigBlock;
    a.PR = out->block / a.CV;
    need = ceil_div(d->HW, a.PR);
    a.chunks = 1;
    a.pc = d->HW;
  } else {
    out->block = kGnBlock;
    a.PR = pr_small;
    need = kGnMaxVpt;
    a.pc = a.PR * kGnMaxVpt;
    a.chunks = ceil_div(d->HW, a.pc);
    MXDET_REQUIRE(a.chunks <= 65535 * 32, MXDET_ESHAPE, "%s: HW = %d too large", who, d->HW);
  }
  a.Teff = a.PR * a.CV;
  out->vpt = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 8;
  return MXDET_OK;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct GnWs {
  size_t rows, gpart, gsum, stats, total;   // byte offsets (backward) / stats (forward)
};
GnWs gn_workspace(const GnPlan& p, int backward) {
  GnWs w = {0, 0, 0, 0, 0};
  const GnGeom& a = p.a;
  if (!backward) {
    w.total = p.resident ? 0 : align_up((size_t)a.N * a.chunks * a.G * 2 * sizeof(float), 256);
    return w;
  }
  size_t off = align_up((size_t)a.N * a.chunks * 2 * a.C * sizeof(float), 256);
  if (!p.resident) {
    w.gpart = off;
    off += align_up((size_t)a.N * a.chunks * a.G * 2 * sizeof(float), 256);
    w.gsum = off;
    off += align_up((size_t)a.N * a.G * 2 * sizeof(float), 256);
  }
  w.total = off;
  return w;
}

template <bool STATS_ONLY>
void launch_fwd(const GnPlan& p, hipStream_t s, const uint16_t* x, const float* gamma, const float* beta, uint16_t* y,
                float* mean, float* rstd, float* part) {
  const GnGeom& a = p.a;
  const dim3 grid(a.chunks, a.N < kGnGridY ? a.N : kGnGridY, ceil_div(a.N, kGnGridY)), block(p.block);
  const size_t lds = (size_t)(a.Teff + a.CV) * sizeof(float);
#define GN_FWD(V, TB) \
  hipLaunchKernelGGL((gn_fwd_kernel<V, STATS_ONLY, TB>), grid, block, lds, s, a, x, gamma, beta, y, mean, rstd, part)
  if (p.block == kGnBigBlock && !STATS_ONLY) {   // only samples past 8 vectors per thread of the small workgroup
    GN_FWD(8, kGnBigBlock);
    return;
  }
  switch (p.vpt) {
    case 1: GN_FWD(1, kGnBlock); break;
    case 2: GN_FWD(2, kGnBlock); break;
    case 4: GN_FWD(4, kGnBlock); break;
    default: GN_FWD(8, kGnBlock); break;
  }
#undef GN_FWD
}

template <int PHASE>
void launch_bwd(const GnPlan& p, hipStream_t s, const uint16_t* x, const uint16_t* dy, const uint16_t* y, const float* mean,
                const float* rstd, const float* gamma, const float* beta, uint16_t* dx, float* rows, float* gpart,
                const float* gsum) {
  const GnGeom& a = p.a;
  const dim3 grid(a.chunks, a.N < kGnGridY ? a.N : kGnGridY, ceil_div(a.N, kGnGridY)), block(p.block);
  const size_t lds = PHASE == 2 ? 0 : (size_t)(8 * a.Teff + 8 * a.CV) * sizeof(float);
#define GN_BWD(V, TB) \
  hipLaunchKernelGGL((gn_bwd_kernel<V, PHASE, TB>), grid, block, lds, s, a, x, dy, y, mean, rstd, gamma, beta, dx, rows, gpart, gsum)
  if (p.block == kGnBigBlock && PHASE == 0) {
    GN_BWD(8, kGnBigBlock);
    return;
  }
  switch (p.vpt) {
    case 1: GN_BWD(1, kGnBlock); break;
    case 2: GN_BWD(2, kGnBlock); break;
    case 4: GN_BWD(4, kGnBlock); break;
    default: GN_BWD(8, kGnBlock); break;
  }
#undef GN_BWD
}

}  // namespace
}  // namespace mxdet

using namespace mxdet;

extern "C" size_t mxdet_group_norm_workspace_bytes(const mxdet_gn_desc_t* d, int32_t backward) {
  GnPlan p;
  if (gn_plan(d, "group_norm_workspace_bytes", &p) != MXDET_OK) return 0;
  clear_error();
  return gn_workspace(p, backward).total;
}

extern "C" int mxdet_debug_group_norm_route(const mxdet_gn_desc_t* d) {
  clear_error();
  GnPlan p;
  const int rc = gn_plan(d, "debug_group_norm_route", &p);
  if (rc != MXDET_OK) return rc;
  return p.resident ? MXDET_GN_ROUTE_RESIDENT : MXDET_GN_ROUTE_TILED;
}

extern "C" int mxdet_group_norm_fwd(const mxdet_gn_desc_t* d, const uint16_t* x, const float* gamma, const float* beta,
                                    uint16_t* y, float* mean, float* rstd, void* workspace, size_t workspace_bytes,
                                    mxdet_stream_t stream) {
  clear_error();
  GnPlan p;
  const int rc = gn_plan(d, "group_norm_fwd", &p);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(x && gamma && beta && y && mean && rstd, MXDET_EINVAL, "group_norm_fwd: null pointer");
  MXDET_REQUIRE(aligned16(x) && aligned16(y) && aligned16(gamma) && aligned16(beta), MXDET_EINVAL,
                "group_norm_fwd: x, y, gamma and beta must be 16-byte aligned");
  const GnWs w = gn_workspace(p, 0);
  MXDET_REQUIRE(w.total == 0 || (workspace && workspace_bytes >= w.total), MXDET_EWORKSPACE,
                "group_norm_fwd: workspace %zu < %zu", workspace ? workspace_bytes : (size_t)0, w.total);
  hipStream_t s = as_stream(stream);
  if (p.resident) {
    launch_fwd<false>(p, s, x, gamma, beta, y, mean, rstd, nullptr);
  } else {
    float* part = (float*)workspace;
    launch_fwd<true>(p, s, x, gamma, beta, y, mean, rstd, part);
    const int waves = p.a.N * p.a.G;
    hipLaunchKernelGGL(gn_merge_stats_kernel, dim3(ceil_div(waves, kGnBlock / kWave)), dim3(kGnBlock), 0, s, p.a,
                       (const float*)part, mean, rstd);
    hipLaunchKernelGGL(gn_apply_kernel, dim3(p.a.chunks, p.a.N < kGnGridY ? p.a.N : kGnGridY, ceil_div(p.a.N, kGnGridY)), dim3(kGnBlock), 0, s, p.a, x, gamma, beta,
                       (const float*)mean, (const float*)rstd, y);
  }
  return check_launch("group_norm_fwd");
}

extern "C" int mxdet_group_norm_bwd(const mxdet_gn_desc_t* d, const uint16_t* x, const uint16_t* dy, const uint16_t* y,
                                    const float* mean, const float* rstd, const float* gamma, const float* beta,
                                    uint16_t* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                    mxdet_stream_t stream) {
  clear_error();
  GnPlan p;
  const int rc = gn_plan(d, "group_norm_bwd", &p);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(x && dy && mean && rstd && gamma && dx && dgamma && dbeta, MXDET_EINVAL, "group_norm_bwd: null pointer");
  MXDET_REQUIRE(!d->relu || y || beta, MXDET_EINVAL, "group_norm_bwd: null pointer (relu needs y, or beta to recompute it)");
  MXDET_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(y) && aligned16(dx), MXDET_EINVAL,
                "group_norm_bwd: x, dy, y and dx must be 16-byte aligned");
  const GnWs w = gn_workspace(p, 1);
  MXDET_REQUIRE(workspace && workspace_bytes >= w.total, MXDET_EWORKSPACE, "group_norm_bwd: workspace %zu < %zu",
                workspace ? workspace_bytes : (size_t)0, w.total);
  hipStream_t s = as_stream(stream);
  char* base = (char*)workspace;
  float* rows = (float*)(base + w.rows);
  if (p.resident) {
    launch_bwd<0>(p, s, x, dy, y, mean, rstd, gamma, beta, dx, rows, nullptr, nullptr);
  } else {
    float* gpart = (float*)(base + w.gpart);
    float* gsum = (float*)(base + w.gsum);
    launch_bwd<1>(p, s, x, dy, y, mean, rstd, gamma, beta, dx, rows, gpart, nullptr);
    const int waves = p.a.N * p.a.G;
    hipLaunchKernelGGL(gn_merge_sums_kernel, dim3(ceil_div(waves, kGnBlock / kWave)), dim3(kGnBlock), 0, s, p.a,
                       (const float*)gpart, gsum);
    launch_bwd<2>(p, s, x, dy, y, mean, rstd, gamma, beta, dx, nullptr, nullptr, gsum);
  }
  const long long P = (long long)p.a.N * p.a.chunks;
  hipLaunchKernelGGL(gn_fold_kernel, dim3(ceil_div(2 * p.a.C, 64)), dim3(kGnFoldRows * 64), 0, s, (const float*)rows, P,
                     p.a.C, d->accumulate ? 1 : 0, dgamma, dbeta);
  return check_launch("group_norm_bwd");
}
