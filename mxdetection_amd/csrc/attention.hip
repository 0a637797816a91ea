// attention.hip -- batched single-head softmax attention over rows of a packed bf16 tensor, forward and backward
// (include/mxdet.h). The activation x activation products of Libra R-CNN's non-local refine.
//
// Slot: models/necks. Q, K and V are d-wide column slices of one [N, L, row_stride] tensor
// (what one 1x1 convolution C -> 3 Ci writes), so nothing is split or copied. The L x L matrix lives in accumulators and
// LDS only.
//
// Every product is mfma_f32_16x16x32_bf16, a wave owns 16 rows of its workgroup's block, and both operands come from one
// of two places: the wave's own rows sit in registers as A fragments for the whole kernel, the tiles it walks are
// staged in LDS ([64 rows][d + 8] bf16: the 16-byte pad spreads the rows over the banks). A tile is read as
//   frag_row: the reduction index runs along the tile's rows' columns (S = Q K^T, dP = dO V^T): one 16-byte read;
//   frag_col: the reduction index runs down the tile's rows (P V, P^T dO, dS^T Q, dS K): two ds_read_b64_tr_b16.
// The softmax factor (P, P^T, dS, dS^T) crosses LDS once per tile, rounded to bf16 there and nowhere else, into a
// region of the wave's own.
//
// forward    workgroup = 32 query rows, walks the key tiles: online softmax (running maximum m, running sum l kept per
//            lane and folded across the 16 lanes of a row once, at the end), O and LSE = m + ln l.
// backward   two sweeps, so that every output element is summed by ONE wave in a fixed order: no float atomics, no
//            hand-off between workgroups, the same bits on every run.
//              delta:  delta_i = sum_c dO_ic O_ic (fp32, workspace), on the MFMA chain of dP
//              dkv:    workgroup = 32 keys, walks the query tiles; S^T and dP^T with the key on the accumulator row, so
//                      dV += P^T dO and dK += dS^T Q accumulate in registers
//              dq:     workgroup = 32 query rows, walks the key tiles; dQ += dS K
//            S and dP are computed in both sweeps: seven products instead of five.
// The next tile's global loads are issued into registers before the current tile's products and written to LDS after
// them, so their latency sits under the MFMAs. One wave per SIMD at most is resident at the sizes this runs at, so a
// phase's fragment reads are all issued ahead of its first MFMA (sched_barrier): one exposed LDS latency per phase.
#include "common.h"

namespace mxdet {

constexpr int kAttnThreads = 128;        // two waves
constexpr int kAttnRows = 32;            // rows a workgroup owns: 16 per wave
constexpr int kAttnTile = 64;            // rows of a walked tile
constexpr int kAttnPS = kAttnTile + 8;   // row stride (elements) of a wave's [16][64] softmax-factor image

struct AttnK {
  const uint16_t* qkv;
  const uint16_t* out;      // O (backward: read)
  const uint16_t* d_out;
  uint16_t* o;              // O (forward: written)
  float* lse;
  float* delta;
  uint16_t* d_qkv;
  int N, L, rs, q_off, k_off, v_off;
  float scale;
};

typedef __attribute__((ext_vector_type(8))) short s16x8_t;

// operand fragment whose reduction index is contiguous in a tile row: rows r0 .. r0+15, reduction positions k0 .. k0+31
__device__ __forceinline__ bf16x8_t frag_row(const uint16_t* t, int stride, int r0, int k0, int lane) {
  return *(const bf16x8_t*)(t + (r0 + (lane & 15)) * stride + k0 + 8 * (lane >> 4));
}
// operand fragment whose reduction index is the tile row: rows k0 .. k0+31, columns c0 .. c0+15. Lane 16g + 4q + pp
// addresses row 8g + q (second read: + 4), columns 4pp .. 4pp+3, and receives column (lane & 15) of rows 8g .. 8g+7.
__device__ __forceinline__ bf16x8_t frag_col(const uint16_t* t, int stride, int k0, int c0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const uint16_t* a = t + (k0 + 8 * g + q) * stride + c0 + 4 * pp;
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)a);
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(a + 4 * stride));
  return __builtin_bit_cast(bf16x8_t, (s16x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
}
// one float -> bf16 by the hardware conversion (round to nearest even), as pack_bf16x2
__device__ __forceinline__ uint16_t bf16_hw(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }
// the maximum over the 16 lanes that share (lane >> 4), left in all of them: four DPP moves (quad_perm [1,0,3,2] and
// [2,3,0,1], row_half_mirror, row_mirror) instead of four ds_bpermute round trips
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_max(float x) {
  x = fmaxf(x, dpp_mov<0xB1>(x));
  x = fmaxf(x, dpp_mov<0x4E>(x));
  x = fmaxf(x, dpp_mov<0x141>(x));
  return fmaxf(x, dpp_mov<0x140>(x));
}
__device__ __forceinline__ f32x4_t mfma16(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// A [64][D] tile of rows row0 .. row0+63 of `src` (row stride `rs` elements; rows >= L read as zero): the workgroup's
// 128 threads hold it as NV 16-byte chunks each between tile_load and tile_store.
template <int D>
struct Tile {
  static constexpr int NV = kAttnTile * D / 8 / kAttnThreads;
  uint4 v[NV];
  __device__ __forceinline__ void load(const uint16_t* src, size_t rs, int row0, int L) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = threadIdx.x + kAttnThreads * i, row = c / (D / 8), ch = c % (D / 8);
      v[i] = row0 + row < L ? *(const uint4*)(src + (size_t)(row0 + row) * rs + ch * 8) : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  __device__ __forceinline__ void store(uint16_t* lds) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = threadIdx.x + kAttnThreads * i, row = c / (D / 8), ch = c % (D / 8);
      *(uint4*)(lds + row * (D + 8) + ch * 8) = v[i];
    }
  }
};

// the wave's own 16 rows (row0 .. row0+15) as A fragments, one per 32 columns; rows >= L are zero
template <int D>
__device__ __forceinline__ void own_rows(const uint16_t* src, size_t rs, int row0, int L, int lane, bf16x8_t (&f)[D / 32]) {
  const int row = row0 + (lane & 15);
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    const uint4 z = row < L ? *(const uint4*)(src + (size_t)row * rs + ks * 32 + 8 * (lane >> 4)) : make_uint4(0u, 0u, 0u, 0u);
    f[ks] = __builtin_bit_cast(bf16x8_t, z);
  }
}

// acc[nt] (16 rows x D columns, `mul` applied) -> bf16 rows row0 .. row0+31 of dst (row stride rs; rows >= L are not
// stored), through the [32][D + 8] image `img`: whole 16-byte chunks leave the workgroup. Contains __syncthreads.
template <int D>
__device__ __forceinline__ void store_rows(const f32x4_t (&acc)[D / 16], const float (&mul)[4], uint16_t* img, uint16_t* dst,
                                           size_t rs, int row0, int L, int w, int lane) {
  __syncthreads();                                   // every reader of the image's previous contents is done
#pragma unroll
  for (int nt = 0; nt < D / 16; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      img[(w * 16 + (lane >> 4) * 4 + r) * (D + 8) + nt * 16 + (lane & 15)] = bf16_hw(acc[nt][r] * mul[r]);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kAttnRows * D / 8 / kAttnThreads; ++i) {
    const int c = threadIdx.x + kAttnThreads * i, row = c / (D / 8), ch = c % (D / 8);
    if (row0 + row < L) *(uint4*)(dst + (size_t)(row0 + row) * rs + ch * 8) = *(const uint4*)(img + row * (D + 8) + ch * 8);
  }
}

template <int D>
__global__ void __launch_bounds__(kAttnThreads)
attn_fwd_kernel(const AttnK p) {
  constexpr int S = D + 8;
  __shared__ __attribute__((aligned(16))) uint16_t Ks[kAttnTile * S];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[kAttnTile * S];
  __shared__ __attribute__((aligned(16))) uint16_t Ps[2][16 * kAttnPS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = blockIdx.y, i0 = blockIdx.x * kAttnRows, L = p.L;
  const size_t rs = (size_t)p.rs;
  const uint16_t* base = p.qkv + (size_t)n * L * rs;
  bf16x8_t qf[D / 32];
  own_rows<D>(base + p.q_off, rs, i0 + w * 16, L, lane, qf);
  f32x4_t o[D / 16];
#pragma unroll
  for (int nt = 0; nt < D / 16; ++nt) o[nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  float m[4], l[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
  const int ntiles = (L + kAttnTile - 1) / kAttnTile;
  Tile<D> kt, vt;
  kt.load(base + p.k_off, rs, 0, L);
  vt.load(base + p.v_off, rs, 0, L);
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();                                 // the previous tile's reads are done
    kt.store(Ks);
    vt.store(Vs);
    __syncthreads();
    if (t + 1 < ntiles) {
      kt.load(base + p.k_off, rs, (t + 1) * kAttnTile, L);
      vt.load(base + p.v_off, rs, (t + 1) * kAttnTile, L);
    }
    // (a phase's fragment reads are all issued before its first MFMA: one exposed LDS latency per phase, not per MFMA)
    f32x4_t s[4];
    bf16x8_t kb[4][D / 32];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) kb[nt][ks] = frag_row(Ks, S, nt * 16, ks * 32, lane);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      s[nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) s[nt] = mfma16(qf[ks], kb[nt][ks], s[nt]);
      const bool valid = t * kAttnTile + nt * 16 + (lane & 15) < L;   // key columns >= L: out of the maximum and the sum
#pragma unroll
      for (int r = 0; r < 4; ++r) s[nt][r] = valid ? s[nt][r] * p.scale : -INFINITY;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mx = row16_max(fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r])));
      const float mn = fmaxf(m[r], mx);               // finite: every tile holds at least one key < L
      const float alpha = __expf(m[r] - mn);
      m[r] = mn;
      float sum = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float pv = __expf(s[nt][r] - mn);
        sum += pv;
        Ps[w][((lane >> 4) * 4 + r) * kAttnPS + nt * 16 + (lane & 15)] = bf16_hw(pv);
      }
      l[r] = l[r] * alpha + sum;
#pragma unroll
      for (int nt = 0; nt < D / 16; ++nt) o[nt][r] *= alpha;
    }
    __syncthreads();                                 // P is in LDS
#pragma unroll
    for (int ks = 0; ks < kAttnTile / 32; ++ks) {
      const bf16x8_t pf = frag_row(Ps[w], kAttnPS, 0, ks * 32, lane);
      bf16x8_t vb[D / 16];
#pragma unroll
      for (int nt = 0; nt < D / 16; ++nt) vb[nt] = frag_col(Vs, S, ks * 32, nt * 16, lane);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int nt = 0; nt < D / 16; ++nt) o[nt] = mfma16(pf, vb[nt], o[nt]);
    }
  }
  float inv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int sh = 1; sh < 16; sh <<= 1) l[r] += __shfl_xor(l[r], sh);
    inv[r] = 1.f / l[r];
    const int i = i0 + w * 16 + (lane >> 4) * 4 + r;
    if ((lane & 15) == 0 && i < L) p.lse[(size_t)n * L + i] = m[r] + __logf(l[r]);
  }
  store_rows<D>(o, inv, Ks, p.o + (size_t)n * L * D, (size_t)D, i0, L, w, lane);
}

// delta_i = sum_c dO_ic O_ic, 16 rows per wave: the diagonal of dO O^T on the MFMA chain (k order, zero start) that the
// sweeps' dP = dO V^T runs on, so where O_i equals V_j bit for bit (L = 1) dP_ij - delta_i is exactly zero
template <int D>
__global__ void __launch_bounds__(kAttnThreads)
attn_delta_kernel(const AttnK p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = blockIdx.y, row0 = blockIdx.x * kAttnRows + w * 16, L = p.L;
  bf16x8_t gf[D / 32], of[D / 32];
  own_rows<D>(p.d_out + (size_t)n * L * D, (size_t)D, row0, L, lane, gf);
  own_rows<D>(p.out + (size_t)n * L * D, (size_t)D, row0, L, lane, of);
  f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) acc = mfma16(gf[ks], of[ks], acc);
  const int i = row0 + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if ((lane >> 4) * 4 + r == (lane & 15) && i < L) p.delta[(size_t)n * L + i] = acc[r];
}

template <int D>
__global__ void __launch_bounds__(kAttnThreads)
attn_bwd_dkv_kernel(const AttnK p) {
  constexpr int S = D + 8;
  __shared__ __attribute__((aligned(16))) uint16_t Qs[kAttnTile * S];
  __shared__ __attribute__((aligned(16))) uint16_t Gs[kAttnTile * S];          // dO
  __shared__ __attribute__((aligned(16))) uint16_t Pt[2][16 * kAttnPS];        // P^T  [key][query]
  __shared__ __attribute__((aligned(16))) uint16_t St[2][16 * kAttnPS];        // dS^T [key][query]
  __shared__ float lse_s[kAttnTile], delta_s[kAttnTile];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = blockIdx.y, j0 = blockIdx.x * kAttnRows, L = p.L;
  const size_t rs = (size_t)p.rs;
  const uint16_t* base = p.qkv + (size_t)n * L * rs;
  const uint16_t* gbase = p.d_out + (size_t)n * L * D;
  bf16x8_t kf[D / 32], vf[D / 32];
  own_rows<D>(base + p.k_off, rs, j0 + w * 16, L, lane, kf);
  own_rows<D>(base + p.v_off, rs, j0 + w * 16, L, lane, vf);
  f32x4_t dk[D / 16], dv[D / 16];
#pragma unroll
  for (int nt = 0; nt < D / 16; ++nt) dk[nt] = dv[nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (L + kAttnTile - 1) / kAttnTile;
  Tile<D> qt, gt;
  float lse_r = 0.f, delta_r = 0.f;                  // threads 0 .. 63: the tile's row constants
  auto load_consts = [&](int row0) {
    const int i = row0 + (int)threadIdx.x;
    const bool ok = threadIdx.x < kAttnTile && i < L;
    lse_r = ok ? p.lse[(size_t)n * L + i] : 0.f;
    delta_r = ok ? p.delta[(size_t)n * L + i] : 0.f;
  };
  qt.load(base + p.q_off, rs, 0, L);
  gt.load(gbase, (size_t)D, 0, L);
  load_consts(0);
  for (int t = 0; t < ntiles; ++t) {
    const int i0 = t * kAttnTile;
    __syncthreads();
    qt.store(Qs);
    gt.store(Gs);
    if (threadIdx.x < kAttnTile) { lse_s[threadIdx.x] = lse_r; delta_s[threadIdx.x] = delta_r; }
    __syncthreads();
    if (t + 1 < ntiles) {
      qt.load(base + p.q_off, rs, i0 + kAttnTile, L);
      gt.load(gbase, (size_t)D, i0 + kAttnTile, L);
      load_consts(i0 + kAttnTile);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {                 // 16 queries: S^T and dP^T, key on the accumulator row
      f32x4_t st = (f32x4_t){0.f, 0.f, 0.f, 0.f}, dpt = (f32x4_t){0.f, 0.f, 0.f, 0.f};
      bf16x8_t qb[D / 32], gb[D / 32];
#pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) {
        qb[ks] = frag_row(Qs, S, nt * 16, ks * 32, lane);
        gb[ks] = frag_row(Gs, S, nt * 16, ks * 32, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) {
        st = mfma16(kf[ks], qb[ks], st);
        dpt = mfma16(vf[ks], gb[ks], dpt);
      }
      const int iq = nt * 16 + (lane & 15);
      const float lse = lse_s[iq], delta = delta_s[iq];
      const bool qok = i0 + iq < L;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kr = (lane >> 4) * 4 + r;
        const bool ok = qok && j0 + w * 16 + kr < L;
        const float pv = ok ? __expf(st[r] * p.scale - lse) : 0.f;
        Pt[w][kr * kAttnPS + iq] = bf16_hw(pv);
        St[w][kr * kAttnPS + iq] = bf16_hw(pv * (dpt[r] - delta));
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kAttnTile / 32; ++ks) {
      const bf16x8_t pf = frag_row(Pt[w], kAttnPS, 0, ks * 32, lane), sf = frag_row(St[w], kAttnPS, 0, ks * 32, lane);
#pragma unroll
      for (int n4 = 0; n4 < D / 16; n4 += 4) {
        bf16x8_t gb[4], qb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          gb[j] = frag_col(Gs, S, ks * 32, (n4 + j) * 16, lane);
          qb[j] = frag_col(Qs, S, ks * 32, (n4 + j) * 16, lane);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dv[n4 + j] = mfma16(pf, gb[j], dv[n4 + j]);
          dk[n4 + j] = mfma16(sf, qb[j], dk[n4 + j]);
        }
      }
    }
  }
  uint16_t* dbase = p.d_qkv + (size_t)n * L * rs;
  const float sc[4] = {p.scale, p.scale, p.scale, p.scale}, one[4] = {1.f, 1.f, 1.f, 1.f};
  store_rows<D>(dk, sc, Qs, dbase + p.k_off, rs, j0, L, w, lane);
  store_rows<D>(dv, one, Gs, dbase + p.v_off, rs, j0, L, w, lane);
}

template <int D>
__global__ void __launch_bounds__(kAttnThreads)
attn_bwd_dq_kernel(const AttnK p) {
  constexpr int S = D + 8;
  __shared__ __attribute__((aligned(16))) uint16_t Ks[kAttnTile * S];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[kAttnTile * S];
  __shared__ __attribute__((aligned(16))) uint16_t Ss[2][16 * kAttnPS];        // dS [query][key]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = blockIdx.y, i0 = blockIdx.x * kAttnRows, L = p.L;
  const size_t rs = (size_t)p.rs;
  const uint16_t* base = p.qkv + (size_t)n * L * rs;
  bf16x8_t qf[D / 32], gf[D / 32];
  own_rows<D>(base + p.q_off, rs, i0 + w * 16, L, lane, qf);
  own_rows<D>(p.d_out + (size_t)n * L * D, (size_t)D, i0 + w * 16, L, lane, gf);
  float lse[4], delta[4];
  bool qok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + w * 16 + (lane >> 4) * 4 + r;
    qok[r] = i < L;
    lse[r] = qok[r] ? p.lse[(size_t)n * L + i] : 0.f;
    delta[r] = qok[r] ? p.delta[(size_t)n * L + i] : 0.f;
  }
  f32x4_t dq[D / 16];
#pragma unroll
  for (int nt = 0; nt < D / 16; ++nt) dq[nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (L + kAttnTile - 1) / kAttnTile;
  Tile<D> kt, vt;
  kt.load(base + p.k_off, rs, 0, L);
  vt.load(base + p.v_off, rs, 0, L);
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();
    kt.store(Ks);
    vt.store(Vs);
    __syncthreads();
    if (t + 1 < ntiles) {
      kt.load(base + p.k_off, rs, (t + 1) * kAttnTile, L);
      vt.load(base + p.v_off, rs, (t + 1) * kAttnTile, L);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      f32x4_t s = (f32x4_t){0.f, 0.f, 0.f, 0.f}, dp = (f32x4_t){0.f, 0.f, 0.f, 0.f};
      bf16x8_t kb[D / 32], vb[D / 32];
#pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) {
        kb[ks] = frag_row(Ks, S, nt * 16, ks * 32, lane);
        vb[ks] = frag_row(Vs, S, nt * 16, ks * 32, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) {
        s = mfma16(qf[ks], kb[ks], s);
        dp = mfma16(gf[ks], vb[ks], dp);
      }
      const bool kok = t * kAttnTile + nt * 16 + (lane & 15) < L;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = kok && qok[r] ? __expf(s[r] * p.scale - lse[r]) : 0.f;
        Ss[w][((lane >> 4) * 4 + r) * kAttnPS + nt * 16 + (lane & 15)] = bf16_hw(pv * (dp[r] - delta[r]));
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kAttnTile / 32; ++ks) {
      const bf16x8_t sf = frag_row(Ss[w], kAttnPS, 0, ks * 32, lane);
      bf16x8_t kb[D / 16];
#pragma unroll
      for (int nt = 0; nt < D / 16; ++nt) kb[nt] = frag_col(Ks, S, ks * 32, nt * 16, lane);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int nt = 0; nt < D / 16; ++nt) dq[nt] = mfma16(sf, kb[nt], dq[nt]);
    }
  }
  const float sc[4] = {p.scale, p.scale, p.scale, p.scale};
  store_rows<D>(dq, sc, Ks, p.d_qkv + (size_t)n * L * rs + p.q_off, rs, i0, L, w, lane);
}

constexpr int kAttnMaxL = 65536, kAttnMaxN = 65535;

// The descriptor's checks (before any launch), the kernels' view of it and the workspace size.
static int attn_prepare(const char* entry, const mxdet_attn_desc_t* d, AttnK* k, size_t* workspace_bytes) {
  MXDET_REQUIRE(d != nullptr, MXDET_EINVAL, "%s: null descriptor", entry);
  MXDET_REQUIRE(d->d == 64 || d->d == 128, MXDET_ESHAPE, "%s: d = %d is not supported (64 or 128)", entry, d->d);
  MXDET_REQUIRE(d->N >= 1 && d->N <= kAttnMaxN, MXDET_ESHAPE, "%s: N = %d not in 1..%d", entry, d->N, kAttnMaxN);
  MXDET_REQUIRE(d->L >= 1 && d->L <= kAttnMaxL, MXDET_ESHAPE, "%s: L = %d not in 1..%d", entry, d->L, kAttnMaxL);
  MXDET_REQUIRE(d->row_stride > 0 && d->row_stride % 8 == 0, MXDET_ESHAPE, "%s: row_stride %d is no positive multiple of 8",
                entry, d->row_stride);
  const int off[3] = {d->q_off, d->k_off, d->v_off};
  const char* name[3] = {"q_off", "k_off", "v_off"};
  for (int i = 0; i < 3; ++i) {
    MXDET_REQUIRE(off[i] >= 0 && off[i] % 8 == 0, MXDET_ESHAPE, "%s: %s %d is no non-negative multiple of 8", entry, name[i],
                  off[i]);
    MXDET_REQUIRE((long long)off[i] + d->d <= d->row_stride, MXDET_ESHAPE, "%s: %s + d = %d exceeds row_stride %d", entry,
                  name[i], off[i] + d->d, d->row_stride);
  }
  MXDET_REQUIRE(d->scale > 0.f && d->scale < INFINITY, MXDET_EINVAL, "%s: scale must be positive and finite", entry);
  k->N = d->N; k->L = d->L; k->rs = d->row_stride;
  k->q_off = d->q_off; k->k_off = d->k_off; k->v_off = d->v_off;
  k->scale = d->scale;
  *workspace_bytes = align_up((size_t)d->N * d->L * sizeof(float), 256);
  return MXDET_OK;
}

static bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace mxdet

using namespace mxdet;

extern "C" size_t mxdet_attention_workspace_bytes(const mxdet_attn_desc_t* d) {
  AttnK k;
  size_t total = 0;
  if (attn_prepare("attention_workspace_bytes", d, &k, &total) != MXDET_OK) return 0;
  return total;
}

extern "C" int mxdet_attention_fwd(const mxdet_attn_desc_t* d, const uint16_t* qkv, uint16_t* out, float* lse,
                                   mxdet_stream_t stream) {
  clear_error();
  AttnK k = {};
  size_t total = 0;
  const int rc = attn_prepare("attention_fwd", d, &k, &total);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(qkv != nullptr && out != nullptr && lse != nullptr, MXDET_EINVAL, "attention_fwd: null pointer");
  MXDET_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(lse), MXDET_EINVAL,
                "attention_fwd: pointers must be 16-byte aligned");
  k.qkv = qkv; k.o = out; k.lse = lse;
  const dim3 grid((unsigned)ceil_div(d->L, kAttnRows), (unsigned)d->N);
  if (d->d == 64)
    hipLaunchKernelGGL(attn_fwd_kernel<64>, grid, dim3(kAttnThreads), 0, as_stream(stream), k);
  else
    hipLaunchKernelGGL(attn_fwd_kernel<128>, grid, dim3(kAttnThreads), 0, as_stream(stream), k);
  return check_launch("attention_fwd");
}

extern "C" int mxdet_attention_bwd(const mxdet_attn_desc_t* d, const uint16_t* qkv, const uint16_t* out, const uint16_t* d_out,
                                   const float* lse, uint16_t* d_qkv, void* workspace, size_t workspace_bytes,
                                   mxdet_stream_t stream) {
  clear_error();
  AttnK k = {};
  size_t total = 0;
  const int rc = attn_prepare("attention_bwd", d, &k, &total);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(qkv != nullptr && out != nullptr && d_out != nullptr && lse != nullptr && d_qkv != nullptr &&
                    workspace != nullptr, MXDET_EINVAL, "attention_bwd: null pointer");
  MXDET_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(d_out) && aligned16(lse) && aligned16(d_qkv) &&
                    aligned16(workspace), MXDET_EINVAL, "attention_bwd: pointers must be 16-byte aligned");
  MXDET_REQUIRE(workspace_bytes >= total, MXDET_EWORKSPACE, "attention_bwd: workspace %zu < %zu", workspace_bytes, total);
  k.qkv = qkv; k.out = out; k.d_out = d_out; k.lse = const_cast<float*>(lse); k.d_qkv = d_qkv;
  k.delta = (float*)workspace;
  const hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)ceil_div(d->L, kAttnRows), (unsigned)d->N);
  if (d->d == 64) {
    hipLaunchKernelGGL(attn_delta_kernel<64>, grid, dim3(kAttnThreads), 0, s, k);
    hipLaunchKernelGGL(attn_bwd_dkv_kernel<64>, grid, dim3(kAttnThreads), 0, s, k);
    hipLaunchKernelGGL(attn_bwd_dq_kernel<64>, grid, dim3(kAttnThreads), 0, s, k);
  } else {
    hipLaunchKernelGGL(attn_delta_kernel<128>, grid, dim3(kAttnThreads), 0, s, k);
    hipLaunchKernelGGL(attn_bwd_dkv_kernel<128>, grid, dim3(kAttnThreads), 0, s, k);
    hipLaunchKernelGGL(attn_bwd_dq_kernel<128>, grid, dim3(kAttnThreads), 0, s, k);
  }
  return check_launch("attention_bwd");
}
