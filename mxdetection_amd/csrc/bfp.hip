// bfp.hip -- Balanced Feature Pyramid (Libra R-CNN, Pang et al., CVPR 2019): the gather and scatter stages around the
// refine convolution, forward and backward (include/mxdet.h).
//
// Slot: models/necks (/root/reference/README.md:31). Four streaming kernels, one launch each for all pyramid levels: a
// thread owns eight channels of one pixel (one 16-byte load / store per operand), sums in fp32 in a fixed order and
// rounds once. The pool windows are a few pixels wide (4 x 4 for P2 -> P4, at most 5 x 5 where they overlap); their
// re-reads hit the caches, so the floor is the bytes of the pyramid: ~91 MB read by a gather, ~91 MB read and written by
// a scatter at the benchmark size. The backward kernels are exact adjoints in gather form: every thread sums the
// contributions to its own output, no atomics, the same bits on every run. The forward kernels store each pooled
// element's arg-maximum (one byte), so the backward ones read gradients only.
#include "common.h"

namespace mxdet {

constexpr int kBfpLevels = MXDET_BFP_MAX_LEVELS;
constexpr int kBfpThreads = 256;

struct BfpK {
  int L, r, N, C8;                       // C8 = C / 8: 16-byte vectors per pixel
  int H[kBfpLevels], W[kBfpLevels];
  const uint4* in[kBfpLevels];
  uint4* out[kBfpLevels];
  unsigned char* amax[kBfpLevels];       // l < r: gather's arg-maxima [N,h,w,C]; l > r: scatter's [N,H[l],W[l],C]
  long long nvec[kBfpLevels];            // N * H * W * C8 of the level
  int blk_off[kBfpLevels + 1];           // first workgroup of each level in the launches that cover the whole pyramid
};

// adaptive pool window of output o along an axis: [lo, hi)
__device__ __forceinline__ int pool_lo(int o, int in, int out) { return (o * in) / out; }
__device__ __forceinline__ int pool_hi(int o, int in, int out) { return ((o + 1) * in + out - 1) / out; }
// the outputs o0..o1 (inclusive) whose pool window holds input y
__device__ __forceinline__ void pool_cover(int y, int in, int out, int& o0, int& o1) {
  o0 = (y * out) / in;
  o1 = ((y + 1) * out + in - 1) / in - 1;
  if (o1 > out - 1) o1 = out - 1;
}
// nearest resize reads src = (dst * in) / out: the dsts [d0, d1) that read src y
__device__ __forceinline__ void near_cover(int y, int in, int out, int& d0, int& d1) {
  d0 = (y * out + in - 1) / in;
  d1 = ((y + 1) * out + in - 1) / in;
  if (d1 > out) d1 = out;
}

struct BfpPix { int n, y, x, c8; };
__device__ __forceinline__ BfpPix bfp_pixel(long long v, int H, int W, int C8) {
  BfpPix p;
  p.c8 = (int)(v % C8);
  long long t = v / C8;
  p.x = (int)(t % W);
  t /= W;
  p.y = (int)(t % H);
  p.n = (int)(t / H);
  return p;
}
__device__ __forceinline__ long long bfp_vec(int n, int y, int x, int c8, int H, int W, int C8) {
  return (((long long)n * H + y) * W + x) * C8 + c8;
}
// the level of this workgroup and the thread's vector inside it (-1: past the level's end)
__device__ __forceinline__ long long bfp_level_vec(const BfpK& k, int& l) {
  l = 0;
  while (l + 1 < k.L && (int)blockIdx.x >= k.blk_off[l + 1]) ++l;
  const long long v = (long long)((int)blockIdx.x - k.blk_off[l]) * kBfpThreads + threadIdx.x;
  return v < k.nvec[l] ? v : -1;
}

// maximum and arg-maximum (16 * dy + dx, first in row-major order on ties) of eight channels over a window of src
__device__ __forceinline__ void window_max8(const uint4* __restrict__ src, int n, int c8, int H, int W, int C8, int y0, int y1,
                                            int x0, int x1, float* best, unsigned* arg) {
#pragma unroll
  for (int j = 0; j < 8; ++j) { best[j] = -3.402823466e+38f; arg[j] = 0u; }
  bool first = true;
  for (int yy = y0; yy < y1; ++yy)
    for (int xx = x0; xx < x1; ++xx) {
      float v[8];
      unpack8_bf16(src[bfp_vec(n, yy, xx, c8, H, W, C8)], v);
      const unsigned code = (unsigned)((yy - y0) * 16 + (xx - x0));
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (first || v[j] > best[j]) { best[j] = v[j]; arg[j] = code; }
      first = false;
    }
}
__device__ __forceinline__ void store_arg8(unsigned char* amax, long long vec, const unsigned* a) {
  uint2 o;
  o.x = a[0] | (a[1] << 8) | (a[2] << 16) | (a[3] << 24);
  o.y = a[4] | (a[5] << 8) | (a[6] << 16) | (a[7] << 24);
  *(uint2*)(amax + vec * 8) = o;
}
__device__ __forceinline__ void load_arg8(const unsigned char* amax, long long vec, unsigned* a) {
  const uint2 o = *(const uint2*)(amax + vec * 8);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[j] = (o.x >> (8 * j)) & 255u;
    a[4 + j] = (o.y >> (8 * j)) & 255u;
  }
}

// B = bf16((((g_0 + g_1) + ...) + g_{L-1}) / L) on the refine level's grid
__global__ void __launch_bounds__(kBfpThreads)
bfp_gather_fwd_kernel(const BfpK k, uint4* __restrict__ B) {
  const int h = k.H[k.r], w = k.W[k.r];
  const long long v = (long long)blockIdx.x * kBfpThreads + threadIdx.x;
  if (v >= k.nvec[k.r]) return;
  const BfpPix p = bfp_pixel(v, h, w, k.C8);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int l = 0; l < k.L; ++l) {
    const int H = k.H[l], W = k.W[l];
    float g[8];
    if (l < k.r) {
      unsigned arg[8];
      window_max8(k.in[l], p.n, p.c8, H, W, k.C8, pool_lo(p.y, H, h), pool_hi(p.y, H, h), pool_lo(p.x, W, w),
                  pool_hi(p.x, W, w), g, arg);
      store_arg8(k.amax[l], v, arg);
    } else if (l == k.r) {
      unpack8_bf16(k.in[l][v], g);
    } else {
      unpack8_bf16(k.in[l][bfp_vec(p.n, (p.y * H) / h, (p.x * W) / w, p.c8, H, W, k.C8)], g);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = l == 0 ? g[j] : acc[j] + g[j];
  }
  const float Lf = (float)k.L;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = acc[j] / Lf;
  B[v] = pack8_bf16_hw(acc);
}

// Q_l = bf16(P_l + s_l), every level in one launch
__global__ void __launch_bounds__(kBfpThreads)
bfp_scatter_fwd_kernel(const BfpK k, const uint4* __restrict__ Rf) {
  int l;
  const long long v = bfp_level_vec(k, l);
  if (v < 0) return;
  const int h = k.H[k.r], w = k.W[k.r], H = k.H[l], W = k.W[l];
  const BfpPix p = bfp_pixel(v, H, W, k.C8);
  float s[8], x[8];
  if (l < k.r) {
    unpack8_bf16(Rf[bfp_vec(p.n, (p.y * h) / H, (p.x * w) / W, p.c8, h, w, k.C8)], s);
  } else if (l == k.r) {
    unpack8_bf16(Rf[v], s);
  } else {
    unsigned arg[8];
    window_max8(Rf, p.n, p.c8, h, w, k.C8, pool_lo(p.y, h, H), pool_hi(p.y, h, H), pool_lo(p.x, w, W), pool_hi(p.x, w, W), s,
                arg);
    store_arg8(k.amax[l], v, arg);
  }
  unpack8_bf16(k.in[l][v], x);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = x[j] + s[j];
  k.out[l][v] = pack8_bf16_hw(x);
}

// dRf = bf16(sum_l adj(s_l)(dQ_l)) on the refine level's grid
__global__ void __launch_bounds__(kBfpThreads)
bfp_scatter_bwd_kernel(const BfpK k, uint4* __restrict__ dRf) {
  const int h = k.H[k.r], w = k.W[k.r];
  const long long v = (long long)blockIdx.x * kBfpThreads + threadIdx.x;
  if (v >= k.nvec[k.r]) return;
  const BfpPix p = bfp_pixel(v, h, w, k.C8);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int l = 0; l < k.L; ++l) {
    const int H = k.H[l], W = k.W[l];
    float g[8];
    if (l < k.r) {                       // s_l = nearest resize of Rf: every pixel of the level that read (y, x)
      int y0, y1, x0, x1;
      near_cover(p.y, h, H, y0, y1);
      near_cover(p.x, w, W, x0, x1);
      for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
          unpack8_bf16(k.in[l][bfp_vec(p.n, yy, xx, p.c8, H, W, k.C8)], g);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += g[j];
        }
    } else if (l == k.r) {
      unpack8_bf16(k.in[l][v], g);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += g[j];
    } else {                             // s_l = max pool of Rf: the outputs whose maximum sits at (y, x)
      int y0, y1, x0, x1;
      pool_cover(p.y, h, H, y0, y1);
      pool_cover(p.x, w, W, x0, x1);
      for (int oy = y0; oy <= y1; ++oy)
        for (int ox = x0; ox <= x1; ++ox) {
          const long long o = bfp_vec(p.n, oy, ox, p.c8, H, W, k.C8);
          const unsigned code = (unsigned)((p.y - pool_lo(oy, h, H)) * 16 + (p.x - pool_lo(ox, w, W)));
          unsigned arg[8];
          load_arg8(k.amax[l], o, arg);
          unpack8_bf16(k.in[l][o], g);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (arg[j] == code) acc[j] += g[j];
        }
    }
  }
  dRf[v] = pack8_bf16_hw(acc);
}

// dP_l = bf16(dQ_l + adj(g_l)(dB / L)), every level in one launch; out[l] may be in[l]
__global__ void __launch_bounds__(kBfpThreads)
bfp_gather_bwd_kernel(const BfpK k, const uint4* __restrict__ dB) {
  int l;
  const long long v = bfp_level_vec(k, l);
  if (v < 0) return;
  const int h = k.H[k.r], w = k.W[k.r], H = k.H[l], W = k.W[l];
  const BfpPix p = bfp_pixel(v, H, W, k.C8);
  const float Lf = (float)k.L;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float g[8];
  if (l < k.r) {                         // g_l = max pool of P_l: the cells of B whose maximum sits at (y, x)
    int y0, y1, x0, x1;
    pool_cover(p.y, H, h, y0, y1);
    pool_cover(p.x, W, w, x0, x1);
    for (int oy = y0; oy <= y1; ++oy)
      for (int ox = x0; ox <= x1; ++ox) {
        const long long o = bfp_vec(p.n, oy, ox, p.c8, h, w, k.C8);
        const unsigned code = (unsigned)((p.y - pool_lo(oy, H, h)) * 16 + (p.x - pool_lo(ox, W, w)));
        unsigned arg[8];
        load_arg8(k.amax[l], o, arg);
        unpack8_bf16(dB[o], g);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (arg[j] == code) acc[j] += g[j] / Lf;
      }
  } else if (l == k.r) {
    unpack8_bf16(dB[v], g);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += g[j] / Lf;
  } else {                               // g_l = nearest resize of P_l: every cell of B that read (y, x)
    int y0, y1, x0, x1;
    near_cover(p.y, H, h, y0, y1);
    near_cover(p.x, W, w, x0, x1);
    for (int yy = y0; yy < y1; ++yy)
      for (int xx = x0; xx < x1; ++xx) {
        unpack8_bf16(dB[bfp_vec(p.n, yy, xx, p.c8, h, w, k.C8)], g);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += g[j] / Lf;
      }
  }
  unpack8_bf16(k.in[l][v], g);
#pragma unroll
  for (int j = 0; j < 8; ++j) g[j] = g[j] + acc[j];
  k.out[l][v] = pack8_bf16_hw(g);
}

// host: widest adaptive-pool window of an axis
static int max_window(int in, int out) {
  int m = 0;
  for (int o = 0; o < out; ++o) {
    const int lo = (int)(((long long)o * in) / out), hi = (int)((((long long)o + 1) * in + out - 1) / out);
    m = hi - lo > m ? hi - lo : m;
  }
  return m;
}

// The descriptor's checks, and the kernels' view of it with the workspace carved (base may be NULL: sizes only).
static int bfp_prepare(const char* entry, const mxdet_bfp_desc_t* d, void* base, bool need_out, BfpK* k, size_t* total) {
  MXDET_REQUIRE(d != nullptr, MXDET_EINVAL, "%s: null descriptor", entry);
  const int L = d->num_levels, r = d->refine_level;
  MXDET_REQUIRE(L >= 2 && L <= kBfpLevels, MXDET_ESHAPE, "%s: num_levels %d not in 2..%d", entry, L, kBfpLevels);
  MXDET_REQUIRE(r >= 0 && r < L, MXDET_ESHAPE, "%s: refine_level %d not in [0, %d)", entry, r, L);
  MXDET_REQUIRE(d->N > 0 && d->C > 0 && d->C % 8 == 0, MXDET_ESHAPE, "%s: N must be positive and C a positive multiple of 8",
                entry);
  for (int l = 0; l < L; ++l)
    MXDET_REQUIRE(d->H[l] > 0 && d->W[l] > 0 && d->H[l] <= 32768 && d->W[l] <= 32768, MXDET_ESHAPE,
                  "%s: level %d has size %d x %d", entry, l, d->H[l], d->W[l]);
  const int h = d->H[r], w = d->W[r];
  k->L = L; k->r = r; k->N = d->N; k->C8 = d->C / 8;
  size_t off = 0;
  long long blocks = 0;
  for (int l = 0; l < L; ++l) {
    const int H = d->H[l], W = d->W[l];
    // pooled: level l onto the refine grid (l < r), the refine grid onto level l (l > r)
    const int wy = l < r ? max_window(H, h) : (l > r ? max_window(h, H) : 1);
    const int wx = l < r ? max_window(W, w) : (l > r ? max_window(w, W) : 1);
    MXDET_REQUIRE(wy <= 16 && wx <= 16, MXDET_ESHAPE, "%s: level %d pools over a %d x %d window (at most 16 x 16)", entry, l,
                  wy, wx);
    const long long nvec = (long long)d->N * H * W * k->C8;
    MXDET_REQUIRE(nvec < (1ll << 31), MXDET_ESHAPE, "%s: level %d is too large", entry, l);
    k->H[l] = H; k->W[l] = W; k->nvec[l] = nvec;
    k->in[l] = (const uint4*)d->feat[l];
    k->out[l] = (uint4*)d->out[l];
    k->blk_off[l] = (int)blocks;
    blocks += (nvec + kBfpThreads - 1) / kBfpThreads;
    k->amax[l] = nullptr;
    if (l != r) {
      k->amax[l] = base ? (unsigned char*)base + off : nullptr;
      const size_t cells = l < r ? (size_t)d->N * h * w : (size_t)d->N * H * W;
      off = align_up(off + cells * d->C, 256);
    }
  }
  MXDET_REQUIRE(blocks < (1ll << 31), MXDET_ESHAPE, "%s: pyramid too large", entry);
  k->blk_off[L] = (int)blocks;
  for (int l = L; l < kBfpLevels; ++l) {
    k->H[l] = k->W[l] = 1; k->nvec[l] = 0; k->in[l] = nullptr; k->out[l] = nullptr; k->amax[l] = nullptr;
    k->blk_off[l + 1] = (int)blocks;
  }
  *total = off > 256 ? off : 256;
  if (base == nullptr) return MXDET_OK;      // sizes only
  for (int l = 0; l < L; ++l) {
    MXDET_REQUIRE(d->feat[l] != nullptr && (!need_out || d->out[l] != nullptr), MXDET_EINVAL, "%s: null level pointer", entry);
    MXDET_REQUIRE(((uintptr_t)d->feat[l] % 16) == 0 && (!need_out || ((uintptr_t)d->out[l] % 16) == 0), MXDET_EINVAL,
                  "%s: level pointers must be 16-byte aligned", entry);
  }
  return MXDET_OK;
}

static int bfp_entry(const char* entry, const mxdet_bfp_desc_t* d, const void* dense, const void* workspace,
                     size_t workspace_bytes, bool need_out, BfpK* k) {
  MXDET_REQUIRE(dense != nullptr && workspace != nullptr, MXDET_EINVAL, "%s: null pointer", entry);
  MXDET_REQUIRE(((uintptr_t)dense % 16) == 0 && ((uintptr_t)workspace % 16) == 0, MXDET_EINVAL,
                "%s: pointers must be 16-byte aligned", entry);
  size_t total = 0;
  const int rc = bfp_prepare(entry, d, const_cast<void*>(workspace), need_out, k, &total);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(workspace_bytes >= total, MXDET_EWORKSPACE, "%s: workspace %zu < %zu", entry, workspace_bytes, total);
  return MXDET_OK;
}

}  // namespace mxdet

using namespace mxdet;

extern "C" size_t mxdet_bfp_workspace_bytes(const mxdet_bfp_desc_t* d) {
  BfpK k;
  size_t total = 0;
  if (bfp_prepare("bfp_workspace_bytes", d, nullptr, false, &k, &total) != MXDET_OK) return 0;
  return total;
}

extern "C" int mxdet_bfp_gather_fwd(const mxdet_bfp_desc_t* d, uint16_t* B, void* workspace, size_t workspace_bytes,
                                    mxdet_stream_t stream) {
  clear_error();
  BfpK k;
  const int rc = bfp_entry("bfp_gather_fwd", d, B, workspace, workspace_bytes, false, &k);
  if (rc != MXDET_OK) return rc;
  const unsigned blocks = (unsigned)((k.nvec[k.r] + kBfpThreads - 1) / kBfpThreads);
  hipLaunchKernelGGL(bfp_gather_fwd_kernel, dim3(blocks), dim3(kBfpThreads), 0, as_stream(stream), k, (uint4*)B);
  return check_launch("bfp_gather_fwd");
}

extern "C" int mxdet_bfp_scatter_fwd(const mxdet_bfp_desc_t* d, const uint16_t* Rf, void* workspace, size_t workspace_bytes,
                                     mxdet_stream_t stream) {
  clear_error();
  BfpK k;
  const int rc = bfp_entry("bfp_scatter_fwd", d, Rf, workspace, workspace_bytes, true, &k);
  if (rc != MXDET_OK) return rc;
  hipLaunchKernelGGL(bfp_scatter_fwd_kernel, dim3((unsigned)k.blk_off[k.L]), dim3(kBfpThreads), 0, as_stream(stream), k,
                     (const uint4*)Rf);
  return check_launch("bfp_scatter_fwd");
}

extern "C" int mxdet_bfp_scatter_bwd(const mxdet_bfp_desc_t* d, uint16_t* dRf, const void* workspace, size_t workspace_bytes,
                                     mxdet_stream_t stream) {
  clear_error();
  BfpK k;
  const int rc = bfp_entry("bfp_scatter_bwd", d, dRf, workspace, workspace_bytes, false, &k);
  if (rc != MXDET_OK) return rc;
  const unsigned blocks = (unsigned)((k.nvec[k.r] + kBfpThreads - 1) / kBfpThreads);
  hipLaunchKernelGGL(bfp_scatter_bwd_kernel, dim3(blocks), dim3(kBfpThreads), 0, as_stream(stream), k, (uint4*)dRf);
  return check_launch("bfp_scatter_bwd");
}

extern "C" int mxdet_bfp_gather_bwd(const mxdet_bfp_desc_t* d, const uint16_t* dB, const void* workspace, size_t workspace_bytes,
                                    mxdet_stream_t stream) {
  clear_error();
  BfpK k;
  const int rc = bfp_entry("bfp_gather_bwd", d, dB, workspace, workspace_bytes, true, &k);
  if (rc != MXDET_OK) return rc;
  hipLaunchKernelGGL(bfp_gather_bwd_kernel, dim3((unsigned)k.blk_off[k.L]), dim3(kBfpThreads), 0, as_stream(stream), k,
                     (const uint4*)dB);
  return check_launch("bfp_gather_bwd");
}
