// carafe.hip -- CARAFE upsampling (Wang et al., "Content-Aware ReAssembly of FEatures", ICCV 2019), factor 2, reassembly
// kernel K in {3, 5}: the FPN's learned top-down upsample, forward and backward (include/mxdet.h).
//
// Slot: models/necks (/root/reference/README.md:31). Channels-last bf16 like everything else; a thread owns eight channels
// of a pixel (one 16-byte access per operand), sums in fp32 in a fixed order and rounds once. A source pixel q owns the
// 2 x 2 output pixels (2q + s), s = 2 sy + sx, and 4 K^2 logits M[q, t * 4 + s]; w = softmax over the K^2 taps t.
//   forward   a workgroup stages an 8 x 8 source tile plus halo of a 64-channel slice in LDS once, and the 4 K^2 weights
//             of its 64 source pixels (one thread per (pixel, sub-position) computes them, all channel threads read them);
//             a thread then reads each of the K^2 neighbours ONCE for all four sub-positions (32 accumulators).
//   dM        thread = (source pixel, one of 4 channel lanes): 4 K^2 fp32 dot products over the lane's channels, read
//             straight from memory (K^2 + 4 vectors per 32 K^2 multiply-adds: nothing to gain from staging), folded over
//             the 4 lanes by a butterfly (a fixed order), then lane s finishes sub-position s with the softmax Jacobian.
//   dX        gather form: the weights of the tile's (8 + 2r)^2 neighbourhood are computed once per workgroup into LDS and
//             reused over every channel slice; each thread sums the <= 4 K^2 contributions to its own pixel in row-major
//             order. No atomics anywhere: the same bits on every run.
// The backward recomputes the weights from M with the forward's function (carafe_weights: the one softmax of this file).
// Out-of-map neighbours, cropped output pixels and tile overhang are predicates: no address outside a tensor is formed.
#include "common.h"

namespace mxdet {

constexpr int kCarTile = 8;              // source pixels per tile side
constexpr int kCarThreads = 256;
constexpr int kCarSlice8 = 8;            // 16-byte vectors (64 channels) of a forward workgroup's channel slice

struct CarafeK {
  int N, H, W, C8, Cm, Hf, Wf;           // C8 = C / 8
  int tiles_x, tiles_y;
};

struct CarTile { int n, y0, x0; };
__device__ __forceinline__ CarTile carafe_tile(const CarafeK& k) {
  CarTile t;
  int b = (int)blockIdx.x;
  t.x0 = (b % k.tiles_x) * kCarTile;
  b /= k.tiles_x;
  t.y0 = (b % k.tiles_y) * kCarTile;
  t.n = b / k.tiles_y;
  return t;
}
__device__ __forceinline__ long long car_pix(int n, int y, int x, int H, int W) { return ((long long)n * H + y) * W + x; }

// w[t] = softmax over the K^2 taps of the logits m[4 t] (m points at channel s of a source pixel): fp32, max-subtracted
template <int K>
__device__ __forceinline__ void carafe_weights(const uint16_t* __restrict__ m, float* w) {
  constexpr int T = K * K;
  float mx = -3.402823466e+38f;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    w[t] = bf16_bits_to_f32(m[4 * t]);
    mx = fmaxf(mx, w[t]);
  }
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    w[t] = __expf(w[t] - mx);
    sum += w[t];
  }
  const float inv = 1.0f / sum;
#pragma unroll
  for (int t = 0; t < T; ++t) w[t] *= inv;
}

__device__ __forceinline__ uint16_t car_bf16(float v) { return (uint16_t)(pack_bf16x2(v, 0.f) & 0xffffu); }

// Y[n, 2q + s, c] = bf16(sum_t w[q, s, t] X[n, q + t - r, c]); grid = (N * tiles, channel slices)
template <int K>
__global__ void __launch_bounds__(kCarThreads)
carafe_fwd_kernel(const CarafeK k, const uint4* __restrict__ X, const uint16_t* __restrict__ M, uint4* __restrict__ Y) {
  constexpr int R = K / 2, T = K * K, HT = kCarTile + 2 * R;
  __shared__ uint4 xs[HT * HT * kCarSlice8];
  __shared__ float ws[kCarTile * kCarTile * T * 4];    // [pixel][tap][sub-position]
  const CarTile tile = carafe_tile(k);
  const int tid = (int)threadIdx.x;
  const int c8_0 = (int)blockIdx.y * kCarSlice8;
  for (int i = tid; i < HT * HT * kCarSlice8; i += kCarThreads) {
    const int pix = i >> 3, c8 = c8_0 + (i & 7);
    const int y = tile.y0 + pix / HT - R, x = tile.x0 + pix % HT - R;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (y >= 0 && y < k.H && x >= 0 && x < k.W && c8 < k.C8) v = X[car_pix(tile.n, y, x, k.H, k.W) * k.C8 + c8];
    xs[i] = v;
  }
  {
    const int p = tid >> 2, s = tid & 3;
    const int qy = tile.y0 + (p >> 3), qx = tile.x0 + (p & 7);
    if (qy < k.H && qx < k.W) {
      float w[T];
      carafe_weights<K>(M + car_pix(tile.n, qy, qx, k.H, k.W) * k.Cm + s, w);
#pragma unroll
      for (int t = 0; t < T; ++t) ws[(p * T + t) * 4 + s] = w[t];
    }
  }
  __syncthreads();
  const int v = tid & 7, c8 = c8_0 + v;
  if (c8 >= k.C8) return;
  for (int h = 0; h < 2; ++h) {
    const int p = (tid >> 3) + 32 * h, py = p >> 3, px = p & 7;
    const int qy = tile.y0 + py, qx = tile.x0 + px;
    if (qy >= k.H || qx >= k.W) continue;
    float acc[4][8];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[s][j] = 0.f;
#pragma unroll 1
    for (int a = 0; a < K; ++a)
#pragma unroll
      for (int b = 0; b < K; ++b) {
        float x[8];
        unpack8_bf16(xs[((py + a) * HT + px + b) * kCarSlice8 + v], x);
        const float4 wv = *(const float4*)&ws[(p * T + a * K + b) * 4];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          acc[0][j] += wv.x * x[j];
          acc[1][j] += wv.y * x[j];
          acc[2][j] += wv.z * x[j];
          acc[3][j] += wv.w * x[j];
        }
      }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int oy = 2 * qy + (s >> 1), ox = 2 * qx + (s & 1);
      if (oy < k.Hf && ox < k.Wf) Y[car_pix(tile.n, oy, ox, k.Hf, k.Wf) * k.C8 + c8] = pack8_bf16_hw(acc[s]);
    }
  }
}

// dM[n, q, t * 4 + s] = bf16(w_t (g_t - sum_u w_u g_u)), g_t = sum_c dY[n, 2q + s, c] X[n, q + t - r, c]; 0 for cropped
// sub-positions and in the padding channels; grid = N * tiles
template <int K>
__global__ void __launch_bounds__(kCarThreads)
carafe_bwd_m_kernel(const CarafeK k, const uint4* __restrict__ X, const uint16_t* __restrict__ M,
                    const uint4* __restrict__ dY, uint16_t* __restrict__ dM) {
  constexpr int R = K / 2, T = K * K;
  const CarTile tile = carafe_tile(k);
  const int tid = (int)threadIdx.x, p = tid >> 2, lane = tid & 3;
  const int qy = tile.y0 + (p >> 3), qx = tile.x0 + (p & 7);
  const bool live = qy < k.H && qx < k.W;
  bool valid[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) valid[s] = live && 2 * qy + (s >> 1) < k.Hf && 2 * qx + (s & 1) < k.Wf;
  float g[4][T];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int t = 0; t < T; ++t) g[s][t] = 0.f;
  if (live)
    for (int c8 = lane; c8 < k.C8; c8 += 4) {
      float d[4][8];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (valid[s]) v = dY[car_pix(tile.n, 2 * qy + (s >> 1), 2 * qx + (s & 1), k.Hf, k.Wf) * k.C8 + c8];
        unpack8_bf16(v, d[s]);
      }
#pragma unroll
      for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = 0; b < K; ++b) {
          const int y = qy + a - R, x = qx + b - R;
          if (y < 0 || y >= k.H || x < 0 || x >= k.W) continue;
          float xv[8];
          unpack8_bf16(X[car_pix(tile.n, y, x, k.H, k.W) * k.C8 + c8], xv);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) dot += d[s][j] * xv[j];
            g[s][a * K + b] += dot;
          }
        }
    }
  // fold the four channel lanes of the pixel: a butterfly, the same bits in every lane; then lane s keeps sub-position s
  float gs[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      g[s][t] += __shfl_xor(g[s][t], 1);
      g[s][t] += __shfl_xor(g[s][t], 2);
    }
    gs[t] = lane == 0 ? g[0][t] : (lane == 1 ? g[1][t] : (lane == 2 ? g[2][t] : g[3][t]));
  }
  if (!live) return;
  uint16_t* out = dM + car_pix(tile.n, qy, qx, k.H, k.W) * k.Cm;
  const bool mine = lane == 0 ? valid[0] : (lane == 1 ? valid[1] : (lane == 2 ? valid[2] : valid[3]));
  if (mine) {
    float w[T];
    carafe_weights<K>(M + car_pix(tile.n, qy, qx, k.H, k.W) * k.Cm + lane, w);
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) dot += w[t] * gs[t];
#pragma unroll
    for (int t = 0; t < T; ++t) out[4 * t + lane] = car_bf16(w[t] * (gs[t] - dot));
  } else {
#pragma unroll
    for (int t = 0; t < T; ++t) out[4 * t + lane] = 0;
  }
  for (int c = 4 * T + lane; c < k.Cm; c += 4) out[c] = 0;
}

// dX[n, p, c] (+)= sum over q within r of p and the sub-positions s inside Hf x Wf of w[q, s, t(p - q)] dY[n, 2q + s, c];
// grid = N * tiles
template <int K>
__global__ void __launch_bounds__(kCarThreads)
carafe_bwd_x_kernel(const CarafeK k, const uint16_t* __restrict__ M, const uint4* __restrict__ dY, uint4* __restrict__ dX,
                    const int accumulate) {
  constexpr int R = K / 2, T = K * K, HT = kCarTile + 2 * R;
  __shared__ float ws[HT * HT * T * 4];                // [neighbourhood pixel][tap][sub-position]
  const CarTile tile = carafe_tile(k);
  const int tid = (int)threadIdx.x;
  for (int i = tid; i < HT * HT * 4; i += kCarThreads) {
    const int qi = i >> 2, s = i & 3;
    const int qy = tile.y0 + qi / HT - R, qx = tile.x0 + qi % HT - R;
    if (qy >= 0 && qy < k.H && qx >= 0 && qx < k.W) {
      float w[T];
      carafe_weights<K>(M + car_pix(tile.n, qy, qx, k.H, k.W) * k.Cm + s, w);
#pragma unroll
      for (int t = 0; t < T; ++t) ws[(qi * T + t) * 4 + s] = w[t];
    }
  }
  __syncthreads();
  const int v = tid & 7;
  for (int h = 0; h < 2; ++h) {
    const int p = (tid >> 3) + 32 * h, py = p >> 3, px = p & 7;
    const int Py = tile.y0 + py, Px = tile.x0 + px;
    if (Py >= k.H || Px >= k.W) continue;
    for (int c8 = v; c8 < k.C8; c8 += 8) {
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
      for (int dy = 0; dy < K; ++dy)
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
          const int qy = Py + dy - R, qx = Px + dx - R;
          if (qy < 0 || qy >= k.H || qx < 0 || qx >= k.W) continue;
          // p = q + (a - r, b - r): a = K - 1 - dy, b = K - 1 - dx
          const float4 wv = *(const float4*)&ws[(((py + dy) * HT + px + dx) * T + (K - 1 - dy) * K + (K - 1 - dx)) * 4];
          const float w4[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int oy = 2 * qy + (s >> 1), ox = 2 * qx + (s & 1);
            if (oy < k.Hf && ox < k.Wf) {
              float d[8];
              unpack8_bf16(dY[car_pix(tile.n, oy, ox, k.Hf, k.Wf) * k.C8 + c8], d);
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[j] += w4[s] * d[j];
            }
          }
        }
      const long long o = car_pix(tile.n, Py, Px, k.H, k.W) * k.C8 + c8;
      if (accumulate) {
        float old[8];
        unpack8_bf16(dX[o], old);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = old[j] + acc[j];
      }
      dX[o] = pack8_bf16_hw(acc);
    }
  }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// The descriptor's checks and the kernels' view of it.
static int carafe_prepare(const char* entry, const mxdet_carafe_desc_t* d, CarafeK* k) {
  MXDET_REQUIRE(d != nullptr, MXDET_EINVAL, "%s: null descriptor", entry);
  MXDET_REQUIRE(d->k == 3 || d->k == 5, MXDET_ESHAPE, "%s: k %d must be 3 or 5", entry, d->k);
  MXDET_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->H <= 32768 && d->W <= 32768, MXDET_ESHAPE,
                "%s: N, H, W = %d, %d, %d must be positive (H, W at most 32768)", entry, d->N, d->H, d->W);
  MXDET_REQUIRE(d->C > 0 && d->C % 8 == 0, MXDET_ESHAPE, "%s: C %d must be a positive multiple of 8", entry, d->C);
  MXDET_REQUIRE(d->Cm >= 4 * d->k * d->k, MXDET_ESHAPE, "%s: Cm %d holds fewer than 4 k^2 = %d logits", entry, d->Cm,
                4 * d->k * d->k);
  MXDET_REQUIRE(d->Hf == 2 * d->H || d->Hf == 2 * d->H - 1, MXDET_ESHAPE, "%s: Hf %d must be 2 H or 2 H - 1 (H = %d)", entry,
                d->Hf, d->H);
  MXDET_REQUIRE(d->Wf == 2 * d->W || d->Wf == 2 * d->W - 1, MXDET_ESHAPE, "%s: Wf %d must be 2 W or 2 W - 1 (W = %d)", entry,
                d->Wf, d->W);
  const long long tx = ceil_div(d->W, kCarTile), ty = ceil_div(d->H, kCarTile);
  MXDET_REQUIRE(4ll * d->N * d->H * d->W * (d->C / 8) < (1ll << 31) && (long long)d->N * d->H * d->W * d->Cm < (1ll << 31) &&
                    d->N * tx * ty < (1ll << 31) && ceil_div(d->C / 8, kCarSlice8) <= 65535,
                MXDET_ESHAPE, "%s: tensors too large", entry);
  k->N = d->N; k->H = d->H; k->W = d->W; k->C8 = d->C / 8; k->Cm = d->Cm; k->Hf = d->Hf; k->Wf = d->Wf;
  k->tiles_x = (int)tx; k->tiles_y = (int)ty;
  return MXDET_OK;
}

}  // namespace mxdet

using namespace mxdet;

extern "C" int mxdet_carafe_fwd(const mxdet_carafe_desc_t* d, const uint16_t* X, const uint16_t* M, uint16_t* Y,
                                mxdet_stream_t stream) {
  clear_error();
  CarafeK k;
  const int rc = carafe_prepare("carafe_fwd", d, &k);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(X != nullptr && M != nullptr && Y != nullptr, MXDET_EINVAL, "carafe_fwd: null pointer");
  MXDET_REQUIRE(aligned16(X) && aligned16(Y) && ((uintptr_t)M % 2) == 0, MXDET_EINVAL,
                "carafe_fwd: X and Y must be 16-byte aligned, M 2-byte aligned");
  const dim3 grid((unsigned)(k.N * k.tiles_x * k.tiles_y), (unsigned)ceil_div(k.C8, kCarSlice8));
  if (d->k == 3)
    hipLaunchKernelGGL(carafe_fwd_kernel<3>, grid, dim3(kCarThreads), 0, as_stream(stream), k, (const uint4*)X, M, (uint4*)Y);
  else
    hipLaunchKernelGGL(carafe_fwd_kernel<5>, grid, dim3(kCarThreads), 0, as_stream(stream), k, (const uint4*)X, M, (uint4*)Y);
  return check_launch("carafe_fwd");
}

extern "C" int mxdet_carafe_bwd(const mxdet_carafe_desc_t* d, const uint16_t* X, const uint16_t* M, const uint16_t* dY,
                                uint16_t* dX, uint16_t* dM, int32_t accumulate, mxdet_stream_t stream) {
  clear_error();
  CarafeK k;
  const int rc = carafe_prepare("carafe_bwd", d, &k);
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE(X != nullptr && M != nullptr && dY != nullptr && dX != nullptr && dM != nullptr, MXDET_EINVAL,
                "carafe_bwd: null pointer");
  MXDET_REQUIRE(aligned16(X) && aligned16(dY) && aligned16(dX) && ((uintptr_t)M % 2) == 0 && ((uintptr_t)dM % 2) == 0,
                MXDET_EINVAL, "carafe_bwd: X, dY and dX must be 16-byte aligned, M and dM 2-byte aligned");
  const dim3 grid((unsigned)(k.N * k.tiles_x * k.tiles_y));
  const int acc = accumulate ? 1 : 0;
  if (d->k == 3) {
    hipLaunchKernelGGL(carafe_bwd_x_kernel<3>, grid, dim3(kCarThreads), 0, as_stream(stream), k, M, (const uint4*)dY, (uint4*)dX,
                       acc);
    hipLaunchKernelGGL(carafe_bwd_m_kernel<3>, grid, dim3(kCarThreads), 0, as_stream(stream), k, (const uint4*)X, M,
                       (const uint4*)dY, dM);
  } else {
    hipLaunchKernelGGL(carafe_bwd_x_kernel<5>, grid, dim3(kCarThreads), 0, as_stream(stream), k, M, (const uint4*)dY, (uint4*)dX,
                       acc);
    hipLaunchKernelGGL(carafe_bwd_m_kernel<5>, grid, dim3(kCarThreads), 0, as_stream(stream), k, (const uint4*)X, M,
                       (const uint4*)dY, dM);
  }
  return check_launch("carafe_bwd");
}
