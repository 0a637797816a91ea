// soft_nms.hip -- Soft-NMS (Bodla et al. 2017: hard / linear / Gaussian re-scoring) of independent candidate lists on
// gfx950. Test-time only: core/evaluation's post-processing and the standalone mxdet_soft_nms_batched.
//
// The bitmask NMS of boxes.hip precomputes a 0/1 suppression matrix; here every selection rescales the scores that
// decide the next selection, so the loop is sequential in the selections and parallel in the candidates:
//   one workgroup (256 threads = 4 waves, one per SIMD) per list; candidate p lives in register slot p / 256 of thread
//   p % 256 for the whole loop (box, score, id) and its box also sits in LDS for the broadcast of the selected one.
//   Per selection:  thread arg-max over its live slots of the key float_key(score) << 32 | ~id
//                -> wave max (4 DPP steps inside the rows of 16, 4 v_readlane pairs across them)
//                -> the owning lane of each wave writes (key, position) to LDS, parity double-buffered: ONE barrier
//                -> every thread reads the 4 wave results, takes the largest, reads that box from LDS (one address:
//                   a broadcast) and rescales its own live slots.
// No atomics, no global loads inside the loop; the only global traffic of a trip is thread 0's store of the selection.
// All box / score arithmetic is mxdet_math.h's, one fp32 operation per step, built without FMA contraction: indices and
// score bits are compared bit for bit with the numpy restatement in tests/_soft_nms_ref.py.
#include "soft_nms.h"

namespace mxdet {

constexpr int kSoftThreads = 256;

template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_max_u64(unsigned long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xf, 0xf, false);
  const unsigned long long o = ((unsigned long long)hi << 32) | lo;
  return o > v ? o : v;
}

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

// largest value of the wave, in every lane (all 64 lanes active)
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  v = dpp_max_u64<0xB1>(v);    // quad_perm [1,0,3,2]: lane ^ 1
  v = dpp_max_u64<0x4E>(v);    // quad_perm [2,3,0,1]: lane ^ 2
  v = dpp_max_u64<0x141>(v);   // row_half_mirror: the other quad of the 8
  v = dpp_max_u64<0x140>(v);   // row_mirror: the other half of the row of 16
  const unsigned long long a = readlane_u64(v, 0), b = readlane_u64(v, 16), c = readlane_u64(v, 32), d = readlane_u64(v, 48);
  const unsigned long long ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}

__device__ __forceinline__ float key_score(unsigned long long key) {
  const unsigned fk = (unsigned)(key >> 32);
  return __uint_as_float((fk & 0x80000000u) ? (fk & 0x7fffffffu) : ~fk);   // inverse of mxdet_float_key
}

template <int METHOD>
__device__ __forceinline__ float soft_weight(float o, float nms_thresh, float sigma) {
  if (METHOD == 0) return o > nms_thresh ? 0.0f : 1.0f;
  if (METHOD == 1) return o > nms_thresh ? 1.0f - o : 1.0f;
  float t = o * o;
  t = t / sigma;
  return mxdet_expf(-t);
}

template <int IPT, int METHOD>
__global__ void __launch_bounds__(kSoftThreads)
soft_nms_kernel(const float4* __restrict__ boxes, const float* __restrict__ scores,
                const unsigned long long* __restrict__ skeys, const int32_t* __restrict__ counts, int n_max,
                float nms_thresh, float sigma, float min_score, int max_keep, int out_stride, int pad,
                int32_t* __restrict__ keep_pos, float* __restrict__ keep_scores,
                unsigned long long* __restrict__ keep_keys, int32_t* __restrict__ num_keep) {
  __shared__ float4 sbox[kSoftThreads * IPT];
  __shared__ unsigned long long xkey[2][kSoftThreads / 64];
  __shared__ int xpos[2][kSoftThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int n = counts[b];
  n = n > n_max ? n_max : (n < 0 ? 0 : n);
  const size_t ob = (size_t)b * out_stride;
  int nsel = 0;
  if (n > 0) {
    const float dead = __uint_as_float(0xff800000u);   // -inf: `score > min_score` is false for every min_score
    float4 bx[IPT];
    float sc[IPT];
    unsigned id[IPT];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
      const int p = k * kSoftThreads + tid;
      bx[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      sc[k] = dead;
      id[k] = (unsigned)p;
      if (p < n) {
        bx[k] = boxes[(size_t)b * n_max + p];
        if (scores) {
          sc[k] = scores[(size_t)b * n_max + p];
        } else {
          const unsigned long long key = skeys[(size_t)b * n_max + p];
          sc[k] = key_score(key);
          id[k] = ~(unsigned)key;
        }
      }
      sbox[p] = bx[k];
    }
    // the first barrier of the loop orders these LDS writes before the first read of sbox
    for (int t = 0; t < max_keep; ++t) {
      unsigned long long best = 0ull;    // 0 = no live candidate (a live score is not NaN: its key's high word is not 0)
      int bpos = 0;
#pragma unroll
      for (int k = 0; k < IPT; ++k) {
        const unsigned long long key =
            sc[k] > min_score ? (((unsigned long long)mxdet_float_key(sc[k]) << 32) | (unsigned long long)(~id[k])) : 0ull;
        if (key > best) { best = key; bpos = k * kSoftThreads + tid; }
      }
      const unsigned long long wmax = wave_max_u64(best);
      const int par = t & 1;
      // ids are unique within a list, so exactly one lane owns a non-zero maximum
      if (wmax != 0ull ? best == wmax : lane == 0) { xkey[par][wid] = wmax; xpos[par][wid] = bpos; }
      __syncthreads();   // the only barrier of a trip: trip t+1 writes the other parity, trip t+2 comes after barrier t+1
      unsigned long long win = xkey[par][0];
      int wpos = xpos[par][0];
#pragma unroll
      for (int w = 1; w < kSoftThreads / 64; ++w) {
        const unsigned long long k2 = xkey[par][w];
        const int p2 = xpos[par][w];
        if (k2 > win) { win = k2; wpos = p2; }
      }
      if (win == 0ull) break;            // nothing live: the same LDS words in every thread, so the exit is uniform
      const float4 s = sbox[wpos];
      if (tid == 0) {
        keep_pos[ob + t] = wpos;
        if (keep_scores) keep_scores[ob + t] = key_score(win);
        if (keep_keys) keep_keys[ob + t] = win;
      }
      ++nsel;
#pragma unroll
      for (int k = 0; k < IPT; ++k) {
        if (k * kSoftThreads + tid == wpos) {
          sc[k] = dead;
        } else if (sc[k] > min_score) {
          const float o = mxdet_iou(s.x, s.y, s.z, s.w, bx[k].x, bx[k].y, bx[k].z, bx[k].w);
          const float w = soft_weight<METHOD>(o, nms_thresh, sigma);
          sc[k] = sc[k] * w;
        }
      }
    }
  }
  if (pad) {
    for (int j = nsel + tid; j < max_keep; j += kSoftThreads) {
      keep_pos[ob + j] = -1;
      if (keep_scores) keep_scores[ob + j] = 0.0f;
    }
  }
  if (tid == 0) num_keep[b] = nsel;
}

template <int IPT>
static void soft_nms_launch_ipt(const float4* boxes, const float* scores, const unsigned long long* skeys,
                                const int32_t* counts, int B, int n_max, int method, float nms_thresh, float sigma,
                                float min_score, int max_keep, int out_stride, int pad, int32_t* keep_pos,
                                float* keep_scores, unsigned long long* keep_keys, int32_t* num_keep, hipStream_t s) {
  const dim3 grid(B), block(kSoftThreads);
#define MXDET_SOFT_LAUNCH(M)                                                                                          \
  hipLaunchKernelGGL((soft_nms_kernel<IPT, M>), grid, block, 0, s, boxes, scores, skeys, counts, n_max, nms_thresh,    \
                     sigma, min_score, max_keep, out_stride, pad, keep_pos, keep_scores, keep_keys, num_keep)
  if (method == 0) MXDET_SOFT_LAUNCH(0);
  else if (method == 1) MXDET_SOFT_LAUNCH(1);
  else MXDET_SOFT_LAUNCH(2);
#undef MXDET_SOFT_LAUNCH
}

void soft_nms_launch(const float4* boxes, const float* scores, const unsigned long long* skeys, const int32_t* counts,
                     int B, int n_max, int method, float nms_thresh, float sigma, float min_score, int max_keep,
                     int out_stride, int pad, int32_t* keep_pos, float* keep_scores, unsigned long long* keep_keys,
                     int32_t* num_keep, hipStream_t stream) {
  // register slots per thread: 4 covers the usual 1000-roi lists with a quarter of the per-trip work of 16
  if (n_max <= 4 * kSoftThreads)
    soft_nms_launch_ipt<4>(boxes, scores, skeys, counts, B, n_max, method, nms_thresh, sigma, min_score, max_keep,
                           out_stride, pad, keep_pos, keep_scores, keep_keys, num_keep, stream);
  else
    soft_nms_launch_ipt<16>(boxes, scores, skeys, counts, B, n_max, method, nms_thresh, sigma, min_score, max_keep,
                            out_stride, pad, keep_pos, keep_scores, keep_keys, num_keep, stream);
}

}  // namespace mxdet

using namespace mxdet;

static_assert(kSoftNmsMaxList == 16 * kSoftThreads, "the widest instantiation holds a whole list");

extern "C" int mxdet_soft_nms_batched(const float* boxes, const float* scores, const int32_t* counts, int32_t B,
                                      int32_t n_max, int32_t method, float nms_thresh, float sigma, float min_score,
                                      int32_t max_keep, int32_t* keep_idx, float* keep_scores, int32_t* num_keep,
                                      mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(B >= 0 && n_max >= 0 && max_keep >= 0, MXDET_ESHAPE, "soft_nms_batched: negative size");
  MXDET_REQUIRE(n_max <= kSoftNmsMaxList, MXDET_ESHAPE, "soft_nms_batched: n_max %d > %d unsupported", n_max,
                kSoftNmsMaxList);
  MXDET_REQUIRE(method >= 0 && method <= 2, MXDET_EINVAL, "soft_nms_batched: method %d not in 0..2", method);
  MXDET_REQUIRE(method != 2 || sigma > 0.0f, MXDET_EINVAL, "soft_nms_batched: sigma must be positive for method 2");
  if (B == 0) return MXDET_OK;
  MXDET_REQUIRE(counts && num_keep, MXDET_EINVAL, "soft_nms_batched: null pointer");
  MXDET_REQUIRE((n_max == 0 || (boxes && scores)) && (max_keep == 0 || (keep_idx && keep_scores)), MXDET_EINVAL,
                "soft_nms_batched: null pointer");
  // n_max == 0: every list is empty whatever counts says (the kernel clamps), so nothing is read from boxes / scores
  soft_nms_launch((const float4*)boxes, scores, nullptr, counts, B, n_max, method, nms_thresh, sigma, min_score, max_keep,
                  max_keep, 1, keep_idx, keep_scores, nullptr, num_keep, as_stream(stream));
  return check_launch("soft_nms_batched");
}
