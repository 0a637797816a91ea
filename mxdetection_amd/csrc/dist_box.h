// dist_box.h -- the distribution box head (definition in include/mxdet.h): one box side is R + 1 logits
// over 0..R strides, its distance the distribution's expectation. Shared by the losses and by test-time detection, so
// that both decode the same bits. Float32, no FMA contraction (both files are built with -ffp-contract=off).
#pragma once
#include "common.h"

namespace mxdet {

constexpr int kDistBins = MXDET_REG_MAX_LIMIT + 1;       // the loops below are unrolled to it and cut at the run-time R

// The side's logits x[off + k * sc], k = 0..R, into registers: the loads are independent and leave together (one memory
// latency for the side, not R + 1 of them: a loop over a run-time R waits for each). 2-byte alignment is all that is assumed.
__device__ __forceinline__ void dist_load(const void* x, long long off, long long sc, int dtype, int R, float* xv) {
#pragma unroll
  for (int k = 0; k < kDistBins; ++k)
    if (k <= R) xv[k] = load_as_f32(x, off + k * sc, dtype);
}

// m = max_k x_k; e_k = mxdet_expf(x_k - m), left in xv[k]; Z = sum e_k and S = sum k e_k, both accumulated from 0 with k
// ascending; returns E = S / Z. Every index is a constant after unrolling: xv stays in registers, there is no scratch.
__device__ __forceinline__ float dist_expect(float* xv, int R, float& m, float& Z) {
  m = xv[0];
#pragma unroll
  for (int k = 1; k < kDistBins; ++k)
    if (k <= R) m = xv[k] > m ? xv[k] : m;
  float S = 0.0f;
  Z = 0.0f;
#pragma unroll
  for (int k = 0; k < kDistBins; ++k)
    if (k <= R) {
      const float e = mxdet_expf(xv[k] - m);
      xv[k] = e;
      Z = Z + e;
      S = S + (float)k * e;
    }
  return S / Z;
}

}  // namespace mxdet
