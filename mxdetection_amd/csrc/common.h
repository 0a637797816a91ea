// common.h -- shared host/device helpers for libmxdet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/mxdet.h"
#include "../../include/mxdet_debug.h"
#include "../../include/mxdet_math.h"

namespace mxdet {

// thread-local error string (the only mutable global state of the library)
void set_error(const char* fmt, ...);
void clear_error();

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return MXDET_EHIP;
  }
  return MXDET_OK;
}

#define MXDET_REQUIRE(cond, code, ...)  \
  do {                                  \
    if (!(cond)) {                      \
      ::mxdet::set_error(__VA_ARGS__);  \
      return (code);                    \
    }                                   \
  } while (0)

// plan-time thresholds (mxdet_debug_set_tuning; defaults in capi.hip). The library never reads the environment.
long long tuning(int which);

// Route probe (mxdet_debug_route_probe, include/mxdet_debug.h): while it is on for the calling thread, the dense conv /
// weight-gradient launchers record the instantiation and grid they WOULD launch and return without touching the device.
constexpr int kRouteWords = 16, kRouteMax = 4;
extern thread_local int g_route_probe;                   // 0 = off (the only cost on the launch path: this load)
void route_record(const int32_t (&rec)[kRouteWords]);
static inline bool route_probe_on() { return g_route_probe != 0; }

static inline hipStream_t as_stream(mxdet_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int kWave = 64;
// byte offset that is out of range for every buffer descriptor of the library (tensors are < 2^31 elements): an LDS-DMA
// lane given this offset writes 16 zero bytes into its LDS slot (measured, tools/micro/dma_oob.hip)
constexpr unsigned kDmaOob = 0xfffffff0u;

template <typename T>
__host__ __device__ inline T ceil_div(T a, T b) { return (a + b - 1) / b; }

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Zero `bytes` (a multiple of 4) at `p` with a kernel. Used instead of hipMemsetAsync everywhere: memset NODES of a
// hipGraph did not order reliably against the kernels behind them once a graph started with them (a step captured
// with the RPN branch as its own graph lost the zeroing of the anchor-sampling counters: garbage counts, GPU fault).
__global__ static void zero_u32_kernel(unsigned* __restrict__ p, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0u;
}
static inline hipError_t zero_async(void* p, size_t bytes, hipStream_t s) {
  long long n = (long long)((bytes + 3) / 4);
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(zero_u32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (unsigned*)p, n);
  return hipGetLastError();
}

// ---- device helpers ----------------------------------------------------------------------------
// raw buffer descriptor (stride 0, `bytes` records) over a tensor, built from provably wave-uniform words so that hipcc
// keeps it in SGPRs (a descriptor it cannot prove uniform gets a waterfall loop around every buffer instruction)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
  const unsigned long long a = (unsigned long long)base;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0,
                                           (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

__device__ __forceinline__ float bf16_bits_to_f32(uint16_t h) {
  return __uint_as_float(((uint32_t)h) << 16);
}
__device__ __forceinline__ uint16_t f32_to_bf16_bits(float f) { return mxdet_f32_to_bf16(f); }
// two floats -> packed bf16 pair by the hardware conversion (v_cvt_pk_bf16_f32, round to nearest even: the same bits as
// mxdet_f32_to_bf16 for every finite value; NaNs keep being NaNs). One instruction instead of ~12 integer ones: used
// by the dense epilogues, whose results are tolerance-checked; the bit-exact detection ops keep the shared helper.
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
  const bf16x2_t p = (bf16x2_t){(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, p);
}
// eight (four) packed bf16 -> fp32, exact: element 2k is the low half of word k
__device__ __forceinline__ void unpack8_bf16(const uint4& v, float* f) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}
__device__ __forceinline__ void unpack4_bf16(const uint2& v, float* f) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
}
// eight floats -> packed bf16 by pack_bf16x2 (the hardware conversion: tolerance-checked dense results)
__device__ __forceinline__ uint4 pack8_bf16_hw(const float* f) {
  return make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7]));
}
// ... and by f32_to_bf16_bits (the shared bit-exact helper: results that are compared with the C oracle)
__device__ __forceinline__ uint4 pack8_bf16_exact(const float* v) {
  uint4 o;
  o.x = (uint32_t)f32_to_bf16_bits(v[0]) | ((uint32_t)f32_to_bf16_bits(v[1]) << 16);
  o.y = (uint32_t)f32_to_bf16_bits(v[2]) | ((uint32_t)f32_to_bf16_bits(v[3]) << 16);
  o.z = (uint32_t)f32_to_bf16_bits(v[4]) | ((uint32_t)f32_to_bf16_bits(v[5]) << 16);
  o.w = (uint32_t)f32_to_bf16_bits(v[6]) | ((uint32_t)f32_to_bf16_bits(v[7]) << 16);
  return o;
}

// MFMA operand / accumulator vectors and the LDS pointer type of the LDS-DMA builtins
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// XCD-aware tile order: workgroup `bid` of `nwg` runs on XCD bid % 8. The map gives each XCD a contiguous range of
// tiles, so the blocks that share an XCD walk consecutive tiles and re-read what those tiles share from that XCD's L2.
__device__ __forceinline__ int xcd_tile_order(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// Grouped launches: one grid for the workgroups of `n` table entries, entry i owning those from table[i].*First on
// (First non-decreasing in i, table[0].*First == 0). Index of the entry that owns workgroup `bid`: the last one whose
// First is <= bid. A workgroup past that entry's count is alignment padding; the caller tests for it.
template <typename T, int T::*First>
__device__ __forceinline__ int table_lookup(const T* table, int n, int bid) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].*First <= bid) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// exact floor(n / d) and remainder for 0 <= n < 2^24 through one float multiply + a +-1 correction (an integer division
// is ~40 instructions): the tile prologues do two per row
__device__ __forceinline__ int fast_divmod(int n, int d, float rcp, int* rem) {
  int q = (int)((float)n * rcp);
  int r = n - q * d;
  if (r < 0) { --q; r += d; }
  if (r >= d) { ++q; r -= d; }
  *rem = r;
  return q;
}

__device__ __forceinline__ float load_as_f32(const void* p, int64_t i, int dtype) {
  if (dtype == MXDET_DTYPE_BF16) return bf16_bits_to_f32(((const uint16_t*)p)[i]);
  return ((const float*)p)[i];
}
__device__ __forceinline__ void store_from_f32(void* p, int64_t i, int dtype, float v) {
  if (dtype == MXDET_DTYPE_BF16)
    ((uint16_t*)p)[i] = f32_to_bf16_bits(v);
  else
    ((float*)p)[i] = v;
}

}  // namespace mxdet

// wave / block reduce and scan primitives (lane_id, wave_sum, block4_reduce, block_excl_count, ...)
#include "wave.h"
