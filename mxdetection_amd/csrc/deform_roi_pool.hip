// deform_roi_pool.hip -- (modulated) deformable RoI pooling over a channels-last bf16 feature pyramid.
//
// Slot: roi_extractors (reference README.md:32); MXNet role contrib.DeformablePSROIPooling with group_size 1,
// part_size = pooled, output_dim = C and class-agnostic offsets (Deformable-ConvNets' FPN box branch, mmdetection's
// dpool / mdpool), one launch for all pyramid levels like roi_align.hip. Semantics: include/mxdet.h, mxdet_dpool_*.
//   fwd       : one workgroup per roi, work item = (bin, 8-channel group) as in roi_align_fwd_kernel (16-B corner loads);
//               the S*S samples of a bin walk the same few corner rows, which stay in L1 / L2.
//   bwd_trans : d(trans) and, v2, d(mask logit); one WAVE per (roi, bin), a lane owns 4 channels of every 256-channel
//               chunk, samples inner; the wave is folded by a fixed butterfly: fixed reduction order.
//   bwd_feat  : the feature adjoint WITHOUT float atomics. A prepare launch writes one record per roi (pixel box of its
//               valid samples) and per bin (shifted start, dout scale mask / count, pixel box); the gather gives every
//               8-pixel row segment (one wave, a lane owns 4 channels, 8 x 4 fp32 sums in registers) the rois whose box
//               reaches its row span (ascending, compacted into LDS once per workgroup), and walks their bins (ascending)
//               and samples (ih, iw) in that fixed order, rounding once. Bit-reproducible for any overlap.
// Why not RoIAlign's segment gather: its per-roi separable grid is gone (every bin is shifted on its own) and 49 x S row
// samples exceed its 32-lane sample tables; why not deform_conv.hip's inverted index: under unbounded overlap (1024
// identical proposals) one pixel's list is thousands of entries long, beyond its 64-entry wave sort.
// The pyramid argument, the roi header clamp, packed spans and the gather's skeleton (level of a workgroup, ascending LDS
// roi list, row write-out) are roi_gather.h's, shared with roi_align.hip.
#include "roi_gather.h"

namespace mxdet {

struct DPoolArgs {
  FeatPyr p;
  int C, PH, PW, NB, S, mod, ts, ms, acc;
  float trans_std;
};

struct DRoi {
  int n, lvl, H, W;
  float rsw, rsh, roi_w, roi_h, bin_w, bin_h, sub_w, sub_h;
};

__device__ __forceinline__ DRoi dpool_roi(const DPoolArgs& a, const float* __restrict__ rois,
                                          const int32_t* __restrict__ levels, long long r) {
  DRoi g;
  const float* q = rois + r * 5;
  roi_image_level(a.p, rois, levels, r, &g.lvl, &g.n);
  const float s = a.p.scale[g.lvl];
  g.H = a.p.H[g.lvl]; g.W = a.p.W[g.lvl];
  g.rsw = roundf(q[1]) * s - 0.5f;                    // C round: half away from zero
  g.rsh = roundf(q[2]) * s - 0.5f;
  const float rew = (roundf(q[3]) + 1.0f) * s - 0.5f;
  const float reh = (roundf(q[4]) + 1.0f) * s - 0.5f;
  g.roi_w = rew - g.rsw;
  g.roi_h = reh - g.rsh;
  g.roi_w = g.roi_w > 0.1f ? g.roi_w : 0.1f;
  g.roi_h = g.roi_h > 0.1f ? g.roi_h : 0.1f;
  g.bin_w = g.roi_w / (float)a.PW;
  g.bin_h = g.roi_h / (float)a.PH;
  g.sub_w = g.bin_w / (float)a.S;
  g.sub_h = g.bin_h / (float)a.S;
  return g;
}

// shifted start of bin b and its v2 mask factor (trans == nullptr: the no-trans pass)
__device__ __forceinline__ void dpool_bin(const DPoolArgs& a, const DRoi& g, const uint16_t* __restrict__ trans,
                                          const uint16_t* __restrict__ mask, long long r, int b, float* ws, float* hs,
                                          float* m) {
  const int ph = b / a.PW, pw = b - ph * a.PW;
  float w = (float)pw * g.bin_w + g.rsw;
  float h = (float)ph * g.bin_h + g.rsh;
  if (trans) {
    const float tx = bf16_bits_to_f32(trans[r * a.ts + b]) * a.trans_std;
    const float ty = bf16_bits_to_f32(trans[r * a.ts + a.NB + b]) * a.trans_std;
    w = w + tx * g.roi_w;
    h = h + ty * g.roi_h;
  }
  *ws = w;
  *hs = h;
  *m = 1.0f;
  if (a.mod) *m = 1.0f / (1.0f + expf(-bf16_bits_to_f32(mask[r * a.ms + b])));
}

// one axis of a sample: skipped outside [-0.5, L - 0.5], else clamped to [0, L-1]; corners floor / ceil, d = v - floor
struct DAxis { int lo, hi; float d; bool valid; };

__device__ __forceinline__ DAxis dpool_axis(float v, int L) {
  DAxis x;
  x.valid = v >= -0.5f && v <= (float)L - 0.5f;      // (a NaN position is not valid)
  v = v < 0.0f ? 0.0f : v;
  v = v > (float)(L - 1) ? (float)(L - 1) : v;
  const float f = floorf(v), c = ceilf(v);
  x.lo = (int)f;
  x.hi = (int)c;
  x.d = v - f;
  return x;
}

// ---- forward: one workgroup per roi; work item = (bin, 8-channel group), channel group fastest -------------------------
__global__ void __launch_bounds__(256)
dpool_fwd_kernel(DPoolArgs a, const float* __restrict__ rois, const int32_t* __restrict__ levels,
                 const uint16_t* __restrict__ trans, const uint16_t* __restrict__ mask, uint16_t* __restrict__ out) {
  const long long r = blockIdx.x;
  const DRoi g = dpool_roi(a, rois, levels, r);
  const int CG = a.C >> 3;
  const uint16_t* feat = (const uint16_t*)a.p.feat[g.lvl] + (long long)g.n * g.H * g.W * a.C;
  for (int it = threadIdx.x; it < a.NB * CG; it += blockDim.x) {
    const int cg = it % CG, b = it / CG;
    float ws, hs, m;
    dpool_bin(a, g, trans, mask, r, b, &ws, &hs, &m);
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.0f;
    int cnt = 0;
    for (int ih = 0; ih < a.S; ++ih) {
      const DAxis y = dpool_axis(hs + (float)ih * g.sub_h, g.H);
      if (!y.valid) continue;
      for (int iw = 0; iw < a.S; ++iw) {
        const DAxis x = dpool_axis(ws + (float)iw * g.sub_w, g.W);
        if (!x.valid) continue;
        float v11[8], v12[8], v21[8], v22[8];
        unpack8_bf16(*(const uint4*)(feat + ((long long)y.lo * g.W + x.lo) * a.C + cg * 8), v11);
        unpack8_bf16(*(const uint4*)(feat + ((long long)y.hi * g.W + x.lo) * a.C + cg * 8), v12);
        unpack8_bf16(*(const uint4*)(feat + ((long long)y.lo * g.W + x.hi) * a.C + cg * 8), v21);
        unpack8_bf16(*(const uint4*)(feat + ((long long)y.hi * g.W + x.hi) * a.C + cg * 8), v22);
        const float w11 = (1.0f - x.d) * (1.0f - y.d), w12 = (1.0f - x.d) * y.d;
        const float w21 = x.d * (1.0f - y.d), w22 = x.d * y.d;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float t = w11 * v11[k];
          t = t + w12 * v12[k];
          t = t + w21 * v21[k];
          t = t + w22 * v22[k];
          acc[k] = acc[k] + t;
        }
        ++cnt;
      }
    }
    float o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = cnt ? (acc[k] / (float)cnt) * m : 0.0f;
    *(uint4*)(out + (r * a.NB + b) * a.C + cg * 8) =
        make_uint4(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7]));
  }
}

// number of valid samples of one axis of a bin
__device__ __forceinline__ int dpool_axis_count(float start, float sub, int S, int L) {
  int c = 0;
  for (int i = 0; i < S; ++i) c += dpool_axis(start + (float)i * sub, L).valid ? 1 : 0;
  return c;
}

// ---- trans / mask gradient: one wave per (roi, bin) ---------------------------------------------------------------------
__global__ void __launch_bounds__(256)
dpool_bwd_trans_kernel(DPoolArgs a, long long R, const float* __restrict__ rois, const int32_t* __restrict__ levels,
                       const uint16_t* __restrict__ trans, const uint16_t* __restrict__ mask,
                       const uint16_t* __restrict__ dout, uint16_t* __restrict__ d_trans, uint16_t* __restrict__ d_mask) {
  const long long wv = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wv >= R * a.NB) return;                         // wave-uniform
  const long long r = wv / a.NB;
  const int b = (int)(wv - r * a.NB);
  const DRoi g = dpool_roi(a, rois, levels, r);
  float ws, hs, m;
  dpool_bin(a, g, trans, mask, r, b, &ws, &hs, &m);
  const uint16_t* feat = (const uint16_t*)a.p.feat[g.lvl] + (long long)g.n * g.H * g.W * a.C;
  const uint16_t* drow = dout + (r * a.NB + b) * a.C;
  float gx = 0.0f, gy = 0.0f, gm = 0.0f;
  for (int c0 = lane * 4; c0 < a.C; c0 += 256) {
    float d[4];
    unpack4_bf16(*(const uint2*)(drow + c0), d);
    for (int ih = 0; ih < a.S; ++ih) {
      const DAxis y = dpool_axis(hs + (float)ih * g.sub_h, g.H);
      if (!y.valid) continue;
      for (int iw = 0; iw < a.S; ++iw) {
        const DAxis x = dpool_axis(ws + (float)iw * g.sub_w, g.W);
        if (!x.valid) continue;
        float u00[4], u01[4], u10[4], u11[4];       // MXNet's names: u01 = (y1, x0), u10 = (y0, x1)
        unpack4_bf16(*(const uint2*)(feat + ((long long)y.lo * g.W + x.lo) * a.C + c0), u00);
        unpack4_bf16(*(const uint2*)(feat + ((long long)y.hi * g.W + x.lo) * a.C + c0), u01);
        unpack4_bf16(*(const uint2*)(feat + ((long long)y.lo * g.W + x.hi) * a.C + c0), u10);
        unpack4_bf16(*(const uint2*)(feat + ((long long)y.hi * g.W + x.hi) * a.C + c0), u11);
        const float w00 = (1.0f - x.d) * (1.0f - y.d), w01 = (1.0f - x.d) * y.d;
        const float w10 = x.d * (1.0f - y.d), w11 = x.d * y.d;
        // coinciding corners (integer or clamped position): the derivative is exactly 0, not a rounding residue
        const bool xe = x.lo == x.hi, ye = y.lo == y.hi;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float tx = u11[k] * y.d + u10[k] * (1.0f - y.d);
          tx = tx - u01[k] * y.d;
          tx = tx - u00[k] * (1.0f - y.d);
          tx = xe ? 0.0f : tx;
          float ty = u11[k] * x.d + u01[k] * (1.0f - x.d);
          ty = ty - u10[k] * x.d;
          ty = ty - u00[k] * (1.0f - x.d);
          ty = ye ? 0.0f : ty;
          float v = w00 * u00[k];
          v = v + w01 * u01[k];
          v = v + w10 * u10[k];
          v = v + w11 * u11[k];
          gx = gx + d[k] * tx;
          gy = gy + d[k] * ty;
          gm = gm + d[k] * v;
        }
      }
    }
  }
  wave_reduce_each<Sum>(gx, gy, gm);
  uint16_t* tr = d_trans + r * a.ts;
  uint16_t* mr = a.mod ? d_mask + r * a.ms : nullptr;
  if (lane == 0) {
    const int cnt = dpool_axis_count(hs, g.sub_h, a.S, g.H) * dpool_axis_count(ws, g.sub_w, a.S, g.W);
    float tx = 0.0f, ty = 0.0f, dm = 0.0f;
    if (cnt > 0) {
      const float sc = m / (float)cnt;
      tx = gx * sc * a.trans_std * g.roi_w;
      ty = gy * sc * a.trans_std * g.roi_h;
      dm = (gm / (float)cnt) * (m * (1.0f - m));
    }
    tr[b] = f32_to_bf16_bits(tx);
    tr[a.NB + b] = f32_to_bf16_bits(ty);
    if (mr) mr[b] = f32_to_bf16_bits(dm);
  }
  if (b == 0) {                                       // padding columns: zero (the FC data gradient reads them)
    for (int c = 2 * a.NB + lane; c < a.ts; c += 64) tr[c] = 0;
    if (mr)
      for (int c = a.NB + lane; c < a.ms; c += 64) mr[c] = 0;
  }
}

// ---- feature adjoint: records + gather (kSegW pixels per wave, kSegWaves waves per workgroup: roi_gather.h) -------------
struct DpRoiRec {                 // 32 B
  int nl;                         // image | level << 16 (level 0xffff: no valid sample)
  unsigned yy, xx;                // span_pack(ylo, yhi), span_pack(xlo, xhi): pixel box of its valid samples' corners
  int pad0;
  float sub_h, sub_w;
  int pad1, pad2;
};

struct DpBinRec {                 // 32 B
  float ws, hs, scale;            // shifted start, dout scale = mask factor / count (0: no valid sample)
  unsigned yy, xx;                // pixel box of the bin's corners (ylo > yhi: none)
  int pad0, pad1, pad2;
};

struct DpGrid {
  int block0[9];                  // first workgroup of level l
  int chunks[8];                  // workgroups along a row (kSegWaves * kSegW pixels each)
};

// one WAVE per roi, lane b = bin b; the roi's box is a butterfly min / max over its bins
__global__ void __launch_bounds__(64)
dpool_prepare_kernel(DPoolArgs a, long long R, const float* __restrict__ rois, const int32_t* __restrict__ levels,
                     const uint16_t* __restrict__ trans, const uint16_t* __restrict__ mask, DpRoiRec* __restrict__ roi,
                     DpBinRec* __restrict__ bin) {
  const long long r = blockIdx.x;
  const int lane = threadIdx.x;
  if (r >= R) return;
  const DRoi g = dpool_roi(a, rois, levels, r);
  int ylo = 1 << 30, yhi = -1, xlo = 1 << 30, xhi = -1;
  if (lane < a.NB) {
    float ws, hs, m;
    dpool_bin(a, g, trans, mask, r, lane, &ws, &hs, &m);
    int ny = 0, nx = 0;
    for (int i = 0; i < a.S; ++i) {
      const DAxis y = dpool_axis(hs + (float)i * g.sub_h, g.H);
      if (y.valid) { ylo = y.lo < ylo ? y.lo : ylo; yhi = y.hi > yhi ? y.hi : yhi; ++ny; }
      const DAxis x = dpool_axis(ws + (float)i * g.sub_w, g.W);
      if (x.valid) { xlo = x.lo < xlo ? x.lo : xlo; xhi = x.hi > xhi ? x.hi : xhi; ++nx; }
    }
    const int cnt = ny * nx;
    if (cnt == 0) { ylo = xlo = 1 << 30; yhi = xhi = -1; }
    DpBinRec e;
    e.ws = ws; e.hs = hs;
    e.scale = cnt ? m / (float)cnt : 0.0f;
    e.yy = cnt ? span_pack(ylo, yhi) : kSpanEmpty;
    e.xx = cnt ? span_pack(xlo, xhi) : kSpanEmpty;
    e.pad0 = e.pad1 = e.pad2 = 0;
    bin[r * a.NB + lane] = e;
  }
  wave_reduce_each<MinSel, 64, kAscend>(ylo, xlo);
  wave_reduce_each<MaxSel, 64, kAscend>(yhi, xhi);
  if (lane == 0) {
    DpRoiRec o;
    const bool any = yhi >= 0;
    o.nl = g.n | ((any ? g.lvl : 0xffff) << 16);
    o.yy = any ? span_pack(ylo, yhi) : kSpanEmpty;
    o.xx = any ? span_pack(xlo, xhi) : kSpanEmpty;
    o.sub_h = g.sub_h; o.sub_w = g.sub_w;
    o.pad0 = o.pad1 = o.pad2 = 0;
    roi[r] = o;
  }
}

// acc[j] += w * go for a wave-uniform j in [0, kSegW) (registers cannot be indexed at run time)
__device__ __forceinline__ void dp_add(float (&acc)[kSegW][4], int j, float w, const float* go) {
#pragma unroll
  for (int i = 0; i < kSegW; ++i) {
    const float wi = i == j ? w : 0.0f;        // adds +0 elsewhere: the sums are unchanged
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[i][k] = acc[i][k] + wi * go[k];
  }
}

__global__ void __launch_bounds__(kSegWaves * 64)
dpool_gather_kernel(DPoolArgs a, DpGrid gr, int R, const DpRoiRec* __restrict__ roi, const DpBinRec* __restrict__ bin,
                    const uint16_t* __restrict__ dout) {
  __shared__ int e_r[kSegChunk];
  __shared__ unsigned e_xx[kSegChunk];
  __shared__ int wcnt[kSegWaves];
  __shared__ int s_cnt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bid = (int)blockIdx.x;
  const int l = level_of_block(gr.block0, a.p.num_levels, bid);
  const int rel = bid - gr.block0[l];
  const int rowrel = rel / gr.chunks[l], chunk = rel - rowrel * gr.chunks[l];
  const int H = a.p.H[l], W = a.p.W[l];
  const int n = rowrel / H, Y = rowrel - n * H;
  const int X0 = chunk * kSegWaves * kSegW;
  const int X1 = X0 + kSegWaves * kSegW - 1 < W - 1 ? X0 + kSegWaves * kSegW - 1 : W - 1;
  const int x0 = X0 + wid * kSegW;
  const int x1 = x0 + kSegW - 1 < W - 1 ? x0 + kSegW - 1 : W - 1;
  const bool wave_live = x0 < W;
  const int c0 = (int)blockIdx.y * 256 + lane * 4;
  const bool live = c0 < a.C;
  const int key = n | (l << 16);
  float acc[kSegW][4];
#pragma unroll
  for (int j = 0; j < kSegW; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[j][k] = 0.0f;
  bool touched = false;
  for (int rc = 0; rc < R; rc += kSegChunk) {
    // ---- the list of this round: rois rc .. rc+kSegChunk-1 that reach the workgroup's row span, ascending ----
    __syncthreads();
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const int rend = rc + kSegChunk < R ? rc + kSegChunk : R;
    for (int rb = rc; rb < rend; rb += kSegWaves * 64) {
      const int r = rb + tid;
      bool hit = false;
      unsigned xx = 0u;
      if (r < rend) {
        const DpRoiRec t = roi[r];
        xx = t.xx;
        hit = t.nl == key && span_hits(t.yy, Y, Y) && span_hits(t.xx, X0, X1);
      }
      block_compact_ascending<kSegWaves>(hit, lane, wid, wcnt, &s_cnt, [&](int k) {
        e_r[k] = r;
        e_xx[k] = xx;
      });
    }
    const int cnt = s_cnt;
    if (!wave_live) continue;             // (every wave reaches the barriers above)
    // ---- walk: rois ascending, their bins ascending, samples ih-major ----
    for (int base = 0; base < cnt; base += 64) {
      const int kk = base + lane;
      const bool hitk = kk < cnt && span_hits(e_xx[kk < cnt ? kk : 0], x0, x1);
      unsigned long long mr = __ballot(hitk);
      while (mr) {
        const int kb = base + __ffsll((long long)mr) - 1;
        mr &= mr - 1;
        const int r = e_r[kb];
        const float sub_h = roi[r].sub_h, sub_w = roi[r].sub_w;
        DpBinRec e;
        bool hb = false;
        if (lane < a.NB) {
          e = bin[(long long)r * a.NB + lane];
          hb = span_hits(e.yy, Y, Y) && span_hits(e.xx, x0, x1);
        } else {
          e.ws = e.hs = e.scale = 0.0f;
        }
        unsigned long long mb = __ballot(hb);
        if (mb) touched = true;
        while (mb) {
          const int b = __ffsll((long long)mb) - 1;
          mb &= mb - 1;
          const float ws = readlane_f(e.ws, b), hs = readlane_f(e.hs, b), sc = readlane_f(e.scale, b);
          float go[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          if (live) {
            unpack4_bf16(*(const uint2*)(dout + ((long long)r * a.NB + b) * a.C + c0), go);
#pragma unroll
            for (int k = 0; k < 4; ++k) go[k] = go[k] * sc;
          }
          for (int ih = 0; ih < a.S; ++ih) {
            const DAxis y = dpool_axis(hs + (float)ih * sub_h, H);
            if (!y.valid || (y.lo != Y && y.hi != Y)) continue;
            // the sample's row weight on row Y (both corners on Y: 1 - d + d)
            float wy = y.lo == Y ? 1.0f - y.d : 0.0f;
            wy = wy + (y.hi == Y ? y.d : 0.0f);
            for (int iw = 0; iw < a.S; ++iw) {
              const DAxis x = dpool_axis(ws + (float)iw * sub_w, W);
              if (!x.valid || x.hi < x0 || x.lo > x1) continue;
              // corner x0 then x1 (same pixel at an integer / clamped position: the second adds d = 0)
              dp_add(acc, x.lo - x0, wy * (1.0f - x.d), go);
              dp_add(acc, x.hi - x0, wy * x.d, go);
            }
          }
        }
      }
    }
  }
  if (!wave_live || !live || (a.acc && !touched)) return;     // nothing to add: leave the map as it is
  uint16_t* out = (uint16_t*)a.p.feat[l] + ((long long)(n * H + Y) * W + x0) * a.C + c0;
#pragma unroll
  for (int j = 0; j < kSegW; ++j) {
    if (x0 + j > x1) break;
    seg_store4<false>(out + (long long)j * a.C, acc[j], a.acc);
  }
}

static int dpool_check(const mxdet_dpool_desc_t* d, DPoolArgs* a, long long R, const uint16_t* trans,
                       const uint16_t* mask, const char* who) {
  MXDET_REQUIRE(d != nullptr, MXDET_EINVAL, "%s: null descriptor", who);
  const mxdet_feat_pyramid_t& f = d->pyr;
  MXDET_REQUIRE(f.num_levels > 0 && f.num_levels <= 8, MXDET_ESHAPE, "%s: bad level count %d", who, f.num_levels);
  MXDET_REQUIRE(d->N > 0 && d->C > 0 && d->C % 8 == 0, MXDET_ESHAPE, "%s: bad N / C (C must be a multiple of 8)", who);
  MXDET_REQUIRE(d->PH > 0 && d->PW > 0 && d->PH * d->PW <= 64, MXDET_ESHAPE, "%s: needs 0 < PH * PW <= 64 (got %dx%d)",
                who, d->PH, d->PW);
  MXDET_REQUIRE(d->sample_per_part >= 1 && d->sample_per_part <= 16, MXDET_ESHAPE,
                "%s: sample_per_part must be in [1, 16] (got %d)", who, d->sample_per_part);
  MXDET_REQUIRE(R >= 0 && R <= 65535, MXDET_ESHAPE, "%s: roi count must be in [0, 65535]", who);
  for (int l = 0; l < f.num_levels; ++l) {
    MXDET_REQUIRE(f.H[l] > 0 && f.W[l] > 0 && f.H[l] < 32768 && f.W[l] < 32768, MXDET_ESHAPE, "%s: level %d bad size",
                  who, l);
    MXDET_REQUIRE(f.feat[l] != nullptr, MXDET_EINVAL, "%s: level %d has no map", who, l);
  }
  const int NB = d->PH * d->PW;
  MXDET_REQUIRE(!trans || d->trans_stride >= 2 * NB, MXDET_ESHAPE, "%s: trans_stride %d < 2 * PH * PW", who,
                d->trans_stride);
  MXDET_REQUIRE(!d->modulated || (trans && mask), MXDET_EINVAL, "%s: modulated needs trans and mask_logit", who);
  MXDET_REQUIRE(!d->modulated || d->mask_stride >= NB, MXDET_ESHAPE, "%s: mask_stride %d < PH * PW", who,
                d->mask_stride);
  memset(a, 0, sizeof(*a));
  pyr_copy(a->p, f, d->N);
  a->C = d->C;
  a->PH = d->PH; a->PW = d->PW; a->NB = NB; a->S = d->sample_per_part;
  a->mod = d->modulated ? 1 : 0; a->ts = d->trans_stride; a->ms = d->mask_stride; a->acc = d->accumulate ? 1 : 0;
  a->trans_std = d->trans_std;
  return MXDET_OK;
}

static size_t dpool_carve(long long R, int NB, size_t* o_roi, size_t* o_bin) {
  size_t off = 0;
  *o_roi = off; off = align_up(off + (size_t)R * sizeof(DpRoiRec), 256);
  *o_bin = off; off = align_up(off + (size_t)R * NB * sizeof(DpBinRec), 256);
  return off > 256 ? off : 256;
}

}  // namespace mxdet

using namespace mxdet;

extern "C" int mxdet_dpool_fwd(const mxdet_dpool_desc_t* d, const float* rois, const int32_t* levels, int64_t R,
                               const uint16_t* trans, const uint16_t* mask_logit, uint16_t* out, mxdet_stream_t stream) {
  clear_error();
  DPoolArgs a;
  int rc = dpool_check(d, &a, R, trans, mask_logit, "dpool_fwd");
  if (rc) return rc;
  if (R == 0) return MXDET_OK;
  MXDET_REQUIRE(rois && levels && out, MXDET_EINVAL, "dpool_fwd: null pointer");
  hipLaunchKernelGGL(dpool_fwd_kernel, dim3((unsigned)R), dim3(256), 0, as_stream(stream), a, rois, levels, trans,
                     a.mod ? mask_logit : nullptr, out);
  return check_launch("dpool_fwd");
}

extern "C" int mxdet_dpool_bwd_trans(const mxdet_dpool_desc_t* d, const float* rois, const int32_t* levels, int64_t R,
                                     const uint16_t* trans, const uint16_t* mask_logit, const uint16_t* dout,
                                     uint16_t* d_trans, uint16_t* d_mask, mxdet_stream_t stream) {
  clear_error();
  DPoolArgs a;
  int rc = dpool_check(d, &a, R, trans, mask_logit, "dpool_bwd_trans");
  if (rc) return rc;
  MXDET_REQUIRE(trans && d_trans && (!a.mod || d_mask), MXDET_EINVAL,
                "dpool_bwd_trans: needs trans, d_trans and (modulated) d_mask");
  if (R == 0) return MXDET_OK;
  MXDET_REQUIRE(rois && levels && dout, MXDET_EINVAL, "dpool_bwd_trans: null pointer");
  const long long items = (long long)R * a.NB * 64;
  hipLaunchKernelGGL(dpool_bwd_trans_kernel, dim3((unsigned)ceil_div(items, 256ll)), dim3(256), 0, as_stream(stream), a,
                     (long long)R, rois, levels, trans, a.mod ? mask_logit : nullptr, dout, d_trans, d_mask);
  return check_launch("dpool_bwd_trans");
}

extern "C" size_t mxdet_dpool_bwd_feat_workspace_bytes(const mxdet_dpool_desc_t* d, int64_t R) {
  if (!d || R < 0 || d->PH <= 0 || d->PW <= 0 || d->PH * d->PW > 64) return 0;
  size_t a, b;
  return dpool_carve(R, d->PH * d->PW, &a, &b);
}

extern "C" int mxdet_dpool_bwd_feat(const mxdet_dpool_desc_t* d, const float* rois, const int32_t* levels, int64_t R,
                                    const uint16_t* trans, const uint16_t* mask_logit, const uint16_t* dout,
                                    void* workspace, size_t workspace_bytes, mxdet_stream_t stream) {
  clear_error();
  DPoolArgs a;
  int rc = dpool_check(d, &a, R, trans, mask_logit, "dpool_bwd_feat");
  if (rc) return rc;
  MXDET_REQUIRE(R == 0 || (rois && levels && dout), MXDET_EINVAL, "dpool_bwd_feat: null pointer");
  size_t o_roi, o_bin;
  const size_t need = dpool_carve(R, a.NB, &o_roi, &o_bin);
  MXDET_REQUIRE(workspace && workspace_bytes >= need, MXDET_EWORKSPACE, "dpool_bwd_feat: workspace %zu < %zu",
                workspace_bytes, need);
  if (R == 0 && a.acc) return MXDET_OK;
  hipStream_t s = as_stream(stream);
  DpRoiRec* roi = (DpRoiRec*)((char*)workspace + o_roi);
  DpBinRec* bin = (DpBinRec*)((char*)workspace + o_bin);
  if (R > 0)
    hipLaunchKernelGGL(dpool_prepare_kernel, dim3((unsigned)R), dim3(64), 0, s, a, (long long)R, rois, levels, trans,
                       a.mod ? mask_logit : nullptr, roi, bin);
  DpGrid gr;
  memset(&gr, 0, sizeof(gr));
  int blocks_of[8];
  for (int l = 0; l < a.p.num_levels; ++l) {
    gr.chunks[l] = ceil_div(a.p.W[l], kSegWaves * kSegW);
    blocks_of[l] = a.p.N * a.p.H[l] * gr.chunks[l];
  }
  const int blocks = layout_block0(gr.block0, blocks_of, a.p.num_levels);
  hipLaunchKernelGGL(dpool_gather_kernel, dim3((unsigned)blocks, (unsigned)ceil_div(a.C, 256)), dim3(kSegWaves * 64), 0, s,
                     a, gr, (int)R, (const DpRoiRec*)roi, (const DpBinRec*)bin, dout);
  return check_launch("dpool_bwd_feat");
}
