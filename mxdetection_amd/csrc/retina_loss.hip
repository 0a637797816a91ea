// retina_loss.hip -- RetinaNet (BASELINE.json config 5): dense-anchor class labels and the fused class + box loss of one
// level, forward and backward in one pass (the conventions of losses.hip). Four entries share one grid (256 consecutive
// anchors per workgroup), one vector / scalar split and the pieces below: smooth-L1 (mxdet_retina_loss_level), an IoU-family
// box term (_iou), that with a quality-aware class term (_quality, 5j), and the distribution head (_dfl, 5k).
// The gradient-harmonized losses (5v) add a histogram pass on the same grid, a weights kernel and a fifth level entry (_ghm).
#include "common.h"
#include "loss_elem.h"

namespace mxdet {

// cls_label = class of the matched GT for foreground anchors, else the {-1, 0} label itself
__global__ void anchor_class_labels_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ matched,
                                           const float* __restrict__ gt, long long A_total, int G_max, long long total,
                                           int32_t* __restrict__ cls_labels, int* __restrict__ num_fg) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int lab = -1;
  bool fg = false;
  if (i < total) {
    lab = labels[i];
    if (lab == 1) {
      int n = (int)(i / A_total);
      lab = (int)gt[((long long)n * G_max + matched[i]) * 5 + 4];
      fg = true;
    }
    cls_labels[i] = lab;
  }
  unsigned long long m = __ballot(fg);
  if (lane_id() == 0 && m) atomicAdd(num_fg, __popcll(m));
}

// Anchor idx of the level's N * HW * A, in the order of the head's output: anchor a of cell `cell` = n * HW + local.
// ai: its row of the anchor table, gi: its row of the [N, A_total] label / match / target tables.
struct LevelAnchor {
  int a, n;
  long long cell, ai, gi;
  __device__ __forceinline__ long long cls_off(int ld_cls, int C) const { return cell * ld_cls + (long long)a * C; }
  __device__ __forceinline__ long long box_off(int ld_reg, int per) const { return cell * ld_reg + (long long)a * per; }
};
__device__ __forceinline__ LevelAnchor level_anchor(long long idx, int HW, int A, long long A_total, long long level_offset) {
  LevelAnchor la;
  la.a = (int)(idx % A);
  la.cell = idx / A;
  la.n = (int)(la.cell / HW);
  la.ai = level_offset + (la.cell - (long long)la.n * HW) * A + la.a;
  la.gi = (long long)la.n * A_total + la.ai;
  return la;
}

// Class walk of the vector form (C % 8 == 0): the workgroup's 256 anchors, 16 bytes of class logits per lane and step,
// consecutive lanes on consecutive addresses -- the scalar form below has every lane striding C*2 bytes apart with 2-byte
// accesses (920 us per step on RetinaNet-R101 for 129 MB). elem: FocalElem or QualityElem; qs (not read for focal): the
// quality of the workgroup's anchor al in LDS, 0 unless it is foreground with a match inside gt_boxes. Returns this
// thread's loss sum.
template <class Elem>
__device__ __forceinline__ float class_walk_vec(const uint16_t* __restrict__ cls, int HW, int A, int C, int ld_cls,
                                                const int32_t* __restrict__ cls_labels, long long A_total,
                                                long long level_offset, const Elem elem, const float* __restrict__ qs,
                                                float inv, float loss_scale, long long a_first, long long total,
                                                uint16_t* __restrict__ gcls) {
  const int CH = C >> 3;
  float lc = 0.0f;
  for (int it = threadIdx.x; it < 256 * CH; it += 256) {
    const int al = it / CH, ck = it - al * CH;
    const long long idx = a_first + al;
    if (idx >= total) continue;
    const LevelAnchor la = level_anchor(idx, HW, A, A_total, level_offset);
    const int lab = cls_labels[la.gi];
    const long long off = la.cls_off(ld_cls, C) + ck * 8;
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    if (lab >= 0) {
      const float qa = Elem::kQuality ? qs[al] : 0.0f;
      const uint4 zv = *(const uint4*)(cls + off);
      const unsigned zw[4] = {zv.x, zv.y, zv.z, zv.w};
      unsigned ow[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        unsigned packed = 0u;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int c = ck * 8 + 2 * k + h;
          const float x = h ? __uint_as_float(zw[k] & 0xffff0000u) : __uint_as_float(zw[k] << 16);
          float g;
          lc += elem(x, lab == c + 1, qa, g);
          packed |= (unsigned)f32_to_bf16_bits(g * inv * loss_scale) << (16 * h);
        }
        ow[k] = packed;
      }
      o = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    }
    *(uint4*)(gcls + off) = o;
  }
  return lc;
}

// class walk of the scalar form: the C logits of one anchor, its quality in a register
template <class Elem>
__device__ __forceinline__ float class_walk_anchor(const uint16_t* __restrict__ z, int C, int lab, const Elem elem, float qa,
                                                   float inv, float loss_scale, uint16_t* __restrict__ gz) {
  float lc = 0.0f;
  for (int c = 0; c < C; ++c) {
    float g = 0.0f;
    if (lab >= 0) lc += elem(bf16_bits_to_f32(z[c]), lab == c + 1, qa, g);
    gz[c] = f32_to_bf16_bits(g * inv * loss_scale);
  }
  return lc;
}

// an anchor's four bf16 box channels: one 8-byte access (VEC) or four 2-byte ones
template <bool VEC>
__device__ __forceinline__ void load_box4(const uint16_t* __restrict__ d, float* dd) {
  if (VEC) {
    unpack4_bf16(*(const uint2*)d, dd);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) dd[k] = bf16_bits_to_f32(d[k]);
  }
}
template <bool VEC>
__device__ __forceinline__ void store_box4(uint16_t* __restrict__ gd, const unsigned short* gb) {
  if (VEC) {
    *(uint2*)gd = make_uint2((unsigned)gb[0] | ((unsigned)gb[1] << 16), (unsigned)gb[2] | ((unsigned)gb[3] << 16));
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) gd[k] = gb[k];
  }
}

// Smooth-L1 box part of one anchor: deltas at d against *target (null: the anchor regresses nothing), gradient to gd.
template <bool VEC>
__device__ __forceinline__ float smooth_l1_box_part(const uint16_t* __restrict__ d, const float4* __restrict__ target,
                                                    float sigma2, float inv, float loss_scale, uint16_t* __restrict__ gd) {
  float lr = 0.0f;
  unsigned short gb[4] = {0, 0, 0, 0};
  if (target) {
    const float4 t = *target;
    const float tt[4] = {t.x, t.y, t.z, t.w};
    float dd[4];
    load_box4<VEC>(d, dd);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float e = dd[k] - tt[k];
      lr += mxdet_smooth_l1(e, sigma2);
      gb[k] = f32_to_bf16_bits(mxdet_smooth_l1_grad(e, sigma2) * inv * loss_scale);
    }
  }
  store_box4<VEC>(gd, gb);
  return lr;
}

// IoU-family box part of one anchor on its raw deltas: the anchor and the GT row as 16-byte loads, nothing staged (it is
// a few bytes per anchor next to the C class logits). m: the matched row of image n's gt_boxes; outside [0, G_max) the
// anchor regresses nothing. Returns the weighted loss; *iou (optional) = inter / union, untouched without a match.
template <bool VEC>
__device__ __forceinline__ float delta_box_part(const uint16_t* __restrict__ d, const float4* __restrict__ anchor,
                                                const float* __restrict__ gt, int n, int m, int G_max, int kind, BoxStds sd,
                                                float reg_weight, float inv, float loss_scale, uint16_t* __restrict__ gd,
                                                float* iou) {
  float lr = 0.0f;
  unsigned short gb[4] = {0, 0, 0, 0};
  if (m >= 0 && m < G_max) {
    float dd[4], g4[4];
    load_box4<VEC>(d, dd);
    const float4 g = load_f4_a4(gt + ((long long)n * G_max + m) * 5);
    lr = reg_weight * box_iou_loss_elem(*anchor, g, dd, sd, kind, g4, iou);
    const float gs = reg_weight * inv * loss_scale;
#pragma unroll
    for (int k = 0; k < 4; ++k) gb[k] = f32_to_bf16_bits(g4[k] * gs);
  }
  store_box4<VEC>(gd, gb);
  return lr;
}

// one thread per (cell, anchor): C contiguous class logits at cls[cell*ld_cls + a*C], 4 deltas at reg[cell*ld_reg + a*4].
// VEC: the 16-byte class walk and 8-byte box accesses; a workgroup owns 256 consecutive anchors in either form, so the
// partial-sum layout does not depend on it.
template <bool VEC>
__global__ void __launch_bounds__(256)
retina_loss_kernel(const uint16_t* __restrict__ cls, const uint16_t* __restrict__ reg, int N, int HW, int A, int C,
                   int ld_cls, int ld_reg, const int32_t* __restrict__ cls_labels, const float4* __restrict__ targets,
                   long long A_total, long long level_offset, float alpha, float gamma, float sigma2,
                   const int* __restrict__ num_fg, float loss_scale, uint16_t* __restrict__ gcls,
                   uint16_t* __restrict__ greg, float* __restrict__ partial) {
  __shared__ float red[8];
  const long long total = (long long)N * HW * A;
  const long long a_first = (long long)blockIdx.x * 256;
  const long long idx = a_first + threadIdx.x;
  const int nf = *num_fg;
  const float inv = 1.0f / (float)(nf > 1 ? nf : 1);
  const FocalElem elem = {alpha, gamma};
  float lc = 0.0f, lr = 0.0f;
  if (VEC)
    lc = class_walk_vec(cls, HW, A, C, ld_cls, cls_labels, A_total, level_offset, elem, nullptr, inv, loss_scale, a_first,
                        total, gcls);
  if (idx < total) {
    const LevelAnchor la = level_anchor(idx, HW, A, A_total, level_offset);
    const int lab = cls_labels[la.gi];
    const long long coff = la.cls_off(ld_cls, C), roff = la.box_off(ld_reg, 4);
    if (!VEC) lc = class_walk_anchor(cls + coff, C, lab, elem, 0.0f, inv, loss_scale, gcls + coff);
    lr = smooth_l1_box_part<VEC>(reg + roff, lab > 0 ? targets + la.gi : nullptr, sigma2, inv, loss_scale, greg + roff);
  }
  store_block_partials<2>({lc, lr}, inv, red, partial);
}

// The level loss with an IoU-family box term, and (QUALITY) a quality-aware class term in place of the focal one
// (DESIGN.md 5f, 5j): grid, partial sums and the vector / scalar split of retina_loss_kernel<VEC>. Without QUALITY the
// class walk comes first, as in that kernel. With it the box part runs FIRST -- lane t on anchor a_first + t -- and leaves
// the anchor's quality inter / union; the 16-byte class walk visits the workgroup's anchors with another lane mapping, so
// the 256 qualities cross through LDS behind one barrier that every lane reaches. The scalar form keeps it in a register.
template <bool VEC, bool QUALITY>
__global__ void __launch_bounds__(256)
retina_loss_iou_kernel(const uint16_t* __restrict__ cls, const uint16_t* __restrict__ reg, int N, int HW, int A, int C,
                       int ld_cls, int ld_reg, const int32_t* __restrict__ cls_labels, const float4* __restrict__ anchors,
                       const int32_t* __restrict__ matched, const float* __restrict__ gt, int G_max, long long A_total,
                       long long level_offset, int cls_kind, float alpha, float gamma, int kind, BoxStds sd,
                       float reg_weight, const int* __restrict__ num_fg, float loss_scale, uint16_t* __restrict__ gcls,
                       uint16_t* __restrict__ greg, float* __restrict__ partial) {
  __shared__ float red[8];
  const long long total = (long long)N * HW * A;
  const long long a_first = (long long)blockIdx.x * 256;
  const long long idx = a_first + threadIdx.x;
  const int nf = *num_fg;
  const float inv = 1.0f / (float)(nf > 1 ? nf : 1);
  const FocalElem focal = {alpha, gamma};
  float lc = 0.0f, lr = 0.0f, qa = 0.0f;
  int lab = -1;
  long long coff = 0;                                     // this lane's anchor: first class logit
  if constexpr (VEC && !QUALITY)
    lc = class_walk_vec(cls, HW, A, C, ld_cls, cls_labels, A_total, level_offset, focal, nullptr, inv, loss_scale, a_first,
                        total, gcls);
  if (idx < total) {
    const LevelAnchor la = level_anchor(idx, HW, A, A_total, level_offset);
    lab = cls_labels[la.gi];
    coff = la.cls_off(ld_cls, C);
    if constexpr (!VEC && !QUALITY) lc = class_walk_anchor(cls + coff, C, lab, focal, 0.0f, inv, loss_scale, gcls + coff);
    const long long roff = la.box_off(ld_reg, 4);
    lr = delta_box_part<VEC>(reg + roff, anchors + la.ai, gt, la.n, lab > 0 ? matched[la.gi] : -1, G_max, kind, sd, reg_weight,
                             inv, loss_scale, greg + roff, QUALITY ? &qa : nullptr);
  }
  if constexpr (QUALITY) {
    const QualityElem elem = {cls_kind, alpha, gamma};
    if constexpr (VEC) {
      __shared__ float qs[256];
      qs[threadIdx.x] = qa;
      __syncthreads();
      lc = class_walk_vec(cls, HW, A, C, ld_cls, cls_labels, A_total, level_offset, elem, qs, inv, loss_scale, a_first, total,
                          gcls);
    } else if (idx < total) {
      lc = class_walk_anchor(cls + coff, C, lab, elem, qa, inv, loss_scale, gcls + coff);
    }
  }
  store_block_partials<2>({lc, lr}, inv, red, partial);
}

// The level loss of the distribution head: the grid of the other level kernels (256 anchors per workgroup),
// three partial sums per workgroup (class, box, DFL). Phases, each behind a barrier that every lane reaches:
//   1  lane t on anchor a_first + t: label and match -> ms[t] (>= 0: the anchor regresses against that row of gt_boxes)
//   2  zeros into the 4 (R + 1) gradient channels of every anchor that does not regress: 8-byte stores on consecutive
//      addresses (VEC) or 2-byte ones; an anchor's channels start a multiple of 8 bytes into its 8-byte aligned row
//   3  four lanes per regressing anchor, 64 anchors per pass over the workgroup's COMPACTED list of them (dist_box_quad);
//      side 0 keeps the sums and leaves the quality in qs[]. A workgroup holds a handful of positives: one pass, where
//      a fixed anchor-to-quad map needs four, each as long as its slowest quad.
//   4  the class walk of the other level kernels, on the focal element (FOCAL) or the quality one with qs[]
template <bool VEC, bool FOCAL>
__global__ void __launch_bounds__(256)
retina_loss_dfl_kernel(const uint16_t* __restrict__ cls, const uint16_t* __restrict__ reg, int N, int HW, int A, int C,
                       int ld_cls, int ld_reg, const int32_t* __restrict__ cls_labels, const float4* __restrict__ anchors,
                       const int32_t* __restrict__ matched, const float* __restrict__ gt, int G_max, long long A_total,
                       long long level_offset, int cls_kind, float alpha, float gamma, int kind, int R, float stride,
                       float reg_weight, float dfl_weight, const int* __restrict__ num_fg, float loss_scale,
                       uint16_t* __restrict__ gcls, uint16_t* __restrict__ greg, float* __restrict__ partial) {
  __shared__ float red[8];
  __shared__ float qs[256];
  __shared__ int ms[256];
  __shared__ long long roff[256];                         // first gradient channel of the workgroup's anchors
  __shared__ int plist[256], cnt[5];                      // the regressing anchors, in anchor order
  const long long total = (long long)N * HW * A;
  const long long a_first = (long long)blockIdx.x * 256;
  const long long idx = a_first + threadIdx.x;
  const int nf = *num_fg;
  const float inv = 1.0f / (float)(nf > 1 ? nf : 1);
  const int nb = R + 1;
  float lc = 0.0f, lr = 0.0f, ldf = 0.0f;
  int lab = -1, mt = -2;                                  // mt -2: no such anchor
  long long coff = 0, goff = 0;
  if (idx < total) {
    const LevelAnchor la = level_anchor(idx, HW, A, A_total, level_offset);
    lab = cls_labels[la.gi];
    coff = la.cls_off(ld_cls, C);
    goff = la.box_off(ld_reg, 4 * nb);
    const int m = lab > 0 ? matched[la.gi] : -1;
    mt = (m >= 0 && m < G_max) ? m : -1;                  // a match outside gt_boxes: regresses nothing, quality 0
  }
  ms[threadIdx.x] = mt;
  roff[threadIdx.x] = goff;
  qs[threadIdx.x] = 0.0f;
  int npos;
  const int rank = block_excl_count(mt >= 0, cnt, &npos);
  if (mt >= 0) plist[rank] = threadIdx.x;
  __syncthreads();
  const int per = VEC ? nb : 4 * nb;                      // stores per anchor (<= 128: it < 2^15, fast_divmod is exact)
  const float rper = 1.0f / (float)per;
  for (int it = threadIdx.x; it < 256 * per; it += 256) {
    int ck;
    const int al = fast_divmod(it, per, rper, &ck);
    if (ms[al] != -1) continue;
    const long long off = roff[al];
    if (VEC)
      *(uint2*)(greg + off + 4 * ck) = make_uint2(0u, 0u);
    else
      greg[off + ck] = 0;
  }
  for (int j = threadIdx.x >> 2; j < npos; j += 64) {     // the four lanes of a quad share j
    const int al = plist[j], side = threadIdx.x & 3;
    const int m = ms[al];
    const LevelAnchor la = level_anchor(a_first + al, HW, A, A_total, level_offset);
    const float4 g = load_f4_a4(gt + ((long long)la.n * G_max + m) * 5);
    float dfl, q;
    const float L = dist_box_quad(reg, roff[al] + side * nb, MXDET_DTYPE_BF16, R, side,
                                  anchors[la.ai], g, stride, kind, reg_weight, dfl_weight, inv * loss_scale, greg, dfl, q);
    const int q0 = lane_id() & ~3;
    const float dsum = ((__shfl(dfl, q0 + 0) + __shfl(dfl, q0 + 1)) + __shfl(dfl, q0 + 2)) + __shfl(dfl, q0 + 3);
    if (side == 0) {
      lr += reg_weight * L;
      ldf += dfl_weight * 0.25f * dsum;
      qs[al] = q;
    }
  }
  __syncthreads();
  const auto walk = [&](const auto elem) {
    if (VEC)
      return class_walk_vec(cls, HW, A, C, ld_cls, cls_labels, A_total, level_offset, elem, qs, inv, loss_scale, a_first, total,
                            gcls);
    if (idx >= total) return 0.0f;
    return class_walk_anchor(cls + coff, C, lab, elem, elem.kQuality ? qs[threadIdx.x] : 0.0f, inv, loss_scale, gcls + coff);
  };
  if constexpr (FOCAL)
    lc = walk(FocalElem{alpha, gamma});
  else
    lc = walk(QualityElem{cls_kind, alpha, gamma});
  store_block_partials<3>({lc, lr, ldf}, inv, red, partial);
}

// ---------------------------------------------------------------------------------------------
// Gradient harmonizing (definition in include/mxdet.h). Three kernels per step: a histogram pass per level
// (ghm_hist_kernel), one weights launch (ghm_weights_kernel), a loss pass per level (retina_loss_ghm_kernel). The two
// passes share the grid, the anchor-to-workgroup map and ghm_cls_norm / ghm_reg_norm / ghm_bin of loss_elem.h.
constexpr int kGhmRow = 2 * MXDET_GHM_MAX_BINS;           // most counts of one row: class bins, then box bins

// One class element of each of the wave's 64 lanes into the wave's own histogram wh; b < 0: the lane has nothing to count.
// Every lane of the wave calls this together. The lanes that agree with the first counting lane's bin go in as ONE add of
// their number -- at initialisation (every g near 0.01) and for the negatives of a trained model that is all of them --
// and only the others add for themselves. Integer counts: the order of the adds does not show in the result.
__device__ __forceinline__ void ghm_wave_count(int* wh, const int b) {
  const unsigned long long vm = __ballot(b >= 0);
  if (vm == 0ull) return;
  const int first = __ffsll(vm) - 1;
  const int b0 = __builtin_amdgcn_readlane(b, first);
  const unsigned long long m = __ballot(b == b0);
  if (lane_id() == first) atomicAdd(&wh[b0], (int)__popcll(m));
  if (b >= 0 && b != b0) atomicAdd(&wh[b], 1);
}

// Histogram pass of one level: workgroup i counts its 256 anchors' valid elements and writes row i of `counts`:
// Bc class bins, then Br box bins (zeros for a half that `flags` leaves out). Per-wave histograms in LDS, summed per row.
template <bool VEC>
__global__ void __launch_bounds__(256)
ghm_hist_kernel(const uint16_t* __restrict__ cls, const uint16_t* __restrict__ reg, int N, int HW, int A, int C, int ld_cls,
                int ld_reg, const int32_t* __restrict__ cls_labels, const float4* __restrict__ targets, long long A_total,
                long long level_offset, int flags, int Bc, int Br, float mu, int32_t* __restrict__ counts) {
  __shared__ int hist[4][kGhmRow];
  for (int i = threadIdx.x; i < 4 * kGhmRow; i += 256) (&hist[0][0])[i] = 0;
  __syncthreads();
  int* wh = hist[threadIdx.x >> 6];
  const long long total = (long long)N * HW * A;
  const long long a_first = (long long)blockIdx.x * 256;
  const long long idx = a_first + threadIdx.x;
  if (flags & MXDET_GHM_CLS) {
    if (VEC) {                                            // the lane map of class_walk_vec; C / 8 trips for every lane
      const int CH = C >> 3;
      for (int it = threadIdx.x; it < 256 * CH; it += 256) {
        const int al = it / CH, ck = it - al * CH;
        const long long ia = a_first + al;
        int lab = -1;
        uint4 zv = make_uint4(0u, 0u, 0u, 0u);
        if (ia < total) {
          const LevelAnchor la = level_anchor(ia, HW, A, A_total, level_offset);
          lab = cls_labels[la.gi];
          if (lab >= 0) zv = *(const uint4*)(cls + la.cls_off(ld_cls, C) + ck * 8);
        }
        const unsigned zw[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int c = ck * 8 + 2 * k + h;
            const float x = h ? __uint_as_float(zw[k] & 0xffff0000u) : __uint_as_float(zw[k] << 16);
            float p, q, logp, log1mp;
            const float g = ghm_cls_norm(x, lab == c + 1, p, q, logp, log1mp);
            ghm_wave_count(wh, lab >= 0 ? ghm_bin(g, Bc) : -1);
          }
        }
      }
    } else {                                              // the lane's own anchor, C trips for every lane
      int lab = -1;
      long long coff = 0;
      if (idx < total) {
        const LevelAnchor la = level_anchor(idx, HW, A, A_total, level_offset);
        lab = cls_labels[la.gi];
        coff = la.cls_off(ld_cls, C);
      }
      for (int c = 0; c < C; ++c) {
        const float x = lab >= 0 ? bf16_bits_to_f32(cls[coff + c]) : 0.0f;
        float p, q, logp, log1mp;
        const float g = ghm_cls_norm(x, lab == c + 1, p, q, logp, log1mp);
        ghm_wave_count(wh, lab >= 0 ? ghm_bin(g, Bc) : -1);
      }
    }
  }
  if ((flags & MXDET_GHM_REG) && idx < total) {           // a handful of anchors per workgroup: plain adds
    const LevelAnchor la = level_anchor(idx, HW, A, A_total, level_offset);
    if (cls_labels[la.gi] > 0) {
      const float4 t = targets[la.gi];
      const float tt[4] = {t.x, t.y, t.z, t.w};
      float dd[4];
      load_box4<VEC>(reg + la.box_off(ld_reg, 4), dd);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float r;
        atomicAdd(&wh[Bc + ghm_bin(ghm_reg_norm(dd[k] - tt[k], mu, r), Br)], 1);
      }
    }
  }
  __syncthreads();
  const int nb = Bc + Br;
  if ((int)threadIdx.x < nb)
    counts[(long long)blockIdx.x * nb + threadIdx.x] =
        ((hist[0][threadIdx.x] + hist[1][threadIdx.x]) + hist[2][threadIdx.x]) + hist[3][threadIdx.x];
}

// The step's weights: cnt = the column sums of the `rows` rows, the moving average acc updated in place for the bins that
// hold something, coef = 1 / (n * acc) for those (n = their number, per histogram) and 0 for the others. One workgroup:
// thread (g, i) sums bin i over the rows r = g mod 8, the eight sums are added in order.
__global__ void __launch_bounds__(1024)
ghm_weights_kernel(const int32_t* __restrict__ counts, int rows, int Bc, int Br, float mmt_c, float mmt_r,
                   float* __restrict__ acc, int32_t* __restrict__ cnt, float* __restrict__ coef) {
  __shared__ int part[8][kGhmRow];
  __shared__ int tot[kGhmRow];
  const int nb = Bc + Br, i = threadIdx.x & (kGhmRow - 1), rg = threadIdx.x >> 7;
  int s = 0;
  if (i < nb)
    for (int r = rg; r < rows; r += 8) s += counts[(long long)r * nb + i];
  part[rg][i] = s;
  __syncthreads();
  if (threadIdx.x < kGhmRow) {
    int c = 0;
    for (int g = 0; g < 8; ++g) c += part[g][i];
    tot[i] = c;
  }
  __syncthreads();
  if ((int)threadIdx.x < nb) {
    const bool is_cls = i < Bc;
    const int lo = is_cls ? 0 : Bc, hi = is_cls ? Bc : nb;
    int n = 0;
    for (int j = lo; j < hi; ++j) n += tot[j] > 0 ? 1 : 0;
    const int c = tot[i];
    const float mmt = is_cls ? mmt_c : mmt_r;
    float w = 0.0f;
    if (c > 0) {
      float a = (float)c;
      if (mmt > 0.0f) {
        const float keep = mmt * acc[i], add = (1.0f - mmt) * (float)c;
        a = keep + add;
      }
      acc[i] = a;
      w = 1.0f / ((float)n * a);
    }
    cnt[i] = c;
    coef[i] = w;
  }
}

// Harmonized box part of one anchor (the deltas of smooth_l1_box_part): sum of coef[bin] * (sqrt(d*d + mu*mu) - mu),
// gradient coef[bin] * d / sqrt(d*d + mu*mu) * w * loss_scale.
template <bool VEC>
__device__ __forceinline__ float ghm_box_part(const uint16_t* __restrict__ d, const float4* __restrict__ target, float mu,
                                              const float* coef, int B, float w, float loss_scale,
                                              uint16_t* __restrict__ gd) {
  float lr = 0.0f;
  unsigned short gb[4] = {0, 0, 0, 0};
  if (target) {
    const float4 t = *target;
    const float tt[4] = {t.x, t.y, t.z, t.w};
    float dd[4];
    load_box4<VEC>(d, dd);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float e = dd[k] - tt[k];
      float r;
      const float c = coef[ghm_bin(ghm_reg_norm(e, mu, r), B)];
      lr += c * (r - mu);
      gb[k] = f32_to_bf16_bits(c * (e / r) * w * loss_scale);
    }
  }
  store_box4<VEC>(gd, gb);
  return lr;
}

// retina_loss_kernel<VEC> with the class element (GC) and / or the box element (GR) harmonized: the step's weights come
// from `coef` (Bc class, then Br box) into LDS once per workgroup. A harmonized term is scaled by its weight w_c / w_r,
// not by 1 / num_fg; the other half is retina_loss_kernel's statement for statement.
template <bool VEC, bool GC, bool GR>
__global__ void __launch_bounds__(256)
retina_loss_ghm_kernel(const uint16_t* __restrict__ cls, const uint16_t* __restrict__ reg, int N, int HW, int A, int C,
                       int ld_cls, int ld_reg, const int32_t* __restrict__ cls_labels, const float4* __restrict__ targets,
                       long long A_total, long long level_offset, float alpha, float gamma, float sigma2,
                       const float* __restrict__ coef, int Bc, int Br, float w_c, float mu, float w_r,
                       const int* __restrict__ num_fg, float loss_scale, uint16_t* __restrict__ gcls,
                       uint16_t* __restrict__ greg, float* __restrict__ partial) {
  __shared__ float red[8];
  __shared__ float cf[kGhmRow];
  if ((int)threadIdx.x < Bc + Br) cf[threadIdx.x] = coef[threadIdx.x];
  __syncthreads();
  const long long total = (long long)N * HW * A;
  const long long a_first = (long long)blockIdx.x * 256;
  const long long idx = a_first + threadIdx.x;
  const int nf = *num_fg;
  const float inv = 1.0f / (float)(nf > 1 ? nf : 1);
  const float sc = GC ? w_c : inv, sr = GR ? w_r : inv;
  int lab = -1;
  long long coff = 0, roff = 0, gi = 0;
  if (idx < total) {
    const LevelAnchor la = level_anchor(idx, HW, A, A_total, level_offset);
    lab = cls_labels[la.gi];
    coff = la.cls_off(ld_cls, C);
    roff = la.box_off(ld_reg, 4);
    gi = la.gi;
  }
  const auto walk = [&](const auto elem) {
    if (VEC)
      return class_walk_vec(cls, HW, A, C, ld_cls, cls_labels, A_total, level_offset, elem, nullptr, sc, loss_scale, a_first,
                            total, gcls);
    if (idx >= total) return 0.0f;
    return class_walk_anchor(cls + coff, C, lab, elem, 0.0f, sc, loss_scale, gcls + coff);
  };
  float lc, lr = 0.0f;
  if constexpr (GC)
    lc = walk(GhmClsElem{cf, Bc});
  else
    lc = walk(FocalElem{alpha, gamma});
  if (idx < total) {
    const float4* tgt = lab > 0 ? targets + gi : nullptr;
    if constexpr (GR)
      lr = ghm_box_part<VEC>(reg + roff, tgt, mu, cf + Bc, Br, w_r, loss_scale, greg + roff);
    else
      lr = smooth_l1_box_part<VEC>(reg + roff, tgt, sigma2, inv, loss_scale, greg + roff);
  }
  store_block_partials<2>({lc, lr}, {sc, sr}, red, partial);
}

}  // namespace mxdet

using namespace mxdet;

extern "C" int mxdet_anchor_class_labels(const int32_t* labels, const int32_t* matched_gt, const float* gt_boxes,
                                         int32_t N, int64_t A_total, int32_t G_max, int32_t* cls_labels,
                                         int32_t* num_fg, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(N > 0 && A_total > 0 && G_max > 0, MXDET_ESHAPE, "anchor_class_labels: bad shape");
  MXDET_REQUIRE(labels && matched_gt && gt_boxes && cls_labels && num_fg, MXDET_EINVAL, "anchor_class_labels: null pointer");
  hipStream_t s = as_stream(stream);
  hipError_t e = zero_async(num_fg, sizeof(int32_t), s);
  MXDET_REQUIRE(e == hipSuccess, MXDET_EHIP, "anchor_class_labels: memset failed");
  long long total = (long long)N * A_total;
  hipLaunchKernelGGL(anchor_class_labels_kernel, dim3((unsigned)ceil_div<long long>(total, 256)), dim3(256), 0, s, labels,
                     matched_gt, gt_boxes, (long long)A_total, G_max, total, cls_labels, num_fg);
  return check_launch("anchor_class_labels");
}

// 16-byte form: whole 8-channel chunks per anchor and 16-B / 8-B aligned rows
static bool level_vec_ok(const uint16_t* cls, const uint16_t* reg, int32_t C, int32_t ld_cls, int32_t ld_reg,
                         const uint16_t* grad_cls, const uint16_t* grad_reg) {
  return (C % 8 == 0) && (ld_cls % 8 == 0) && (ld_reg % 4 == 0) && (((uintptr_t)cls | (uintptr_t)grad_cls) % 16 == 0) &&
         (((uintptr_t)reg | (uintptr_t)grad_reg) % 8 == 0);
}

extern "C" int32_t mxdet_retina_loss_num_partials(int32_t N, int32_t H, int32_t W, int32_t A) {
  return (int32_t)(((long long)N * H * W * A + 255) / 256);
}

extern "C" int mxdet_retina_loss_level(const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W,
                                       int32_t A, int32_t C, int32_t ld_cls, int32_t ld_reg,
                                       const int32_t* cls_labels, const float* bbox_targets, int64_t A_total,
                                       int64_t level_offset, float alpha, float gamma, float sigma,
                                       const int32_t* num_fg, float loss_scale, uint16_t* grad_cls,
                                       uint16_t* grad_reg, float* partial, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(N > 0 && H > 0 && W > 0 && A > 0 && C > 0 && ld_cls >= A * C && ld_reg >= 4 * A, MXDET_ESHAPE,
                "retina_loss_level: bad shape");
  MXDET_REQUIRE(cls && reg && cls_labels && bbox_targets && num_fg && grad_cls && grad_reg && partial, MXDET_EINVAL,
                "retina_loss_level: null pointer");
  MXDET_REQUIRE(level_offset >= 0 && level_offset + (int64_t)H * W * A <= A_total, MXDET_ESHAPE,
                "retina_loss_level: level outside the anchor range");
  int blocks = mxdet_retina_loss_num_partials(N, H, W, A);
  const bool vec = level_vec_ok(cls, reg, C, ld_cls, ld_reg, grad_cls, grad_reg);
  if (route_probe_on()) {   // mxdet_debug_route_probe: say which form would run, touch nothing
    const int32_t rec[kRouteWords] = {MXDET_ROUTE_RETINA_LOSS, vec ? 1 : 0, blocks};
    route_record(rec);
    return MXDET_OK;
  }
  hipLaunchKernelGGL(vec ? retina_loss_kernel<true> : retina_loss_kernel<false>, dim3(blocks), dim3(256), 0, as_stream(stream),
                     cls, reg, N, H * W, A, C, ld_cls, ld_reg, cls_labels, (const float4*)bbox_targets, (long long)A_total,
                     (long long)level_offset, alpha, gamma, sigma * sigma, (const int*)num_fg, loss_scale, grad_cls, grad_reg,
                     partial);
  return check_launch("retina_loss_level");
}

// What an anchor-based level entry (_iou, _quality, _dfl) needs to launch: the grid, the form, and whether the route probe
// took the call (then nothing runs).
struct LevelLaunch {
  int blocks;
  bool vec, probed;
};

// The checks common to the three anchor-based level entries, in the order each has had them: shape, the entry's own
// parameter checks (param_error: the message of the first that fails, evaluated by the entry, or null), null pointers, the
// anchor table's alignment, the level's range. Fills *out and records the route if the probe is on.
static int retina_level_prepare(const char* entry, const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W,
                                int32_t A, int32_t C, int32_t ld_cls, int32_t ld_reg, const int32_t* cls_labels,
                                const float* anchors, const int32_t* matched_gt, const float* gt_boxes, int32_t G_max,
                                int64_t A_total, int64_t level_offset, const int32_t* num_fg, const uint16_t* grad_cls,
                                const uint16_t* grad_reg, const float* partial, const char* param_error,
                                int box_channels_per_anchor, int route_id, LevelLaunch* out) {
  MXDET_REQUIRE(N > 0 && H > 0 && W > 0 && A > 0 && C > 0 && ld_cls >= A * C && ld_reg >= box_channels_per_anchor * A &&
                    G_max > 0,
                MXDET_ESHAPE, "%s: bad shape", entry);
  MXDET_REQUIRE(!param_error, MXDET_EINVAL, "%s: %s", entry, param_error);
  MXDET_REQUIRE(cls && reg && cls_labels && anchors && matched_gt && gt_boxes && num_fg && grad_cls && grad_reg && partial,
                MXDET_EINVAL, "%s: null pointer", entry);
  MXDET_REQUIRE((uintptr_t)anchors % 16 == 0, MXDET_EINVAL, "%s: anchors must be 16-byte aligned", entry);
  MXDET_REQUIRE(level_offset >= 0 && level_offset + (int64_t)H * W * A <= A_total, MXDET_ESHAPE,
                "%s: level outside the anchor range", entry);
  out->blocks = mxdet_retina_loss_num_partials(N, H, W, A);
  out->vec = level_vec_ok(cls, reg, C, ld_cls, ld_reg, grad_cls, grad_reg);
  out->probed = route_probe_on();
  if (out->probed) {
    const int32_t rec[kRouteWords] = {route_id, out->vec ? 1 : 0, out->blocks};
    route_record(rec);
  }
  return MXDET_OK;
}

// the entries' own parameter checks: the message of the first one that fails, or null
static bool cls_kind_dfl_ok(int32_t k) { return k == MXDET_CLS_LOSS_FOCAL || cls_kind_ok(k); }
static const char* iou_kind_error(int32_t kind) {
  return iou_kind_ok(kind) ? nullptr : "kind must be MXDET_IOU_LOSS_IOU, _GIOU or _DIOU";
}
static const char* quality_cls_error(int32_t cls_kind, bool focal_too, float gamma) {
  if (!(focal_too ? cls_kind_dfl_ok(cls_kind) : cls_kind_ok(cls_kind)))
    return focal_too ? "cls_kind must be MXDET_CLS_LOSS_FOCAL, _QFL or _VFL" : "cls_kind must be MXDET_CLS_LOSS_QFL or _VFL";
  return gamma > 0.0f ? nullptr : "gamma must be positive";
}
static const char* delta_box_error(int32_t kind, float std_x, float std_y, float std_w, float std_h, float reg_weight) {
  if (const char* e = iou_kind_error(kind)) return e;
  return stds_ok(std_x, std_y, std_w, std_h) && reg_weight > 0.0f ? nullptr : "stds and reg_weight must be positive";
}

extern "C" int mxdet_retina_loss_level_iou(const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W,
                                           int32_t A, int32_t C, int32_t ld_cls, int32_t ld_reg,
                                           const int32_t* cls_labels, const float* anchors, const int32_t* matched_gt,
                                           const float* gt_boxes, int32_t G_max, int64_t A_total, int64_t level_offset,
                                           float alpha, float gamma, int32_t kind, float std_x, float std_y, float std_w,
                                           float std_h, float reg_weight, const int32_t* num_fg, float loss_scale,
                                           uint16_t* grad_cls, uint16_t* grad_reg, float* partial, mxdet_stream_t stream) {
  clear_error();
  LevelLaunch L;
  const int rc = retina_level_prepare("retina_loss_level_iou", cls, reg, N, H, W, A, C, ld_cls, ld_reg, cls_labels, anchors,
                                      matched_gt, gt_boxes, G_max, A_total, level_offset, num_fg, grad_cls, grad_reg, partial,
                                      delta_box_error(kind, std_x, std_y, std_w, std_h, reg_weight), 4,
                                      MXDET_ROUTE_RETINA_LOSS_IOU, &L);
  if (rc != MXDET_OK || L.probed) return rc;
  const BoxStds sd = {std_x, std_y, std_w, std_h};
  const auto k = L.vec ? retina_loss_iou_kernel<true, false> : retina_loss_iou_kernel<false, false>;
  hipLaunchKernelGGL(k, dim3(L.blocks), dim3(256), 0, as_stream(stream), cls, reg, N, H * W, A, C, ld_cls, ld_reg, cls_labels,
                     (const float4*)anchors, matched_gt, gt_boxes, G_max, (long long)A_total, (long long)level_offset,
                     /*cls_kind (unused)*/ 0, alpha, gamma, kind, sd, reg_weight,
                     (const int*)num_fg, loss_scale, grad_cls, grad_reg, partial);
  return check_launch("retina_loss_level_iou");
}

extern "C" int mxdet_retina_loss_level_quality(const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W,
                                               int32_t A, int32_t C, int32_t ld_cls, int32_t ld_reg,
                                               const int32_t* cls_labels, const float* anchors, const int32_t* matched_gt,
                                               const float* gt_boxes, int32_t G_max, int64_t A_total, int64_t level_offset,
                                               int32_t cls_kind, float alpha, float gamma, int32_t kind, float std_x,
                                               float std_y, float std_w, float std_h, float reg_weight, const int32_t* num_fg,
                                               float loss_scale, uint16_t* grad_cls, uint16_t* grad_reg, float* partial,
                                               mxdet_stream_t stream) {
  clear_error();
  const char* bad = quality_cls_error(cls_kind, false, gamma);
  if (!bad) bad = delta_box_error(kind, std_x, std_y, std_w, std_h, reg_weight);
  LevelLaunch L;
  const int rc = retina_level_prepare("retina_loss_level_quality", cls, reg, N, H, W, A, C, ld_cls, ld_reg, cls_labels, anchors,
                                      matched_gt, gt_boxes, G_max, A_total, level_offset, num_fg, grad_cls, grad_reg, partial, bad,
                                      4, MXDET_ROUTE_RETINA_LOSS_QUALITY, &L);
  if (rc != MXDET_OK || L.probed) return rc;
  const BoxStds sd = {std_x, std_y, std_w, std_h};
  const auto k = L.vec ? retina_loss_iou_kernel<true, true> : retina_loss_iou_kernel<false, true>;
  hipLaunchKernelGGL(k, dim3(L.blocks), dim3(256), 0, as_stream(stream), cls, reg, N, H * W, A, C, ld_cls, ld_reg, cls_labels, (const float4*)anchors, matched_gt,
                     gt_boxes, G_max, (long long)A_total, (long long)level_offset, cls_kind, alpha, gamma, kind, sd, reg_weight,
                     (const int*)num_fg, loss_scale, grad_cls, grad_reg, partial);
  return check_launch("retina_loss_level_quality");
}

extern "C" int mxdet_retina_loss_level_dfl(const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W, int32_t A,
                                           int32_t C, int32_t ld_cls, int32_t ld_reg, const int32_t* cls_labels,
                                           const float* anchors, const int32_t* matched_gt, const float* gt_boxes,
                                           int32_t G_max, int64_t A_total, int64_t level_offset, int32_t cls_kind, float alpha,
                                           float gamma, int32_t kind, int32_t reg_max, float stride, float reg_weight,
                                           float dfl_weight, const int32_t* num_fg, float loss_scale, uint16_t* grad_cls,
                                           uint16_t* grad_reg, float* partial, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(reg_max >= 1 && reg_max <= MXDET_REG_MAX_LIMIT, MXDET_EINVAL, "retina_loss_level_dfl: reg_max %d not in 1..%d",
                reg_max, MXDET_REG_MAX_LIMIT);
  const char* bad = quality_cls_error(cls_kind, true, gamma);
  if (!bad) bad = iou_kind_error(kind);
  if (!bad && !(stride > 0.0f && reg_weight > 0.0f && dfl_weight > 0.0f)) bad = "stride, reg_weight and dfl_weight must be positive";
  LevelLaunch L;
  const int rc = retina_level_prepare("retina_loss_level_dfl", cls, reg, N, H, W, A, C, ld_cls, ld_reg, cls_labels, anchors,
                                      matched_gt, gt_boxes, G_max, A_total, level_offset, num_fg, grad_cls, grad_reg, partial, bad,
                                      4 * (reg_max + 1), MXDET_ROUTE_RETINA_LOSS_DFL, &L);
  if (rc != MXDET_OK || L.probed) return rc;
  const bool focal = cls_kind == MXDET_CLS_LOSS_FOCAL;
  const auto k = L.vec ? (focal ? retina_loss_dfl_kernel<true, true> : retina_loss_dfl_kernel<true, false>)
                       : (focal ? retina_loss_dfl_kernel<false, true> : retina_loss_dfl_kernel<false, false>);
  hipLaunchKernelGGL(k, dim3(L.blocks), dim3(256), 0, as_stream(stream), cls, reg, N, H * W, A, C, ld_cls, ld_reg, cls_labels,
                     (const float4*)anchors, matched_gt, gt_boxes, G_max, (long long)A_total, (long long)level_offset, cls_kind,
                     alpha, gamma, kind, reg_max, stride, reg_weight, dfl_weight, (const int*)num_fg, loss_scale, grad_cls,
                     grad_reg, partial);
  return check_launch("retina_loss_level_dfl");
}

// ---- gradient harmonizing: the checks the three entries share ----
static const char* ghm_param_error(int32_t flags, int32_t bins_c, int32_t bins_r, float mu) {
  if (flags < 1 || flags > (MXDET_GHM_CLS | MXDET_GHM_REG)) return "flags must be MXDET_GHM_CLS, MXDET_GHM_REG or both";
  if (bins_c < 1 || bins_c > MXDET_GHM_MAX_BINS || bins_r < 1 || bins_r > MXDET_GHM_MAX_BINS) return "bins must lie in 1..64";
  return mu > 0.0f ? nullptr : "mu must be positive";
}

static int ghm_level_prepare(const char* entry, int32_t N, int32_t H, int32_t W, int32_t A, int32_t C, int32_t ld_cls,
                             int32_t ld_reg, int64_t A_total, int64_t level_offset, const char* param_error, bool nulls) {
  MXDET_REQUIRE(N > 0 && H > 0 && W > 0 && A > 0 && C > 0 && ld_cls >= A * C && ld_reg >= 4 * A, MXDET_ESHAPE, "%s: bad shape",
                entry);
  MXDET_REQUIRE(!param_error, MXDET_EINVAL, "%s: %s", entry, param_error);
  MXDET_REQUIRE(!nulls, MXDET_EINVAL, "%s: null pointer", entry);
  MXDET_REQUIRE(level_offset >= 0 && level_offset + (int64_t)H * W * A <= A_total, MXDET_ESHAPE,
                "%s: level outside the anchor range", entry);
  return MXDET_OK;
}

extern "C" int mxdet_ghm_hist_level(const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W, int32_t A,
                                    int32_t C, int32_t ld_cls, int32_t ld_reg, const int32_t* cls_labels,
                                    const float* bbox_targets, int64_t A_total, int64_t level_offset, int32_t flags,
                                    int32_t bins_c, int32_t bins_r, float mu, int32_t* counts, mxdet_stream_t stream) {
  clear_error();
  const int rc = ghm_level_prepare("ghm_hist_level", N, H, W, A, C, ld_cls, ld_reg, A_total, level_offset,
                                   ghm_param_error(flags, bins_c, bins_r, mu),
                                   !(cls && reg && cls_labels && bbox_targets && counts));
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE((uintptr_t)bbox_targets % 16 == 0, MXDET_EINVAL, "ghm_hist_level: bbox_targets must be 16-byte aligned");
  const int blocks = mxdet_retina_loss_num_partials(N, H, W, A);
  const bool vec = level_vec_ok(cls, reg, C, ld_cls, ld_reg, cls, reg);
  if (route_probe_on()) {
    const int32_t rec[kRouteWords] = {MXDET_ROUTE_GHM_HIST, vec ? 1 : 0, blocks, flags};
    route_record(rec);
    return MXDET_OK;
  }
  hipLaunchKernelGGL(vec ? ghm_hist_kernel<true> : ghm_hist_kernel<false>, dim3(blocks), dim3(256), 0, as_stream(stream), cls,
                     reg, N, H * W, A, C, ld_cls, ld_reg, cls_labels, (const float4*)bbox_targets, (long long)A_total,
                     (long long)level_offset, flags, bins_c, bins_r, mu, counts);
  return check_launch("ghm_hist_level");
}

extern "C" int mxdet_ghm_weights(const int32_t* counts, int32_t rows, int32_t bins_c, int32_t bins_r, float momentum_c,
                                 float momentum_r, float* acc, int32_t* cnt, float* coef, mxdet_stream_t stream) {
  clear_error();
  MXDET_REQUIRE(rows > 0, MXDET_ESHAPE, "ghm_weights: bad shape");
  const char* bad = ghm_param_error(MXDET_GHM_CLS, bins_c, bins_r, 1.0f);
  if (!bad && !(momentum_c >= 0.0f && momentum_c < 1.0f && momentum_r >= 0.0f && momentum_r < 1.0f))
    bad = "momentum must lie in [0, 1)";
  MXDET_REQUIRE(!bad, MXDET_EINVAL, "ghm_weights: %s", bad);
  MXDET_REQUIRE(counts && acc && cnt && coef, MXDET_EINVAL, "ghm_weights: null pointer");
  if (route_probe_on()) return MXDET_OK;                  // one route, nothing to record: like the level entries, no launch
  hipLaunchKernelGGL(ghm_weights_kernel, dim3(1), dim3(1024), 0, as_stream(stream), counts, rows, bins_c, bins_r, momentum_c,
                     momentum_r, acc, cnt, coef);
  return check_launch("ghm_weights");
}

template <bool VEC>
static auto ghm_loss_kernel_of(int32_t flags) {
  if (flags == MXDET_GHM_CLS) return retina_loss_ghm_kernel<VEC, true, false>;
  if (flags == MXDET_GHM_REG) return retina_loss_ghm_kernel<VEC, false, true>;
  return retina_loss_ghm_kernel<VEC, true, true>;
}

extern "C" int mxdet_retina_loss_level_ghm(const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W, int32_t A,
                                           int32_t C, int32_t ld_cls, int32_t ld_reg, const int32_t* cls_labels,
                                           const float* bbox_targets, int64_t A_total, int64_t level_offset, int32_t flags,
                                           float alpha, float gamma, float sigma, const float* coef, int32_t bins_c,
                                           int32_t bins_r, float cls_weight, float mu, float reg_weight, const int32_t* num_fg,
                                           float loss_scale, uint16_t* grad_cls, uint16_t* grad_reg, float* partial,
                                           mxdet_stream_t stream) {
  clear_error();
  const char* bad = ghm_param_error(flags, bins_c, bins_r, mu);
  if (!bad && !(cls_weight > 0.0f && reg_weight > 0.0f)) bad = "cls_weight and reg_weight must be positive";
  const int rc = ghm_level_prepare("retina_loss_level_ghm", N, H, W, A, C, ld_cls, ld_reg, A_total, level_offset, bad,
                                   !(cls && reg && cls_labels && bbox_targets && coef && num_fg && grad_cls && grad_reg && partial));
  if (rc != MXDET_OK) return rc;
  MXDET_REQUIRE((uintptr_t)bbox_targets % 16 == 0, MXDET_EINVAL, "retina_loss_level_ghm: bbox_targets must be 16-byte aligned");
  const int blocks = mxdet_retina_loss_num_partials(N, H, W, A);
  const bool vec = level_vec_ok(cls, reg, C, ld_cls, ld_reg, grad_cls, grad_reg);
  if (route_probe_on()) {
    const int32_t rec[kRouteWords] = {MXDET_ROUTE_RETINA_LOSS_GHM, vec ? 1 : 0, blocks, flags};
    route_record(rec);
    return MXDET_OK;
  }
  hipLaunchKernelGGL(vec ? ghm_loss_kernel_of<true>(flags) : ghm_loss_kernel_of<false>(flags), dim3(blocks), dim3(256), 0,
                     as_stream(stream), cls, reg, N, H * W, A, C, ld_cls, ld_reg, cls_labels, (const float4*)bbox_targets,
                     (long long)A_total, (long long)level_offset, alpha, gamma, sigma * sigma, coef, bins_c, bins_r, cls_weight,
                     mu, reg_weight, (const int*)num_fg, loss_scale, grad_cls, grad_reg, partial);
  return check_launch("retina_loss_level_ghm");
}
