// loss_elem.h -- the device pieces that more than one loss kernel uses (losses.hip, retina_loss.hip, ohem.hip): the
// fixed-order block sum and its partial-sum epilogue, the sigmoid / softplus helpers, the focal and quality class elements
// with their functors, the IoU-family box element, the box head's per-roi walks, and the entries' small host predicates.
// Float32, no FMA contraction (the three files are built with -ffp-contract=off): one definition each, so "same code, same
// bits" holds by construction.
#pragma once
#include "common.h"
#include "dist_box.h"

namespace mxdet {

// deterministic block sum: fixed shuffle tree inside each wave, then wave partials added in order
__device__ inline float block_sum_fixed(float v, float* smem /* >= blockDim/64 floats */) {
  v = wave_sum_lane0(v);
  int wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane_id() == 0) smem[wid] = v;
  __syncthreads();
  float s = 0.0f;
  if (threadIdx.x == 0)
    for (int i = 0; i < nw; ++i) s += smem[i];
  return s;  // valid on thread 0
}

// The workgroup's K loss sums: block_sum_fixed of v[0], v[1], ... in that order, then
// partial[K * blockIdx.x + j] = sum * scale[j] (a kernel whose terms are normalised differently has one scale per sum).
template <int K>
__device__ __forceinline__ void store_block_partials(const float (&v)[K], const float (&scale)[K], float* red,
                                                     float* __restrict__ partial) {
  float s[K];
#pragma unroll
  for (int j = 0; j < K; ++j) s[j] = block_sum_fixed(v[j], red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) partial[K * blockIdx.x + j] = s[j] * scale[j];
  }
}
// the same with one scale for every sum
template <int K>
__device__ __forceinline__ void store_block_partials(const float (&v)[K], float scale, float* red, float* __restrict__ partial) {
  float sc[K];
#pragma unroll
  for (int j = 0; j < K; ++j) sc[j] = scale;
  store_block_partials<K>(v, sc, red, partial);
}

__device__ __forceinline__ float softplus_neg_abs(float z) {
  // log(1 + exp(-|z|))
  float az = z < 0.0f ? -z : z;
  return mxdet_logf(1.0f + mxdet_expf(-az));
}
// p = sigmoid(z), q = 1 - p and sp = log(1 + exp(-|z|)) from ONE exp(-|z|), each with its full relative accuracy at large |z|:
// q is the other quotient of the same division, not 1.0f - p (which cancels once p is near 1), and sp keeps the part of t that
// 1 + t rounds away (log1p: log(d) * t / (d - 1); d - 1 is exact, and sp = t once d rounds to 1). The focal terms
// (1-p)^gamma * log p and p^gamma * log(1-p) of a well-classified element are products of exactly these small numbers.
__device__ __forceinline__ void sigmoid_softplus(float z, float& p, float& q, float& sp) {
  const float az = z < 0.0f ? -z : z;
  const float t = mxdet_expf(-az);
  const float d = 1.0f + t;
  const float dm1 = d - 1.0f;
  sp = dm1 == 0.0f ? t : mxdet_logf(d) * (t / dm1);
  const float big = 1.0f / d, small = t / d;
  p = z >= 0.0f ? big : small;
  q = z >= 0.0f ? small : big;
}
__device__ __forceinline__ float sigmoidf_det(float z) {
  // 1/(1+exp(-z)) evaluated on the stable side
  if (z >= 0.0f) return 1.0f / (1.0f + mxdet_expf(-z));
  float e = mxdet_expf(z);
  return e / (1.0f + e);
}

// p, q = 1 - p and the two logs of one logit: log(p) = -(max(-x,0) + sp); log(1-p) = -(max(x,0) + sp)
__device__ __forceinline__ void sigmoid_logs(const float x, float& p, float& q, float& logp, float& log1mp) {
  float sp;
  sigmoid_softplus(x, p, q, sp);
  logp = -((x < 0.0f ? -x : 0.0f) + sp);
  log1mp = -((x > 0.0f ? x : 0.0f) + sp);
}

// ---------------------------------------------------------------------------------------------
// Sigmoid focal loss of one element: logit x of the anchor's own class column (positive) or of any other. Returns L,
// g = dL / dx.
__device__ __forceinline__ float focal_cls_elem(const float x, const bool positive, const float alpha, const float gamma,
                                                float& g) {
  float p, q, logp, log1mp;
  sigmoid_logs(x, p, q, logp, log1mp);
  if (positive) {
    const float mod = (gamma == 2.0f) ? q * q : mxdet_expf(gamma * mxdet_logf(q > 1e-30f ? q : 1e-30f));
    g = -alpha * mod * (q - gamma * p * logp);
    return -alpha * mod * logp;
  }
  const float mod = (gamma == 2.0f) ? p * p : mxdet_expf(gamma * mxdet_logf(p > 1e-30f ? p : 1e-30f));
  g = (1.0f - alpha) * mod * (p - gamma * q * log1mp);
  return -(1.0f - alpha) * mod * log1mp;
}

// Quality-aware class losses: the matched class column is trained against y = the IoU of the predicted box
// with its ground truth (a constant of the class loss), every other element against y = 0.
//   QFL (Li et al. 2020):   L = |y - s|^beta * BCE(s, y), beta in `gamma`; alpha unused
//   VFL (Zhang et al. 2021): y > 0: L = y * BCE(s, y);  y == 0: L = -alpha * s^gamma * log(1 - s)
// One element: logit x, target y in [0, 1]. Returns L, g = dL / dx. The logs are those of the focal element.
__device__ __forceinline__ float quality_cls_elem(const float x, const float y, const int cls_kind, const float alpha,
                                                  const float gamma, float& g) {
  float p, q, logp, log1mp;
  sigmoid_logs(x, p, q, logp, log1mp);
  if (cls_kind == MXDET_CLS_LOSS_QFL) {
    const float e = p - y;
    const float bce = -y * logp - (1.0f - y) * log1mp;
    float mod, dmod;                                       // |e|^beta and beta * |e|^(beta - 1) * sign(e)
    if (gamma == 2.0f) {
      mod = e * e;
      dmod = 2.0f * e;
    } else {
      const float ae = e < 0.0f ? -e : e, aec = ae > 1e-30f ? ae : 1e-30f;
      mod = mxdet_expf(gamma * mxdet_logf(aec));
      dmod = gamma * (mod / aec);
      if (e < 0.0f) dmod = -dmod;
    }
    g = dmod * (p * q) * bce + mod * e;
    return mod * bce;
  }
  // both sides and two selects: a branch on y would split nearly every wave that holds a foreground anchor
  const float bce = -y * logp - (1.0f - y) * log1mp;
  const float mod = (gamma == 2.0f) ? p * p : mxdet_expf(gamma * mxdet_logf(p > 1e-30f ? p : 1e-30f));
  const float gneg = alpha * (gamma * mod * q * (-log1mp) + mod * p);
  const float lneg = -alpha * mod * log1mp;
  g = y > 0.0f ? y * (p - y) : gneg;
  return y > 0.0f ? y * bce : lneg;
}

// The class elements as the kernels take them: elem(x, positive, quality, g) for the logit x of the row's own class
// column (positive) or of another; quality is that of the row's box, read only where kQuality says the element has one.
// Returns L, g = dL / dx.
struct FocalElem {
  static constexpr bool kQuality = false;
  float alpha, gamma;
  __device__ __forceinline__ float operator()(float x, bool positive, float, float& g) const {
    return focal_cls_elem(x, positive, alpha, gamma, g);
  }
};
struct QualityElem {
  static constexpr bool kQuality = true;
  int cls_kind;
  float alpha, gamma;
  __device__ __forceinline__ float operator()(float x, bool positive, float quality, float& g) const {
    return quality_cls_elem(x, positive ? quality : 0.0f, cls_kind, alpha, gamma, g);
  }
};

// ---------------------------------------------------------------------------------------------
// Gradient harmonizing (GHM, Li et al. 2019; definition in include/mxdet.h). The histogram pass and the
// loss pass of a step call the SAME three functions below on the same inputs, so an element lands in the same bin in both.
//
// bin of a gradient norm g in [0, 1]: unit-region edges k / B, g == 1 in the last bin
__device__ __forceinline__ int ghm_bin(const float g, const int B) {
  const int b = (int)(g * (float)B);
  return b < 0 ? 0 : (b < B - 1 ? b : B - 1);             // b < 0 does not occur for g >= 0: the index stays in the table
}
// class element: g = |sigmoid(x) - t| = 1 - p for the row's own class column, p for any other; p, q = 1 - p, the logs of
// sigmoid_logs come back for the loss (the histogram pass drops them)
__device__ __forceinline__ float ghm_cls_norm(const float x, const bool positive, float& p, float& q, float& logp,
                                              float& log1mp) {
  sigmoid_logs(x, p, q, logp, log1mp);
  return positive ? q : p;
}
// box element: d = delta - target, r = sqrt(d*d + mu*mu); g = |d| / r
__device__ __forceinline__ float ghm_reg_norm(const float d, const float mu, float& r) {
  r = sqrtf(d * d + mu * mu);
  return (d < 0.0f ? -d : d) / r;
}
// The harmonized class element as the class walks take it: coef = the step's B weights (LDS). L = coef[bin] * BCE,
// g = coef[bin] * (s - t), with s - 1 taken as -(1 - s).
struct GhmClsElem {
  static constexpr bool kQuality = false;
  const float* coef;
  int B;
  __device__ __forceinline__ float operator()(float x, bool positive, float, float& g) const {
    float p, q, logp, log1mp;
    const float c = coef[ghm_bin(ghm_cls_norm(x, positive, p, q, logp, log1mp), B)];
    g = c * (positive ? -q : p);
    return c * (positive ? -logp : -log1mp);
  }
};

// ---------------------------------------------------------------------------------------------
// IoU / GIoU / DIoU loss on the decoded box. Everything is evaluated relative to the box's own corner
// (x1, y1): in absolute image coordinates the corners cancel at ulp(1300) = 1.2e-4 px against boxes a few pixels wide.
struct BoxStds { float x, y, w, h; };

// d max(a, b) / da: 1, 0 or -- at an exact tie -- the mean of the two one-sided derivatives
__device__ __forceinline__ float tie_step(float a, float b) { return a > b ? 1.0f : (a == b ? 0.5f : 0.0f); }

// 16 bytes at a 4-byte aligned address (rows of gt_boxes [.,5] are 20 bytes apart)
__device__ __forceinline__ float4 load_f4_a4(const float* p) {
  typedef float f4a4_t __attribute__((ext_vector_type(4), aligned(4)));
  const f4a4_t v = *(const f4a4_t*)p;
  return make_float4(v.x, v.y, v.z, v.w);
}

// The IoU core, shared by the delta decode below and the integral decode of the distribution head. Per
// axis k, in any common origin: predicted corners p1 / p2, centre pc and "+1" length pl; ground-truth corners g1 / g2.
// Returns L. Outputs per axis: d1 / d2 = dL / d p1, p2 through the min / max corners only, gp = dL / d pc through the DIoU
// centre term only, da = dL / d pl through the area only. iou (optional): inter / union -- the quality of the quality-aware
// class losses; 1 - L is not it, GIoU and DIoU add terms.
__device__ __forceinline__ float box_iou_core(const float* p1, const float* p2, const float* pc, const float* pl,
                                              const float* g1, const float* g2, const int kind, float* d1, float* d2,
                                              float* gp, float* da, float* iou) {
  float gl[2], il[2], cl[2], a1[2], a2[2], st[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    gl[k] = g2[k] - g1[k] + 1.0f;
    a1[k] = tie_step(p1[k], g1[k]);                   // share of p1 in max(p1, g1)
    a2[k] = tie_step(g2[k], p2[k]);                   // share of p2 in min(p2, g2)
    const float lo = p1[k] > g1[k] ? p1[k] : g1[k], hi = p2[k] < g2[k] ? p2[k] : g2[k];
    const float r = hi - lo + 1.0f;
    st[k] = tie_step(r, 0.0f);
    il[k] = r > 0.0f ? r : 0.0f;
    cl[k] = (p2[k] > g2[k] ? p2[k] : g2[k]) - (p1[k] < g1[k] ? p1[k] : g1[k]) + 1.0f;
  }
  const float inter = il[0] * il[1];
  const float uni = pl[0] * pl[1] + gl[0] * gl[1] - inter;
  float L = 1.0f - inter / uni;
  if (iou) *iou = inter / uni;
  const float iu2 = 1.0f / (uni * uni);
  float dI = -(uni + inter) * iu2, dA = inter * iu2;   // dL / d inter, dL / d (pl0 * pl1)
  float gc[2] = {0.0f, 0.0f};                          // dL / d cl[k]
  gp[0] = 0.0f;
  gp[1] = 0.0f;
  if (kind == MXDET_IOU_LOSS_GIOU) {
    const float C = cl[0] * cl[1], ic = 1.0f / C;
    L += (C - uni) * ic;
    dI += ic;
    dA -= ic;
    const float dC = uni * ic * ic;
    gc[0] = dC * cl[1];
    gc[1] = dC * cl[0];
  } else if (kind == MXDET_IOU_LOSS_DIOU) {
    const float e0 = pc[0] - 0.5f * (g1[0] + g2[0]), e1 = pc[1] - 0.5f * (g1[1] + g2[1]);
    const float rho = e0 * e0 + e1 * e1, iD = 1.0f / (cl[0] * cl[0] + cl[1] * cl[1]);
    L += rho * iD;
    const float q = -2.0f * rho * iD * iD;
    gc[0] = q * cl[0];
    gc[1] = q * cl[1];
    gp[0] = 2.0f * e0 * iD;
    gp[1] = 2.0f * e1 * iD;
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float gi = dI * il[1 - k] * st[k];
    d2[k] = gi * a2[k] + gc[k] * (1.0f - a2[k]);
    d1[k] = -(gi * a1[k] + gc[k] * (1.0f - a1[k]));
    da[k] = dA * pl[1 - k];
  }
  return L;
}

// b: roi / anchor, g: ground truth (absolute corners), d: raw deltas. Returns L, gd[4] = dL / d(raw delta).
// iou (optional): see box_iou_core. Callers that pass none compile to what they were.
__device__ __forceinline__ float box_iou_loss_elem(const float4 b, const float4 g, const float* d, const BoxStds sd,
                                                   const int kind, float* gd, float* iou = nullptr) {
  const float b1[2] = {b.x, b.y}, b2[2] = {b.z, b.w}, ga[2] = {g.x, g.y}, gb[2] = {g.z, g.w};
  const float sc[2] = {sd.x, sd.y}, ss[2] = {sd.w, sd.h};
  float len[2], pc[2], pl[2], p1[2], p2[2], g1[2], g2[2], ck[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    g1[k] = ga[k] - b1[k];
    g2[k] = gb[k] - b1[k];
    len[k] = b2[k] - b1[k] + 1.0f;
    const float c0 = 0.5f * (len[k] - 1.0f);
    float t = d[2 + k] * ss[k];
    ck[k] = tie_step(MXDET_BBOX_XFORM_CLIP, t);
    if (t > MXDET_BBOX_XFORM_CLIP) t = MXDET_BBOX_XFORM_CLIP;
    float c = d[k] * sc[k];
    c = c * len[k];
    pc[k] = c + c0;
    pl[k] = mxdet_expf(t) * len[k];
    const float hl = 0.5f * (pl[k] - 1.0f);
    p1[k] = pc[k] - hl;
    p2[k] = pc[k] + hl;
  }
  float d1[2], d2[2], gp[2], da[2];
  const float L = box_iou_core(p1, p2, pc, pl, g1, g2, kind, d1, d2, gp, da, iou);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float dpl = da[k] + 0.5f * (d2[k] - d1[k]);
    gd[k] = (d1[k] + d2[k] + gp[k]) * (sc[k] * len[k]);
    gd[2 + k] = dpl * (pl[k] * ss[k]) * ck[k];
  }
  return L;
}

__device__ __forceinline__ void load_deltas4(const void* p, long long i, int dtype, float* d) {
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] = load_as_f32(p, i + k, dtype);
}

// ---------------------------------------------------------------------------------------------
// Distribution box regression (definition in include/mxdet.h): four lanes per box, lane `side` (l, t, r, b)
// on the R + 1 logits at x[off ..]. All four lanes of a quad call this together: the expectations cross by lane reads
// inside the quad, then every lane evaluates the (cheap) IoU core on the whole box and keeps its own side's dL / dE.
// Writes the side's R + 1 gradients: (reg_weight * dL/dE * p_k (k - E) + dfl_weight / 4 * (p_k - target_k)) * gscale.
// Returns L (unweighted, equal on the four lanes); dfl = this side's DFL, q = inter / union.
__device__ __forceinline__ float dist_box_quad(const void* x, long long off, int dtype, int R, int side, const float4 b,
                                               const float4 g, float s, int kind, float reg_weight, float dfl_weight,
                                               float gscale, void* gx, float& dfl, float& q) {
  float xv[kDistBins], m, Z;                              // the logits, then e_k = exp(x_k - m)
  dist_load(x, off, 1, dtype, R, xv);
  const float E = dist_expect(xv, R, m, Z);
  const int q0 = lane_id() & ~3;
  const float El = __shfl(E, q0 + 0), Et = __shfl(E, q0 + 1), Er = __shfl(E, q0 + 2), Eb = __shfl(E, q0 + 3);
  const float cx = 0.5f * (b.x + b.z), cy = 0.5f * (b.y + b.w);
  const float g1[2] = {g.x - cx, g.y - cy}, g2[2] = {g.z - cx, g.w - cy};
  const float p1[2] = {-(s * El), -(s * Et)}, p2[2] = {s * Er, s * Eb};
  float pl[2], pc[2], d1[2], d2[2], gp[2], da[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    pl[k] = p2[k] - p1[k] + 1.0f;
    pc[k] = 0.5f * (p1[k] + p2[k]);
  }
  const float L = box_iou_core(p1, p2, pc, pl, g1, g2, kind, d1, d2, gp, da, &q);
  const int ax = side & 1;
  // pc = (p1 + p2) / 2 and pl = p2 - p1 + 1: dL / d p1 = d1 + gp / 2 - da, dL / d p2 = d2 + gp / 2 + da
  const float dp = side < 2 ? d1[ax] + 0.5f * gp[ax] - da[ax] : d2[ax] + 0.5f * gp[ax] + da[ax];
  const float dE = side < 2 ? -(s * dp) : s * dp;
  const float dist = side < 2 ? -g1[ax] : g2[ax];
  const float ymax = (float)R - 0.1f;
  float y = dist / s;
  y = y < 0.0f ? 0.0f : y;
  y = y > ymax ? ymax : y;
  const int yl = (int)y;                                  // y >= 0: truncation is floor
  const float wl = (float)yl + 1.0f - y, wr = y - (float)yl;
  const float lse = m + mxdet_logf(Z);
  dfl = wl * (lse - load_as_f32(x, off + yl, dtype)) + wr * (lse - load_as_f32(x, off + yl + 1, dtype));
  const float gb = reg_weight * dE, gd = dfl_weight * 0.25f;
#pragma unroll
  for (int k = 0; k < kDistBins; ++k)
    if (k <= R) {
      const float p = xv[k] / Z;
      const float t = (k == yl ? wl : 0.0f) + (k == yl + 1 ? wr : 0.0f);
      store_from_f32(gx, off + k, dtype, (gb * (p * ((float)k - E)) + gd * (p - t)) * gscale);
    }
  return L;
}

// ---------------------------------------------------------------------------------------------
// The box head's per-roi walks, one wave per roi (rcnn_loss_kernel, rcnn_loss_iou_kernel in losses.hip; ohem_score_kernel
// in ohem.hip). kGrad = false evaluates the same loss and writes nothing: the gradient is no operand of the loss, so the
// two instantiations return the same bits.
//
// softmax CE of roi r (ignore label -1); kGrad: writes columns [0, num_classes) of the grad_cls row. Every lane returns
// the row's loss (fixed xor tree).
template <bool kGrad>
__device__ __forceinline__ float rcnn_softmax_ce(const void* __restrict__ cls, int dtype, int ld_cls, long long r, int lab,
                                                 int lane, int num_classes, float norm, float loss_scale,
                                                 void* __restrict__ gcls) {
  float mx = -3.0e38f;
  for (int c = lane; c < num_classes; c += 64) {
    float z = load_as_f32(cls, r * ld_cls + c, dtype);
    mx = z > mx ? z : mx;
  }
  mx = wave_reduce<MaxSel>(mx);
  float se = 0.0f;
  for (int c = lane; c < num_classes; c += 64)
    se += mxdet_expf(load_as_f32(cls, r * ld_cls + c, dtype) - mx);
  se = wave_sum(se);
  float lse = mxdet_logf(se);
  float lcls = 0.0f;
  for (int c = lane; c < num_classes; c += 64) {
    float z = load_as_f32(cls, r * ld_cls + c, dtype);
    float g = 0.0f;
    if (lab >= 0) {
      if (kGrad) {
        float p = mxdet_expf(z - mx) / se;
        g = (p - (c == lab ? 1.0f : 0.0f)) * norm * loss_scale;
      }
      if (c == lab) lcls = -(z - mx - lse);
    }
    if (kGrad) store_from_f32(gcls, r * ld_cls + c, dtype, g);
  }
  return wave_sum(lcls);
}

// Balanced L1 (Pang et al., CVPR 2019) of one weighted difference d, a = |d|:
//   a < beta:  L = (alpha / b) * (b * a + 1) * log(b * a / beta + 1) - alpha * a,   dL/dd = sign(d) * alpha * log(b * a / beta + 1)
//   else:      L = gamma * a + gamma / b - alpha * beta,                            dL/dd = sign(d) * gamma
// b = exp(gamma / alpha) - 1 comes from the host (the two branches then meet at a = beta). One fp32 operation per
// statement, in this order; the log is mxdet_logf.
__device__ __forceinline__ float balanced_l1_log(float a, float beta, float b) {
  float t = b * a;
  t = t / beta;
  t = t + 1.0f;
  return mxdet_logf(t);
}
__device__ __forceinline__ float balanced_l1(float d, float alpha, float gamma, float beta, float b) {
  const float a = d < 0.0f ? -d : d;
  if (a < beta) {
    const float lg = balanced_l1_log(a, beta, b);
    float p = b * a;
    p = p + 1.0f;
    float q = alpha / b;
    q = q * p;
    q = q * lg;
    const float s = alpha * a;
    return q - s;
  }
  float L = gamma * a;
  const float c0 = gamma / b;
  L = L + c0;
  const float c1 = alpha * beta;
  return L - c1;
}
__device__ __forceinline__ float balanced_l1_grad(float d, float alpha, float gamma, float beta, float b) {
  const float a = d < 0.0f ? -d : d;
  const float m = a < beta ? alpha * balanced_l1_log(a, beta, b) : gamma;
  return d > 0.0f ? m : (d < 0.0f ? -m : 0.0f);
}

// The regression elements as rcnn_reg_elem takes them: loss(d) and grad(d) = dL/dd of one weighted difference.
struct SmoothL1Elem {
  float sigma2;
  __device__ __forceinline__ float loss(float d) const { return mxdet_smooth_l1(d, sigma2); }
  __device__ __forceinline__ float grad(float d) const { return mxdet_smooth_l1_grad(d, sigma2); }
};
struct BalancedL1Elem {      // reg_weight scales the gradient here and the row's loss in the kernel
  float alpha, gamma, beta, b, reg_weight;
  __device__ __forceinline__ float loss(float d) const { return balanced_l1(d, alpha, gamma, beta, b); }
  __device__ __forceinline__ float grad(float d) const { return balanced_l1_grad(d, alpha, gamma, beta, b) * reg_weight; }
};

// An element-wise regression loss of roi r's reg_dim columns against its targets / weights; kGrad: writes columns
// [0, reg_dim) of the grad_reg row. Every lane returns the row's loss.
template <bool kGrad, class Elem>
__device__ __forceinline__ float rcnn_reg_elem(const void* __restrict__ reg, int dtype, int ld_reg, long long r, int lab,
                                               int lane, const float* __restrict__ tgt, const float* __restrict__ wgt,
                                               int reg_dim, const Elem elem, float norm, float loss_scale,
                                               void* __restrict__ greg) {
  float lreg = 0.0f;
  for (int c = lane; c < reg_dim; c += 64) {
    float w = wgt[r * reg_dim + c];
    float g = 0.0f;
    if (w != 0.0f && lab > 0) {
      float d = (load_as_f32(reg, r * ld_reg + c, dtype) - tgt[r * reg_dim + c]) * w;
      lreg += elem.loss(d);
      if (kGrad) g = elem.grad(d) * w * norm * loss_scale;
    }
    if (kGrad) store_from_f32(greg, r * ld_reg + c, dtype, g);
  }
  return wave_sum(lreg);   // every lane ends with the same value
}
// smooth-L1 (the name ohem.hip scores rows with)
template <bool kGrad>
__device__ __forceinline__ float rcnn_reg_smooth_l1(const void* __restrict__ reg, int dtype, int ld_reg, long long r, int lab,
                                                    int lane, const float* __restrict__ tgt, const float* __restrict__ wgt,
                                                    int reg_dim, float sigma2, float norm, float loss_scale,
                                                    void* __restrict__ greg) {
  return rcnn_reg_elem<kGrad>(reg, dtype, ld_reg, r, lab, lane, tgt, wgt, reg_dim, SmoothL1Elem{sigma2}, norm, loss_scale, greg);
}

// The IoU-family term of roi r: every lane evaluates the roi's one box (wave-uniform); kGrad: the lanes share the row's
// reg_dim gradient columns. Returns reg_weight * L (0 for a roi that regresses nothing).
template <bool kGrad>
__device__ __forceinline__ float rcnn_reg_iou(const void* __restrict__ reg, int dtype, int ld_reg, long long r, int lab, int lane,
                                              const float* __restrict__ rois, const int32_t* __restrict__ matched,
                                              const float* __restrict__ gt, int N, int G_max, int num_classes, int reg_dim,
                                              int kind, BoxStds sd, float reg_weight, float norm, float loss_scale,
                                              void* __restrict__ greg) {
  float lreg = 0.0f, gd[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int first = -4;                                       // first column of the label's four deltas; none for label <= 0
  if (lab > 0 && lab < num_classes) {
    const float* ro = rois + r * 5;
    const int img = (int)ro[0], m = matched[r];
    if (img >= 0 && img < N && m >= 0 && m < G_max) {   // an index outside gt_boxes: the roi regresses nothing
      first = 4 * lab;
      float d[4];
      load_deltas4(reg, r * ld_reg + first, dtype, d);
      const float4 g = load_f4_a4(gt + ((long long)img * G_max + m) * 5);
      lreg = reg_weight * box_iou_loss_elem(make_float4(ro[1], ro[2], ro[3], ro[4]), g, d, sd, kind, gd);
    }
  }
  if (kGrad) {
    const float gs = reg_weight * norm * loss_scale;
    for (int c = lane; c < reg_dim; c += 64) {
      const int k = c - first;
      float gv = 0.0f;
      if (k >= 0 && k < 4) gv = (k == 0 ? gd[0] : k == 1 ? gd[1] : k == 2 ? gd[2] : gd[3]) * gs;
      store_from_f32(greg, r * ld_reg + c, dtype, gv);
    }
  }
  return lreg;
}

// ---------------------------------------------------------------------------------------------
// the entries' argument predicates (host)
static inline bool cls_kind_ok(int32_t k) { return k == MXDET_CLS_LOSS_QFL || k == MXDET_CLS_LOSS_VFL; }
static inline bool iou_kind_ok(int32_t kind) {
  return kind == MXDET_IOU_LOSS_IOU || kind == MXDET_IOU_LOSS_GIOU || kind == MXDET_IOU_LOSS_DIOU;
}
static inline bool stds_ok(float a, float b, float c, float d) { return a > 0.0f && b > 0.0f && c > 0.0f && d > 0.0f; }

}  // namespace mxdet
