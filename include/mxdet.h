/*
 * mxdet.h -- C-ABI of libmxdet_hip.so: the MI355X (gfx950) two-stage-detector hot path.
 *
 * Drop-in boundary. The reference (jiangzhengkai/mxdetection) declares the
 * plugin slots only by name -- /root/reference/README.md:24 (`mxdetection/ops`), README.md:15-19
 * (`core/{anchor,bbox,mask,loss}`), README.md:27-32 (`models/{backbones,rpn_heads,bbox_heads,
 * mask_heads,necks,roi_extractors}`) -- and delegates all arithmetic to MXNet 1.3.0 operators
 * (README.md:37). Each entry below names the slot it sits behind and the MXNet-1.3.0 operator whose
 * role it takes; INTEGRATION.md shows the `mx.operator.CustomOp` / ctypes stub a maintainer would add.
 *
 * Conventions (every entry):
 *   - raw device pointers + explicit sizes; no torch / MXNet types; the caller owns every buffer,
 *     workspace included; the library never allocates device memory, frees, or keeps a pointer.
 *   - asynchronous on `stream` (a hipStream_t passed as void*); re-entrant; no global mutable state
 *     except the thread-local error string.
 *   - returns 0 on success or a negative MXDET_E* code; never throws, aborts or prints.
 *   - boxes are fp32 (x1,y1,x2,y2) in the legacy "+1" pixel convention; rois are (batch,x1,y1,x2,y2).
 *   - activations are bf16 channels-last [N,H,W,C]; `bf16` buffers are passed as uint16_t*.
 *   - `accumulate` on backward entries mirrors MXNet's req: 0 = kWriteTo, 1 = kAddTo.
 */
#ifndef MXDET_H_
#define MXDET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MXDET_OK 0
#define MXDET_EINVAL (-1)
#define MXDET_ESHAPE (-2)
#define MXDET_EWORKSPACE (-3)
#define MXDET_EHIP (-4)
#define MXDET_ERCCL (-5)

#define MXDET_DTYPE_F32 0
#define MXDET_DTYPE_BF16 1

typedef void* mxdet_stream_t; /* hipStream_t */

/* thread-local description of the last failure on this thread ("" if none) */
const char* mxdet_last_error(void);
/* library version / build arch string, e.g. "mxdet-hip 0.1 gfx950" */
const char* mxdet_version(void);

/* ------------------------------------------------------------------------------------------------
 * core/bbox  (README.md:17)  -- bbox_overlaps; MXNet role: Cython bbox_overlaps / contrib.box_iou
 * out[na,nb] = IoU(a_i, b_j), legacy +1 convention. */
int mxdet_box_iou(const float* boxes_a, int64_t na, const float* boxes_b, int64_t nb, float* out,
                  mxdet_stream_t stream);

/* core/anchor (README.md:16) -- dense anchor grid of one pyramid level.
 * out[(y*W+x)*A+a] = base[a] + (x*stride, y*stride, x*stride, y*stride). */
int mxdet_generate_anchors(const float* base_anchors, int32_t A, int32_t H, int32_t W, int32_t stride,
                           float* out, mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * ops (README.md:24) -- batched NMS over B independent score-sorted lists.
 * boxes[B,n_max,4] sorted by descending score; counts[B] valid entries per list; invalid[B,n_max]
 * (may be NULL) marks boxes to drop before NMS. A box suppresses a later one when IoU > thresh.
 * keep_idx[B,n_max] receives the kept positions in ascending order, num_keep[B] their number
 * (at most max_keep each). MXNet role: contrib.box_nms / Cython cpu_nms / gpu_nms. */
size_t mxdet_nms_batched_workspace_bytes(int32_t B, int32_t n_max);
int mxdet_nms_batched(const float* boxes, const int32_t* counts, const uint8_t* invalid, int32_t B,
                      int32_t n_max, float thresh, int32_t max_keep, int32_t* keep_idx,
                      int32_t* num_keep, void* workspace, size_t workspace_bytes,
                      mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * core/evaluation (README.md:20) + ops (README.md:24) -- test-time detection post-processing
 * (MXNet-lineage role: the host-side im_detect -> per-class threshold -> nms ->
 * max_per_image loop of py-faster-rcnn / mx-rcnn).
 * cls_logits [N*R, ld_cls] (columns 0..C-1, class 0 = background) and bbox_pred [N*R, ld_reg] (class-specific
 * deltas, 4 per class, normalised: delta = pred * stds + means) in `dtype`; rois [N*R,5] = (image, x1,y1,x2,y2), the
 * first num_rois[n] rows of image n valid; im_info [N,3] = (h, w, scale).
 * score = softmax(logits) (m = max, e_c = exp(x_c - m), s = sum in class order, e_c / s); box = decode + clip.
 * Per image and foreground class: keep score > score_thresh, sort by (score desc, roi asc), greedy NMS at
 * nms_thresh; then the max_per_image best over all classes by (score desc, roi asc, class asc).
 * dets [N, max_per_image, 6] = (x1, y1, x2, y2, score, class), padding rows zero with class -1; num_dets [N]. */
size_t mxdet_detection_postprocess_workspace_bytes(int32_t N, int32_t rois_per_image, int32_t num_classes);
int mxdet_detection_postprocess(const void* cls_logits, const void* bbox_pred, int32_t dtype, int32_t ld_cls,
                                int32_t ld_reg, const float* rois, const int32_t* num_rois, const float* im_info,
                                int32_t N, int32_t rois_per_image, int32_t num_classes, const float* means,
                                const float* stds, float score_thresh, float nms_thresh, int32_t max_per_image,
                                float* dets, int32_t* num_dets, void* workspace, size_t workspace_bytes,
                                mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * ops (README.md:24) + core/evaluation (README.md:20) -- Soft-NMS (Bodla et al. 2017), the test-time alternative to
 * greedy NMS (TEST.SOFT_NMS / nms.type=soft_nms of the toolboxes of this lineage). DESIGN.md 5g.
 * One list of candidates (box, score, id), ids unique within the list:
 *   a candidate is live while score > min_score (strict, as score_thresh above);
 *   repeat until max_keep selections are made or nothing is live:
 *     select the live candidate with the largest (score, then lower id); output it with its CURRENT score; remove it;
 *     for every other live candidate: o = mxdet_iou(selected, candidate); score = score * w, where
 *       method 0 (hard):     w = o > nms_thresh ? 0 : 1
 *       method 1 (linear):   w = o > nms_thresh ? 1 - o : 1
 *       method 2 (Gaussian): t = o * o; t = t / sigma; w = mxdet_expf(-t)
 *   each step one fp32 operation in this order, no FMA contraction. mxdet_expf(-0.0f) == 1.0f exactly, so a box that
 *   does not overlap the selected one keeps its score bits under every method.
 * The selected (score, id) keys strictly decrease along a list's output (scores only decay; intended for
 * min_score >= 0 -- with a negative min_score a candidate suppressed by method 0 stays live at score 0).
 *
 * mxdet_soft_nms_batched: B independent lists, boxes [B,n_max,4], scores [B,n_max], the first counts[b] entries of list
 * b valid, in any order; id = position in the list; n_max <= 4096. keep_idx [B,max_keep] receives the selected
 * positions in selection order (padding -1), keep_scores [B,max_keep] their scores at selection (padding 0),
 * num_keep [B] their number. method outside 0..2, or sigma <= 0 with method 2: MXDET_EINVAL. */
int mxdet_soft_nms_batched(const float* boxes, const float* scores, const int32_t* counts, int32_t B, int32_t n_max,
                           int32_t method, float nms_thresh, float sigma, float min_score, int32_t max_keep,
                           int32_t* keep_idx, float* keep_scores, int32_t* num_keep, mxdet_stream_t stream);
/* mxdet_detection_postprocess with its per-class greedy NMS replaced by Soft-NMS: per image and foreground class the
 * candidates with score > score_thresh form one list (id = roi index, min_score = score_thresh, max_keep =
 * max_per_image -- a later selection of a class cannot reach the image's best max_per_image); then the max_per_image best
 * over all classes by (score at selection desc, roi asc, class asc). dets carries the score at selection. Same
 * workspace as mxdet_detection_postprocess. */
int mxdet_detection_postprocess_soft(const void* cls_logits, const void* bbox_pred, int32_t dtype, int32_t ld_cls,
                                     int32_t ld_reg, const float* rois, const int32_t* num_rois, const float* im_info,
                                     int32_t N, int32_t rois_per_image, int32_t num_classes, const float* means,
                                     const float* stds, float score_thresh, float nms_thresh, int32_t max_per_image,
                                     float* dets, int32_t* num_dets, void* workspace, size_t workspace_bytes,
                                     int32_t method, float sigma, mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * rpn_heads + ops (README.md:28, :24) -- pyramid proposal generation.
 * MXNet role: contrib.Proposal / MultiProposal, or the lineage's pyramid-proposal CustomOp.
 * Per image and level: top `pre_nms_top_n` anchors by objectness logit (ties: lower anchor index
 * first) -> decode deltas at the anchors, clip to the image -> drop boxes with w or h < min_size ->
 * NMS(thresh) -> at most post_nms_top_n per level; levels merged per image by (score desc, global
 * anchor index asc) and cut to post_nms_top_n.
 *
 * Level l has H[l] x W[l] cells, A anchors per cell, feature stride stride[l]; its logits and deltas
 * live in one tensor each, addressed with element strides so NCHW and NHWC producers both fit:
 *   score(n,y,x,a)   = cls[l][n*cls_sn[l] + y*cls_sy[l] + x*cls_sx[l] + a*cls_sa[l]]
 *   delta(n,y,x,a,k) = reg[l][n*reg_sn[l] + y*reg_sy[l] + x*reg_sx[l] + (a*4+k)*reg_sc[l]]
 * Outputs: rois[N,post_nms_top_n,5] (batch index, box; zero padded), roi_scores[N,post_nms_top_n],
 * roi_anchor[N,post_nms_top_n] (global anchor index, -1 padding), num_rois[N]. */
typedef struct {
  int32_t num_levels;       /* <= 8 */
  int32_t A;                /* anchors per cell */
  int32_t H[8], W[8], stride[8];
  const void* cls[8];
  const void* reg[8];
  int64_t cls_sn[8], cls_sy[8], cls_sx[8], cls_sa[8];
  int64_t reg_sn[8], reg_sy[8], reg_sx[8], reg_sc[8];
  int32_t dtype;            /* MXDET_DTYPE_F32 | MXDET_DTYPE_BF16 (both tensors) */
  int32_t classes;          /* 0 or 1: plain. C > 1 (dense one-stage heads): A counts (anchor, class) pairs, a = anchor*C + c;
                             * deltas and base anchors are looked up with a / C (base_anchors stays [A/C,4]) */
  const float* base_anchors[8]; /* device, [A,4] per level */
} mxdet_pyramid_t;

size_t mxdet_proposal_workspace_bytes(const mxdet_pyramid_t* p, int32_t N, int32_t pre_nms_top_n);
int mxdet_proposal(const mxdet_pyramid_t* p, int32_t N, const float* im_info /* [N,3] h,w,scale */,
                   int32_t pre_nms_top_n, int32_t post_nms_top_n, float nms_thresh, float min_size,
                   float* rois, float* roi_scores, int32_t* roi_anchor, int32_t* num_rois,
                   void* workspace, size_t workspace_bytes, mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * core/anchor (README.md:16) -- anchor <-> GT assignment and RPN target sampling.
 * anchors[A_total,4]; gt_boxes[N,G_max,5] (x1,y1,x2,y2,class; rows with class < 0 are padding).
 * label = 1 if max IoU >= fg_thresh or the anchor attains some GT's maximum IoU (> 0);
 *         0 if max IoU < bg_thresh; -1 otherwise; anchors reaching outside the image by more than
 * allowed_border are -1. Then subsample to `batch_size` per image (at most fg_fraction*batch_size
 * foreground) with Philox keys (mxdet_math.h: mxdet_sample_key, streams 0/1); batch_size <= 0 keeps
 * every label (RetinaNet). Outputs: labels[N,A_total] int32, matched_gt[N,A_total] int32 (argmax GT,
 * lowest index on ties), bbox_targets[N,A_total,4] (encoded for label==1, else 0),
 * max_iou[N,A_total] (may be NULL). step_dev (may be NULL): device word that overrides `step` when
 * the launch is replayed from a hipGraph (kernel arguments are frozen at capture). */
size_t mxdet_anchor_target_workspace_bytes(int32_t N, int64_t A_total, int32_t G_max);
int mxdet_anchor_target(const float* anchors, int64_t A_total, const float* gt_boxes, int32_t N,
                        int32_t G_max, const float* im_info, float fg_thresh, float bg_thresh,
                        float allowed_border, int32_t batch_size, float fg_fraction, uint32_t seed,
                        uint32_t step, const uint32_t* step_dev, uint32_t image_offset, int32_t* labels,
                        int32_t* matched_gt,
                        float* bbox_targets, float* max_iou, void* workspace, size_t workspace_bytes,
                        mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * core/anchor (README.md:16) -- ATSS anchor assignment (Adaptive Training Sample Selection, Zhang et al., CVPR 2020)
 * for the dense head: the alternative to mxdet_anchor_target's max-IoU rule with batch_size <= 0. DESIGN.md 5h.
 * Inputs:
 *   anchors[A_total,4]   fp32, the head's global order (level, y, x, a).
 *   level_offsets[L+1]   level l owns anchors [off[l], off[l+1]).
 *   gt_boxes[N,G_max,5]  rows with class < 0 are padding, anywhere in the list.
 *   topk = k.
 * Every step below is one fp32 operation in the order written, without FMA contraction.
 *   1. Centres. Anchor centre cx = 0.5f*(x1+x2), cy = 0.5f*(y1+y2). Ground-truth centre the same.
 *   2. Distance key. dx = cx-gx; dy = cy-gy; d = dx*dx + dy*dy (a product, a product and one add; no square root:
 *      ranking needs none).
 *   3. Candidates of (image n, valid GT g, level l): the min(k, n_l) anchors of the level with the smallest
 *      (d, anchor index) -- a total order on the float bit pattern of d, which is non-negative; ties go to the lower
 *      global anchor index. There is no inside-image filter (RetinaNet already runs with allowed_border = 1e6).
 *   4. Statistics of g. Take all its candidates over the levels in ascending global anchor index, with
 *      v_i = mxdet_iou(anchor_i, gt_g) (the +1 convention):
 *        s = ((v_0 + v_1) + v_2) + ...;  mean = s / (float)count;
 *        ss = sum in the same order of t = v_i - mean; t*t;
 *        var = count > 1 ? ss / (float)(count-1) : 0   (the unbiased form, as the published code's .std()).
 *   5. Positive candidates. The threshold test is v_i >= mean and (v_i-mean)*(v_i-mean) >= var -- the squared form of
 *      v_i >= mean + std, chosen so that no square root has to agree between CPU and GPU. The centre test is
 *      min(cx-gx1, cy-gy1, gx2-cx, gy2-cy) > 0.01f. A candidate is positive when both hold.
 *   6. Conflicts. An anchor positive for several ground-truth boxes goes to the one with the largest IoU, by float
 *      bits; ties go to the lower GT index.
 *   7. Outputs, with the shapes and meaning of mxdet_anchor_target (mxdet_anchor_class_labels and both
 *      mxdet_retina_loss_level* entries consume them unchanged):
 *        labels[N,A_total]         1 for positive, 0 for everything else; never -1 (ATSS has no ignore band); an image
 *                                  without a valid GT is all 0.
 *        matched_gt[N,A_total]     g for positives, -1 otherwise.
 *        bbox_targets[N,A_total,4] mxdet_encode(anchor, gt) for positives, 0 otherwise.
 *        matched_iou[N,A_total]    optional, may be NULL: the IoU with the matched GT, 0 otherwise.
 * Limits: 1 <= topk <= 16, 1 <= L <= 8, G_max <= 1024, every level non-empty, offsets ascending from 0 with
 * off[L] == A_total; violations return MXDET_ESHAPE / MXDET_EINVAL (topk, null pointers) from the host check before any
 * launch, with a message naming the argument. level_offsets is a HOST array, read at call time and passed by value to
 * the kernels (no device copy, no retained pointer). No allocation, no host synchronisation: the result is a pure
 * function of the inputs, so a captured graph replays it with new gt_boxes contents. */
size_t mxdet_atss_assign_workspace_bytes(int32_t N, int64_t A_total, int32_t G_max);
int mxdet_atss_assign(const float* anchors, int64_t A_total, const int64_t* level_offsets /* host, L+1 */, int32_t L,
                      const float* gt_boxes, int32_t N, int32_t G_max, int32_t topk,
                      int32_t* labels, int32_t* matched_gt, float* bbox_targets, float* matched_iou /* may be NULL */,
                      void* workspace, size_t workspace_bytes, mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * core/bbox (README.md:17) -- proposal-target: RoI sampling for the box head.
 * Candidates of image n = its first num_rois[n] proposals followed by its valid GT boxes.
 * fg: max IoU >= fg_thresh; bg: bg_lo <= max IoU < bg_hi. Sample min(fg_fraction*rois_per_image,
 * #fg) foreground and fill up with background, both by Philox keys (streams 2/3); selected rois are
 * written foreground first, each group in ascending candidate order; unfilled slots are padding
 * (label -1, zero box, zero weights).
 * Outputs: out_rois[N,R,5], labels[N,R] int32 (class, 0 = background), bbox_targets[N,R,4*num_reg]
 * and bbox_weights[N,R,4*num_reg] (class-specific slot, normalised (t-mean)/std), matched_gt[N,R],
 * num_fg[N]. num_reg = num_classes (class-specific) or 1 (class-agnostic). */
int mxdet_proposal_target(const float* rois, const int32_t* num_rois, int32_t rois_stride,
                          const float* gt_boxes, int32_t N, int32_t G_max, int32_t rois_per_image,
                          float fg_fraction, float fg_thresh, float bg_hi, float bg_lo,
                          int32_t num_classes, int32_t class_agnostic,
                          const float* means /* HOST [4] */, const float* stds /* HOST [4] */,
                          uint32_t seed, uint32_t step, const uint32_t* step_dev,
                          uint32_t image_offset, float* out_rois, int32_t* labels,
                          float* bbox_targets, float* bbox_weights, int32_t* matched_gt,
                          int32_t* num_fg, mxdet_stream_t stream);
/* IoU-balanced negative sampling (Libra R-CNN, Pang et al., CVPR 2019): mxdet_proposal_target with the
 * background quota spread over num_bins = K (1..MXDET_SAMPLER_MAX_BINS) IoU bins. Foreground selection, candidate set,
 * Philox streams (2 = fg, 3 = bg) and output layout are those of mxdet_proposal_target. A background candidate
 * (bg_lo <= iou < bg_hi) belongs to bin k = the number of edges e_j, j = 1..K-1, with iou >= e_j, where
 * e_j = bg_lo + (bg_hi - bg_lo) * ((float)j / (float)K), each operation one fp32 operation (the edges are FIXED; they do
 * not depend on the largest background IoU as mmdetection's do). With want = rois_per_image - nfg and per = want / K
 * (integer division), bin k gives its min(per, count_k) candidates of smallest (key, index); the shortfall
 * want - sum(taken) is filled with the smallest (key, index) among the background candidates not yet chosen, from any
 * bin; fewer candidates than want leaves padding. K = 1 is mxdet_proposal_target bit for bit. No host synchronisation,
 * no allocation, no float atomics; capturable; a pure function of its inputs. Bad num_bins: MXDET_EINVAL, no launch. */
#define MXDET_SAMPLER_MAX_BINS 8
int mxdet_proposal_target_balanced(const float* rois, const int32_t* num_rois, int32_t rois_stride,
                                   const float* gt_boxes, int32_t N, int32_t G_max, int32_t rois_per_image,
                                   float fg_fraction, float fg_thresh, float bg_hi, float bg_lo, int32_t num_classes,
                                   int32_t class_agnostic, const float* means /* HOST [4] */,
                                   const float* stds /* HOST [4] */, uint32_t seed, uint32_t step,
                                   const uint32_t* step_dev, uint32_t image_offset, int32_t num_bins, float* out_rois,
                                   int32_t* labels, float* bbox_targets, float* bbox_weights, int32_t* matched_gt,
                                   int32_t* num_fg, mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * core/bbox -- online hard example mining for the box head (Shrivastava et al., CVPR 2016).
 * An image's pool of P rows is a proposal-target output with rois_per_image = P, fg_fraction = 1: every candidate,
 * foreground first, then padding (label -1). A read-only forward of the box head over the N*P pool rows is scored, the
 * candidates are ordered by score, deduplicated by NMS, and the first R survivors become the head's training rois.
 * All entries: host argument checks before any launch, no allocation, no host synchronisation, no float atomics;
 * capturable, and a pure function of the inputs. P <= 16384 + 1024 and R >= 1, else MXDET_ESHAPE.
 *
 * mxdet_ohem_roi_score: score[r] (f32 [R]) = cls_r + reg_r in one fp32 add, where cls_r / reg_r are loss_out[0] / [1] of
 * mxdet_rcnn_loss (kind = -1: bbox_targets, bbox_weights, sigma are read; rois, matched_gt, gt_boxes may be NULL) or of
 * mxdet_rcnn_loss_iou (kind = MXDET_IOU_LOSS_*: rois, matched_gt, gt_boxes, N, G_max, stds, reg_weight are read;
 * bbox_targets, bbox_weights may be NULL) called on row r alone with R = 1, norm = 1, loss_scale = 1 -- the same device
 * code, the same bits. Rows with labels[r] < 0 get -1.0f. Writes no gradients. One wave per row. */
int mxdet_ohem_roi_score(const void* cls_logits, const void* bbox_pred, int32_t dtype, int32_t ld_cls, int32_t ld_reg,
                         const int32_t* labels, const float* bbox_targets, const float* bbox_weights, const float* rois,
                         const int32_t* matched_gt, const float* gt_boxes, int32_t N, int32_t G_max, int64_t R,
                         int32_t num_classes, int32_t reg_dim, int32_t kind, float sigma, float std_x, float std_y,
                         float std_w, float std_h, float reg_weight, float* score, mxdet_stream_t stream);
/* mxdet_ohem_select: score / labels [N,P], rois [N,P,5]. Candidates of image n: rows with label >= 0. Order: the
 * score's IEEE bit pattern as uint32 descending, then pool slot ascending (for scores >= 0 the numeric order; a NaN comes
 * first; the order is total). Dedup: greedy NMS over that order on rois[:, 1:5] -- a kept box suppresses a later one when
 * mxdet_iou ("+1" convention) > nms_thresh, as mxdet_nms_batched; nms_thresh >= 1 launches no NMS; nms_thresh < 1
 * needs P <= 4096 (the keep scan's limit), else MXDET_ESHAPE. The first min(R, kept) kept candidates are chosen.
 * sel [N,R] int32: the chosen pool slots, foreground (label > 0) in ascending slot, then background in ascending slot,
 * then -1. num_sel [N]: chosen; num_fg [N]: chosen foreground. */
size_t mxdet_ohem_select_workspace_bytes(int32_t N, int32_t P);
int mxdet_ohem_select(const float* score, const int32_t* labels, const float* rois, int32_t N, int32_t P, int32_t R,
                      float nms_thresh, int32_t* sel, int32_t* num_sel, int32_t* num_fg, void* workspace,
                      size_t workspace_bytes, mxdet_stream_t stream);
/* mxdet_ohem_gather: output row (n, s) = pool row (n, sel[n, s]) in mxdet_proposal_target's layout (out_rois [N,R,5],
 * labels [N,R], bbox_targets / bbox_weights [N,R,reg_dim], matched_gt [N,R]); sel < 0: the padding row of
 * mxdet_proposal_target (roi (n,0,0,0,0), label -1, matched -1, zero targets and weights). The four target / weight
 * pointers (16-byte aligned, reg_dim % 4 == 0) may be NULL together: the IoU-family losses do not read them. */
int mxdet_ohem_gather(const int32_t* sel, const float* pool_rois, const int32_t* pool_labels,
                      const int32_t* pool_matched_gt, const float* pool_bbox_targets, const float* pool_bbox_weights,
                      int32_t N, int32_t P, int32_t R, int32_t reg_dim, float* out_rois, int32_t* labels,
                      float* bbox_targets, float* bbox_weights, int32_t* matched_gt, mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * roi_extractors (README.md:32) -- FPN level map + RoIAlign. MXNet role: contrib.ROIAlign
 * (Detectron aligned=False semantics), one call covering all pyramid levels.
 * feats[l]: bf16 [N,H[l],W[l],C] channels-last; rois[R,5]; levels[R] int32 in [lvl_min, lvl_min+L).
 * out: bf16 [R,PH,PW,C]. Bilinear taps in fp32 in the fixed order ((w1*v1+w2*v2)+w3*v3)+w4*v4,
 * samples summed iy-major then ix, times 1/count, rounded to bf16 once. */
int mxdet_fpn_level_map(const float* rois, int64_t R, int32_t lvl_min, int32_t lvl_max,
                        int32_t* levels, mxdet_stream_t stream);
typedef struct {
  int32_t num_levels, lvl_min;
  int32_t H[8], W[8];
  float spatial_scale[8];
  void* feat[8]; /* bf16 [N,H,W,C]; for bwd: fp32 gradient accumulators of the same shape */
} mxdet_feat_pyramid_t;
int mxdet_roi_align_fwd(const mxdet_feat_pyramid_t* f, int32_t N, int32_t C, const float* rois,
                        const int32_t* levels, int64_t R, int32_t PH, int32_t PW,
                        int32_t sampling_ratio, uint16_t* out, mxdet_stream_t stream);
/* bwd: scatter-adds grad_out (bf16 [R,PH,PW,C]) into fp32 [N,H,W,C] accumulators f->feat[l]
 * (caller zeroes them for accumulate = 0 semantics). fp32 atomics: order-dependent in the last bits. */
int mxdet_roi_align_bwd(const mxdet_feat_pyramid_t* f, int32_t N, int32_t C, const float* rois,
                        const int32_t* levels, int64_t R, int32_t PH, int32_t PW,
                        int32_t sampling_ratio, const uint16_t* grad_out, mxdet_stream_t stream);
/* bwd, gather form: deterministic, no atomics, no fp32 accumulators. f->feat[l] are the bf16 [N,H,W,C] GRADIENT maps
 * themselves: every pixel is written (accumulate = 0) or added to (accumulate = 1, one bf16 rounding of the sum).
 * Per pixel the contributions are summed in fp32 in a fixed order: roi index ascending; inside a roi the bilinear
 * weights are collapsed per pooling bin (they are separable), row bins before column bins -- bit-reproducible run to
 * run, last-bit different from the sample-by-sample order of mxdet_roi_align_bwd. Requires sampling_ratio > 0 and at
 * most 32 samples per axis. The per-roi records the gather reads depend only on the rois: `_prepare` writes them into
 * the workspace (it can be issued as soon as the rois exist, e.g. in the forward pass) and `_prepared` is the gather
 * without that pass; the plain call does both. R = 0 is the limit of the definition: all-zero maps (accumulate = 0) or
 * untouched ones (accumulate = 1); rois, levels and grad_out may be null then, the workspace (sized for R = 0) may not. */
size_t mxdet_roi_align_bwd_gather_workspace_bytes(const mxdet_feat_pyramid_t* f, int32_t N, int64_t R);
int mxdet_roi_align_bwd_gather(const mxdet_feat_pyramid_t* f, int32_t N, int32_t C, const float* rois,
                               const int32_t* levels, int64_t R, int32_t PH, int32_t PW, int32_t sampling_ratio,
                               const uint16_t* grad_out, int32_t accumulate, void* workspace, size_t workspace_bytes,
                               mxdet_stream_t stream);
int mxdet_roi_align_bwd_gather_prepare(const mxdet_feat_pyramid_t* f, int32_t N, const float* rois,
                                       const int32_t* levels, int64_t R, int32_t PH, int32_t PW, int32_t sampling_ratio,
                                       void* workspace, size_t workspace_bytes, mxdet_stream_t stream);
int mxdet_roi_align_bwd_gather_prepared(const mxdet_feat_pyramid_t* f, int32_t N, int32_t C, const float* rois,
                                        const int32_t* levels, int64_t R, int32_t PH, int32_t PW, int32_t sampling_ratio,
                                        const uint16_t* grad_out, int32_t accumulate, void* workspace,
                                        size_t workspace_bytes, mxdet_stream_t stream);

/* (Modulated) deformable RoI pooling, MXNet role contrib.DeformablePSROIPooling with group_size 1, part_size = pooled,
 * output_dim = C, class-agnostic offsets (mmdetection dpool / mdpool), over the same pyramid and level map as RoIAlign,
 * one launch for all levels. For roi r (batch n = rois[r][0], box x1,y1,x2,y2, level l, s = spatial_scale[l]):
 *   rsw = round(x1)*s - 0.5, rew = (round(x2) + 1)*s - 0.5 (C round: half away from zero; likewise h with y1, y2),
 *   roi_w = max(rew - rsw, 0.1), bin_w = roi_w / PW, sub_w = bin_w / S; tx = trans[r][ph*PW + pw] * trans_std,
 *   ty = trans[r][PH*PW + ph*PW + pw] * trans_std (0 without trans); wstart = (pw*bin_w + rsw) + tx*roi_w (h alike);
 *   samples w = wstart + iw*sub_w, h = hstart + ih*sub_h (ih, iw in [0,S)), skipped outside [-0.5, W-0.5] x
 *   [-0.5, H-0.5], else clamped to [0, W-1] x [0, H-1] and mixed bilinearly from floor / ceil corners;
 *   out[r,ph,pw,c] = count ? sum/count : 0, modulated: times sigmoid(mask_logit[r][ph*PW + pw]). bf16, rounded once.
 * trans / mask_logit: bf16 rows of trans_stride / mask_stride elements (columns past 2*PH*PW / PH*PW are padding, never
 * read). A call without trans (trans == NULL) is the no-trans pass; modulated needs trans and mask_logit. */
typedef struct {
  mxdet_feat_pyramid_t pyr;   /* fwd / bwd_trans: the features; bwd_feat: the bf16 GRADIENT maps */
  int32_t N, C;               /* C % 8 == 0 */
  int32_t PH, PW;             /* PH * PW <= 64 */
  int32_t sample_per_part;    /* S in [1, 16] */
  float trans_std;
  int32_t modulated;
  int32_t trans_stride, mask_stride;
  int32_t accumulate;         /* bwd_feat: add into the maps instead of overwriting */
} mxdet_dpool_desc_t;
int mxdet_dpool_fwd(const mxdet_dpool_desc_t* d, const float* rois, const int32_t* levels, int64_t R,
                    const uint16_t* trans, const uint16_t* mask_logit, uint16_t* out, mxdet_stream_t stream);
/* d_trans [R, trans_stride], d_mask [R, mask_stride] (modulated), both written in full (padding columns zero):
 *   d_tx = sum_{samples, c} (U(y1,x1)*dy + U(y0,x1)*(1-dy) - U(y1,x0)*dy - U(y0,x0)*(1-dy)) * trans_std * roi_w * g_c,
 *   g_c = dout[r,ph,pw,c] (* sigmoid) / count, d_ty alike; d_mask = sum_c dout * (sum/count) * sigma * (1 - sigma).
 *   Channels reduced in a fixed order (one wave per (roi, bin), a fixed butterfly). Needs trans. */
int mxdet_dpool_bwd_trans(const mxdet_dpool_desc_t* d, const float* rois, const int32_t* levels, int64_t R,
                          const uint16_t* trans, const uint16_t* mask_logit, const uint16_t* dout, uint16_t* d_trans,
                          uint16_t* d_mask, mxdet_stream_t stream);
/* The feature adjoint: d->pyr.feat[l] (=, or += under accumulate) the transpose of the pooling applied to dout, without
 * float atomics: per-bin records, then a gather in which every 8-pixel row segment walks the rois that reach it
 * (ascending), their bins (ascending) and samples (ih, iw) and sums in fp32 in that order, rounding once. Bit-
 * reproducible, any overlap. R <= 65535, level sides < 32768. Workspace: mxdet_dpool_bwd_feat_workspace_bytes. */
size_t mxdet_dpool_bwd_feat_workspace_bytes(const mxdet_dpool_desc_t* d, int64_t R);
int mxdet_dpool_bwd_feat(const mxdet_dpool_desc_t* d, const float* rois, const int32_t* levels, int64_t R,
                         const uint16_t* trans, const uint16_t* mask_logit, const uint16_t* dout, void* workspace,
                         size_t workspace_bytes, mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * core/loss (README.md:19)
 * smooth-L1 (MXNet smooth_l1(scalar=sigma)): elementwise on (pred - target) * weight. */
int mxdet_smooth_l1_fwd(const float* pred, const float* target, const float* weight, int64_t n,
                        float sigma, float* out, mxdet_stream_t stream);
int mxdet_smooth_l1_bwd(const float* pred, const float* target, const float* weight,
                        const float* grad_out, int64_t n, float sigma, int32_t accumulate,
                        float* grad_pred, mxdet_stream_t stream);

/* Sigmoid focal loss (RetinaNet): logits [n,C] (dtype f32|bf16), labels[n] int32 (-1 ignore,
 * 0 background, c in 1..C foreground class c), normaliser = max(1, #foreground) computed on device.
 * loss_out[1] fp32 (sum / normaliser, fixed reduction order); grad written in the logits dtype: exactly the n*C
 * elements (zeros for ignored rows), scaled by grad_scale.
 * workspace: mxdet_loss_workspace_bytes(n). */
size_t mxdet_loss_workspace_bytes(int64_t n);
int mxdet_focal_loss(const void* logits, int32_t dtype, const int32_t* labels, int64_t n, int32_t C,
                     float alpha, float gamma, float grad_scale, float* loss_out, void* grad_logits,
                     void* workspace, size_t workspace_bytes, mxdet_stream_t stream);

/* RetinaNet: per-anchor class labels (class of the matched GT for label == 1, else the -1 / 0 label) and the
 * number of foreground anchors (device word, the loss normaliser). */
int mxdet_anchor_class_labels(const int32_t* labels, const int32_t* matched_gt, const float* gt_boxes, int32_t N,
                              int64_t A_total, int32_t G_max, int32_t* cls_labels, int32_t* num_fg,
                              mxdet_stream_t stream);
/* RetinaNet losses fused fwd+bwd over one pyramid level: sigmoid focal loss on cls[cell*ld_cls + a*C + c] and
 * smooth-L1 on reg[cell*ld_reg + a*4 + k] (bf16 channels-last head outputs), both normalised by max(1, *num_fg);
 * gradients written in place of the same layout (padding channels untouched); partial sums (cls, reg) per
 * workgroup, reduced by mxdet_loss_finalize. */
int32_t mxdet_retina_loss_num_partials(int32_t N, int32_t H, int32_t W, int32_t A);
int mxdet_retina_loss_level(const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W, int32_t A,
                            int32_t C, int32_t ld_cls, int32_t ld_reg, const int32_t* cls_labels,
                            const float* bbox_targets, int64_t A_total, int64_t level_offset, float alpha,
                            float gamma, float sigma, const int32_t* num_fg, float loss_scale, uint16_t* grad_cls,
                            uint16_t* grad_reg, float* partial, mxdet_stream_t stream);

/* RPN losses fused fwd+bwd over one pyramid level's head output.
 * head: bf16 [N,H,W,Cpad] channels-last, channel a = objectness logit of anchor a, channel
 * A + 4a + k = delta k of anchor a. labels / bbox_targets are the mxdet_anchor_target outputs
 * (global anchor order), level_offset = index of this level's first anchor.
 * cls: sigmoid BCE over label >= 0; reg: smooth-L1(sigma) over label == 1; both * norm
 * (norm = 1 / sampled batch, chosen by the caller). Partial sums are appended to
 * partial[2*num_blocks] and reduced in fixed order by mxdet_loss_finalize.
 * grad_head: bf16 [N,H,W,Cpad] = d(loss)/d(head) * loss_scale (channels >= 5A are written 0).
 * Per-workgroup partial sums (cls, reg) go to partial[2*i + {0,1}], i < mxdet_rpn_loss_num_partials;
 * the caller lays the levels' partial ranges back to back and reduces them in index order with
 * mxdet_loss_finalize, so the scalar losses are reproducible bit for bit. */
int32_t mxdet_rpn_loss_num_partials(int32_t N, int32_t H, int32_t W);
int mxdet_rpn_loss_level(const uint16_t* head, int32_t N, int32_t H, int32_t W, int32_t A,
                         int32_t Cpad, const int32_t* labels, const float* bbox_targets,
                         int64_t A_total, int64_t level_offset, float sigma, float norm,
                         float loss_scale, uint16_t* grad_head, float* partial,
                         mxdet_stream_t stream);
/* out[j] = sum over i < count of partial[i*ncomp + j], fixed order, one workgroup */
int mxdet_loss_finalize(const float* partial, int32_t count, int32_t ncomp, float* out,
                        mxdet_stream_t stream);

/* Box-head losses fused fwd+bwd. cls_logits: [R,num_classes] (dtype), softmax CE with ignore label
 * -1, normalised by norm; bbox_pred [R,4*num_reg] vs targets/weights, smooth-L1(sigma) * norm.
 * loss_out[2] = (cls, reg); grads written in the logits dtype scaled by loss_scale: columns [0,num_classes) of every
 * grad_cls row and [0,reg_dim) of every grad_reg row (zeros for ignored rows / zero weights); columns from there up to
 * ld_cls / ld_reg are left untouched, so both may be column views of one fused buffer. */
int mxdet_rcnn_loss(const void* cls_logits, const void* bbox_pred, int32_t dtype, int32_t ld_cls,
                    int32_t ld_reg, const int32_t* labels, const float* bbox_targets,
                    const float* bbox_weights, int64_t R, int32_t num_classes, int32_t reg_dim,
                    float sigma, float norm, float loss_scale, float* loss_out, void* grad_cls,
                    void* grad_reg, void* workspace, size_t workspace_bytes, mxdet_stream_t stream);
/* mxdet_rcnn_loss with Balanced L1 (Libra R-CNN, Pang et al., CVPR 2019) in place of smooth-L1: same row
 * walk, targets and weights convention, columns left untouched alike; loss_out[0] and grad_cls are bit-identical to
 * mxdet_rcnn_loss. Per column with weight w != 0 of a row with label > 0: d = (pred - target) * w, a = |d|,
 *   a < beta:  L = (alpha / b) * (b*a + 1) * log(b*a/beta + 1) - alpha*a,  dL/dd = sign(d) * alpha * log(b*a/beta + 1)
 *   else:      L = gamma*a + gamma/b - alpha*beta,                           dL/dd = sign(d) * gamma
 * (log = mxdet_logf; fp32 operation order: DESIGN.md section 3). b is the caller's float32(exp(gamma/alpha) - 1): the
 * kernel never evaluates it. The closed-form gradient is the paper's: the derivative of L exactly when beta = 1 (the
 * published setting); value and gradient are continuous at a = beta for every beta. loss_out[1] = sum_r (reg_weight * sum_c L) * norm; grad_reg = dL/dd * reg_weight * w * norm *
 * loss_scale. alpha, gamma, beta, b, reg_weight > 0, else MXDET_EINVAL. */
int mxdet_rcnn_loss_balanced(const void* cls_logits, const void* bbox_pred, int32_t dtype, int32_t ld_cls, int32_t ld_reg,
                             const int32_t* labels, const float* bbox_targets, const float* bbox_weights, int64_t R,
                             int32_t num_classes, int32_t reg_dim, float alpha, float gamma, float beta, float b,
                             float reg_weight, float norm, float loss_scale, float* loss_out, void* grad_cls,
                             void* grad_reg, void* workspace, size_t workspace_bytes, mxdet_stream_t stream);

/* IoU-family box losses on the DECODED box. Per element: a box b (roi / anchor), a ground-truth box g and
 * four raw deltas d; the prediction is b decoded by d * stds ("+1" convention, means 0, dw / dh clamped at
 * MXDET_BBOX_XFORM_CLIP, no image clip), evaluated relative to b's corner (x1, y1). L = 1 - IoU (MXDET_IOU_LOSS_IOU),
 * + (C - U) / C with C the enclosing box's area (_GIOU), or + rho^2 / (cw^2 + ch^2) with rho the centre distance and
 * cw, ch the enclosing box's sides (_DIOU). No eps: the union is positive for every finite input. At an exact tie of a
 * max / min pair the gradient is the mean of the two one-sided gradients. stds are passed by value as four floats.
 * No entry synchronises with the host or uses atomics (capturable; sums in fixed order). */
#define MXDET_IOU_LOSS_IOU 0
#define MXDET_IOU_LOSS_GIOU 1
#define MXDET_IOU_LOSS_DIOU 2
/* The unfused primitive. boxes / gt [n,4] f32 (16-byte aligned), deltas and grad_deltas rows of ld >= 4 elements (dtype
 * f32 | bf16), weight [n] or NULL. loss[i] = weight[i] * L_i; grad_deltas[i, 0..3] = weight[i] * grad_scale * dL_i / dd
 * (columns 4 .. ld are left untouched). n == 0 returns MXDET_OK. */
int mxdet_box_iou_loss(const float* boxes, const float* gt, const void* deltas, int32_t dtype, int32_t ld,
                       const float* weight, int64_t n, int32_t kind, float std_x, float std_y, float std_w, float std_h,
                       float grad_scale, float* loss, void* grad_deltas, mxdet_stream_t stream);
/* mxdet_rcnn_loss with the regression term replaced: for labels[r] > 0 the box is rois[r, 1..4] ([R,5], column 0 = image),
 * the ground truth gt_boxes[image, matched_gt[r], 0..3] ([N,G_max,5]) and the deltas columns 4 * label .. 4 * label + 3 of
 * the bbox_pred row (reg_dim == 4 * num_classes); loss_out[1] = sum reg_weight * norm * L. grad_reg: those four columns
 * and zeros in every other column < reg_dim of every row. loss_out[0] and grad_cls are bit-identical to mxdet_rcnn_loss.
 * A roi whose image or match index lies outside gt_boxes regresses nothing. */
int mxdet_rcnn_loss_iou(const void* cls_logits, const void* bbox_pred, int32_t dtype, int32_t ld_cls, int32_t ld_reg,
                        const int32_t* labels, const float* rois, const int32_t* matched_gt, const float* gt_boxes,
                        int32_t N, int32_t G_max, int64_t R, int32_t num_classes, int32_t reg_dim, int32_t kind,
                        float std_x, float std_y, float std_w, float std_h, float reg_weight, float norm, float loss_scale,
                        float* loss_out, void* grad_cls, void* grad_reg, void* workspace, size_t workspace_bytes,
                        mxdet_stream_t stream);
/* mxdet_retina_loss_level with the regression term replaced: for cls_labels > 0 the box is anchors[global anchor index]
 * ([A_total,4] f32, 16-byte aligned), the ground truth gt_boxes[n, matched_gt[n, anchor], 0..3]; the term is
 * reg_weight * L / max(1, *num_fg). Same grid, partial layout (mxdet_retina_loss_num_partials) and vector / scalar split
 * as mxdet_retina_loss_level; partial[2i] and grad_cls are bit-identical to it. */
int mxdet_retina_loss_level_iou(const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W, int32_t A,
                                int32_t C, int32_t ld_cls, int32_t ld_reg, const int32_t* cls_labels, const float* anchors,
                                const int32_t* matched_gt, const float* gt_boxes, int32_t G_max, int64_t A_total,
                                int64_t level_offset, float alpha, float gamma, int32_t kind, float std_x, float std_y,
                                float std_w, float std_h, float reg_weight, const int32_t* num_fg, float loss_scale,
                                uint16_t* grad_cls, uint16_t* grad_reg, float* partial, mxdet_stream_t stream);

/* Quality-aware class losses for the RetinaNet head: QFL (Li et al., NeurIPS 2020) and the IoU-weighted
 * Varifocal loss (Zhang et al., CVPR 2021). They train the matched class column against the IoU of the predicted box with
 * its ground truth, so that the test-time score sigmoid(cls) ranks detections by localisation quality.
 * Per anchor: lab = cls_labels[n, anchor], m = matched_gt[n, anchor], q = the anchor's quality. For lab > 0 and
 * 0 <= m < G_max, q = inter / union of the decoded prediction against gt_boxes[n, m]: exactly the inter, union of the
 * IoU-family box losses above (corner-relative decode, "+1" convention, dw / dh clamp, stds by value). Otherwise q = 0.
 * q is a constant of the class loss: no gradient flows from the class term into the deltas.
 * Per element (anchor, class c): x the logit, s = sigmoid(x), y = q if lab == c + 1, else 0. With lab < 0 (ignore) every
 * element contributes 0 and its gradient is 0. BCE(s, y) = -y log s - (1 - y) log(1 - s), in the log forms of the focal loss.
 *   MXDET_CLS_LOSS_QFL, parameter beta passed in `gamma` (alpha is ignored):
 *     L = |y - s|^beta * BCE(s, y);  dL/dx = beta |e|^(beta-1) sign(e) s (1 - s) BCE + |e|^beta e, with e = s - y.
 *     beta = 2 takes the product form, any other beta > 0 mxdet_expf(beta * mxdet_logf(max(|e|, 1e-30f))).
 *   MXDET_CLS_LOSS_VFL, parameters alpha and gamma:
 *     y > 0:  L = y * BCE(s, y) and dL/dx = y (s - y);
 *     else:   L = -alpha s^gamma log(1 - s) and dL/dx = alpha (gamma s^gamma (1 - s) (-log(1 - s)) + s^gamma s).
 *     A matched anchor whose prediction does not overlap its ground truth (q == 0) is a negative in its own class column.
 * Both terms are normalised by max(1, *num_fg) and scaled by loss_scale / grad_scale as in the entries above. */
#define MXDET_CLS_LOSS_QFL 1
#define MXDET_CLS_LOSS_VFL 2
/* The unfused primitive, with the contract of mxdet_focal_loss (workspace mxdet_loss_workspace_bytes(n), fixed reduction
 * order, gradient in the logits dtype, normaliser = max(1, #labels > 0) counted on the device): logits [n,C] (f32 | bf16),
 * labels[n], quality[n] f32 = the y of row r's column labels[r] - 1. n == 0 writes loss_out[0] = 0 and returns MXDET_OK. */
int mxdet_quality_focal_loss(const void* logits, int32_t dtype, const int32_t* labels, const float* quality, int64_t n,
                             int32_t C, int32_t cls_kind, float alpha, float gamma, float grad_scale, float* loss_out,
                             void* grad_logits, void* workspace, size_t workspace_bytes, mxdet_stream_t stream);
/* mxdet_retina_loss_level_iou with the class term replaced by cls_kind: the box term (kind, stds, reg_weight), grid,
 * partial layout and vector / scalar split are that entry's; grad_reg and partial[2i+1] are bit-identical to it. The box
 * part of a workgroup runs first and hands the 256 qualities to the class walk through LDS: no atomics, no host
 * synchronisation, capturable; a replay follows new gt_boxes. gamma must be positive. */
int mxdet_retina_loss_level_quality(const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W, int32_t A,
                                    int32_t C, int32_t ld_cls, int32_t ld_reg, const int32_t* cls_labels,
                                    const float* anchors, const int32_t* matched_gt, const float* gt_boxes, int32_t G_max,
                                    int64_t A_total, int64_t level_offset, int32_t cls_kind, float alpha, float gamma,
                                    int32_t kind, float std_x, float std_y, float std_w, float std_h, float reg_weight,
                                    const int32_t* num_fg, float loss_scale, uint16_t* grad_cls, uint16_t* grad_reg,
                                    float* partial, mxdet_stream_t stream);

/* Distribution box regression for the RetinaNet head: the box half of Generalized Focal Loss (Li et al.,
 * NeurIPS 2020). R = reg_max in 1..MXDET_REG_MAX_LIMIT, s = the level's stride, b the anchor box, cx = 0.5 (b.x1 + b.x2),
 * cy = 0.5 (b.y1 + b.y2), g the matched ground truth.
 * Layout: 4 (R + 1) logits per anchor, the logit of bin k of side `side` (0..3 = l, t, r, b) of anchor a at channel
 *   a * 4 (R + 1) + side * (R + 1) + k: the published layout, so converted weights keep their order.
 * Integral decode, float32, no FMA contraction, in this order per side: m = max_k x_k; e_k = mxdet_expf(x_k - m);
 *   Z = sum_k e_k and S = sum_k (float)k * e_k, both from 0 with k ascending; E = S / Z; p_k = e_k / Z.
 *   Box (cx - s E_l, cy - s E_t, cx + s E_r, cy + s E_b); the losses work relative to (cx, cy): p1 = (-(s E_l), -(s E_t)),
 *   p2 = (s E_r, s E_b), g1 = (g.x1 - cx, g.y1 - cy), g2 = (g.x2 - cx, g.y2 - cy), length p2 - p1 + 1, centre 0.5 (p1 + p2).
 * Box term: reg_weight * L, L the IoU / GIoU / DIoU loss above on that box ("+1" convention, the same inter / union and tie
 *   rule); the gradient reaches the logits through dE / dx_k = p_k (k - E).
 * Quality (cls_kind QFL / VFL): q = inter / union of that box, a constant of the class loss: no gradient flows from the
 *   class term into the distribution. q = 0 for background, ignored anchors and matches outside gt_boxes.
 * DFL: per side dist = (cx - g.x1, cy - g.y1, g.x2 - cx, g.y2 - cy), y = clamp(dist / s, 0, (float)R - 0.1f) (0.1: the
 *   published epsilon), yl = floor(y), CE(x, j) = (m + mxdet_logf(Z)) - x_j:
 *   DFL = (yl + 1 - y) CE(x, yl) + (y - yl) CE(x, yl + 1); y is a constant. The anchor's term is dfl_weight * (1/4) * the sum
 *   of its four sides, added in the order l, t, r, b.
 * Only cls_labels > 0 with 0 <= matched < G_max regresses. The level entry normalises all three terms by max(1, *num_fg)
 * and scales by loss_scale. Not part of this: weighting the box and DFL terms by the detached class score. */
#define MXDET_CLS_LOSS_FOCAL 0
#define MXDET_REG_MAX_LIMIT 31
/* The unfused primitive (what a CustomOp binding calls), four lanes per row: boxes[n,4], gt[n,4] (16-byte aligned), logits
 * rows of ld >= 4 (R + 1) elements (f32 | bf16). Per row: loss_box = reg_weight * L, loss_dfl, quality (may be NULL), and
 * grad_logits (logits dtype and ld) = grad_scale * d(loss_box + loss_dfl) / dx. Columns past 4 (R + 1) are untouched.
 * n == 0 returns MXDET_OK. */
int mxdet_box_dist_loss(const float* boxes, const float* gt, const void* logits, int32_t dtype, int32_t ld, int64_t n,
                        int32_t reg_max, float stride, int32_t kind, float reg_weight, float dfl_weight, float grad_scale,
                        float* loss_box, float* loss_dfl, float* quality, void* grad_logits, mxdet_stream_t stream);
/* The fused level entry: the arguments of mxdet_retina_loss_level_quality without the stds, with reg_max, stride and
 * dfl_weight; cls_kind also accepts MXDET_CLS_LOSS_FOCAL (alpha, gamma: the focal loss's). reg / grad_reg rows hold
 * ld_reg >= 4 (R + 1) A elements. Grid: mxdet_retina_loss_num_partials workgroups of 256 anchors; partial holds THREE words
 * per workgroup (class, box, DFL): finalize with ncomp = 3. grad_reg: every real channel of every anchor of the level is
 * written (zeros where nothing regresses), padding channels are untouched. For equal logits, labels and quality, grad_cls
 * and the class partial are bit-identical to the _quality (focal: _iou) entry. Vector / scalar split: the condition of
 * mxdet_retina_loss_level. No atomics, no host synchronisation, nothing allocated, capturable; a replay follows new
 * gt_boxes. */
int mxdet_retina_loss_level_dfl(const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W, int32_t A,
                                int32_t C, int32_t ld_cls, int32_t ld_reg, const int32_t* cls_labels, const float* anchors,
                                const int32_t* matched_gt, const float* gt_boxes, int32_t G_max, int64_t A_total,
                                int64_t level_offset, int32_t cls_kind, float alpha, float gamma, int32_t kind,
                                int32_t reg_max, float stride, float reg_weight, float dfl_weight, const int32_t* num_fg,
                                float loss_scale, uint16_t* grad_cls, uint16_t* grad_reg, float* partial,
                                mxdet_stream_t stream);

/* Gradient harmonizing for the RetinaNet head (GHM-C / GHM-R; Li et al., AAAI 2019): every element of the
 * dense head is weighted by the inverse density of its gradient norm, counted over ALL levels and images of the step.
 * Valid sets. Class elements: every (anchor, class c) with cls_labels >= 0; target t = 1 if cls_labels == c + 1, else 0;
 *   padding columns of ld_cls are no elements. Box elements: the four deltas of every anchor with cls_labels > 0 against
 *   the bbox_targets of mxdet_retina_loss_level (encoded deltas).
 * Gradient norm. Class: g = |sigmoid(x) - t|. Box: d = delta - target, g = |d| / sqrt(d*d + mu*mu), mu > 0. g is a
 *   constant of the loss: no gradient flows through the weights.
 * Bin. For B bins, bin(g) = min(B - 1, (int)(g * (float)B)): unit-region edges k / B, g == 1 in the last bin. One device
 *   function (csrc/loss_elem.h) and one g expression serve both passes, so no element changes bin between them.
 * Per step, per histogram (one for class, one for box; per rank, no all-reduce):
 *   cnt[i] = number of valid elements in bin i (int32).
 *   acc[i] (float32 device state, starts at 0): for cnt[i] > 0, acc[i] = momentum * acc[i] + (1 - momentum) * cnt[i] if
 *     momentum > 0, else acc[i] = cnt[i]; bins with cnt[i] == 0 keep their acc and are not counted.
 *   n = number of bins with cnt[i] > 0; coef[i] = 1 / (n * acc[i]) for those bins, 0 for the others.
 *   Class loss  = cls_weight * sum coef_c[bin(g)] * BCE(x, t) (the sigmoid_softplus log forms of the focal loss);
 *     dL/dx = cls_weight * coef * (s - t).
 *   Box loss    = reg_weight * sum coef_r[bin(g)] * (sqrt(d*d + mu*mu) - mu);
 *     dL/d delta = reg_weight * coef * d / sqrt(d*d + mu*mu).
 *   *num_fg does not enter a harmonized term; loss_scale scales gradients as in the entries above. A step without a valid
 *   element has cnt == 0 everywhere: loss 0, gradients 0, acc untouched, no NaN or Inf.
 * Published settings: class 30 bins, momentum 0.75, weight 1; box 10 bins, momentum 0.7, weight 10, mu 0.02.
 * Limits: 1 <= bins <= MXDET_GHM_MAX_BINS, 0 <= momentum < 1, mu > 0, weights > 0; anything else is MXDET_EINVAL.
 * flags: which halves are harmonized; a row of the count table, acc, cnt and coef hold bins_c class words, then bins_r box
 * words, whatever the flags (a half left out counts 0, so its coef is 0 and its acc is untouched). */
#define MXDET_GHM_CLS 1
#define MXDET_GHM_REG 2
#define MXDET_GHM_MAX_BINS 64
/* Histogram pass of one level: the grid and anchor-to-workgroup map of mxdet_retina_loss_level
 * (mxdet_retina_loss_num_partials workgroups of 256 anchors, the 16-byte class walk under the same condition on cls / reg).
 * Workgroup i writes row i of counts ([blocks][bins_c + bins_r] int32): the caller lays the levels' rows back to back, as
 * it does with `partial`. Every row is written whole: nothing has to be zeroed between steps. Integer LDS atomics
 * (per-wave histograms; lanes that agree on a bin add once): counts do not depend on order. bbox_targets 16-byte aligned. */
int mxdet_ghm_hist_level(const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W, int32_t A, int32_t C,
                         int32_t ld_cls, int32_t ld_reg, const int32_t* cls_labels, const float* bbox_targets,
                         int64_t A_total, int64_t level_offset, int32_t flags, int32_t bins_c, int32_t bins_r, float mu,
                         int32_t* counts, mxdet_stream_t stream);
/* The step's weights, one workgroup: cnt = column sums of the `rows` rows of counts (fixed order), acc updated in place,
 * coef written; all three [bins_c + bins_r]. The only entry that writes acc. */
int mxdet_ghm_weights(const int32_t* counts, int32_t rows, int32_t bins_c, int32_t bins_r, float momentum_c,
                      float momentum_r, float* acc, int32_t* cnt, float* coef, mxdet_stream_t stream);
/* Loss pass of one level: mxdet_retina_loss_level with the class term (MXDET_GHM_CLS) and / or the box term
 * (MXDET_GHM_REG) harmonized by coef. Same grid, two-word partial layout, vector / scalar split and finalize (ncomp = 2).
 * The half that flags leaves out is the focal (alpha, gamma) or smooth-L1 (sigma) half of mxdet_retina_loss_level: its
 * partial word and gradient are bit-identical to that entry's. coef is read into LDS once per workgroup. No float atomics,
 * no host synchronisation, nothing allocated, capturable; a replay follows new gt_boxes. */
int mxdet_retina_loss_level_ghm(const uint16_t* cls, const uint16_t* reg, int32_t N, int32_t H, int32_t W, int32_t A,
                                int32_t C, int32_t ld_cls, int32_t ld_reg, const int32_t* cls_labels,
                                const float* bbox_targets, int64_t A_total, int64_t level_offset, int32_t flags, float alpha,
                                float gamma, float sigma, const float* coef, int32_t bins_c, int32_t bins_r,
                                float cls_weight, float mu, float reg_weight, const int32_t* num_fg, float loss_scale,
                                uint16_t* grad_cls, uint16_t* grad_reg, float* partial, mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * core/mask + mask_heads (README.md:18, :30) -- Mask R-CNN.
 * mask targets: for roi r (batch, box) with matched GT g = matched_gt[r] and class labels[r] > 0, resample the
 * instance bitmask gt_masks[batch, g] ([N,G_max,H,W] u8, 0/1) inside the box to S x S (bilinear at bin centres,
 * RoIAlign aligned=False tap rules) and threshold at 0.5. cls_out[r] = class (1..) or -1 for non-foreground rois. */
int mxdet_mask_target(const float* rois, const int32_t* matched_gt, const int32_t* labels,
                      const uint8_t* gt_masks, int64_t R, int32_t G_max, int32_t H, int32_t W, int32_t S,
                      uint8_t* targets, int32_t* cls_out, mxdet_stream_t stream);
/* x [R,H,W,4*C] (channel = (dy*2+dx)*C + c) -> y [R,2H,2W,C] (inverse = 0) or back (inverse = 1): with a 1x1
 * conv C_in -> 4*C this is Deconvolution(kernel=2, stride=2). */
int mxdet_pixel_shuffle2(const uint16_t* x, int64_t R, int32_t H, int32_t W, int32_t C, int32_t inverse,
                         uint16_t* y, mxdet_stream_t stream);
/* backward of conv1x1 -> ReLU -> pixel shuffle in one pass: dx[r,h,w,(dy*2+dx)*C+c] = dy_up[r,2h+dy,2w+dx,c] where the
 * packed activation act (same layout as dx, [R,H,W,4*C]) is > 0, else 0 */
int mxdet_pixel_shuffle2_inv_relu(const uint16_t* dy_up, const uint16_t* act, int64_t R, int32_t H, int32_t W, int32_t C,
                                  uint16_t* dx, mxdet_stream_t stream);
/* per-pixel sigmoid BCE on channel cls[r]-1 of logits [R,S,S,Cpad] (bf16), normalised by (#fg rois * S*S);
 * grad (bf16, same shape) is fully written; loss_out[1] fp32, fixed-order reduction. */
size_t mxdet_mask_loss_workspace_bytes(int64_t R, int32_t S);
int mxdet_mask_loss(const uint16_t* logits, const int32_t* cls, const uint8_t* targets, int64_t R, int32_t S,
                    int32_t Cpad, float loss_scale, float* loss_out, uint16_t* grad, void* workspace,
                    size_t workspace_bytes, mxdet_stream_t stream);
/* Inference paste-back (MXNet-lineage role: sigmoid -> cv2.resize(mask, (w, h)) -> > 0.5 -> place at the box, on the
 * host). dets [R,6] = (x1,y1,x2,y2,score,class) in the frame of the OUTPUT masks; logits [R,S,S,Cpad] bf16.
 * prob = sigmoid(logit of channel class-1); box corners rounded half-even to integers, w = x2-x1+1, h = y2-y1+1;
 * pixel (x,y) inside the box samples prob bilinearly at ((x-x1+0.5)*S/w-0.5, (y-y1+0.5)*S/h-0.5) (clamped, fp32,
 * unfused: top/bottom rows first, then vertical) and is 1 where the value > thresh. masks [R,H,W] u8, W % 4 == 0;
 * rows with class <= 0 are all zero. */
size_t mxdet_mask_paste_workspace_bytes(int64_t R, int32_t S);
int mxdet_mask_paste(const uint16_t* logits, const float* dets, int64_t R, int32_t S, int32_t Cpad, int32_t H, int32_t W,
                     float thresh, uint8_t* masks, void* workspace, size_t workspace_bytes, mxdet_stream_t stream);
/* Mask Scoring R-CNN (Huang et al., CVPR 2019): a MaskIoU head regresses the IoU between the predicted
 * mask and its ground truth; the test-time mask score is the box score times that IoU. All fp32 arithmetic below is
 * unfused, one IEEE operation per product / quotient / sum in the order written.
 *
 * MaskIoU target, out fp32 [R]. rois [R,5], matched_gt / cls [R] as mxdet_mask_target takes / writes them, gt_boxes
 * [N,G_boxes,5] (class < 0: padding; G_boxes >= G, rows past G unused), gt_masks [N,G,H,W] u8, logits bf16 [R,S,S,Cpad], targets u8 [R,S,S]. Rows with
 * cls <= 0 (or > Cpad), matched_gt outside [0,G) or an image index outside [0,N) give 0 and read no mask memory. Else,
 * with n = (int)rois[r,0], g = matched_gt[r]:
 *   a_full = set pixels of gt_masks[n,g] (0 for a padding instance: those are never read);
 *   ix1 = max(0, floor(x1)), iy1 = max(0, floor(y1)), ix2 = min(W-1, ceil(x2)), iy2 = min(H-1, ceil(y2));
 *   a_in = set pixels with ix1 <= x <= ix2, iy1 <= y <= iy2 (0 for an empty clipped box);
 *   over the S x S map: pred = logit of channel cls-1 > 0; a_pred = sum pred, a_tgt = sum targets, a_ovr = sum pred & targets;
 *   a_in == 0: 0; else gt_s = ((float)a_tgt * (float)a_full) / (float)a_in, uni = ((float)a_pred + gt_s) - (float)a_ovr,
 *   out = (float)a_ovr / fmaxf(uni, 1e-7f).
 * The counts are integers, so the result does not depend on the order of summation. N*G <= 65535. */
size_t mxdet_maskiou_target_workspace_bytes(int32_t N, int32_t G);
int mxdet_maskiou_target(const float* rois, const int32_t* matched_gt, const int32_t* cls, const float* gt_boxes,
                         const uint8_t* gt_masks, const uint16_t* logits, const uint8_t* targets, int64_t R, int32_t N,
                         int32_t G, int32_t G_boxes, int32_t H, int32_t W, int32_t S, int32_t Cpad, float* out,
                         void* workspace, size_t workspace_bytes, mxdet_stream_t stream);
/* MaskIoU head input, out bf16 [R,S/2,S/2,Ctot] (Ctot % 8 == 0, Ctot > C, C % 8 == 0; every channel is written):
 * channels [0,C) = mpooled [R,S/2,S/2,C]; channel C = bf16(sigmoid(z)), z = the max of the four logits
 * [2y..2y+1, 2x..2x+1] of channel cls[r]-1 (sigmoid(z) = z >= 0 ? 1/(1+e^-z) : e^z/(1+e^z) with mxdet_expf), 0 for rows
 * with cls <= 0 or > Cpad; channels (C,Ctot) = 0. */
int mxdet_maskiou_input(const uint16_t* mpooled, const uint16_t* logits, const int32_t* cls, int64_t R, int32_t S,
                        int32_t C, int32_t Cpad, int32_t Ctot, uint16_t* out, mxdet_stream_t stream);
/* Its adjoint for the feature part (the mask channel is a constant): d_mpooled[p,c] = bf16((float)d_mpooled[p,c] +
 * (float)d_in[p,c]) for c < C over `pixels` rows of d_in [pixels,Ctot] / d_mpooled [pixels,C]; channels >= C are not read. */
int mxdet_maskiou_input_bwd(const uint16_t* d_in, int64_t pixels, int32_t C, int32_t Ctot, uint16_t* d_mpooled,
                            mxdet_stream_t stream);
/* L2 MaskIoU loss. pred / grad bf16 [R,ld] (ld % 8 == 0), cls [R], targets fp32 [R] (mxdet_maskiou_target).
 * pos = {r: 0 < cls[r] <= ld and targets[r] > 0}, n_pos counted on the device, k = (loss_scale * weight) / (float)max(n_pos,1);
 * loss_out[0] = k * sum_pos 0.5 * (d*d), d = (float)pred[r,cls-1] - targets[r] (fp32, fixed order: one workgroup);
 * grad[r,cls-1] = bf16(d * k) for r in pos, every other entry of grad is written as zero. */
int mxdet_maskiou_loss(const uint16_t* pred, const int32_t* cls, const float* targets, int64_t R, int32_t ld,
                       float loss_scale, float weight, float* loss_out, uint16_t* grad, mxdet_stream_t stream);
/* Test time: scores[r] = dets[r,4] * (float)pred[r, class-1] (one fp32 product) with class = (int)dets[r,5]; rows with
 * class <= 0 (padding) or > ld give 0. dets [R,6] as mxdet_mask_paste takes them, pred bf16 [R,ld]. */
int mxdet_maskiou_score(const float* dets, const uint16_t* pred, int64_t R, int32_t ld, float* scores,
                        mxdet_stream_t stream);

/* Keypoint R-CNN (He et al., ICCV 2017, section 5). logits bf16 [R,S_in,S_in,Kpad] (Kpad % 8 == 0, channels
 * [K,Kpad) are padding). The map the loss and the decode see is the fixed x2 bilinear upsample U [S,S], S = 2*S_in, of a
 * channel (half-pixel centres, edge replication, horizontal first; each product and sum one unfused fp32 operation):
 *   h[i][2j+p] = 0.75f*in[i][j] + 0.25f*in[i][clamp(j-1+2p, 0, S_in-1)],  U[2i+q][X] = 0.75f*h[i][X] + 0.25f*h[clamp(i-1+2q)][X].
 * It is formed in LDS / registers and never stored.
 *
 * Target, int32 [R,K] (-1 = not trained). rois [R,5] (batch index, x1,y1,x2,y2), matched_gt / labels [R], gt_keypoints fp32
 * [N,G,K,3] = (x, y, v) in the frame of the network input, v > 0 = labelled. Rows with labels <= 0, matched_gt outside
 * [0,G) or (int)rois[r,0] outside [0,N) give -1 and read no keypoint memory. Else, with rw = fmaxf(x2-x1, 1.0f):
 *   bx = (kx == x2) ? S-1 : (int)floorf((kx - x1) * ((float)S / rw)), by alike in y;
 *   target = by*S + bx when v > 0, 0 <= bx < S and 0 <= by < S, else -1. */
int mxdet_keypoint_target(const float* rois, const int32_t* matched_gt, const int32_t* labels, const float* gt_keypoints,
                          int64_t R, int32_t N, int32_t G, int32_t K, int32_t S_in, int32_t* targets, mxdet_stream_t stream);
/* Heatmap loss. targets int32 [R,K] as above (values outside [0,S*S) count as -1). n_valid = number of valid targets,
 * counted on the device; k = (loss_scale * weight) / (float)max(n_valid, 1);
 *   loss_out[0] = k * sum over valid (r,j) of log(sum_i exp(U_i - max U)) - (U_target - max U)   (mxdet_expf / mxdet_logf;
 *   fp32, fixed order: per roi over ascending channels, then over ascending rois);
 *   grad bf16 [R,S_in,S_in,Kpad], fully written: ((softmax(U) - onehot) * k) through the adjoint of the upsample in gather
 *   form -- d_in[i][j] = sum_t w_t * (sum_s w_s * Q[clamp(2i-1+s, 0, S-1)][clamp(2j-1+t, 0, S-1)]), w = (.25,.75,.75,.25),
 *   s and t ascending --, zeros for invalid (r,j) and channels >= K.
 * No atomics: bit-identical from run to run. One workgroup per roi holds the roi's block in LDS: S_in <= 32 and
 * 16*S_in^2 + 2*K*S_in^2 + 12*K + 160 <= 65536 bytes (MXDET_ESHAPE otherwise). R = 0 writes loss_out[0] = 0. */
size_t mxdet_keypoint_loss_workspace_bytes(int64_t R);
int mxdet_keypoint_loss(const uint16_t* logits, const int32_t* targets, int64_t R, int32_t S_in, int32_t Kpad, int32_t K,
                        float loss_scale, float weight, float* loss_out, uint16_t* grad, void* workspace,
                        size_t workspace_bytes, mxdet_stream_t stream);
/* Test time, out fp32 [R,K,3] = (x, y, score). dets [R,6] = (x1,y1,x2,y2,score,class) in the frame the keypoints are wanted
 * in. Per channel j < K: the argmax of U (ties: the lowest linear index) = (by, bx);
 *   x = x1 + ((float)bx + 0.5f) * (rw / (float)S), y alike, score = the maximal value of U.
 * Rows with (int)class <= 0 (padding) give zeros and read no logits. 2*K*S_in^2 <= 65536 bytes of LDS. */
int mxdet_keypoint_decode(const uint16_t* logits, const float* dets, int64_t R, int32_t S_in, int32_t Kpad, int32_t K,
                          float* out, mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * backbones / necks / rpn_heads / bbox_heads / mask_heads (README.md:27-31) -- dense contractions.
 * MXNet roles: Convolution (+ BatchNorm(use_global_stats) + Activation + elemwise_add),
 * FullyConnected, Pooling, UpSampling. All bf16 in / fp32 accumulate on MFMA / bf16 out.
 *
 * conv2d: x bf16 [N,H,W,Cin] channels-last, w bf16 [Cout,KH,KW,Cin], y bf16 [N,Ho,Wo,Cout].
 * Epilogue: y = act( conv + bias[c] + residual ), residual optional, of shape y or -- with
 * res_upsample = 1 -- [N,ceil(Ho/2),ceil(Wo/2),Cout] read nearest-neighbour (FPN top-down add).
 * A fully-connected layer is the 1x1 case with H = W = 1 and N = rows. */
typedef struct {
  int32_t N, H, W, Cin;      /* input  */
  int32_t Cout, KH, KW;      /* filter */
  int32_t stride, pad;       /* same in both dims */
  int32_t Ho, Wo;            /* output; must equal floor((H + 2*pad - KH)/stride) + 1 etc. */
  int32_t relu;              /* fwd: apply ReLU;   dgrad: multiply by (mask > 0) */
  int32_t res_upsample;      /* fwd only */
  int32_t accumulate;        /* dgrad / wgrad: add into the output instead of overwriting */
  /* Optional hint (fwd / dgrad, single launches): device memory the caller will read NEXT -- the filter of the layer
   * that follows -- or null. Every workgroup reads a slice of it (up to 16 KiB) while its epilogue runs, so the bytes
   * sit in the Infinity Cache when the next launch starts: a layer's filter was last touched a whole step earlier and
   * its first touch otherwise costs an HBM round trip in front of every workgroup's K loop (measured: a C5 3x3 layer
   * 32.7 us with a cold filter, 24.0 us with a warm one). The contents are never used. */
  const void* prefetch;
  int64_t prefetch_bytes;
  /* Optional 1-bit ReLU mask, byte [pixel][channel / 8], bit k = (value of channel 8 j + k) > 0 (the channel count must
   * be a multiple of 8). fwd: if non-null the kernel ALSO writes the mask of the values it stores (the activation's
   * ReLU mask for the backward pass, 1/16 of its bytes). dgrad with relu = 1: if non-null it is read INSTEAD of the
   * 16-bit relu_mask operand (which may then be null) -- same result, 1/16 of the operand traffic: the expand-layer
   * data gradients are HBM-bound and their mask is a forward activation that is cold in every cache. */
  void* relu_bits;
} mxdet_conv_desc_t;

int mxdet_conv2d_fwd(const mxdet_conv_desc_t* d, const uint16_t* x, const uint16_t* w,
                     const float* bias, const uint16_t* residual, uint16_t* y,
                     mxdet_stream_t stream);
/* Chained forward: y2 = act2( act( conv3x3(x, w) + bias ) (*) w2 + bias2 + residual2 ), act = ReLU if d->relu, act2 = ReLU if
 * relu2 -- the tail of a bottleneck block (conv2 -> conv3 + shortcut) whose intermediate map nobody needs afterwards, i.e.
 * a FROZEN block (models/backbones, /root/reference/README.md:27: ResNet stage C2 with frozen_stages = 1). d describes the
 * 3x3 (stride 1, pad 1, Cin % 64 == 0, Cout == 64); w2 is [cout2][1][1][64] with cout2 == 256; residual2 / y2 are
 * [N, Ho, Wo, cout2]. One launch, the 64-channel intermediate never reaches memory; bit-identical to mxdet_conv2d_fwd
 * twice. d->prefetch is honoured; d->relu_bits and d->res_upsample must be unset.
 * w3 != NULL adds a third convolution in the same launch: y3 = act3( y2 (*) w3 + bias3 ), w3 [cout3][1][1][cout2] with
 * cout3 == 64, y3 [N, Ho, Wo, cout3] -- the NEXT block's conv1, computed from the block output's stored bf16 values as
 * they leave the workgroup (bit-identical to a further mxdet_conv2d_fwd on y2). */
int mxdet_conv2d_fwd_chain(const mxdet_conv_desc_t* d, const uint16_t* x, const uint16_t* w, const float* bias,
                           const uint16_t* w2, const float* bias2, int32_t cout2, int32_t relu2,
                           const uint16_t* residual2, uint16_t* y2, const uint16_t* w3, const float* bias3,
                           int32_t cout3, int32_t relu3, uint16_t* y3, mxdet_stream_t stream);
/* Forward with the reduction split over `ksplit` ranges of 64-channel slices, for 1x1 / stride-1 layers with a long
 * reduction on few rows (fully connected layers on pooled rois): raw fp32 tiles in the caller's workspace, folded in
 * split order (deterministic) with bias / residual / ReLU by a second kernel. Last-bit different from mxdet_conv2d_fwd
 * (another summation order); ksplit = 1 is that call. */
size_t mxdet_conv2d_fwd_splitk_workspace_bytes(const mxdet_conv_desc_t* d, int32_t ksplit);
int mxdet_conv2d_fwd_splitk(const mxdet_conv_desc_t* d, const uint16_t* x, const uint16_t* w, const float* bias,
                            const uint16_t* residual, uint16_t* y, int32_t ksplit, void* workspace,
                            size_t workspace_bytes, mxdet_stream_t stream);
/* dgrad: dx[N,H,W,Cin] = (sum over taps dy[N,Ho,Wo,Cout] * w  +  residual) * (relu_mask > 0), with
 * wt = the same filter stored [Cin,KH,KW,Cout] (mxdet_filter_transpose). residual (bf16, shape of dx;
 * may be NULL) is the gradient arriving over a parallel branch (identity shortcut / sibling conv);
 * d->accumulate with residual == NULL means residual = dx. The mask factor applies only if d->relu:
 * relu_mask is then the forward activation x (bf16, post-ReLU). */
int mxdet_conv2d_dgrad(const mxdet_conv_desc_t* d, const uint16_t* dy, const uint16_t* wt,
                       const uint16_t* residual, const uint16_t* relu_mask, uint16_t* dx,
                       mxdet_stream_t stream);
/* wgrad: dw fp32 [Cout,KH,KW,Cin] (+)= sum over pixels dy * x; deterministic split-K through
 * workspace slabs reduced in fixed order; db fp32 [Cout] (may be NULL) (+)= sum over pixels dy. */
size_t mxdet_conv2d_wgrad_workspace_bytes(const mxdet_conv_desc_t* d);
int mxdet_conv2d_wgrad(const mxdet_conv_desc_t* d, const uint16_t* x, const uint16_t* dy, float* dw,
                       float* db, void* workspace, size_t workspace_bytes, mxdet_stream_t stream);
/* Grouped convolutions: independent forward convolutions (kind 0) or stride-1 data gradients (kind 1) that can share
 * one tile configuration -- the 3x3 of every pyramid level of an RPN / RetinaNet head, the FPN output convs -- as ONE
 * grid: the small levels ride in the shadow of the large ones instead of running latency-bound on their own.
 * Same protocol as the grouped weight gradients: _plan writes a host table (+ tile configuration and grid size), the
 * caller uploads it once, mxdet_conv2d_grouped launches it. Per item the semantics are exactly those of
 * mxdet_conv2d_fwd (src = x, filt = w, dst = y; bias / residual / desc.relu / desc.res_upsample) or
 * mxdet_conv2d_dgrad (src = dy, filt = wt, dst = dx; residual / relu_mask / desc.accumulate). */
typedef struct {
  mxdet_conv_desc_t desc;
  const void* src;
  const void* filt;
  const float* bias;
  const void* residual;
  const void* relu_mask;
  void* dst;
} mxdet_conv_item_t;
size_t mxdet_conv2d_grouped_table_bytes(int32_t n);
int mxdet_conv2d_grouped_plan(const mxdet_conv_item_t* items, int32_t n, int32_t kind, void* table_host,
                              size_t table_bytes, int32_t* cfg, int32_t* grid);
int mxdet_conv2d_grouped(const void* table_dev, int32_t n, int32_t kind, int32_t cfg, int32_t grid,
                         mxdet_stream_t stream);
/* Grouped weight gradients: the wgrads of many layers (a ResNet stage, the FPN, a head) in ONE launch pair (MFMA
 * workgroups of all layers in one grid + one fold launch). At batch 2 a layer's own grid is one or two workgroups per
 * CU; a group runs at the occupancy of the largest layers, needs less split-K and two launches instead of 2 per layer.
 * Usage: fill items[] (descriptor + device pointers, accumulate honoured per item), call _plan once per group -- it
 * writes a table of mxdet_conv2d_wgrad_grouped_table_bytes(n) bytes to HOST memory and reports the workspace size and
 * the two grid sizes --, copy the table to device memory (it stays valid while the pointers do, e.g. across hipGraph
 * replays), then launch with mxdet_conv2d_wgrad_grouped. Results equal mxdet_conv2d_wgrad's up to the split-K
 * partition (fp32 sums in a different, still fixed, order). */
typedef struct {
  mxdet_conv_desc_t desc;
  const void* x;    /* bf16 [N,H,W,Cin] */
  const void* dy;   /* bf16 [N,Ho,Wo,Cout] */
  float* dw;        /* f32 [Cout,KH,KW,Cin] */
  float* db;        /* f32 [Cout] or NULL */
} mxdet_wgrad_item_t;
size_t mxdet_conv2d_wgrad_grouped_table_bytes(int32_t n);
int mxdet_conv2d_wgrad_grouped_plan(const mxdet_wgrad_item_t* items, int32_t n, void* table_host, size_t table_bytes,
                                    size_t* workspace_bytes, int32_t* grid_wgrad, int32_t* grid_big,
                                    int32_t* grid_reduce);
int mxdet_conv2d_wgrad_grouped(const void* table_dev, int32_t n, int32_t grid_wgrad, int32_t grid_big,
                               int32_t grid_reduce, void* workspace, size_t workspace_bytes, size_t workspace_needed,
                               mxdet_stream_t stream);
/* The same launch in parts (bit 0: the three-tap kernel of the 3x3 / stride 1 items, grid_big workgroups; bit 1: the
 * one-tap kernel + bias workgroups, grid_wgrad; bit 2: the fold). The two tile kernels are independent of each other
 * (the 3x3 tiles are MFMA-bound, the 1x1 tiles HBM-bound: a caller may issue them on two streams); the fold needs both. */
int mxdet_conv2d_wgrad_grouped_parts(const void* table_dev, int32_t n, int32_t grid_wgrad, int32_t grid_big,
                                     int32_t grid_reduce, int32_t parts, void* workspace, size_t workspace_bytes,
                                     size_t workspace_needed, mxdet_stream_t stream);
/* w [Cout,KH,KW,Cin] -> wt [Cin,KH,KW,Cout] (bf16) */
int mxdet_filter_transpose(const uint16_t* w, int32_t Cout, int32_t KH, int32_t KW, int32_t Cin,
                           uint16_t* wt, mxdet_stream_t stream);

/* All filters of a model in one launch. descs_dev: device array of ndesc records
 * { const uint16_t* w; uint16_t* wt; int32 Cout, taps, Cin, tile0; } (32 bytes each) where tile0 is the running
 * sum of ceil(Cin/64)*ceil(Cout/64)*taps over the preceding records, total_tiles the overall sum. */
int mxdet_filter_transpose_batched(const void* descs_dev, int32_t ndesc, int32_t total_tiles,
                                   mxdet_stream_t stream);

/* Sparse backward of the RPN head (3x3 conv C -> C + ReLU, fused 1x1 C -> Ch): the RPN loss leaves at most
 * smax = N * batch_size cells with a non-zero gradient row, and only those are multiplied. Pyramid of num_levels levels,
 * level l being [N, H[l], W[l], *] channels-last tensors; the global id of cell (n, l, h, w) is
 *   n * CT + coff[l] + h * W[l] + w,  coff[l] = sum of H*W over the levels before l, CT = coff[num_levels]
 * (the anchor index of mxdet_anchor_target divided by A). C % 64 == 0, Ch == 64, smax <= 8192.
 *
 * mxdet_rpn_sparse_list: a cell is active if one of its A labels (labels [N, CT*A] i32) is >= 0. Writes
 *   list [2*smax] i32: the active cell ids in ascending order in [0, S), -1 in [S, smax) (the upper half is scratch);
 *   state [2] i32: state[0] = S (active cells past smax are dropped: the sampler never produces them);
 *   map [N*CT] i32: the slot of every active cell, -1 elsewhere (rewritten in full by every call).
 * mxdet_rpn_sparse_backward runs the parts named in `parts`, in this order, S read from state on the device:
 *   ZERO   every level with accumulate[l] == 0 is cleared;
 *   DT     dts [smax, C] bf16: row s = the 1x1 data gradient of gh's row of cell list[s] (wt_out [C, Ch], the transposed
 *          filter), masked by the cell's ReLU bits (tbits[l] u8 [N,H,W,C/8], or t[l] > 0 where tbits[l] is NULL); ghs
 *          [smax, Ch] = those gh rows; rows past S are zero. The bits are those of mxdet_conv2d_dgrad.
 *   DTMAP  (with DT) the dense maps dt[l] [N,H,W,C] are cleared and the listed rows written into them as well: the
 *          operand of the dense weight gradient (mxdet_conv2d_wgrad*), bit for bit what mxdet_conv2d_dgrad writes.
 *   WGRAD  dw_out [Ch,1,1,C], db_out [Ch], dw_conv [C,3,3,C], db_conv [C] (f32, overwritten): sums over the slots in slot
 *          order, 32 per MFMA step; needs DT's outputs.
 *   DGRAD  the 3x3 / stride 1 / pad 1 data gradient (wt_conv [C,3,3,C] transposed filter) of dts scattered to its cells,
 *          written to (accumulate[l]: added to) the pixels of dP[l] that have an active cell in their 3x3 neighbourhood,
 *          each once, with the bits mxdet_conv2d_dgrad gives them; other pixels are not touched.
 *   WGRAD_ORDERED  the four weight / bias gradients of WGRAD (f32, overwritten) with the BITS of the dense grouped weight
 *          gradient (mxdet_conv2d_wgrad_grouped) on gh / the DTMAP maps: only the 32-pixel MFMA half-steps that hold an
 *          active cell are issued, in the dense order, every active pixel at its dense reduction position, a fresh
 *          accumulator per dense split-K slab and the slab sums added in the dense fold order. Needs DT's outputs,
 *          `ordered` = the schedule mxdet_rpn_ordered_schedule wrote for this pyramid (host memory, 2 * num_levels
 *          records: rpn.out's levels, then rpn.conv's) and `ordered_work` (device, 16-byte aligned, at least
 *          MXDET_RPN_ORDERED_WORK_INTS(smax) i32). One prepass launch re-keys the list into the dense order, one launch
 *          does the rest; an Inf / NaN of P or t beside a zero gradient row is NOT propagated (the dense kernels give NaN). */
#define MXDET_RPN_SPARSE_MAX_LEVELS 8
#define MXDET_RPN_SPARSE_ZERO 1
#define MXDET_RPN_SPARSE_DT 2
#define MXDET_RPN_SPARSE_WGRAD 4
#define MXDET_RPN_SPARSE_DGRAD 8
#define MXDET_RPN_SPARSE_DTMAP 16
#define MXDET_RPN_SPARSE_WGRAD_ORDERED 32
#define MXDET_RPN_ORDERED_WORK_INTS(smax) (10 * (smax) + 32)
/* The dense split-K order of one item (one level of one filter) of a grouped weight-gradient plan. The kernels read kind,
 * H, W, halves_per_slab and bias_pixels and add the slabs in ITEM order; slab0, fold_ksplit and bias_splits record where the
 * plan put the item's slabs in its filter's run: the launch only checks that they follow the item order (slab0 ascending
 * from 0, below fold_ksplit), which mxdet_rpn_ordered_schedule guarantees for the plans it accepts. */
typedef struct {
  int32_t kind;          /* 0: one-tap tile, reduction over the real pixels (n*H + h)*W + w; 1: three-tap tile, over
                            the virtual pixels (n*H + h)*(W + 1) + w */
  int32_t H, W;
  int32_t halves_per_slab;   /* 32-pixel MFMA half-steps per split (slab) */
  int32_t slab0;         /* the item's first slab in its filter's run of slabs */
  int32_t fold_ksplit;   /* slabs in the run (the fold adds them in index order) */
  int32_t bias_pixels;   /* real pixels per split of the bias sums; split ks is slab slab0 + ks of the bias run */
  int32_t bias_splits;
} mxdet_rpn_ordered_item_t;
typedef struct {
  int32_t num_levels, N, A, C, Ch, smax;
  int32_t H[MXDET_RPN_SPARSE_MAX_LEVELS], W[MXDET_RPN_SPARSE_MAX_LEVELS];
  int32_t accumulate[MXDET_RPN_SPARSE_MAX_LEVELS];
  const void* P[MXDET_RPN_SPARSE_MAX_LEVELS];      /* bf16 [N,H,W,C]: the head's input */
  const void* t[MXDET_RPN_SPARSE_MAX_LEVELS];      /* bf16 [N,H,W,C]: relu(conv(P)) */
  const void* tbits[MXDET_RPN_SPARSE_MAX_LEVELS];  /* u8 [N,H,W,C/8] or NULL */
  const void* gh[MXDET_RPN_SPARSE_MAX_LEVELS];     /* bf16 [N,H,W,Ch]: d(loss)/d(head output) */
  void* dP[MXDET_RPN_SPARSE_MAX_LEVELS];           /* bf16 [N,H,W,C] */
  void* dt[MXDET_RPN_SPARSE_MAX_LEVELS];           /* bf16 [N,H,W,C] or NULL (DTMAP) */
  const mxdet_rpn_ordered_item_t* ordered;         /* host, [2 * num_levels] or NULL (WGRAD_ORDERED) */
  void* ordered_work;                              /* device i32 scratch or NULL (WGRAD_ORDERED) */
} mxdet_rpn_sparse_t;
int mxdet_rpn_sparse_list(const mxdet_rpn_sparse_t* d, const int32_t* labels, int32_t* list, int32_t* state,
                          int32_t* map, mxdet_stream_t stream);
int mxdet_rpn_sparse_backward(const mxdet_rpn_sparse_t* d, const int32_t* list, const int32_t* state,
                              const int32_t* map, const uint16_t* wt_out, const uint16_t* wt_conv, uint16_t* dts,
                              uint16_t* ghs, float* dw_out, float* db_out, float* dw_conv, float* db_conv,
                              int32_t parts, mxdet_stream_t stream);
/* The schedule of WGRAD_ORDERED from the HOST table mxdet_conv2d_wgrad_grouped_plan wrote for the head's 2 * num_levels
 * items (rpn.out on (t[l], gh[l]) for every level, then rpn.conv on (P[l], dt[l]); no accumulate): the split parameters
 * are read off that plan, never derived a second time. MXDET_EINVAL when the items are not two filters of num_levels
 * levels each whose slabs follow the item order. */
int mxdet_rpn_ordered_schedule(const void* table_host, int32_t n, int32_t num_levels, mxdet_rpn_ordered_item_t* items);

/* Deformable convolution (DCN v1 / v2), MXNet role contrib.DeformableConvolution (Deformable-ConvNets'
 * deformable_im2col semantics; dilation 1, 3x3 kernels only: anything else is MXDET_ESHAPE).
 * x bf16 [N,H,W,C]; off bf16 [N,Ho,Wo,off_channels] (off_channels % 8 == 0) with G = groups deformable groups:
 *   channel g*18 + 2k = dy, g*18 + 2k + 1 = dx of tap k = 3i + j; modulated (v2): channel 18G + 9g + k = the mask LOGIT;
 *   channels past 18G (v1) / 27G (v2) are padding: read never, written zero by col2im_coord.
 * Input channel c belongs to group g = c / (C/G) (C % (8G) == 0). Sample of output (n,ho,wo), tap (i,j), channel c at
 *   p_y = ho*stride - pad + i + dy,  p_x = wo*stride - pad + j + dx:
 *   0 if p_y <= -1, p_y >= H, p_x <= -1 or p_x >= W; else the bilinear mix of the four corners around
 *   (floor(p_y), floor(p_x)), corners outside [0,H) x [0,W) reading 0; v2 multiplies it by sigmoid(logit) (fused: the
 *   mask is never stored). Gradients w.r.t. p_y / p_x are those of that bilinear form with the floor held fixed
 *   (one-sided at integer positions, as in MXNet). floor(p) and p - floor(p) are those of the real number p: they are
 *   taken from the offset alone (the rest of p is an integer), not from a sum rounded in fp32.
 * col bf16 [N,Ho,Wo,9*C], tap-major then channel: the [Cout,3,3,C] filter seen as [Cout,1,1,9C], so forward, data
 * gradient and weight gradient are mxdet_conv2d_fwd / _dgrad / _wgrad as 1x1 convolutions on col. */
typedef struct {
  int32_t N, H, W, C;
  int32_t Ho, Wo;             /* must equal (H + 2*pad - 3)/stride + 1 etc. */
  int32_t KH, KW;             /* 3, 3 */
  int32_t stride, pad;
  int32_t groups;             /* deformable groups G */
  int32_t modulated;          /* 1: v2 (mask logits in off) */
  int32_t off_channels;       /* Coff */
  int32_t accumulate;         /* col2im: add into dx instead of overwriting */
} mxdet_deform_desc_t;
/* col[n,ho,wo,k*C + c] = sample (bf16, one rounding) */
int mxdet_deform_im2col(const mxdet_deform_desc_t* d, const uint16_t* x, const uint16_t* off, uint16_t* col,
                        mxdet_stream_t stream);
/* doff [N,Ho,Wo,off_channels] (fully written): per (pixel, tap, group) sum over the group's channels of
 * dcol * d(sample)/d(p) (and, v2, dcol * sample * sigma'(logit)), channels reduced in a fixed order; bf16. */
int mxdet_deform_col2im_coord(const mxdet_deform_desc_t* d, const uint16_t* x, const uint16_t* off,
                              const uint16_t* dcol, uint16_t* doff, mxdet_stream_t stream);
/* dx [N,H,W,C] (=, or += under accumulate) the adjoint of im2col applied to dcol, without float atomics: an inverted
 * index (input pixel -> (output pixel, tap, corner, weight) entries in ascending (pixel, tap, corner) order; it depends
 * on off only) and a gather that sums every pixel's entries in fp32 in that order, rounded to bf16 once -- bit-
 * reproducible run to run. Workspace: mxdet_deform_col2im_workspace_bytes(d) (0 for an invalid descriptor). */
size_t mxdet_deform_col2im_workspace_bytes(const mxdet_deform_desc_t* d);
int mxdet_deform_col2im(const mxdet_deform_desc_t* d, const uint16_t* off, const uint16_t* dcol, uint16_t* dx,
                        void* workspace, size_t workspace_bytes, mxdet_stream_t stream);

/* GroupNorm (+ fused ReLU) for the trainable heads (MXNet-lineage role: the GN of Detectron / mmdetection's 4conv1fc box
 * head and GN mask head). x, y, dy, dx: bf16 channels-last [N, HW, C] (16-byte aligned); G groups of C/G adjacent channels;
 * statistics per (sample, group) over m = HW * C/G elements, in fp32:
 *   mean = sum x / m;  var = sum (x - mean)^2 / m  (about the mean, biased);  rstd = 1 / sqrt(var + eps);
 *   y = act(gamma[c] * (x - mean) * rstd + beta[c]), act = ReLU if d->relu; mean, rstd fp32 [N, G] are written for bwd.
 * bwd, with xh = (x - mean) * rstd and g = dy (under d->relu: dy where y > 0, else 0; y is the forward output, or NULL
 * to have the mask recomputed from x, gamma and beta):
 *   dgamma[c] (+)= sum_{n,hw} g * xh;  dbeta[c] (+)= sum_{n,hw} g   (d->accumulate as on the other backward entries);
 *   dx = rstd * (g * gamma - (sum_group g * gamma + xh * sum_group g * gamma * xh) / m).
 * Shapes: C % G == 0, (C/G) % 8 == 0, C <= 1024, any HW >= 1, any N >= 1 (a sample under 2^30 elements: its offsets are
 * 32-bit); else MXDET_ESHAPE.
 * Two routes, chosen from (HW, C) alone (mxdet_debug_group_norm_route): a sample of at most 8 * floor(1024 / (C/8))
 * pixels is RESIDENT -- one workgroup per sample, x (bwd: x and dy) read once into registers, both statistics passes and
 * the store from that copy; a sample's results do not depend on N or on its index. Larger samples are TILED over
 * workgroups: per-chunk (count, mean, M2) in the workspace, merged in chunk order (Chan), then an apply kernel.
 * dgamma / dbeta: per-workgroup fp32 partials in the workspace, folded in a fixed order; no float atomics: every output
 * is bit-reproducible run to run. Workspace: mxdet_group_norm_workspace_bytes(d, backward) (0 for an invalid
 * descriptor; the resident forward needs none and accepts workspace == NULL). */
typedef struct {
  int32_t N, HW, C, G;
  float eps;
  int32_t relu;
  int32_t accumulate;        /* bwd: add into dgamma / dbeta instead of overwriting */
} mxdet_gn_desc_t;
size_t mxdet_group_norm_workspace_bytes(const mxdet_gn_desc_t* d, int32_t backward);
int mxdet_group_norm_fwd(const mxdet_gn_desc_t* d, const uint16_t* x, const float* gamma, const float* beta, uint16_t* y,
                         float* mean, float* rstd, void* workspace, size_t workspace_bytes, mxdet_stream_t stream);
int mxdet_group_norm_bwd(const mxdet_gn_desc_t* d, const uint16_t* x, const uint16_t* dy, const uint16_t* y,
                         const float* mean, const float* rstd, const float* gamma, const float* beta, uint16_t* dx,
                         float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, mxdet_stream_t stream);

/* stem: 7x7 stride-2 pad-3 convolution reading the NCHW fp32/bf16 image [N,3,H,W] directly
 * (coalesced plane reads), + bias + ReLU, writing bf16 [N,Ho,Wo,64]; w bf16 [64,7,7,3]. */
int mxdet_stem_conv7x7(const void* image, int32_t dtype, int32_t N, int32_t H, int32_t W,
                       const uint16_t* w, const float* bias, uint16_t* y, mxdet_stream_t stream);
/* the same followed by the 3x3 stride-2 pad-1 max pooling, in one pass (the stem map is never written): y bf16
 * [N,Hp,Wp,64] with Ho = (H-1)/2+1, Hp = (Ho-1)/2+1 (same for W); bits equal to maxpool3x3s2(stem_conv7x7) up to the
 * order of the fp32 accumulation inside the convolution */
int mxdet_stem_conv7x7_pool(const void* image, int32_t dtype, int32_t N, int32_t H, int32_t W,
                            const uint16_t* w, const float* bias, uint16_t* y, mxdet_stream_t stream);
/* 3x3 stride-2 pad-1 max pooling, bf16 channels-last */
int mxdet_maxpool3x3s2(const uint16_t* x, int32_t N, int32_t H, int32_t W, int32_t C, uint16_t* y,
                       mxdet_stream_t stream);
/* y[N,ceil(H/2),ceil(W/2),C] = x[N, 2i, 2j, C]  (FPN P6) and its adjoint (scatter into zeros / add) */
int mxdet_subsample2(const uint16_t* x, int32_t N, int32_t H, int32_t W, int32_t C, uint16_t* y,
                     mxdet_stream_t stream);
int mxdet_subsample2_bwd(const uint16_t* dy, int32_t N, int32_t H, int32_t W, int32_t C,
                         int32_t accumulate, uint16_t* dx, mxdet_stream_t stream);
/* adjoint of the nearest-neighbour 2x upsample: dcoarse[N,Hc,Wc,C] (+)= sum of the 2x2 fine cells */
int mxdet_upsample2_bwd(const uint16_t* dfine, int32_t N, int32_t Hf, int32_t Wf, int32_t C,
                        int32_t accumulate, uint16_t* dcoarse, mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * models/necks -- Balanced Feature Pyramid (Libra R-CNN, Pang et al., CVPR 2019): the gather and scatter
 * stages around the refine step, which is the caller's (a 3x3 convolution, or none).
 * Levels l = 0..L-1, finest first, bf16 [N,H[l],W[l],C] channels-last; refine level r; (h, w) = (H[r], W[r]).
 *   gather:   g_l = adaptive max pool of P_l to (h, w) for l < r, P_r itself, the nearest resize of P_l for l > r;
 *             B = bf16((((g_0 + g_1) + ...) + g_{L-1}) / (float)L): fp32 sum in level order, one division, one rounding.
 *   scatter:  Q_l = bf16(f32(P_l) + f32(s_l)); s_l = the nearest resize of Rf to (H[l], W[l]) for l < r, Rf itself for
 *             l = r, the adaptive max pool of Rf for l > r.
 * Index rules along an axis (those of torch's interpolate(mode="nearest") and adaptive_max_pool2d at integer ratios and
 * at the shapes of tests/test_libra_cpu.py): nearest src = (dst * in) / out in integers; pool window of output o =
 * [floor(o * in / out), ceil((o + 1) * in / out)) -- windows overlap when in is no multiple of out; the maximum's ties go
 * to the first element in row-major window order. A window may span at most 16 elements per axis (MXDET_ESHAPE).
 * The forward entries store every pooled element's arg-maximum (u8: 16 * dy + dx inside the window) in the workspace:
 * the backward entries read no activation.
 *   scatter_bwd: dRf = bf16(sum_l adj(s_l)(dQ_l)): one fp32 sum over the levels in order and, within a level, over
 *             the contributing pixels in row-major order.
 *   gather_bwd:  dP_l = bf16(f32(dQ_l) + adj(g_l)(f32(dB) / (float)L)): each term is divided first, the terms are
 *             summed in fp32 in row-major order of the contributing pixels, and the sum is added to f32(dQ_l).
 * Gather form, no float atomics: bit-identical run to run. out[l] may equal feat[l] (gather_bwd in place over dQ).
 * Every entry: one launch for all levels; host checks before it (2 <= L <= MXDET_BFP_MAX_LEVELS, 0 <= r < L, N, H, W
 * positive, C % 8 == 0: MXDET_ESHAPE; null pointers: MXDET_EINVAL; workspace: MXDET_EWORKSPACE); no allocation, no
 * host synchronisation; capturable. */
#define MXDET_BFP_MAX_LEVELS 6
typedef struct {
  int32_t num_levels, refine_level, N, C;
  int32_t H[8], W[8];
  void* feat[8]; /* per level: P (gather_fwd, scatter_fwd), dQ (scatter_bwd, gather_bwd) */
  void* out[8];  /* per level: Q (scatter_fwd), dP (gather_bwd); not read by the other two */
} mxdet_bfp_desc_t;
size_t mxdet_bfp_workspace_bytes(const mxdet_bfp_desc_t* d);
int mxdet_bfp_gather_fwd(const mxdet_bfp_desc_t* d, uint16_t* B, void* workspace, size_t workspace_bytes,
                         mxdet_stream_t stream);
int mxdet_bfp_scatter_fwd(const mxdet_bfp_desc_t* d, const uint16_t* Rf, void* workspace, size_t workspace_bytes,
                          mxdet_stream_t stream);
int mxdet_bfp_scatter_bwd(const mxdet_bfp_desc_t* d, uint16_t* dRf, const void* workspace, size_t workspace_bytes,
                          mxdet_stream_t stream);
int mxdet_bfp_gather_bwd(const mxdet_bfp_desc_t* d, const uint16_t* dB, const void* workspace, size_t workspace_bytes,
                         mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * models/necks -- batched single-head softmax attention: the activation x activation products of the
 * Balanced Feature Pyramid's embedded-Gaussian non-local refine (Libra R-CNN; Wang et al., Non-local Neural Networks,
 * CVPR 2018). qkv is bf16 [N, L, row_stride]; Q, K and V are the d columns from q_off, k_off and v_off of every row
 * (what one 1x1 convolution C -> 3 d writes: nothing is split or copied).
 *   fwd:  s_ij = scale * sum_c Q_ic K_jc (fp32); O_i = sum_j P_ij V_j with P_ij = exp(s_ij - m_i) / l_i, online over
 *         64-key tiles; out bf16 [N, L, d] dense, lse f32 [N, L] = m_i + ln l_i. fp32 accumulation; p is rounded to bf16
 *         only as the operand of the P V product. The L x L matrix never reaches memory.
 *   bwd:  P is recomputed from Q, K and lse. d_qkv bf16 [N, L, row_stride] receives dQ, dK and dV at the same offsets;
 *         its other columns are left untouched. delta_i = sum_c dO_ic O_ic goes to the workspace first. Two sweeps (a
 *         workgroup owns a key block for dK and dV, then a query block for dQ): every output element is summed by one
 *         wave in a fixed order -- no float atomics, no hand-off between workgroups, bit-identical run to run.
 * Host checks before any launch: d must be 64 or 128, 1 <= L <= 65536, 1 <= N <= 65535, row_stride and the offsets
 * multiples of 8 with off + d <= row_stride (MXDET_ESHAPE); scale positive and finite, no null pointer, every pointer
 * 16-byte aligned (MXDET_EINVAL); workspace (MXDET_EWORKSPACE). No allocation, no host synchronisation; capturable.
 * mxdet_attention_workspace_bytes returns 0 for a descriptor that fails the checks. */
typedef struct {
  int32_t N, L, d, row_stride;
  int32_t q_off, k_off, v_off;
  float scale;
} mxdet_attn_desc_t;
size_t mxdet_attention_workspace_bytes(const mxdet_attn_desc_t* d);
int mxdet_attention_fwd(const mxdet_attn_desc_t* d, const uint16_t* qkv, uint16_t* out, float* lse, mxdet_stream_t stream);
int mxdet_attention_bwd(const mxdet_attn_desc_t* d, const uint16_t* qkv, const uint16_t* out, const uint16_t* d_out,
                        const float* lse, uint16_t* d_qkv, void* workspace, size_t workspace_bytes, mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * models/necks -- CARAFE upsampling (Wang et al., Content-Aware ReAssembly of FEatures, ICCV 2019): the
 * learned replacement of the FPN's nearest-neighbour top-down upsample. Factor 2; reassembly kernel k = 3 or 5, r = k / 2.
 *   X bf16 [N,H,W,C] the coarse map; M bf16 [N,H,W,Cm] the kernel logits, of which channels 0 .. 4 k^2 - 1 are real and
 *   the others alignment padding that is never read; Y bf16 [N,Hf,Wf,C] with Hf = 2 H or 2 H - 1, Wf = 2 W or 2 W - 1 (what
 *   a pyramid level of (Hf + 1) / 2 rows produces): rows / columns of the 2 H x 2 W grid past Hf / Wf are not computed.
 *   fwd:  output pixel (i, j) has source q = (i >> 1, j >> 1) and sub-position s = (i & 1) * 2 + (j & 1); tap t = a * k + b
 *         reads X at (q_y + a - r, q_x + b - r), zero outside the map; its logit is channel t * 4 + s (the published
 *         pixel-shuffle order); w = softmax over the k^2 taps in fp32, maximum subtracted;
 *         Y[n,i,j,c] = bf16(sum_t w_t X[n,src(t),c]), fp32 sum in tap order, one rounding.
 *   bwd:  the weights are recomputed from M (the forward's function). dX[n,p,c] = bf16((accumulate ? f32(dX) : 0) + sum of
 *         w[q,s,t(p - q)] dY[n,2q+s,c] over the sources q within r of p in row-major order and their sub-positions inside
 *         Hf x Wf); dM[n,q,t*4+s] = bf16(w_t (g_t - sum_u w_u g_u)), g_t = sum_c dY[n,2q+s,c] X[n,src(t),c]; dM is exactly 0
 *         for a cropped sub-position and in every padding channel. Gather form, no float atomics: the same bits run to run.
 * Host checks before any launch: k in {3, 5}, N, H, W positive, C a positive multiple of 8, Cm >= 4 k^2, Hf and Wf as above
 * (MXDET_ESHAPE); no null pointer, X / Y / dY / dX 16-byte aligned (MXDET_EINVAL). No workspace, no allocation, no host
 * synchronisation; capturable. */
typedef struct {
  int32_t N, H, W, C;
  int32_t Cm, k;
  int32_t Hf, Wf;
} mxdet_carafe_desc_t;
int mxdet_carafe_fwd(const mxdet_carafe_desc_t* d, const uint16_t* X, const uint16_t* M, uint16_t* Y, mxdet_stream_t stream);
int mxdet_carafe_bwd(const mxdet_carafe_desc_t* d, const uint16_t* X, const uint16_t* M, const uint16_t* dY, uint16_t* dX,
                     uint16_t* dM, int32_t accumulate, mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * models/backbones -- the global context block of GCNet (Cao et al., GCNet: Non-local Networks Meet Squeeze-Excitation
 * Networks and Beyond, ICCVW 2019): attention pooling, channel_add fusion, placed after a bottleneck's
 * conv3 and in front of its shortcut add. t bf16 [N,HW,C] is conv3's output without residual or ReLU, sc bf16 the shortcut,
 * P the transform's inner width. wk [C], W1 [P,C] and W2 [C,P] are bf16; b1, gamma, beta [P] and b2 [C] fp32.
 *   pool_fwd       logits[n,p] = sum_c t[n,p,c] wk[c] (f32 [N,HW]; no bias: a softmax ignores a shift); per chunk of 64
 *                  positions the online softmax (maximum, sum, weighted column sums) into the workspace.
 *   transform_fwd  folds the chunks in a fixed order: lse[n] = max + ln sum exp(logit - max), ctx[n,c] = sum_p att t with
 *                  att = exp(logit - lse) (f32 [N,C]); h = W1 ctx + b1 [N,P]; mean, rstd [N] of LayerNorm over the P values
 *                  (biased variance, eps); u = relu(gamma (h - mean) rstd + beta); add = W2 u + b2 (f32 [N,C]).
 *   fuse_fwd       y = bf16(relu((f32(t) + add[n,c]) + f32(sc))), one rounding; y_bits (may be null): the 1-bit mask of the
 *                  stored y in the convolution entries' format (mxdet_conv_desc_t.relu_bits).
 *   reduce_bwd     per chunk column sums of ds (the gradient at the pre-activation sum, already masked by y > 0).
 *   transform_bwd  d_add[n,c] = sum_p ds (f32 [N,C]); dW2 = d_add^T u, db2 = sum_n d_add; du = d_add W2; gz = du (u > 0);
 *                  dgamma = sum_n gz xh, dbeta = sum_n gz; gg = gz gamma; dh = rstd (gg - mean_P(gg) - xh mean_P(gg xh));
 *                  dW1 = dh^T ctx, db1 = sum_n dh; d_ctx = dh W1 (f32 [N,C]). The six parameter gradients are fp32 in the
 *                  parameters' shapes, overwritten or, with accumulate, added to.
 *   pool_bwd       e[n,p] = sum_c d_ctx[n,c] t[n,p,c]; S[n] = sum_p att e; dl = att (e - S);
 *                  d_t = bf16((f32(ds) + att d_ctx[n,c]) + dl wk[c]), one rounding; d_wk[c] (+)= sum_{n,p} dl t[n,p,c].
 * All arithmetic is fp32; every summation order depends on the shape alone (DESIGN.md 5u lists them); no float atomics:
 * the same bits run to run. The workspace carries the chunk partials from pool_fwd to transform_fwd, from reduce_bwd to
 * transform_bwd and, inside transform_bwd and pool_bwd, between their kernels: one workspace per block, the calls of a
 * step in the order above on one stream.
 * Host checks before any launch: C % 8 == 0 in [8, 2048], P % 8 == 0 in [8, 512], 1 <= HW < 2^20, 1 <= N <= 65535,
 * N HW C < 2^31 (MXDET_ESHAPE); eps in (0, 1), no null pointer (y_bits excepted), every pointer 16-byte aligned
 * (MXDET_EINVAL); workspace (MXDET_EWORKSPACE). No allocation, no host synchronisation; capturable.
 * mxdet_gc_workspace_bytes returns 0 for a descriptor that fails the checks. */
typedef struct {
  int32_t N, HW, C, P;
  float eps;
} mxdet_gc_desc_t;
size_t mxdet_gc_workspace_bytes(const mxdet_gc_desc_t* d);
int mxdet_gc_pool_fwd(const mxdet_gc_desc_t* d, const uint16_t* t, const uint16_t* wk, float* logits, void* workspace,
                      size_t workspace_bytes, mxdet_stream_t stream);
int mxdet_gc_transform_fwd(const mxdet_gc_desc_t* d, const uint16_t* W1, const float* b1, const float* gamma, const float* beta,
                           const uint16_t* W2, const float* b2, float* lse, float* ctx, float* h, float* mean, float* rstd,
                           float* add, const void* workspace, size_t workspace_bytes, mxdet_stream_t stream);
int mxdet_gc_fuse_fwd(const mxdet_gc_desc_t* d, const uint16_t* t, const float* add, const uint16_t* sc, uint16_t* y,
                      uint8_t* y_bits, mxdet_stream_t stream);
int mxdet_gc_reduce_bwd(const mxdet_gc_desc_t* d, const uint16_t* ds, void* workspace, size_t workspace_bytes,
                        mxdet_stream_t stream);
int mxdet_gc_transform_bwd(const mxdet_gc_desc_t* d, const uint16_t* W1, const float* gamma, const float* beta,
                           const uint16_t* W2, const float* ctx, const float* h, const float* mean, const float* rstd,
                           float* d_add, float* d_ctx, float* dW1, float* db1, float* dgamma, float* dbeta, float* dW2,
                           float* db2, int32_t accumulate, void* workspace, size_t workspace_bytes, mxdet_stream_t stream);
int mxdet_gc_pool_bwd(const mxdet_gc_desc_t* d, const uint16_t* t, const uint16_t* wk, const uint16_t* ds, const float* logits,
                      const float* lse, const float* d_ctx, uint16_t* d_t, float* d_wk, int32_t accumulate, void* workspace,
                      size_t workspace_bytes, mxdet_stream_t stream);

/* One-stage (RetinaNet) test-time detection, MXNet-lineage role: per level top-k of sigmoid scores over (anchor, class),
 * decode, concatenate levels, per-class NMS, max_per_image -- a host loop in the lineage.
 * p describes the head outputs with p->classes = C foreground classes and p->A = anchors_per_cell * C:
 *   score(n,y,x,a*C+c) is the class logit, delta(n,y,x,a,k) the box delta (plain encoding, no normalisation).
 * Per image and level the pre_nms_top_n largest logits (ties: lower (cell, anchor, class) index first) are decoded and
 * clipped; the candidates of all levels are merged by (logit desc, index asc) and cut to 4096; score = sigmoid(logit);
 * then exactly as mxdet_detection_postprocess: per class keep score > score_thresh, greedy NMS at nms_thresh, and the
 * max_per_image best by (score desc, candidate rank asc, class asc). dets [N,max_per_image,6], class in 1..C. */
size_t mxdet_retina_detect_workspace_bytes(const mxdet_pyramid_t* p, int32_t N, int32_t pre_nms_top_n);
int mxdet_retina_detect(const mxdet_pyramid_t* p, int32_t N, const float* im_info, int32_t pre_nms_top_n,
                        float score_thresh, float nms_thresh, int32_t max_per_image, float* dets, int32_t* num_dets,
                        void* workspace, size_t workspace_bytes, mxdet_stream_t stream);
/* mxdet_retina_detect with Soft-NMS per class (semantics at mxdet_soft_nms_batched; id = candidate rank in the merged
 * list, min_score = score_thresh, max_keep = max_per_image). Same workspace as mxdet_retina_detect. */
int mxdet_retina_detect_soft(const mxdet_pyramid_t* p, int32_t N, const float* im_info, int32_t pre_nms_top_n,
                             float score_thresh, float nms_thresh, int32_t max_per_image, float* dets,
                             int32_t* num_dets, void* workspace, size_t workspace_bytes, int32_t method, float sigma,
                             mxdet_stream_t stream);
/* Test-time detection of the distribution head: mxdet_retina_detect_soft with method = -1 for greedy NMS and
 * reg_max in 1..MXDET_REG_MAX_LIMIT. p->reg[l] holds 4 (reg_max + 1) logits per anchor in the layout of mxdet_box_dist_loss,
 * addressed with the same reg_s* strides (channel index times reg_sc). Selection, merge, NMS and ordering are exactly those
 * of mxdet_retina_detect(_soft); only the box of each selected candidate differs: the integral decode at the candidate's
 * global index (level, cell, anchor) with the anchor centre 0.5 (x1 + x2), 0.5 (y1 + y2) of base_anchors + cell * stride,
 * clipped as mxdet_decode_clip clips. Only the at most pre_nms_top_n candidates per level and image are decoded. Same
 * workspace as mxdet_retina_detect. */
int mxdet_retina_detect_dfl(const mxdet_pyramid_t* p, int32_t N, const float* im_info, int32_t pre_nms_top_n,
                            float score_thresh, float nms_thresh, int32_t max_per_image, float* dets, int32_t* num_dets,
                            void* workspace, size_t workspace_bytes, int32_t method, float sigma, int32_t reg_max,
                            mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * process_data (README.md:23) -- the step in front of the path.
 * MXNet-lineage role: the host-side cv2 pipeline  flip -> cv2.resize(fx=fy=scale, INTER_LINEAR) -> BGR->RGB,
 * minus pixel mean (over std) -> NCHW -> zero-pad the batch to a common size. Here one launch turns the decoded
 * 8-bit frames of a batch into the bf16 NCHW tensor the stem kernel reads.
 *
 * Resize arithmetic = OpenCV's 8-bit bilinear (the reference names cv2 as its resizer, README.md:53-56, no version
 * pinned; restated from its published imgproc/resize.cpp, parity with a cv2 build is UNPINNED -- cv2 is not in the
 * image): with inv = 1/scale in double,
 *   fx = (float)((dx + 0.5) * inv - 0.5); sx = floor(fx); fx -= sx; sx < 0 -> (0, 0); sx >= sw-1 -> (sw-1, 0)
 *   a1 = rint(fx * 2048), a0 = rint((1 - fx) * 2048)           (11-bit coefficients, round half even)
 *   row(y) = S[y][sx] * a0 + S[y][min(sx+1, sw-1)] * a1;         same for dy -> (sy, b0, b1)
 *   v = (((b0 * (row(sy) >> 4)) >> 16) + ((b1 * (row(sy+1) >> 4)) >> 16) + 2) >> 2
 * then out = (v - mean[c]) / std[c] in fp32 (IEEE, unfused), rounded to bf16 (nearest even).
 * flip mirrors the SOURCE columns (flip-then-resize, the order the lineage uses); swap_rb reads source channel 2-c.
 * Pixels outside (dst_h, dst_w) of their image are written as zero: out is [N, 3, Hp, Wp], Wp % 8 == 0. */
typedef struct {
  const uint8_t* src;     /* device pointer, [src_h, src_w, 3] 8-bit interleaved, row pitch src_w*3 */
  int32_t src_h, src_w;
  int32_t dst_h, dst_w;   /* rint(src * scale), <= Hp / Wp */
  int32_t flip;           /* mirror columns */
  int32_t pad_;
  double inv_scale;       /* 1 / scale */
} mxdet_image_desc_t;
#define MXDET_PREPROCESS_MAX_BATCH 64
int mxdet_image_preprocess(const mxdet_image_desc_t* images /* host array */, int32_t N, int32_t Hp, int32_t Wp,
                           const float* mean3 /* host */, const float* std3 /* host */, int32_t swap_rb,
                           uint16_t* out, mxdet_stream_t stream);

/* Instance masks from polygons (datasets: COCO "segmentation" lists), written straight at network resolution.
 * verts [V,2] f32 (x,y) already scaled/flipped into the resized image; poly_start [P+1] i32 offsets into verts
 * (polygons of one instance adjacent, instances in n*G+g order); inst_first [N*G+1] i32 offsets into the polygon list. masks [N,G,H,W] u8: 1 where the pixel centre (x+0.5, y+0.5) is inside an odd number of edges
 * of ANY polygon of the instance (union of even-odd fills), else 0; instances without polygons are all zero.
 * Edge rule: (y0 <= py) != (y1 <= py) and px < x0 + (py - y0) * (x1 - x0) / (y1 - y0), fp32 unfused.
 * pycocotools' frPoly walks a 5x upsampled boundary instead; the two differ only on boundary pixels (unpinned). */
int mxdet_polygon_masks(const float* verts, const int32_t* poly_start, const int32_t* inst_first, int32_t N,
                        int32_t G, int32_t H, int32_t W, uint8_t* masks, mxdet_stream_t stream);

/* elementwise helpers on channels-last tensors */
int mxdet_add_bf16(const uint16_t* a, const uint16_t* b, int64_t n, uint16_t* out,
                   mxdet_stream_t stream);
int mxdet_relu_bwd_bf16(const uint16_t* dy, const uint16_t* y, int64_t n, uint16_t* dx,
                        mxdet_stream_t stream);
int mxdet_f32_to_bf16(const float* x, int64_t n, uint16_t* y, mxdet_stream_t stream);
/* y[i] (+)= bf16(x[i]) as fp32->bf16 with optional mask y*(mask>0): used to fold the RoIAlign
 * fp32 gradient accumulators into the bf16 pyramid gradients */
int mxdet_f32_accum_to_bf16(const float* x, int64_t n, int32_t accumulate, uint16_t* y,
                            mxdet_stream_t stream);
/* layout converters at the boundary (MXNet tensors are NCHW) */
int mxdet_nchw_to_nhwc_bf16(const void* x, int32_t dtype, int32_t N, int32_t C, int32_t H, int32_t W,
                            uint16_t* y, mxdet_stream_t stream);
int mxdet_nhwc_to_nchw_f32(const uint16_t* x, int32_t N, int32_t C, int32_t H, int32_t W, float* y,
                           mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * optimizer step (MXNet role: sgd_mom_update after kvstore reduce).
 * Flat fp32 parameter / gradient / momentum arenas of n elements:
 *   g = grad * rescale (+ wd * w);  m = momentum * m + g;  w -= lr_mult[i] * lr * m
 * and the bf16 working copy of w is refreshed in the same pass. per-element scale arrays may be
 * NULL. */
int mxdet_sgd_momentum_update(float* w, const float* grad, float* mom, uint16_t* w_bf16, int64_t n,
                              float lr, float momentum, float wd, float rescale,
                              mxdet_stream_t stream);
/* Same update with the learning rate read from device memory (lr_dev[0]) when the kernel runs: a step captured into
 * a hipGraph follows the warm-up / step schedule (MXNet role: lr_scheduler feeding the optimizer) without re-capture. */
int mxdet_sgd_momentum_update_sched(float* w, const float* grad, float* mom, uint16_t* w_bf16, int64_t n,
                                    const float* lr_dev, float momentum, float wd, float rescale,
                                    mxdet_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * data-parallel gradient exchange (MXNet role: kvstore push/pull, /root/reference/README.md:37; SURVEY.md
 * sections 8a10, 8b, 8e). One process per GPU; the only exchange of the hot path is the fp32 sum of contiguous slices
 * ("buckets") of the flat gradient arena, over RCCL (xGMI). `mxdet_comm_t` is the one explicit handle of the library:
 * an RCCL communicator + a side stream of its own + a ring of events, created and destroyed by the caller. The library
 * resolves RCCL at run time (the copy already mapped into the process, else librccl.so.1); without it every entry
 * below returns MXDET_ERCCL.
 *
 *   rank 0: mxdet_comm_unique_id(id) -> the caller hands the MXDET_COMM_ID_BYTES bytes to every rank by any channel
 *   every rank, with its device current: mxdet_comm_create(id, world, rank, &comm)           (collective)
 *   per bucket, as soon as backward has finalised it: mxdet_allreduce_bucket(comm, g + lo, hi - lo, s, &ticket)
 *       the sum is ordered behind everything enqueued on stream `s` so far and runs on the communicator's side
 *       stream: `s` itself does not wait (the rest of backward overlaps the exchange);
 *   before the bucket is consumed: mxdet_comm_wait(comm, ticket, t) makes stream `t` wait for that bucket's sum
 *       (ticket -1: for every bucket issued so far).
 * Sums are fp32, in place, in RCCL's fixed order for the communicator (run-to-run identical); the 1/world average is
 * the optimizer's `rescale`. At most MXDET_COMM_MAX_INFLIGHT buckets may be un-waited at a time. */
typedef struct mxdet_comm mxdet_comm_t;
#define MXDET_COMM_ID_BYTES 128
#define MXDET_COMM_MAX_INFLIGHT 64
int mxdet_comm_unique_id(uint8_t* id /* host, MXDET_COMM_ID_BYTES */);
int mxdet_comm_create(const uint8_t* id, int32_t world, int32_t rank, mxdet_comm_t** comm_out);
int mxdet_comm_destroy(mxdet_comm_t* comm);
int mxdet_allreduce_bucket(mxdet_comm_t* comm, float* grad, int64_t count, mxdet_stream_t stream,
                           int32_t* ticket_out);
int mxdet_comm_wait(mxdet_comm_t* comm, int32_t ticket, mxdet_stream_t stream);
/* replicate `bytes` bytes of `buf` from rank `root` (initial weights); ordered on `stream` itself */
int mxdet_comm_broadcast(mxdet_comm_t* comm, void* buf, size_t bytes, int32_t root, mxdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MXDET_H_ */
