// soft_nms.h -- the Soft-NMS list kernel's launcher, shared by soft_nms.hip (standalone entry) and postprocess.hip.
#pragma once
#include "common.h"

namespace mxdet {

constexpr int kSoftNmsMaxList = 4096;   // candidates of one list: 256 threads x 16 register slots

// One workgroup per list b of B. Candidate p < counts[b] of list b has box boxes[b*n_max + p] and
//   scores != null: score scores[b*n_max + p], id p                                   (standalone entry)
//   skeys  != null: score / id unpacked from skeys[b*n_max + p] = float_key(score) << 32 | ~id  (det_class_sort_kernel)
// Selection t of list b writes keep_pos[b*out_stride + t] = p and, where given, keep_scores[b*out_stride + t] = the score
// at selection and keep_keys[b*out_stride + t] = its key. With `pad` the unused tail of keep_pos / keep_scores is filled
// with -1 / 0. The caller has checked: n_max <= kSoftNmsMaxList, method in 0..2, 0 <= max_keep <= out_stride.
void soft_nms_launch(const float4* boxes, const float* scores, const unsigned long long* skeys, const int32_t* counts,
                     int B, int n_max, int method, float nms_thresh, float sigma, float min_score, int max_keep,
                     int out_stride, int pad, int32_t* keep_pos, float* keep_scores, unsigned long long* keep_keys,
                     int32_t* num_keep, hipStream_t stream);

}  // namespace mxdet
