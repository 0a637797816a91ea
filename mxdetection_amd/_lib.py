"""ctypes binding of libmxdet_hip.so (the C-ABI in include/mxdet.h).

The product path has no CPU fallback: if the HIP library is missing, importing an op raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MXDET_LIB") or os.path.join(_HERE, "libmxdet_hip.so")   # MXDET_LIB: ablation builds

c_i32, c_i64, c_u32, c_f32, c_sz, c_vp = C.c_int32, C.c_int64, C.c_uint32, C.c_float, C.c_size_t, C.c_void_p


class PyramidT(C.Structure):
    _fields_ = [
        ("num_levels", c_i32), ("A", c_i32),
        ("H", c_i32 * 8), ("W", c_i32 * 8), ("stride", c_i32 * 8),
        ("cls", c_vp * 8), ("reg", c_vp * 8),
        ("cls_sn", c_i64 * 8), ("cls_sy", c_i64 * 8), ("cls_sx", c_i64 * 8), ("cls_sa", c_i64 * 8),
        ("reg_sn", c_i64 * 8), ("reg_sy", c_i64 * 8), ("reg_sx", c_i64 * 8), ("reg_sc", c_i64 * 8),
        ("dtype", c_i32), ("classes", c_i32),
        ("base_anchors", c_vp * 8),
    ]


class FeatPyramidT(C.Structure):
    _fields_ = [
        ("num_levels", c_i32), ("lvl_min", c_i32),
        ("H", c_i32 * 8), ("W", c_i32 * 8),
        ("spatial_scale", c_f32 * 8),
        ("feat", c_vp * 8),
    ]


class ImageDescT(C.Structure):
    """mxdet_image_desc_t (include/mxdet.h)."""
    _fields_ = [("src", C.c_void_p), ("src_h", C.c_int32), ("src_w", C.c_int32), ("dst_h", C.c_int32),
                ("dst_w", C.c_int32), ("flip", C.c_int32), ("pad_", C.c_int32), ("inv_scale", C.c_double)]


class WgradItemT(C.Structure):
    pass


class ConvItemT(C.Structure):
    pass


class ConvDescT(C.Structure):
    _fields_ = [
        ("N", c_i32), ("H", c_i32), ("W", c_i32), ("Cin", c_i32),
        ("Cout", c_i32), ("KH", c_i32), ("KW", c_i32),
        ("stride", c_i32), ("pad", c_i32),
        ("Ho", c_i32), ("Wo", c_i32),
        ("relu", c_i32), ("res_upsample", c_i32), ("accumulate", c_i32),
        ("prefetch", c_vp), ("prefetch_bytes", c_i64), ("relu_bits", c_vp),
    ]


class DeformDescT(C.Structure):
    """mxdet_deform_desc_t (include/mxdet.h)."""
    _fields_ = [
        ("N", c_i32), ("H", c_i32), ("W", c_i32), ("C", c_i32),
        ("Ho", c_i32), ("Wo", c_i32), ("KH", c_i32), ("KW", c_i32),
        ("stride", c_i32), ("pad", c_i32), ("groups", c_i32), ("modulated", c_i32),
        ("off_channels", c_i32), ("accumulate", c_i32),
    ]


class DpoolDescT(C.Structure):
    """mxdet_dpool_desc_t (include/mxdet.h)."""
    _fields_ = [
        ("pyr", FeatPyramidT), ("N", c_i32), ("C", c_i32), ("PH", c_i32), ("PW", c_i32),
        ("sample_per_part", c_i32), ("trans_std", c_f32), ("modulated", c_i32),
        ("trans_stride", c_i32), ("mask_stride", c_i32), ("accumulate", c_i32),
    ]


class GnDescT(C.Structure):
    """mxdet_gn_desc_t (include/mxdet.h)."""
    _fields_ = [("N", c_i32), ("HW", c_i32), ("C", c_i32), ("G", c_i32), ("eps", c_f32), ("relu", c_i32),
                ("accumulate", c_i32)]


class BfpDescT(C.Structure):
    """mxdet_bfp_desc_t (include/mxdet.h)."""
    _fields_ = [("num_levels", c_i32), ("refine_level", c_i32), ("N", c_i32), ("C", c_i32), ("H", c_i32 * 8), ("W", c_i32 * 8),
                ("feat", c_vp * 8), ("out", c_vp * 8)]


class AttnDescT(C.Structure):
    """mxdet_attn_desc_t (include/mxdet.h)."""
    _fields_ = [("N", c_i32), ("L", c_i32), ("d", c_i32), ("row_stride", c_i32), ("q_off", c_i32), ("k_off", c_i32),
                ("v_off", c_i32), ("scale", c_f32)]


class CarafeDescT(C.Structure):
    """mxdet_carafe_desc_t (include/mxdet.h)."""
    _fields_ = [("N", c_i32), ("H", c_i32), ("W", c_i32), ("C", c_i32), ("Cm", c_i32), ("k", c_i32), ("Hf", c_i32),
                ("Wf", c_i32)]


class GcDescT(C.Structure):
    """mxdet_gc_desc_t (include/mxdet.h)."""
    _fields_ = [("N", c_i32), ("HW", c_i32), ("C", c_i32), ("P", c_i32), ("eps", c_f32)]


class RpnOrderedItemT(C.Structure):
    """mxdet_rpn_ordered_item_t (include/mxdet.h)."""
    _fields_ = [("kind", c_i32), ("H", c_i32), ("W", c_i32), ("halves_per_slab", c_i32), ("slab0", c_i32),
                ("fold_ksplit", c_i32), ("bias_pixels", c_i32), ("bias_splits", c_i32)]


class RpnSparseT(C.Structure):
    """mxdet_rpn_sparse_t (include/mxdet.h)."""
    _fields_ = [("num_levels", c_i32), ("N", c_i32), ("A", c_i32), ("C", c_i32), ("Ch", c_i32), ("smax", c_i32),
                ("H", c_i32 * 8), ("W", c_i32 * 8), ("accumulate", c_i32 * 8),
                ("P", c_vp * 8), ("t", c_vp * 8), ("tbits", c_vp * 8), ("gh", c_vp * 8), ("dP", c_vp * 8), ("dt", c_vp * 8),
                ("ordered", C.POINTER(RpnOrderedItemT)), ("ordered_work", c_vp)]


WgradItemT._fields_ = [("desc", ConvDescT), ("x", c_vp), ("dy", c_vp), ("dw", c_vp), ("db", c_vp)]
ConvItemT._fields_ = [("desc", ConvDescT), ("src", c_vp), ("filt", c_vp), ("bias", c_vp), ("residual", c_vp),
                      ("relu_mask", c_vp), ("dst", c_vp)]

P = C.POINTER

# name -> (restype, argtypes). Every symbol include/mxdet.h declares must appear here
# (tests/test_abi.py checks the header against this table and the built library).
SIGNATURES = {
    "mxdet_last_error": (C.c_char_p, []),
    "mxdet_version": (C.c_char_p, []),
    "mxdet_box_iou": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp]),
    "mxdet_generate_anchors": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_nms_batched_workspace_bytes": (c_sz, [c_i32, c_i32]),
    "mxdet_nms_batched": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_f32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_soft_nms_batched": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_i32, c_vp, c_vp, c_vp,
                                       c_vp]),
    "mxdet_pixel_shuffle2_inv_relu": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_mask_paste_workspace_bytes": (c_sz, [c_i64, c_i32]),
    "mxdet_mask_paste": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_retina_detect_workspace_bytes": (c_sz, [c_vp, c_i32, c_i32]),
    "mxdet_retina_detect": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_f32, c_f32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_retina_detect_soft": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_f32, c_f32, c_i32, c_vp, c_vp, c_vp, c_sz, c_i32, c_f32,
                                         c_vp]),
    "mxdet_retina_detect_dfl": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_f32, c_f32, c_i32, c_vp, c_vp, c_vp, c_sz, c_i32, c_f32,
                                        c_i32, c_vp]),
    "mxdet_debug_preprocess_direct": (c_i32, [c_i32]),
    "mxdet_image_preprocess": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp]),
    "mxdet_polygon_masks": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_detection_postprocess_workspace_bytes": (c_sz, [c_i32, c_i32, c_i32]),
    "mxdet_detection_postprocess": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32,
                                            P(c_f32), P(c_f32), c_f32, c_f32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_detection_postprocess_soft": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32,
                                                 P(c_f32), P(c_f32), c_f32, c_f32, c_i32, c_vp, c_vp, c_vp, c_sz, c_i32,
                                                 c_f32, c_vp]),
    "mxdet_proposal_workspace_bytes": (c_sz, [P(PyramidT), c_i32, c_i32]),
    "mxdet_proposal": (c_i32, [P(PyramidT), c_i32, c_vp, c_i32, c_i32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp,
                               c_vp, c_sz, c_vp]),
    "mxdet_anchor_target_workspace_bytes": (c_sz, [c_i32, c_i64, c_i32]),
    "mxdet_anchor_target": (c_i32, [c_vp, c_i64, c_vp, c_i32, c_i32, c_vp, c_f32, c_f32, c_f32, c_i32, c_f32,
                                    c_u32, c_u32, c_vp, c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_atss_assign_workspace_bytes": (c_sz, [c_i32, c_i64, c_i32]),
    "mxdet_atss_assign": (c_i32, [c_vp, c_i64, P(c_i64), c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz,
                                  c_vp]),
    "mxdet_proposal_target": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32,
                                      c_i32, c_i32, P(c_f32), P(c_f32), c_u32, c_u32, c_vp, c_u32, c_vp, c_vp, c_vp,
                                      c_vp, c_vp, c_vp, c_vp]),
    "mxdet_proposal_target_balanced": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32,
                                               c_i32, c_i32, P(c_f32), P(c_f32), c_u32, c_u32, c_vp, c_u32, c_i32, c_vp, c_vp,
                                               c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_ohem_roi_score": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i64,
                                     c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32, c_f32, c_f32, c_vp, c_vp]),
    "mxdet_ohem_select_workspace_bytes": (c_sz, [c_i32, c_i32]),
    "mxdet_ohem_select": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_ohem_gather": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp,
                                  c_vp, c_vp]),
    "mxdet_fpn_level_map": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_roi_align_fwd": (c_i32, [P(FeatPyramidT), c_i32, c_i32, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp,
                                    c_vp]),
    "mxdet_roi_align_bwd": (c_i32, [P(FeatPyramidT), c_i32, c_i32, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp,
                                    c_vp]),
    "mxdet_roi_align_bwd_gather_workspace_bytes": (c_sz, [P(FeatPyramidT), c_i32, c_i64]),
    "mxdet_roi_align_bwd_gather": (c_i32, [P(FeatPyramidT), c_i32, c_i32, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp,
                                           c_i32, c_vp, c_sz, c_vp]),
    "mxdet_roi_align_bwd_gather_prepare": (c_i32, [P(FeatPyramidT), c_i32, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32,
                                                   c_vp, c_sz, c_vp]),
    "mxdet_roi_align_bwd_gather_prepared": (c_i32, [P(FeatPyramidT), c_i32, c_i32, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32,
                                                    c_vp, c_i32, c_vp, c_sz, c_vp]),
    "mxdet_smooth_l1_fwd": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_f32, c_vp, c_vp]),
    "mxdet_smooth_l1_bwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_i32, c_vp, c_vp]),
    "mxdet_loss_workspace_bytes": (c_sz, [c_i64]),
    "mxdet_focal_loss": (c_i32, [c_vp, c_i32, c_vp, c_i64, c_i32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_sz,
                                 c_vp]),
    "mxdet_anchor_class_labels": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "mxdet_retina_loss_num_partials": (c_i32, [c_i32, c_i32, c_i32, c_i32]),
    "mxdet_retina_loss_level": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64,
                                        c_i64, c_f32, c_f32, c_f32, c_vp, c_f32, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_rpn_loss_num_partials": (c_i32, [c_i32, c_i32, c_i32]),
    "mxdet_rpn_loss_level": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_i64, c_f32,
                                     c_f32, c_f32, c_vp, c_vp, c_vp]),
    "mxdet_loss_finalize": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_rcnn_loss": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_f32,
                                c_f32, c_f32, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_rcnn_loss_balanced": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_f32, c_f32,
                                         c_f32, c_f32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_box_iou_loss": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_i64, c_i32, c_f32, c_f32, c_f32, c_f32, c_f32, c_vp,
                                   c_vp, c_vp]),
    "mxdet_rcnn_loss_iou": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i64, c_i32, c_i32,
                                    c_i32, c_f32, c_f32, c_f32, c_f32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp, c_sz,
                                    c_vp]),
    "mxdet_retina_loss_level_iou": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp,
                                            c_i32, c_i64, c_i64, c_f32, c_f32, c_i32, c_f32, c_f32, c_f32, c_f32, c_f32, c_vp,
                                            c_f32, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_quality_focal_loss": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i64, c_i32, c_i32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_sz,
                                         c_vp]),
    "mxdet_retina_loss_level_quality": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp,
                                                c_vp, c_i32, c_i64, c_i64, c_i32, c_f32, c_f32, c_i32, c_f32, c_f32, c_f32, c_f32,
                                                c_f32, c_vp, c_f32, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_box_dist_loss": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i64, c_i32, c_f32, c_i32, c_f32, c_f32, c_f32, c_vp, c_vp,
                                    c_vp, c_vp, c_vp]),
    "mxdet_retina_loss_level_dfl": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp,
                                            c_i32, c_i64, c_i64, c_i32, c_f32, c_f32, c_i32, c_i32, c_f32, c_f32, c_f32, c_vp,
                                            c_f32, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_ghm_hist_level": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_i64, c_i32,
                                     c_i32, c_i32, c_f32, c_vp, c_vp]),
    "mxdet_ghm_weights": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_retina_loss_level_ghm": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_i64,
                                            c_i32, c_f32, c_f32, c_f32, c_vp, c_i32, c_i32, c_f32, c_f32, c_f32, c_vp, c_f32,
                                            c_vp, c_vp, c_vp, c_vp]),
    "mxdet_mask_target": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "mxdet_pixel_shuffle2": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_mask_loss_workspace_bytes": (c_sz, [c_i64, c_i32]),
    "mxdet_mask_loss": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_maskiou_target_workspace_bytes": (c_sz, [c_i32, c_i32]),
    "mxdet_maskiou_target": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32,
                                     c_i32, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_maskiou_input": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_maskiou_input_bwd": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_maskiou_loss": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_f32, c_f32, c_vp, c_vp, c_vp]),
    "mxdet_maskiou_score": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp]),
    "mxdet_keypoint_target": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_keypoint_loss_workspace_bytes": (c_sz, [c_i64]),
    "mxdet_keypoint_loss": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_f32, c_f32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_keypoint_decode": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_conv2d_fwd": (c_i32, [P(ConvDescT), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_conv2d_fwd_chain": (c_i32, [P(ConvDescT), c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32,
                                       c_i32, c_vp, c_vp]),
    "mxdet_conv2d_fwd_splitk_workspace_bytes": (c_sz, [P(ConvDescT), c_i32]),
    "mxdet_conv2d_fwd_splitk": (c_i32, [P(ConvDescT), c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_sz, c_vp]),
    "mxdet_conv2d_dgrad": (c_i32, [P(ConvDescT), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_conv2d_wgrad_workspace_bytes": (c_sz, [P(ConvDescT)]),
    "mxdet_conv2d_wgrad": (c_i32, [P(ConvDescT), c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_conv2d_grouped_table_bytes": (c_sz, [c_i32]),
    "mxdet_conv2d_grouped_plan": (c_i32, [P(ConvItemT), c_i32, c_i32, c_vp, c_sz, P(c_i32), P(c_i32)]),
    "mxdet_conv2d_grouped": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "mxdet_conv2d_wgrad_grouped_table_bytes": (c_sz, [c_i32]),
    "mxdet_conv2d_wgrad_grouped_plan": (c_i32, [P(WgradItemT), c_i32, c_vp, c_sz, P(c_sz), P(c_i32), P(c_i32), P(c_i32)]),
    "mxdet_conv2d_wgrad_grouped": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_sz, c_sz, c_vp]),
    "mxdet_conv2d_wgrad_grouped_parts": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_sz, c_sz, c_vp]),
    "mxdet_debug_force_conv_cfg": (c_i32, [c_i32]),
    "mxdet_debug_force_wgrad_ksplit": (c_i32, [c_i32]),
    "mxdet_rpn_sparse_list": (c_i32, [P(RpnSparseT), c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_rpn_sparse_backward": (c_i32, [P(RpnSparseT), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                          c_i32, c_vp]),
    "mxdet_rpn_ordered_schedule": (c_i32, [c_vp, c_i32, c_i32, P(RpnOrderedItemT)]),
    "mxdet_filter_transpose": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_filter_transpose_batched": (c_i32, [c_vp, c_i32, c_i32, c_vp]),
    "mxdet_deform_im2col": (c_i32, [P(DeformDescT), c_vp, c_vp, c_vp, c_vp]),
    "mxdet_deform_col2im_coord": (c_i32, [P(DeformDescT), c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_deform_col2im_workspace_bytes": (c_sz, [P(DeformDescT)]),
    "mxdet_deform_col2im": (c_i32, [P(DeformDescT), c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_dpool_fwd": (c_i32, [P(DpoolDescT), c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_dpool_bwd_trans": (c_i32, [P(DpoolDescT), c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_dpool_bwd_feat_workspace_bytes": (c_sz, [P(DpoolDescT), c_i64]),
    "mxdet_dpool_bwd_feat": (c_i32, [P(DpoolDescT), c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_group_norm_workspace_bytes": (c_sz, [P(GnDescT), c_i32]),
    "mxdet_group_norm_fwd": (c_i32, [P(GnDescT), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_group_norm_bwd": (c_i32, [P(GnDescT), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz,
                                     c_vp]),
    "mxdet_debug_group_norm_route": (c_i32, [P(GnDescT)]),
    "mxdet_stem_conv7x7": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_stem_conv7x7_pool": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_maxpool3x3s2": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_subsample2": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_subsample2_bwd": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_upsample2_bwd": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_bfp_workspace_bytes": (c_sz, [P(BfpDescT)]),
    "mxdet_bfp_gather_fwd": (c_i32, [P(BfpDescT), c_vp, c_vp, c_sz, c_vp]),
    "mxdet_bfp_scatter_fwd": (c_i32, [P(BfpDescT), c_vp, c_vp, c_sz, c_vp]),
    "mxdet_bfp_scatter_bwd": (c_i32, [P(BfpDescT), c_vp, c_vp, c_sz, c_vp]),
    "mxdet_bfp_gather_bwd": (c_i32, [P(BfpDescT), c_vp, c_vp, c_sz, c_vp]),
    "mxdet_attention_workspace_bytes": (c_sz, [P(AttnDescT)]),
    "mxdet_attention_fwd": (c_i32, [P(AttnDescT), c_vp, c_vp, c_vp, c_vp]),
    "mxdet_attention_bwd": (c_i32, [P(AttnDescT), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_carafe_fwd": (c_i32, [P(CarafeDescT), c_vp, c_vp, c_vp, c_vp]),
    "mxdet_carafe_bwd": (c_i32, [P(CarafeDescT), c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp]),
    "mxdet_gc_workspace_bytes": (c_sz, [P(GcDescT)]),
    "mxdet_gc_pool_fwd": (c_i32, [P(GcDescT), c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mxdet_gc_transform_fwd": (c_i32, [P(GcDescT)] + [c_vp] * 13 + [c_sz, c_vp]),
    "mxdet_gc_fuse_fwd": (c_i32, [P(GcDescT), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mxdet_gc_reduce_bwd": (c_i32, [P(GcDescT), c_vp, c_vp, c_sz, c_vp]),
    "mxdet_gc_transform_bwd": (c_i32, [P(GcDescT)] + [c_vp] * 16 + [c_i32, c_vp, c_sz, c_vp]),
    "mxdet_gc_pool_bwd": (c_i32, [P(GcDescT)] + [c_vp] * 8 + [c_i32, c_vp, c_sz, c_vp]),
    "mxdet_add_bf16": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp]),
    "mxdet_relu_bwd_bf16": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp]),
    "mxdet_f32_to_bf16": (c_i32, [c_vp, c_i64, c_vp, c_vp]),
    "mxdet_f32_accum_to_bf16": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_vp]),
    "mxdet_nchw_to_nhwc_bf16": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_nhwc_to_nchw_f32": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mxdet_sgd_momentum_update": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_f32, c_f32, c_f32, c_vp]),
    "mxdet_sgd_momentum_update_sched": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_f32, c_f32, c_f32, c_vp]),
    "mxdet_comm_unique_id": (c_i32, [c_vp]),
    "mxdet_comm_create": (c_i32, [c_vp, c_i32, c_i32, P(c_vp)]),
    "mxdet_comm_destroy": (c_i32, [c_vp]),
    "mxdet_allreduce_bucket": (c_i32, [c_vp, c_vp, c_i64, c_vp, P(c_i32)]),
    "mxdet_comm_wait": (c_i32, [c_vp, c_i32, c_vp]),
    "mxdet_comm_broadcast": (c_i32, [c_vp, c_vp, c_sz, c_i32, c_vp]),
    "mxdet_debug_set_tuning": (c_i32, [c_i32, c_i64]),
    "mxdet_debug_get_tuning": (c_i64, [c_i32]),
    "mxdet_debug_route_probe": (c_i32, [c_i32]),
    "mxdet_debug_route_read": (c_i32, [P(c_i32), c_i32]),
}

# entries declared in include/mxdet_debug.h (tuning / test hooks, not part of the drop-in boundary)
DEBUG_SYMBOLS = ("mxdet_debug_force_conv_cfg", "mxdet_debug_force_wgrad_ksplit", "mxdet_debug_preprocess_direct",
                 "mxdet_debug_set_tuning", "mxdet_debug_get_tuning", "mxdet_debug_route_probe", "mxdet_debug_route_read",
                 "mxdet_debug_group_norm_route")
TUNING_KEYS = {"T64": 0, "T128": 1, "PAR64": 2, "WG_TARGET": 3, "WG_MINSTEPS": 4, "WG_MAXSTEPS": 5, "T3_ENABLE": 6,
               "T3_TARGET": 7, "T3_MINSTEPS": 8, "T3_NS": 9, "TAIL": 10, "WG_NS": 11, "ROI_TABLE": 12, "ROI_ROWS": 13, "STATIC_TAPS": 14,
               "T128W": 15, "T3_MIX": 16, "SPLITK_TILE": 17, "T3_PER_ITEM": 18}
# word 0 of a route-probe record (MXDET_ROUTE_* in include/mxdet_debug.h)
ROUTE_KINDS = {"CONV": 1, "WGRAD": 2, "CONV_GROUPED": 3, "WGRAD_GROUPED": 4, "RETINA_LOSS": 5, "RETINA_LOSS_IOU": 6,
               "RETINA_LOSS_QUALITY": 7, "RETINA_LOSS_DFL": 8, "RETINA_LOSS_GHM": 9, "GHM_HIST": 10}

# `kind` of the IoU-family box losses (MXDET_IOU_LOSS_* in include/mxdet.h)
IOU_LOSS_KINDS = {"iou": 0, "giou": 1, "diou": 2}
# `cls_kind` of the quality-aware class losses (MXDET_CLS_LOSS_* in include/mxdet.h)
CLS_LOSS_KINDS = {"qfl": 1, "vfl": 2}
# `cls_kind` of mxdet_retina_loss_level_dfl: the above and MXDET_CLS_LOSS_FOCAL; reg_max's bound (MXDET_REG_MAX_LIMIT)
CLS_LOSS_KINDS_DFL = {"focal": 0, "qfl": 1, "vfl": 2}
REG_MAX_LIMIT = 31
# `flags` of the gradient-harmonizing entries (MXDET_GHM_CLS / _REG) and the bound of their bins (MXDET_GHM_MAX_BINS)
GHM_FLAGS = {"cls": 1, "reg": 2, "both": 3}
GHM_MAX_BINS = 64
# bounds of the Libra R-CNN entries (MXDET_SAMPLER_MAX_BINS, MXDET_BFP_MAX_LEVELS)
SAMPLER_MAX_BINS = 8
BFP_MAX_LEVELS = 6
# head widths of the attention entries (mxdet_attn_desc_t.d)
ATTN_HEAD_DIMS = (64, 128)
# reassembly kernel sizes of the CARAFE entries (mxdet_carafe_desc_t.k)
CARAFE_KERNELS = (3, 5)
# positions per workgroup of the global context entries' map kernels (kGcChunk in csrc/context.hip) and their bounds
GC_CHUNK = 64
GC_MAX_C, GC_MAX_P = 2048, 512

_lib = None


class MxdetError(RuntimeError):
    pass


def load():
    """Load libmxdet_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MxdetError(
            "libmxdet_hip.so not found at %s -- build it with `python -m mxdetection_amd.build` "
            "(there is no CPU fallback)" % LIB_PATH)
    # torch owns device memory and streams on the host side and bundles its own libamdhip64/libhsa-runtime64 with
    # the same SONAME as /opt/rocm's. It must be mapped FIRST so that this library's DT_NEEDED entries resolve to
    # the runtime torch uses; two HIP/HSA runtimes in one process leave the second one without a device.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)  # tests/test_abi.py asserts that no declared symbol is missing
        if fn is None:
            continue
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    # sweep tooling (tools/tune_sweep.sh): MXDET_TUNE_<KEY>=value is read HERE, by the Python host side, and handed to
    # the debug hook; the library itself never reads the environment
    for key, idx in TUNING_KEYS.items():
        v = os.environ.get("MXDET_TUNE_" + key)
        if v:
            lib.mxdet_debug_set_tuning(idx, int(v))
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().mxdet_last_error().decode("utf-8", "replace")
        raise MxdetError("%s failed (%d): %s" % (what or "mxdet call", rc, msg))


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
