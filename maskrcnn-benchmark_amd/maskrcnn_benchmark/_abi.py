"""The C ABI of the detops library (include/detops.h) as data: one table of ctypes signatures, the ABI version, the
error and dtype codes and the tuning keys.  Both builds of the HIP sources are bound from it: libdetops_gfx950.so by
`_lib.py`, the host emulation of the test suite by `tests/emu`.  tests/test_abi.py parses the header and compares every
return type, argument, code and key with this module, so it imports nothing but ctypes and loads no library.
"""
import ctypes

ABI_VERSION = 1  # DETOPS_ABI_VERSION

ERRORS = {-1: "DETOPS_EINVAL (bad shape / null pointer)", -2: "DETOPS_EWORKSPACE (workspace too small)",
          -3: "DETOPS_EUNSUPPORTED (configuration not implemented)",
          -4: "DETOPS_EGTCAP (a problem has more ground truths than detops_eval_match serves)"}

F32, F16, BF16 = 0, 1, 2  # DETOPS_F32 / DETOPS_F16 / DETOPS_BF16

# DETOPS_RLE_*: the per-mask status bits of detops_rle_decode_write, lowest bit first
RLE_STATUS = {1: "DETOPS_RLE_BAD_BYTE (a byte outside 48..111)", 2: "DETOPS_RLE_TRUNCATED (the last byte continues)",
              4: "DETOPS_RLE_LONG_VALUE (a value of more than 7 bytes)", 8: "DETOPS_RLE_BAD_RUN (a run outside [0, 2^31))",
              16: "DETOPS_RLE_BAD_SUM (the runs do not sum to h * w)"}
MASK_PACK_RLE_MAX_H = 4096  # DETOPS_MASK_PACK_RLE_MAX_H
EVAL_OKS_MAX_K = 32  # DETOPS_EVAL_OKS_MAX_K
EVAL_PROPOSALS_MAX_DT, EVAL_PROPOSALS_MAX_GT = 2048, 1024  # DETOPS_EVAL_PROPOSALS_MAX_DT / _MAX_GT
WINDOW_COUNTS_MAX_ITEMS = 1 << 24  # DETOPS_WINDOW_COUNTS_MAX_ITEMS

# the fields of struct DetopsTuning (csrc/detops_common.h) = the keys of detops_tuning_set / detops_tuning_get
TUNING_KEYS = ("roi_bwd_impl", "roi_bwd_seg", "nms_fault", "nms_spin_budget", "roi_bwd_ring", "roi_bwd_ct", "roi_bwd_split",
               "roi_bwd_maxseg", "roi_bwd_extras", "roi_bwd_groups", "roi_bwd_scan_ct", "roi_bwd_debug", "roi_fwd_impl",
               "roi_fwd_records", "roi_fwd_ct", "roi_fwd_order", "roi_fwd_order_mink", "dcn_col2im", "dcn_fused",
               "dcn_gather_xcd", "dcn_nhwc", "dcn_ell_build", "nms_fused", "nms_no_repair", "nms_no_presorted", "nms_debug")

c_int, c_float, c_void_p, c_size_t = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t

# name -> (restype, argtypes); mirrors include/detops.h one to one
_P = c_void_p
SIGNATURES = {
    "detops_version": (c_int, [_P]),
    "detops_tuning_set": (c_int, [ctypes.c_char_p, c_int]),
    "detops_tuning_get": (c_int, [ctypes.c_char_p, _P]),
    "detops_roi_align_forward_f32": (c_int, [_P, _P, _P] + [c_int] * 7 + [c_float, c_int, _P]),
    "detops_roi_align_backward_f32": (c_int, [_P, _P, _P] + [c_int] * 7 + [c_float, c_int, c_int, _P]),
    "detops_roi_align_fpn_forward_f32": (
        c_int, [_P, _P, _P, _P, c_int, _P, _P, _P] + [c_int] * 8 + [c_float, c_float, c_float, _P]),
    "detops_roi_align_fpn_backward_f32": (
        c_int, [_P, _P, _P, _P, _P, _P, _P] + [c_int] * 8 + [_P]),
    "detops_roi_align_fpn_backward_ws_f32": (
        c_int, [_P, _P, _P, _P, _P, _P, _P] + [c_int] * 8 + [_P, c_size_t, _P]),
    "detops_roi_align_fpn_backward_prepare_f32": (c_int, [_P] * 5 + [c_int] * 7 + [_P, c_size_t, _P]),
    "detops_roi_align_fpn_backward_prepared_f32": (c_int, [_P] * 5 + [c_int] * 7 + [_P, c_size_t, _P]),
    "detops_roi_align_backward_ws_f32": (
        c_int, [_P, _P, _P] + [c_int] * 7 + [c_float, c_int, c_int, _P, c_size_t, _P]),
    "detops_roi_align_backward_workspace_bytes": (c_size_t, [_P, _P] + [c_int] * 6),
    "detops_roi_align_forward_workspace_bytes": (c_size_t, [c_int] * 4),
    "detops_nms_cpu_f32": (c_int, [_P, _P, c_int, c_float, _P, _P]),
    "detops_rpn_loss_workspace_bytes": (c_size_t, []),
    "detops_rpn_loss_f32": (c_int, [_P, _P, _P, _P, c_int, c_int, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_float,
                                    _P, _P, _P, _P, _P, c_size_t, _P]),
    "detops_rpn_loss_backward_f32": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "detops_rpn_head_backward_workspace_bytes": (c_size_t, [c_int] * 4),
    "detops_rpn_head_backward_f32": (c_int, [_P] * 7 + [c_int] * 6 + [_P] * 10 + [_P, c_size_t, _P]),
    "detops_roi_align_forward_cpu_f32": (c_int, [_P, _P, _P] + [c_int] * 7 + [c_float, c_int]),
    "detops_roi_align_forward_ws_f32": (c_int, [_P, _P, _P] + [c_int] * 7 + [c_float, c_int, _P, c_size_t, _P]),
    "detops_roi_align_fpn_forward_ws_f32": (
        c_int, [_P, _P, _P, _P, c_int, _P, _P, _P] + [c_int] * 8 + [c_float, c_float, c_float, _P, c_size_t, _P]),
    "detops_match_boxes_workspace_bytes": (c_size_t, [c_int, c_int]),
    "detops_match_boxes_f32": (c_int, [_P, _P, _P] + [c_int] * 4 + [c_float, c_float, c_int, _P, _P, c_size_t, _P]),
    "detops_sample_labels_workspace_bytes": (c_size_t, [c_int, c_int]),
    "detops_sample_labels": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, ctypes.c_uint64, _P, _P, _P, _P, _P, c_size_t, _P]),
    "detops_sample_labels_dseed": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, ctypes.c_uint64, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "detops_mask_targets": (c_int, [_P, c_int, _P, _P] + [c_int] * 5 + [_P, _P]),
    "detops_match_labels": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "detops_roi_head_targets_f32": (c_int, [_P] * 8 + [c_int] * 4 + [c_float] * 4 + [_P] * 6),
    "detops_fastrcnn_loss_workspace_bytes": (c_size_t, [c_int]),
    "detops_fastrcnn_loss_f32": (c_int, [_P] * 4 + [c_int] * 4 + [c_float] + [_P] * 4 + [c_size_t, _P]),
    "detops_mask_loss_workspace_bytes": (c_size_t, [c_int]),
    "detops_mask_loss_f32": (c_int, [_P] * 3 + [c_int] * 3 + [_P] * 3 + [c_size_t, _P]),
    "detops_head_loss_backward_f32": (c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_int64, _P, _P]),
    "detops_keypoint_targets": (c_int, [_P] * 5 + [c_int] * 4 + [_P] * 3),
    "detops_keypoint_loss_workspace_bytes": (c_size_t, [c_int, c_int]),
    "detops_keypoint_loss_f32": (c_int, [_P] * 4 + [c_int] * 4 + [_P] * 3 + [_P, c_size_t, _P]),
    "detops_heatmaps_to_keypoints_f32": (c_int, [_P] * 3 + [c_int] * 4 + [_P] * 3),
    "detops_paste_masks": (c_int, [_P, c_int, _P, _P, _P, c_int, c_int, c_int, c_float, _P, _P]),
    "detops_paste_masks_rle_workspace_bytes": (c_size_t, [c_int, c_int]),
    "detops_paste_masks_rle_count": (c_int, [_P, c_int, _P, _P, c_int, c_int, c_int, c_float, c_int, _P, _P, c_size_t, _P]),
    "detops_paste_masks_rle_write": (c_int, [_P, c_int, _P, _P, c_int, c_int, c_int, c_float, c_int, _P, _P, _P, c_size_t, _P]),
    "detops_rle_string_workspace_bytes": (c_size_t, [ctypes.c_int64]),
    "detops_rle_string_count": (c_int, [_P, _P, ctypes.c_int64, c_int, _P, _P, c_size_t, _P]),
    "detops_rle_string_write": (c_int, [_P, _P, ctypes.c_int64, c_int, _P, _P, _P, c_size_t, _P]),
    "detops_rle_decode_workspace_bytes": (c_size_t, [ctypes.c_int64, c_int]),
    "detops_rle_decode_count": (c_int, [_P, _P, ctypes.c_int64, c_int, _P, _P, c_size_t, _P]),
    "detops_rle_decode_write": (c_int, [_P, _P, ctypes.c_int64, c_int, _P, ctypes.c_int64, _P, _P, _P, _P, c_size_t, _P]),
    "detops_polygon_mask_targets": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, _P, _P, c_int, c_int, _P, _P]),
    "detops_polygons_to_masks": (c_int, [_P, _P, _P] + [c_int] * 5 + [_P, _P]),
    "detops_image_batch_u8": (c_int, [_P, ctypes.c_int64, _P, _P, _P, c_int, _P] + [c_int] * 4 + [_P, _P]),
    "detops_color_jitter_u8": (c_int, [_P, ctypes.c_int64] + [_P] * 5 + [c_int, _P, c_size_t, _P]),
    "detops_bbox_aug_merge_workspace_bytes": (c_size_t, [c_int] * 3),
    "detops_bbox_aug_merge_count": (c_int, [_P, _P, _P] + [c_int] * 4 + [c_float, _P, _P, _P, c_size_t, _P]),
    "detops_bbox_aug_merge_write": (c_int, [_P] * 6 + [c_int] * 4 + [c_float, _P, ctypes.c_int64, _P, _P, _P, c_size_t, _P]),
    "detops_mask_pack": (c_int, [_P, _P, _P, c_int, ctypes.c_int64, _P, _P, _P, _P, _P]),
    "detops_mask_pack_rle_workspace_bytes": (c_size_t, [ctypes.c_int64]),
    "detops_mask_pack_rle": (c_int, [_P, _P, ctypes.c_int64, _P, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    "detops_mask_pair_counts": (c_int, [_P] * 11 + [c_int, ctypes.c_int64, _P, _P]),
    "detops_eval_iou": (c_int, [c_int] + [_P] * 9 + [c_int, ctypes.c_int64, _P, _P]),
    "detops_eval_match": (c_int, [c_int] + [_P] * 4 + [c_int, ctypes.c_int64, ctypes.c_int64, c_int] + [_P] * 4
                          + [c_int, _P, c_int] + [_P] * 5),
    "detops_eval_oks": (c_int, [_P] * 5 + [c_int] + [_P] * 3 + [c_int, ctypes.c_int64, ctypes.c_int64, _P, _P, _P]),
    "detops_eval_proposal_overlaps": (c_int, [_P] * 6 + [c_int] * 3 + [ctypes.c_int64] * 2 + [c_int, c_int, _P, _P]),
    "detops_window_counts": (c_int, [_P, _P, c_int, _P, _P] + [c_int] * 3 + [_P] * 5),
    "detops_roi_align_fpn_forward_nhwc_workspace_bytes": (c_size_t, [c_int]),
    "detops_roi_align_fpn_forward_nhwc_f32": (c_int, [_P, _P, _P, _P, c_int, _P, _P, c_int, _P] + [c_int] * 8 + [c_float] * 3 + [_P, c_size_t, _P]),
    "detops_roi_align_fpn_backward_ring_nhwc_f32": (c_int, [_P] * 7 + [c_int] * 8 + [_P, c_size_t, _P]),
    "detops_roi_align_fpn_backward_nhwc_workspace_bytes": (c_size_t, [_P, _P] + [c_int] * 6),
    "detops_roi_align_fpn_backward_nhwc_f32": (c_int, [_P, c_int, _P, _P, _P, _P, _P, _P] + [c_int] * 8 + [_P, c_size_t, _P]),
    "detops_fpn_topdown_forward": (c_int, [_P, _P, _P] + [c_int] * 6 + [_P]),
    "detops_fpn_topdown_backward": (c_int, [_P, _P] + [c_int] * 6 + [_P]),
    "detops_fpn_topdown_forward_nhwc": (c_int, [_P, _P, _P] + [c_int] * 7 + [_P]),
    "detops_fpn_topdown_backward_nhwc": (c_int, [_P, _P] + [c_int] * 7 + [_P]),
    "detops_pack_max_tensors": (c_int, []),
    "detops_pack_f32": (c_int, [_P, _P, _P, c_int, _P, _P]),
    "detops_bias_act_supported": (c_int, [c_int]),
    "detops_bias_act_backward_workspace_bytes": (c_size_t, [ctypes.c_int64, c_int]),
    "detops_bias_act_backward_nhwc_f32": (c_int, [_P, _P, _P, _P, ctypes.c_int64, c_int, c_int, _P, c_size_t, _P]),
    "detops_bias_act_backward_nhwc": (c_int, [_P, _P, _P, _P, c_int, ctypes.c_int64, c_int, c_int, _P, c_size_t, _P]),
    "detops_column_sum": (c_int, [_P, _P, c_int, ctypes.c_int64, c_int, _P, c_size_t, _P]),
    "detops_column_sum_workspace_bytes": (c_size_t, [ctypes.c_int64, c_int]),
    "detops_column_sum_f32": (c_int, [_P, _P, ctypes.c_int64, c_int, _P, c_size_t, _P]),
    "detops_group_norm_supported": (c_int, [c_int, c_int]),
    "detops_group_norm_workspace_bytes": (c_size_t, [c_int, ctypes.c_int64, c_int, c_int]),
    "detops_group_norm_forward_nhwc": (c_int, [_P] * 7 + [c_int, c_int, ctypes.c_int64, c_int, c_int, c_float, c_int, _P, c_size_t, _P]),
    "detops_group_norm_backward_nhwc": (c_int, [_P] * 10 + [c_int, c_int, ctypes.c_int64, c_int, c_int, c_int, _P, c_size_t, _P]),
    "detops_roi_align_forward_f64": (c_int, [_P, _P, _P] + [c_int] * 7 + [c_float, c_int, _P]),
    "detops_roi_align_backward_f64": (c_int, [_P, _P, _P] + [c_int] * 7 + [c_float, c_int, c_int, _P]),
    "detops_roi_pool_forward_f64": (c_int, [_P, _P, _P, _P] + [c_int] * 7 + [c_float, _P]),
    "detops_roi_pool_backward_f64": (c_int, [_P, _P, _P, _P] + [c_int] * 8 + [_P]),
    "detops_sigmoid_focal_loss_forward_f64": (c_int, [_P, _P, _P, c_int, c_int, c_float, c_float, _P]),
    "detops_sigmoid_focal_loss_backward_f64": (c_int, [_P, _P, _P, _P, c_int, c_int, c_float, c_float, _P]),
    "detops_nms_sorted_f64_workspace_bytes": (c_size_t, [c_int]),
    "detops_nms_sorted_f64": (c_int, [_P, c_int, c_float, _P, _P, c_size_t, _P]),
    "detops_roi_align_forward_cpu_f64": (c_int, [_P, _P, _P] + [c_int] * 7 + [c_float, c_int]),
    "detops_nms_cpu_f64": (c_int, [_P, _P, c_int, c_float, _P, _P]),
    "detops_debug_occupy": (c_int, [c_int, c_int, _P]),
    "detops_debug_nms_timeline": (c_int, [_P, c_int]),
    "detops_sgd_momentum_flat_f32": (c_int, [_P, _P, _P, ctypes.c_int64, ctypes.c_int64] + [c_float] * 5 + [_P]),
    "detops_rpn_decode_f32": (c_int, [_P] * 5 + [c_int] * 5 + [c_float] * 6 + [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, _P]),
    "detops_roi_pool_forward_f32": (c_int, [_P, _P, _P, _P] + [c_int] * 7 + [c_float, _P]),
    "detops_roi_pool_backward_f32": (c_int, [_P, _P, _P, _P] + [c_int] * 8 + [_P]),
    "detops_nms_workspace_bytes": (c_size_t, [c_int]),
    "detops_nms_f32": (c_int, [_P, _P, c_int, c_float, _P, _P, _P, c_size_t, _P]),
    "detops_nms_batched_workspace_bytes": (c_size_t, [c_int, c_int]),
    "detops_nms_batched_f32": (c_int, [_P, _P, _P, c_int, c_int, c_float, _P, _P, _P, c_size_t, _P]),
    "detops_nms_batched_mask_f32": (c_int, [_P, _P, _P, c_int, c_int, c_float, _P, _P, _P, c_size_t, _P]),
    "detops_nms_batched_status_f32": (c_int, [_P, _P, _P, c_int, c_int, c_float, _P, _P, _P, _P, _P, c_size_t, _P]),
    "detops_sigmoid_focal_loss_forward_f32": (c_int, [_P, _P, _P, c_int, c_int, c_float, c_float, _P]),
    "detops_sigmoid_focal_loss_backward_f32": (
        c_int, [_P, _P, _P, _P, c_int, c_int, c_float, c_float, _P]),
    "detops_sigmoid_focal_loss_backward_scalar_f32": (
        c_int, [_P, _P, _P, _P, c_int, c_int, c_float, c_float, _P]),
    "detops_sigmoid_focal_loss_forward_sum_f32": (
        c_int, [_P, _P, _P, _P, c_int, c_int, c_float, c_float, _P]),
    "detops_sigmoid_focal_loss_forward_partial_sums_f32": (
        c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_float, c_float, _P]),
    "detops_sigmoid_focal_loss_sum_workspace_bytes": (c_size_t, []),
    "detops_sigmoid_focal_loss_forward_sum_ws_f32": (
        c_int, [_P, _P, _P, _P, c_int, c_int, c_float, c_float, _P, c_size_t, _P]),
    "detops_frozen_bn_act_forward": (c_int, [_P, _P, _P, _P, _P] + [c_int] * 5 + [_P]),
    "detops_frozen_bn_act_backward": (c_int, [_P, _P, _P, _P, _P] + [c_int] * 5 + [_P]),
    "detops_frozen_bn_act_forward_nhwc": (c_int, [_P, _P, _P, _P, _P, c_int, ctypes.c_int64, c_int, c_int, _P]),
    "detops_frozen_bn_act_backward_nhwc": (c_int, [_P, _P, _P, _P, _P, c_int, ctypes.c_int64, c_int, c_int, _P]),
    "detops_conv1x1_frozen_bn_act_supported": (c_int, [c_int] * 8),
    "detops_conv1x1_frozen_bn_act_forward_nhwc_f32": (c_int, [_P] * 6 + [c_int] * 8 + [_P]),
    "detops_deformable_im2col": (c_int, [_P, _P, _P, _P] + [c_int] * 14 + [_P]),
    "detops_deformable_col2im": (c_int, [_P, _P, _P, _P] + [c_int] * 14 + [_P]),
    "detops_deformable_col2im_workspace_bytes": (c_size_t, [c_int] * 13),
    "detops_deformable_col2im_ws": (c_int, [_P, _P, _P, _P] + [c_int] * 14 + [_P, c_size_t, _P]),
    "detops_deform_conv_forward_fused_workspace_bytes": (c_size_t, [c_int] * 15),
    "detops_deform_conv_forward_fused": (c_int, [_P] * 6 + [c_int] * 15 + [_P, c_size_t, _P]),
    "detops_nchw_to_nhwc": (c_int, [_P, _P] + [c_int] * 4 + [_P]),
    "detops_deformable_nhwc_supported": (c_int, [c_int] * 4),
    "detops_deformable_im2col_nhwc": (c_int, [_P, _P, _P, _P] + [c_int] * 14 + [_P]),
    "detops_deformable_coord_nhwc": (c_int, [_P] * 6 + [c_int] * 14 + [_P]),
    "detops_deformable_transposed_sample_workspace_bytes": (c_size_t, [c_int] * 13),
    "detops_deformable_transposed_sample": (c_int, [_P, _P, _P, _P] + [c_int] * 15 + [_P, c_size_t, _P]),
    "detops_deformable_col2im_nhwc": (c_int, [_P, _P, _P, _P] + [c_int] * 14 + [_P, c_size_t, _P]),
    "detops_deformable_col2im_coord": (c_int, [_P, _P, _P, _P, _P, _P] + [c_int] * 14 + [_P]),
    "detops_deform_psroi_pool_forward_f32": (
        c_int, [_P] * 5 + [c_int] * 7 + [c_float] + [c_int] * 5 + [c_float, _P]),
    "detops_deform_psroi_pool_backward_f32": (
        c_int, [_P] * 7 + [c_int] * 7 + [c_float] + [c_int] * 5 + [c_float, c_int, _P]),
}


def bind(lib, require_all):
    """Set restype and argtypes of every table entry on the CDLL `lib`; -> the set of bound names.  require_all: a symbol
    the library does not export raises AttributeError; otherwise it is left out of the returned set."""
    bound = set()
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name) if require_all else getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
            bound.add(name)
    return bound
