"""ctypes binding of libfrcnn_hip.so (include/frcnn_hip.h).

The library is the product: there is NO CPU fallback.  Importing this module never touches
the GPU; the first compute call on a machine without the built library or without a HIP
device raises ``FrcnnError``.
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_int, c_size_t, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
# (FRCNN_LIB_PATH: another BUILD of this same library -- A/B runs of two kernel versions on one box; there is still no CPU fallback)
LIB_PATH = os.environ.get("FRCNN_LIB_PATH") or os.path.join(HERE, "libfrcnn_hip.so")


class FrcnnError(RuntimeError):
    pass


ABI_VERSION = 110       # include/frcnn_hip.h FRCNN_ABI_VERSION (tests/test_abi.py holds the two together)
P = c_void_p
I = c_int
F32 = ctypes.c_float
# name -> (restype, argtypes).  Must list every symbol include/frcnn_hip.h declares
# (tests/test_abi.py parses the header and checks this table and the .so against it).
SIGNATURES = {
    "frcnn_last_error": (c_char_p, []),
    "frcnn_version": (I, []),
    "frcnn_device_count": (I, []),
    "frcnn_preprocess_u8": (I, [P, c_size_t, P, P, P]),
    "frcnn_resize_cubic_taps": (I, [I, I, P]),
    "frcnn_resize_cubic_u8": (I, [P, I, I, P, P, I, I, I, P, P]),
    "frcnn_anchors_image": (I, [I, I, P, I, I, P, P]),
    "frcnn_anchors_conv": (I, [I, I, P, I, P, P]),
    "frcnn_cross_ious_f32": (I, [P, I, P, I, P, P]),
    "frcnn_cross_ious_i16": (I, [P, I, P, I, P, P]),
    "frcnn_rpn_assign_workspace_bytes": (c_size_t, [I, I, I, I]),
    "frcnn_rpn_assign": (I, [I, I, P, I, I, P, I, I, I, P, P, P, P, P, c_size_t, P]),
    "frcnn_rpn_sample_lists": (I, [P, P, I, P, P, P, P]),
    "frcnn_rpn_pack_targets": (I, [P, P, P, I, I, P, I, P, I, P, I, P, I, P, P, P]),
    "frcnn_host_mt_sample_range": (I, [P, P, I, I, I, P]),
    "frcnn_decode_proposals": (I, [P, I, I, P, I, P, P, P]),
    "frcnn_transform_inplace": (I, [P, P, I, P]),
    "frcnn_preprocess_u8_canvas": (I, [P, I, I, I, I, I, I, P, P, P]),
    "frcnn_zero_outside": (I, [P, I, I, I, I, P, P]),
    "frcnn_decode_proposals_canvas": (I, [P, I, I, P, I, P, P, P, P]),
    "frcnn_topk_workspace_bytes": (c_size_t, [I]),
    "frcnn_topk_order": (I, [P, P, I, I, P, P, P, c_size_t, P]),
    "frcnn_gather_candidates": (I, [P, P, P, P, I, P, P, P]),
    "frcnn_nms_workspace_bytes": (c_size_t, [I]),
    "frcnn_nms_i16": (I, [P, P, I, c_double, I, P, P, P, c_size_t, P]),
    "frcnn_nms_f64": (I, [P, P, I, c_double, I, P, P, P, c_size_t, P]),
    "frcnn_gather_rois": (I, [P, P, P, I, I, P, P]),
    "frcnn_roi_targets": (I, [P, I, P, P, P, I, I, P, P, P, P]),
    "frcnn_roi_crop_resize_fwd": (I, [P, I, I, I, P, I, I, P, P]),
    "frcnn_roi_crop_resize_fwd_ex": (I, [P, I, I, I, P, I, I, P, I, I, P, P]),
    "frcnn_roi_crop_resize_bwd": (I, [P, I, I, I, P, I, I, P, P]),
    "frcnn_conv_packed_k": (I, [I, I, I]),
    "frcnn_pack_conv_weights": (I, [P, I, I, I, I, P, P]),
    "frcnn_conv2d_fwd": (I, [P, P, P, P, P, P, P, P]),
    "frcnn_conv2d_config": (I, [P]),
    "frcnn_conv2d_fwd_masked": (I, [P, P, P, P, P, P, P, P, P]),
    "frcnn_conv2d_workspace_bytes": (c_size_t, [P]),
    "frcnn_conv2d_fwd_ws": (I, [P, P, P, P, P, P, P, P, P, c_size_t, P]),
    "frcnn_conv2d_dual_workspace_bytes": (c_size_t, [P]),
    "frcnn_conv2d_fwd_dual": (I, [P, P, P, P, P, P, I, I, P, I, P, c_size_t, P]),
    "frcnn_conv2d_dual_config": (I, [P, I]),
    "frcnn_conv2d_x6_config": (I, [P, I]),
    "frcnn_pack_conv_weights_x6": (I, [P, I, I, P, P]),
    "frcnn_refresh_x6_planes": (I, [P, I, P]),
    "frcnn_refresh_h3_planes": (I, [P, I, P]),
    "frcnn_conv2d_x6_workspace_bytes": (c_size_t, [P]),
    "frcnn_conv2d_fwd_x6": (I, [P, P, P, P, P, P, P, P, P, c_size_t, P]),
    "frcnn_conv2d_fwd_dual_x6": (I, [P, P, P, P, P, P, I, I, P, I, P]),
    "frcnn_conv2d_engine": (I, [P, I, I]),
    "frcnn_conv_h3_planes_bytes": (c_size_t, [I, I]),
    "frcnn_pack_conv_weights_h3": (I, [P, I, I, P, P]),
    "frcnn_amax_record_floats": (I, []),
    "frcnn_amax_clear": (I, [P, I, P]),
    "frcnn_amax_f32": (I, [P, c_size_t, P, P]),
    "frcnn_amax_merge": (I, [P, P, ctypes.c_float, P, P]),
    "frcnn_amax_status": (I, [P, I, P, P]),
    "frcnn_roi_crop_resize_fwd_planes": (I, [P, I, I, I, P, I, I, P, I, I, P, P]),
    "frcnn_roi_crop_resize_fwd_batch": (I, [P, I, I, I, P, I, I, I, P, I, I, P, P, P]),
    "frcnn_conv2d_h3_config": (I, [P, I]),
    "frcnn_conv2d_h3_workspace_bytes": (c_size_t, [P]),
    "frcnn_conv2d_fwd_h3": (I, [P, P, P, P, P, P, P, P, P, P, P, c_size_t, P]),
    "frcnn_conv2d_fwd_dual_h3": (I, [P, P, P, P, P, P, P, I, I, P, P, I, P, P]),
    "frcnn_stem_h3_packed_bytes": (c_size_t, []),
    "frcnn_pack_stem_weights_h3": (I, [P, P, P]),
    "frcnn_stem_h3_fwd": (I, [P, P, I, I, I, P, P, P, P, P, P]),
    "frcnn_conv2d_fwd_h3_planes": (I, [P, P, P, P, P, P, P, P, P, P, P, P, ctypes.c_float, ctypes.c_float, P]),
    "frcnn_conv2d_fwd_h3_planes_res": (I, [P, P, P, P, P, P, P, P, P, P, P, P, P, ctypes.c_float, ctypes.c_float, P]),
    "frcnn_conv2d_fwd_ws_amax": (I, [P, P, P, P, P, P, P, P, P, P, c_size_t, P]),
    "frcnn_pack_conv_weights_dgrad": (I, [P, P, I, I, I, I, P, P]),
    "frcnn_conv2d_wgrad_workspace_bytes": (c_size_t, [P]),
    "frcnn_conv2d_wgrad": (I, [P, P, P, P, P, P, P, c_size_t, P]),
    "frcnn_conv2d_wgrad_batch_workspace_bytes": (c_size_t, [P, I]),
    "frcnn_conv2d_wgrad_batch": (I, [P, I, P, c_size_t, P]),
    "frcnn_refresh_packed": (I, [P, I, P]),
    "frcnn_colsum_batch": (I, [P, I, P]),
    "frcnn_pool2d_fwd": (I, [P, I, I, I, I, I, I, I, P, P]),
    "frcnn_pool2d_fwd_planes": (I, [P, I, I, I, I, I, I, I, P, P]),
    "frcnn_avgpool_pos_major": (I, [P, I, I, I, P, P]),
    "frcnn_softmax_rows": (I, [P, I, I, I, P, I, P]),
    "frcnn_dense_heads_split": (I, [P, I, I, I, I, P, P, P]),
    "frcnn_loss_rpn_cls": (I, [P, P, I, I, P, P, P]),
    "frcnn_loss_rpn_reg": (I, [P, P, I, I, P, P, P]),
    "frcnn_loss_workspace_bytes": (ctypes.c_size_t, []),
    "frcnn_loss_rpn_cls_ws": (I, [P, P, I, I, P, P, P, P]),
    "frcnn_loss_rpn_reg_ws": (I, [P, P, I, I, P, P, P, P]),
    "frcnn_loss_det_cls": (I, [P, P, I, I, P, P, I, P]),
    "frcnn_loss_det_reg": (I, [P, P, I, I, P, P, I, P]),
    "frcnn_relu_bwd_inplace": (I, [P, P, c_size_t, P]),
    "frcnn_avgpool_bwd_masked": (I, [P, P, I, I, I, P, P]),
    "frcnn_maxpool_bwd": (I, [P, P, P, I, I, I, I, I, P, P]),
    "frcnn_sgd_momentum": (I, [P, P, P, c_size_t, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, P]),
    "frcnn_adam": (I, [P, P, P, P, c_size_t, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, I, ctypes.c_float, ctypes.c_float, P]),
    "frcnn_sumsq_workspace_bytes": (c_size_t, []),
    "frcnn_sumsq": (I, [P, c_size_t, P, P, c_size_t, P]),
    "frcnn_fold_bias": (I, [P, P, P, P, I, P]),
    "frcnn_stem_bf16_packed_elems": (I, []),
    "frcnn_pack_stem_weights_bf16": (I, [P, P, P]),
    "frcnn_stem_bf16_fwd": (I, [P, I, I, I, P, P, P, P, P]),
    "frcnn_conv_packed_k_bf16": (I, [I, I, I]),
    "frcnn_pack_conv_weights_bf16": (I, [P, I, I, I, I, P, P]),
    "frcnn_conv2d_fwd_bf16": (I, [P, P, P, P, P, P, P, I, P]),
    "frcnn_conv2d_workspace_bytes_bf16": (c_size_t, [P]),
    "frcnn_conv2d_fwd_bf16_ws": (I, [P, P, P, P, P, P, P, I, P, c_size_t, P]),
    "frcnn_conv2d_fwd_bf16_masked": (I, [P, P, P, P, P, P, P, P, I, P, c_size_t, P]),
    "frcnn_refresh_packed_bf16": (I, [P, I, P]),
    "frcnn_conv2d_wgrad_bf16": (I, [P, P, P, P, P, P, P, c_size_t, P]),
    "frcnn_cast_bf16_to_f32": (I, [P, c_size_t, P, P]),
    "frcnn_relu_bwd_inplace_bf16": (I, [P, P, c_size_t, P]),
    "frcnn_avgpool_bwd_masked_bf16": (I, [P, P, I, I, I, P, P]),
    "frcnn_roi_crop_resize_bwd_bf16": (I, [P, I, I, I, P, I, I, P, P]),
    "frcnn_cast_f32_to_bf16": (I, [P, c_size_t, P, P]),
    "frcnn_avgpool_bf16_to_f32": (I, [P, I, I, I, P, P]),
    "frcnn_avgpool_bf16_to_f32_ex": (I, [P, I, I, I, I, P, P]),
    "frcnn_roi_crop_resize_fwd_bf16": (I, [P, I, I, I, P, I, I, P, P]),
    "frcnn_roi_crop_resize_fwd_bf16_ex": (I, [P, I, I, I, P, I, I, P, I, I, P, P]),
    "frcnn_roi_crop_resize_fwd_bf16_batch": (I, [P, I, I, I, I, P, I, I, P, I, I, P, P]),
    "frcnn_detections": (I, [P, P, I, P, P, I, I, c_double, c_double, c_double, c_double, P, P, P, P, P, P]),
    "frcnn_detections_dyn": (I, [P, P, I, I, P, P, I, I, c_double, c_double, P, P, P, P, P, P, P]),
    "frcnn_annotate_u8": (I, [P, I, I, P, P, P, P, I, P, P, I, I, P, P]),
    "frcnn_vgg_conv1_bf16_packed_elems": (I, []),
    "frcnn_pack_vgg_conv1_weights_bf16": (I, [P, P, P]),
    "frcnn_vgg_conv1_bf16_fwd": (I, [P, I, I, I, P, P, P, P]),
    "frcnn_pool2d_fwd_bf16": (I, [P, I, I, I, I, I, I, P, P]),
}

# Extensions: entry points of the same library declared in headers of their own under include/ext/, each with its own revision (the
# table above and ABI_VERSION are include/frcnn_hip.h's and stay as they are).  load() binds them too.
VGG_CANVAS_VERSION = 1  # include/ext/frcnn_hip_vgg_canvas.h FRCNN_VGG_CANVAS_VERSION
EXT_SIGNATURES = {
    "frcnn_vgg_canvas_version": (I, []),
    "frcnn_pool2d_fwd_extents": (I, [P, I, I, I, I, P, P, P]),
    "frcnn_pool2d_fwd_bf16_extents": (I, [P, I, I, I, I, P, P, P]),
    "frcnn_vgg_conv1_bf16_fwd_extents": (I, [P, I, I, I, P, P, P, P, P]),
}

ROI_RES_VERSION = 1     # include/ext/frcnn_hip_roi_res.h FRCNN_ROI_RES_VERSION
ROI_TAP_BYTES = 32      # ... FRCNN_ROI_TAP_BYTES
ROI_RES_SIGNATURES = {
    "frcnn_roi_res_version": (I, []),
    "frcnn_roi_tap_table": (I, [I, I, I, P, I, I, I, I, I, P, P]),
    "frcnn_conv2d_roi_res_available": (I, [P, I, I]),
    "frcnn_conv2d_fwd_h3_roi_res": (I, [P, P, P, P, P, P, P, P, P, P, P, P, ctypes.c_float, ctypes.c_float, P]),
}


POOL_EPILOGUE_VERSION = 1     # include/ext/frcnn_hip_pool_epilogue.h FRCNN_POOL_EPILOGUE_VERSION
POOL_EPILOGUE_SIGNATURES = {
    "frcnn_pool_epilogue_version": (I, []),
    "frcnn_conv2d_pool_available": (I, [P, I, I, I]),
    "frcnn_conv2d_fwd_h3_pool": (I, [P, P, P, P, P, P, P, P, P, P, I, P, P, P, P]),
}


ROWMAP_VERSION = 1            # include/ext/frcnn_hip_rowmap.h FRCNN_ROWMAP_VERSION
ROWMAP_TILE_ROWS = 256        # the row tile of the one launch form that reads a map (frcnn_conv2d_rowmap_available)
ROWMAP_SIGNATURES = {
    "frcnn_rowmap_version": (I, []),
    "frcnn_conv_rowmap_build": (I, [P, I, I, P, c_size_t, P, c_size_t, P, P]),
    "frcnn_conv2d_rowmap_available": (I, [P, I, I]),
    "frcnn_conv2d_fwd_h3_rowmap": (I, [P, P, P, P, P, P, P, P, P, ctypes.c_float, ctypes.c_float, P, P]),
}


class RowMap(ctypes.Structure):
    """frcnn_rowmap (include/ext/frcnn_hip_rowmap.h)."""
    _fields_ = [("row_map", c_void_p), ("tile_taps", c_void_p), ("rows", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class RoiRes(ctypes.Structure):
    """frcnn_roi_res (include/ext/frcnn_hip_roi_res.h)."""
    _fields_ = [("map", c_void_p), ("taps", c_void_p), ("fill", c_void_p), ("map_rows", ctypes.c_int32), ("reserved", ctypes.c_int32)]


PNG_VERSION = 1         # include/ext/frcnn_hip_png.h FRCNN_PNG_VERSION
PNG_SIGNATURES = {
    "frcnn_png_version": (I, []),
    "frcnn_png_band_rows": (I, []),
    "frcnn_png_bound": (c_size_t, [I, I]),
    "frcnn_png_workspace_bytes": (c_size_t, [I, I]),
    "frcnn_png_encode_u8": (I, [P, I, I, I, P, c_size_t, P, P, P]),
}

PNG_HUFF_VERSION = 1    # include/ext/frcnn_hip_png_huff.h FRCNN_PNG_HUFF_VERSION
PNG_HUFF_SIGNATURES = {
    "frcnn_png_huff_version": (I, []),
    "frcnn_png_huff_band_rows": (I, []),
    "frcnn_png_huff_bound": (c_size_t, [I, I]),
    "frcnn_png_huff_workspace_bytes": (c_size_t, [I, I]),
    "frcnn_png_huff_encode_u8": (I, [P, I, I, I, P, c_size_t, P, P, P]),
}

JPEG_VERSION = 1        # include/ext/frcnn_hip_jpeg.h FRCNN_JPEG_VERSION
JPEG_SIGNATURES = {
    "frcnn_jpeg_version": (I, []),
    "frcnn_jpeg_restart_mcus": (I, []),
    "frcnn_jpeg_header_bytes": (c_size_t, []),
    "frcnn_jpeg_bound": (c_size_t, [I, I]),
    "frcnn_jpeg_workspace_bytes": (c_size_t, [I, I]),
    "frcnn_jpeg_encode_u8": (I, [P, I, I, I, I, P, c_size_t, P, P, P]),
}

JPEG_OPT_VERSION = 1    # include/ext/frcnn_hip_jpeg_opt.h FRCNN_JPEG_OPT_VERSION
JPEG_OPT_SIGNATURES = {
    "frcnn_jpeg_opt_version": (I, []),
    "frcnn_jpeg_opt_restart_mcus": (I, [I]),
    "frcnn_jpeg_opt_bound": (c_size_t, [I, I, I]),
    "frcnn_jpeg_opt_workspace_bytes": (c_size_t, [I, I, I, I]),
    "frcnn_jpeg_opt_encode_u8": (I, [P, I, I, I, I, I, I, P, c_size_t, P, P, P]),
    "frcnn_jpeg_opt_build_tables": (I, [P, P, P]),
}
JPEG_OPT_SUBSAMPLINGS = (444, 420)                              # FRCNN_JPEG_OPT_444 / _420
JPEG_OPT_HUFFMANS = {"standard": 0, "optimized": 1}             # FRCNN_JPEG_OPT_STANDARD / _OPTIMIZED


class JpegOptTable(ctypes.Structure):
    """frcnn_jpeg_opt_table_t (include/ext/frcnn_hip_jpeg_opt.h)."""
    _fields_ = [("bits", ctypes.c_uint8 * 16), ("huffval", ctypes.c_uint8 * 256), ("count", ctypes.c_uint32)]


JPEG_DEC_VERSION = 1    # include/ext/frcnn_hip_jpeg_dec.h FRCNN_JPEG_DEC_VERSION
JPEG_DEC_SIGNATURES = {
    "frcnn_jpeg_dec_version": (I, []),
    "frcnn_jpeg_dec_plan": (I, [P, c_size_t, P]),
    "frcnn_jpeg_dec_workspace_bytes": (c_size_t, [P]),
    "frcnn_jpeg_decode_u8": (I, [P, P, I, P, c_size_t, P, P, P]),
}
JPEG_DEC_BATCH_VERSION = 1      # include/ext/frcnn_hip_jpeg_dec_batch.h FRCNN_JPEG_DEC_BATCH_VERSION
JPEG_DEC_BATCH_MAX = 64         # ... FRCNN_JPEG_DEC_BATCH_MAX
JPEG_DEC_BATCH_SIGNATURES = {
    "frcnn_jpeg_dec_batch_version": (I, []),
    "frcnn_jpeg_dec_batch_layout": (c_size_t, [P, I, P]),
    "frcnn_jpeg_decode_batch_u8": (I, [P, P, I, P, c_size_t, I, P, c_size_t, P, P, c_size_t, P]),
}
E_UNSUPPORTED = -4     # include/frcnn_hip.h FRCNN_E_UNSUPPORTED
JPEG_DEC_BLOCKS, JPEG_DEC_ZIGZAG, JPEG_DEC_CODE, JPEG_DEC_TABLE = 1, 2, 4, 8     # FRCNN_JPEG_DEC_* status bits


PNG_DEC_VERSION = 1     # include/ext/frcnn_hip_png_dec.h FRCNN_PNG_DEC_VERSION
PNG_DEC_BATCH_MAX = 64  # ... FRCNN_PNG_DEC_BATCH_MAX
PNG_DEC_WINDOW_BYTES = 8192     # ... FRCNN_PNG_DEC_WINDOW_BYTES: compressed bytes per window of the inflate kernel
PNG_DEC_MAX_STREAM = 1 << 24    # ... FRCNN_PNG_DEC_MAX_STREAM
PNG_DEC_SIGNATURES = {
    "frcnn_png_dec_version": (I, []),
    "frcnn_png_dec_plan": (I, [P, c_size_t, P]),
    "frcnn_png_dec_spans": (I, [P, c_size_t, P, P, c_size_t]),
    "frcnn_png_dec_workspace_bytes": (c_size_t, [P]),
    "frcnn_png_dec_batch_layout": (c_size_t, [P, I, P]),
    "frcnn_png_decode_batch_u8": (I, [P, P, I, P, c_size_t, I, P, c_size_t, P, P, c_size_t, P]),
}
# FRCNN_PNG_DEC_* status bits
PNG_DEC_CODE, PNG_DEC_BLOCK, PNG_DEC_OVERSUBSCRIBED, PNG_DEC_DISTANCE, PNG_DEC_OVERRUN, PNG_DEC_UNDERRUN, PNG_DEC_ADLER, PNG_DEC_FILTER = \
    1, 2, 4, 8, 16, 32, 64, 128


class PngDecPlan(ctypes.Structure):
    """frcnn_png_dec_plan_t (include/ext/frcnn_hip_png_dec.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("h", "w", "channels")] + \
               [(k, ctypes.c_uint32) for k in ("file_len", "idat_off", "idat_count", "stream_len", "inflated_len")]


class PngDecBatchItem(ctypes.Structure):
    """frcnn_png_dec_batch_item_t (include/ext/frcnn_hip_png_dec.h)."""
    _fields_ = [("plan", PngDecPlan), ("file_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("ws_off", ctypes.c_uint64)]


PNG_DEC_FULL_VERSION = 1        # include/ext/frcnn_hip_png_dec_full.h FRCNN_PNG_DEC_FULL_VERSION
PNG_DEC_FULL_PLTE_BYTES = 768   # ... FRCNN_PNG_DEC_FULL_PLTE_BYTES: the staged palette of a colour-type-3 file
PNG_DEC_FULL_SIGNATURES = {
    "frcnn_png_dec_full_version": (I, []),
    "frcnn_png_dec_full_plan": (I, [P, c_size_t, P]),
    "frcnn_png_dec_full_spans": (I, [P, c_size_t, P, P, c_size_t]),
    "frcnn_png_dec_full_workspace_bytes": (c_size_t, [P]),
    "frcnn_png_dec_full_batch_layout": (c_size_t, [P, I, P]),
    "frcnn_png_decode_full_batch_u8": (I, [P, P, I, P, c_size_t, I, P, c_size_t, P, P, c_size_t, P]),
}


class PngDecFullPlan(ctypes.Structure):
    """frcnn_png_dec_full_plan_t (include/ext/frcnn_hip_png_dec_full.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("h", "w", "colour_type", "bit_depth", "interlace")] + \
               [(k, ctypes.c_uint32) for k in ("file_len", "idat_off", "idat_count", "stream_len", "inflated_len", "plte_off", "plte_entries")]


class PngDecFullBatchItem(ctypes.Structure):
    """frcnn_png_dec_full_batch_item_t (include/ext/frcnn_hip_png_dec_full.h)."""
    _fields_ = [("plan", PngDecFullPlan), ("file_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("ws_off", ctypes.c_uint64),
                ("plte_off", ctypes.c_uint64)]


class JpegDecPlan(ctypes.Structure):
    """frcnn_jpeg_dec_plan_t (include/ext/frcnn_hip_jpeg_dec.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("h", "w", "components", "hs", "vs", "mcus_x", "mcus_y", "blocks_per_mcu")] + \
               [(k, ctypes.c_uint32) for k in ("expected_blocks", "restart_interval", "file_len", "scan_off", "scan_len")] + \
               [("dqt_off", ctypes.c_uint32 * 3), ("dht_off", ctypes.c_uint32 * 2 * 2), ("dht_count", ctypes.c_uint32 * 2 * 2),
                ("comp_dc", ctypes.c_uint8 * 4), ("comp_ac", ctypes.c_uint8 * 4),
                ("subsequence_bytes", ctypes.c_uint32), ("subsequences", ctypes.c_uint32)]


class JpegDecBatchItem(ctypes.Structure):
    """frcnn_jpeg_dec_batch_item_t (include/ext/frcnn_hip_jpeg_dec_batch.h)."""
    _fields_ = [("plan", JpegDecPlan), ("file_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("ws_off", ctypes.c_uint64)]


JPEG_DEC_FULL_VERSION = 1       # include/ext/frcnn_hip_jpeg_dec_full.h FRCNN_JPEG_DEC_FULL_VERSION
JPEG_DEC_FULL_MAX_SCANS = 64    # ... FRCNN_JPEG_DEC_FULL_MAX_SCANS
JPEG_DEC_FULL_SIGNATURES = {
    "frcnn_jpeg_dec_full_version": (I, []),
    "frcnn_jpeg_dec_full_plan": (I, [P, c_size_t, P]),
    "frcnn_jpeg_dec_full_workspace_bytes": (c_size_t, [P]),
    "frcnn_jpeg_dec_full_batch_layout": (c_size_t, [P, I, P]),
    "frcnn_jpeg_decode_full_batch_u8": (I, [P, P, I, P, c_size_t, I, P, c_size_t, P, P, c_size_t, P]),
    "frcnn_jpeg_decode_full_u8": (I, [P, P, P, I, P, c_size_t, P, P, c_size_t, P]),
}
# FRCNN_JPEG_DEC_FULL_* status bits
JPEG_DEC_FULL_BLOCKS, JPEG_DEC_FULL_ZIGZAG, JPEG_DEC_FULL_CODE, JPEG_DEC_FULL_TABLE, JPEG_DEC_FULL_EOBRUN = 1, 2, 4, 8, 16


class JpegDecFullScan(ctypes.Structure):
    """frcnn_jpeg_dec_full_scan_t (include/ext/frcnn_hip_jpeg_dec_full.h)."""
    _fields_ = [(k, ctypes.c_uint32) for k in ("off", "len", "restart_interval", "subsequence_bytes", "subsequences")] + \
               [(k, ctypes.c_uint32 * 3) for k in ("dc_off", "dc_count", "ac_off", "ac_count")] + \
               [(k, ctypes.c_uint8) for k in ("comps", "ss", "se", "ah", "al")] + [("reserved", ctypes.c_uint8 * 3)]


class JpegDecFullPlan(ctypes.Structure):
    """frcnn_jpeg_dec_full_plan_t (include/ext/frcnn_hip_jpeg_dec_full.h).  ``h`` / ``w`` / ``file_len``: the frame's, under the names
    every decoder's plan has them."""
    _fields_ = [("frame", JpegDecPlan), ("scans", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("scan", JpegDecFullScan * JPEG_DEC_FULL_MAX_SCANS)]
    h = property(lambda self: self.frame.h)
    w = property(lambda self: self.frame.w)
    file_len = property(lambda self: self.frame.file_len)


class JpegDecFullBatchItem(ctypes.Structure):
    """frcnn_jpeg_dec_full_batch_item_t (include/ext/frcnn_hip_jpeg_dec_full.h)."""
    _fields_ = [("plan", JpegDecFullPlan), ("file_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("ws_off", ctypes.c_uint64)]


Y4M_VERSION = 1                 # include/ext/frcnn_hip_y4m.h FRCNN_Y4M_VERSION
Y4M_BATCH_MAX = 64              # ... FRCNN_Y4M_BATCH_MAX
Y4M_MAX_SIDE = 32768            # ... FRCNN_Y4M_MAX_SIDE
Y4M_SIGNATURES = {
    "frcnn_y4m_version": (I, []),
    "frcnn_y4m_frame_bytes": (c_size_t, [I, I, I]),
    "frcnn_y4m_decode_batch_u8": (I, [P, P, I, P, c_size_t, I, P, c_size_t, P, P, c_size_t, P]),
    "frcnn_y4m_decode_u8": (I, [P, c_size_t, P, I, P, c_size_t, P]),
    "frcnn_y4m_encode_u8": (I, [P, c_size_t, I, I, I, I, I, I, P, c_size_t, c_size_t, P]),
}
Y4M_CHROMAS = {"420jpeg": 0, "420mpeg2": 1, "422": 2, "444": 3, "mono": 4}      # FRCNN_Y4M_C*
Y4M_OUT_CHROMAS = ("420jpeg", "444")
Y4M_RANGES = {"limited": 0, "full": 1}                                          # FRCNN_Y4M_LIMITED / _FULL


class Y4mPlan(ctypes.Structure):
    """frcnn_y4m_plan_t (include/ext/frcnn_hip_y4m.h).  ``y4m.parse_header`` hangs the stream's tags on the instance (``tags``,
    ``header_len``): Python attributes beside the C fields, which is all that travels to the device."""
    _fields_ = [(k, ctypes.c_int32) for k in ("h", "w", "chroma", "range")] + [(k, ctypes.c_uint32) for k in ("frame_bytes", "reserved")]
    chroma_name = property(lambda self: next(k for k, v in Y4M_CHROMAS.items() if v == self.chroma))
    range_name = property(lambda self: next(k for k, v in Y4M_RANGES.items() if v == self.range))


class Y4mBatchItem(ctypes.Structure):
    """frcnn_y4m_batch_item_t (include/ext/frcnn_hip_y4m.h)."""
    _fields_ = [("plan", Y4mPlan), ("file_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("ws_off", ctypes.c_uint64)]


REDACT_VERSION = 1              # include/ext/frcnn_hip_redact.h FRCNN_REDACT_VERSION
REDACT_MAX_ROWS = 512           # ... FRCNN_REDACT_MAX_ROWS
REDACT_MAX_SIDE = 32768         # ... FRCNN_REDACT_MAX_SIDE
REDACT_SIGNATURES = {
    "frcnn_redact_version": (I, []),
    "frcnn_redact_ws_bytes": (c_size_t, [I, I, I, I]),
    "frcnn_redact_u8": (I, [P, I, I, P, P, P, I, P, I, I, I, I, P, c_size_t, P]),
}
REDACT_MODES = {"fill": 0, "pixelate": 1, "blur": 2}                               # FRCNN_REDACT_FILL / _PIXELATE / _BLUR
# mode -> (smallest size, largest size, the default): FRCNN_REDACT_PIXELATE_MIN / _MAX, FRCNN_REDACT_BLUR_MIN / _MAX; fill takes none (0)
REDACT_SIZES = {"fill": (0, 0, 0), "pixelate": (2, 64, 16), "blur": (1, 32, 12)}

REDACT_SHAPE_VERSION = 1        # include/ext/frcnn_hip_redact_shape.h FRCNN_REDACT_SHAPE_VERSION
REDACT_SHAPE_SIGNATURES = {
    "frcnn_redact_shape_version": (I, []),
    "frcnn_redact_shaped_u8": (I, [P, I, I, P, P, P, I, P, I, I, I, I, I, I, P, c_size_t, P]),
}
REDACT_SHAPES = {"box": 0, "ellipse": 1}                                           # FRCNN_REDACT_SHAPE_BOX / _ELLIPSE
REDACT_FEATHER = (0, 32)                                                           # 0..FRCNN_REDACT_FEATHER_MAX

REDACT_REGION_VERSION = 1       # include/ext/frcnn_hip_redact_region.h FRCNN_REDACT_REGION_VERSION
REDACT_REGION_SIGNATURES = {
    "frcnn_redact_region_version": (I, []),
    "frcnn_redact_region_plane_bytes": (c_size_t, [I, I]),
    "frcnn_redact_region_build": (I, [P, I, I, P, P, I, P, I, P]),
    "frcnn_redact_region_prepare": (I, [P, I, I, P, I, I, P, c_size_t, P]),
    "frcnn_redact_region_apply_u8": (I, [P, I, I, P, I, I, P, c_size_t, P]),
}
REDACT_REGION_MAX = 8                                                              # FRCNN_REDACT_REGION_MAX
REDACT_REGION_FEATHER = (0, 32)                                                    # 0..FRCNN_REDACT_REGION_FEATHER_MAX
REDACT_REGION_HEAD_WORDS = 8                                                       # FRCNN_REDACT_REGION_HEAD_WORDS

REDACT_MOVING_VERSION = 1       # include/ext/frcnn_hip_redact_moving.h FRCNN_REDACT_MOVING_VERSION
REDACT_MOVING_SIGNATURES = {
    "frcnn_redact_moving_version": (I, []),
    "frcnn_redact_moving_state_bytes": (c_size_t, [I, I]),
    "frcnn_redact_moving_build": (I, [P, P, P, I, I, P, P, P, I, I, P, I, I, I, I, I, I, I, I, I, P, P, P, P]),
}
# (smallest, largest, the default) tolerance D, vote K, hold H, grow G and feather F (FRCNN_REDACT_MOVING_*): the defaults of the first
# four are PROVISIONAL, not measured on real footage
REDACT_MOVING_TOL = (0, 255, 24)
REDACT_MOVING_VOTE = (1, 64, 8)
REDACT_MOVING_HOLD = (0, 255, 4)
REDACT_MOVING_GROW = (0, 32, 8)
REDACT_MOVING_FEATHER = (0, 32, 0)
REDACT_MOVING_CELL = 8                                                             # FRCNN_REDACT_MOVING_CELL
REDACT_MOVING_STATS_WORDS = 4                                                      # FRCNN_REDACT_MOVING_STATS_WORDS

TRACK_VERSION = 1               # include/ext/frcnn_hip_track.h FRCNN_TRACK_VERSION
TRACK_MAX = 128                 # ... FRCNN_TRACK_MAX: slots of a state
TRACK_MAX_FRAMES = 64           # ... FRCNN_TRACK_MAX_FRAMES: frames of one call
TRACK_SIGNATURES = {
    "frcnn_track_version": (I, []),
    "frcnn_track_state_bytes": (c_size_t, [I]),
    "frcnn_track_update": (I, [P, I, P, ctypes.c_longlong, I, P, I, P, I, I, I, I, I, I, P, ctypes.c_longlong, P]),
    "frcnn_annotate_ids_u8": (I, [P, I, I, P, P, P, P, P, I, P, P, I, I, P, P]),
}
# (thr, hold, grow): the defaults, and the range of each (FRCNN_TRACK_MAX_HOLD, FRCNN_TRACK_MAX_GROW)
TRACK_DEFAULTS = (30, 8, 0)
TRACK_RANGES = ((1, 100), (0, 255), (0, 64))

TRACK_MOTION_VERSION = 1        # include/ext/frcnn_hip_track_motion.h FRCNN_TRACK_MOTION_VERSION
TRACK_MOTION_SIGNATURES = {
    "frcnn_track_motion_version": (I, []),
    "frcnn_track_motion_state_bytes": (c_size_t, [I, I]),
    "frcnn_track_update_motion": (I, [P, I, P, P, ctypes.c_longlong, P, ctypes.c_longlong, I, P, I, P, I, I, I, I, I, I, I, P,
                                      ctypes.c_longlong, P]),
}
# the block match's search radius: (smallest, largest, the default) (FRCNN_TRACK_MOTION_MIN_RADIUS / _MAX_RADIUS)
TRACK_MOTION_RADIUS = (1, 16, 8)

TRACK_INTERVAL_VERSION = 1      # include/ext/frcnn_hip_track_interval.h FRCNN_TRACK_INTERVAL_VERSION
TRACK_INTERVAL_SIGNATURES = {
    "frcnn_track_interval_version": (I, []),
    "frcnn_track_update_interval": (I, [P, I, P, P, ctypes.c_longlong, P, ctypes.c_longlong, I, P, I, P, I, I, I, I, I, I, I, I, P,
                                        ctypes.c_longlong, P]),
}
# frames from one key frame to the next: (smallest at the ABI, largest) (FRCNN_TRACK_INTERVAL_MIN / _MAX); the public option starts at 2
TRACK_INTERVAL = (1, 16)

TRACK_CUT_VERSION = 1           # include/ext/frcnn_hip_track_cut.h FRCNN_TRACK_CUT_VERSION
TRACK_CUT_SIGNATURES = {
    "frcnn_track_cut_version": (I, []),
    "frcnn_track_cut_workspace_bytes": (c_size_t, [I]),
    "frcnn_track_update_cut": (I, [P, I, P, P, ctypes.c_longlong, P, ctypes.c_longlong, I, P, I, P, I, I, I, I, I, I, I, I, P,
                                   ctypes.c_longlong, I, P, P, P]),
}
# the share of the largest signature distance at which a frame is a cut, in percent: (smallest, largest, the default)
# (FRCNN_TRACK_CUT_MIN_PCT / _MAX_PCT; the default is provisional: no threshold has been measured on real footage)
TRACK_CUT_PCT = (1, 100, 40)

TRACK_WEAK_VERSION = 1          # include/ext/frcnn_hip_track_weak.h FRCNN_TRACK_WEAK_VERSION
# each parent's signature with ``float strong`` in front of ``out``
TRACK_WEAK_SIGNATURES = {
    "frcnn_track_weak_version": (I, []),
    "frcnn_track_update_weak": (I, [P, I, P, ctypes.c_longlong, I, P, I, P, I, I, I, I, I, I, F32, P, ctypes.c_longlong, P]),
    "frcnn_track_update_motion_weak": (I, [P, I, P, P, ctypes.c_longlong, P, ctypes.c_longlong, I, P, I, P, I, I, I, I, I, I, I, F32, P,
                                           ctypes.c_longlong, P]),
    "frcnn_track_update_interval_weak": (I, [P, I, P, P, ctypes.c_longlong, P, ctypes.c_longlong, I, P, I, P, I, I, I, I, I, I, I, I, F32, P,
                                             ctypes.c_longlong, P]),
    "frcnn_track_update_cut_weak": (I, [P, I, P, P, ctypes.c_longlong, P, ctypes.c_longlong, I, P, I, P, I, I, I, I, I, I, I, I, F32, P,
                                        ctypes.c_longlong, I, P, P, P]),
}

TRACK_TRAILS_VERSION = 1        # include/ext/frcnn_hip_track_trails.h FRCNN_TRACK_TRAILS_VERSION
TRACK_TRAILS_SIGNATURES = {
    "frcnn_track_trails_version": (I, []),
    "frcnn_track_trails_state_bytes": (c_size_t, [I, I]),
    "frcnn_track_trails_list_words": (c_size_t, [I, I]),
    "frcnn_track_trails_update": (I, [P, I, P, ctypes.c_longlong, I, I, P, P, I, I, I, I, P, P]),
    "frcnn_track_trails_draw_u8": (I, [P, I, I, P, I, I, I, P]),
}
# the points a trail keeps and the width it is drawn with, each (smallest, largest, the default), and the largest expiry in frames
# (FRCNN_TRACK_TRAILS_MIN_LENGTH / _MAX_LENGTH, 1 / _MAX_WIDTH, _MAX_EXPIRE)
TRACK_TRAILS = ((2, 64, 16), (1, 9, 3), 4095)

HEAT_VERSION = 1                # include/ext/frcnn_hip_heat.h FRCNN_HEAT_VERSION
HEAT_SIGNATURES = {
    "frcnn_heat_version": (I, []),
    "frcnn_heat_state_bytes": (c_size_t, [I, I]),
    "frcnn_heat_update": (I, [P, I, I, P, I, I, P, I, I, I, P, P, P]),
    "frcnn_heat_draw_u8": (I, [P, I, I, P, I, I, P]),
}
# (smallest, largest, the default) alpha and decay (1 / 255 / FRCNN_HEAT_DEFAULT_ALPHA, 0 / FRCNN_HEAT_MAX_DECAY / 0), the value a pixel stops
# at (FRCNN_HEAT_MAX), the frame indices of a call (FRCNN_HEAT_MAX_FRAMES) and the update kernel's tile (FRCNN_HEAT_TILE_W, _TILE_H)
HEAT_ALPHA = (1, 255, 160)
HEAT_DECAY = (0, 15, 0)
HEAT_MAX = 1 << 30
HEAT_MAX_FRAMES = 65536
HEAT_TILE = (64, 16)

COUNT_VERSION = 1               # include/ext/frcnn_hip_count.h FRCNN_COUNT_VERSION
COUNT_SIGNATURES = {
    "frcnn_count_version": (I, []),
    "frcnn_count_state_bytes": (c_size_t, [I]),
    "frcnn_count_list_words": (c_size_t, []),
    "frcnn_count_update": (I, [P, I, P, ctypes.c_longlong, I, I, P, P, P, I, P, I, I, I, I, P, P]),
    "frcnn_count_draw_u8": (I, [P, I, I, P, P, I, I, I, P]),
}
# the counting lines of a call at most, the events a frame's list holds (FRCNN_COUNT_MAX_LINES, _MAX_EVENTS), the range of a line's
# coordinates (_MIN_COORD, _MAX_COORD), (smallest, largest, the default) width (1 / _MAX_WIDTH / _DEFAULT_WIDTH), the largest expiry in
# frames (_MAX_EXPIRE) and the words of a count list (_LIST_WORDS)
COUNT_MAX_LINES = 8
COUNT_MAX_EVENTS = 64
COUNT_COORD = (-32768, 65535)
COUNT_WIDTH = (1, 9, 3)
COUNT_MAX_EXPIRE = 4095
COUNT_LIST_WORDS = 4 + 2 * COUNT_MAX_LINES + 4 * COUNT_MAX_EVENTS

ZONE_VERSION = 1                # include/ext/frcnn_hip_zone.h FRCNN_ZONE_VERSION
ZONE_SIGNATURES = {
    "frcnn_zone_version": (I, []),
    "frcnn_zone_state_bytes": (c_size_t, [I]),
    "frcnn_zone_list_words": (c_size_t, []),
    "frcnn_zone_update": (I, [P, I, P, ctypes.c_longlong, I, I, P, P, P, P, I, P, I, I, I, I, I, P, P]),
    "frcnn_zone_draw_u8": (I, [P, I, I, P, P, P, I, I, I, P]),
}
# the zones of a call at most, (fewest, most) vertices of one, the events a frame's list holds (FRCNN_ZONE_MAX_ZONES, _MIN_VERTS /
# _MAX_VERTS, _MAX_EVENTS), the range of a coordinate (_MIN_COORD, _MAX_COORD), (smallest, largest, the default) width (1 / _MAX_WIDTH /
# _DEFAULT_WIDTH), the largest expiry in frames (_MAX_EXPIRE), where a zone's dwell stops (_MAX_DWELL), and the words of a state's
# header, of an entry and of a zone list (_HEAD_WORDS, _ENTRY_WORDS, _LIST_WORDS)
ZONE_MAX_ZONES = 8
ZONE_VERTS = (3, 16)
ZONE_MAX_EVENTS = 64
ZONE_COORD = (-32768, 65535)
ZONE_WIDTH = (1, 9, 3)
ZONE_MAX_EXPIRE = 4095
ZONE_MAX_DWELL = 1 << 30
ZONE_HEAD_WORDS = 4 + 4 * ZONE_MAX_ZONES
ZONE_ENTRY_WORDS = 5 + ZONE_MAX_ZONES
ZONE_LIST_WORDS = 4 + 5 * ZONE_MAX_ZONES + 5 * ZONE_MAX_EVENTS

PLATE_VERSION = 1               # include/ext/frcnn_hip_plate.h FRCNN_PLATE_VERSION
PLATE_SIGNATURES = {
    "frcnn_plate_version": (I, []),
    "frcnn_plate_state_bytes": (c_size_t, [I, I]),
    "frcnn_plate_update": (I, [P, I, I, P, P, I, I, I, I, I, I, P, P, P, P]),
    "frcnn_plate_fill_u8": (I, [P, I, I, P, P, I, I, P, I, I, I, P]),
}
# (smallest, largest, the default) settle, tolerance and margin (1 / FRCNN_PLATE_MAX_SETTLE / _DEFAULT_SETTLE, 0 / 255 / _DEFAULT_TOL,
# 0 / _MAX_MARGIN / _DEFAULT_MARGIN: the defaults are PROVISIONAL, not measured on real footage), the frame indices of a call
# (FRCNN_PLATE_MAX_FRAMES) and the update kernel's tile (FRCNN_PLATE_TILE_W, _TILE_H)
PLATE_SETTLE = (1, 255, 8)
PLATE_TOL = (0, 255, 10)
PLATE_MARGIN = (0, 64, 8)
PLATE_MAX_FRAMES = 65536
PLATE_TILE = (128, 8)

TRACK_REID_VERSION = 1          # include/ext/frcnn_hip_track_reid.h FRCNN_TRACK_REID_VERSION
TRACK_REID_SIGNATURES = {
    "frcnn_track_reid_version": (I, []),
    "frcnn_track_reid_state_bytes": (c_size_t, [I]),
    "frcnn_track_reid_workspace_bytes": (c_size_t, [I, I]),
    "frcnn_track_reid_update": (I, [P, I, P, ctypes.c_longlong, I, I, I, P, ctypes.c_longlong, I, I, P, P, P, I, I, I, P, P, ctypes.c_longlong,
                                    P, P]),
}
# (smallest, largest, the default) pct and keep (1 / 100 / FRCNN_TRACK_REID_DEFAULT_PCT, 1 / _MAX_KEEP / _DEFAULT_KEEP: the defaults are
# PROVISIONAL, not measured on real footage), the entries of a state at most (_MAX), the words of a signature, of an entry and of a
# frame's list (_SIG_WORDS, _ENTRY_WORDS, _LIST_WORDS), the events a list holds (_MAX_EVENTS) and the largest distance (_MAX_DISTANCE)
TRACK_REID_PCT = (1, 100, 25)
TRACK_REID_KEEP = (1, 4095, 250)
TRACK_REID_MAX = 256
TRACK_REID_SIG_WORDS = 192
TRACK_REID_ENTRY_WORDS = 5 + TRACK_REID_SIG_WORDS
TRACK_REID_MAX_EVENTS = 32
TRACK_REID_LIST_WORDS = 4 + 5 * TRACK_REID_MAX_EVENTS
TRACK_REID_MAX_DISTANCE = 8192

DETECT_POST_VERSION = 1         # include/ext/frcnn_hip_detect_post.h FRCNN_DETECT_POST_VERSION
DETECT_POST_SIGNATURES = {
    "frcnn_detect_post_version": (I, []),
    "frcnn_detections_post": (I, [P, P, I, P, P, I, I, c_double, c_double, c_double, c_double, P, P, P, P, P, I, c_double, c_double, c_double, P]),
    "frcnn_detections_post_dyn": (I, [P, P, I, I, P, P, I, I, c_double, c_double, P, P, P, P, P, P, I, c_double, c_double, c_double, P]),
}
# FRCNN_NMS_HARD / _SOFT_LINEAR / _SOFT_GAUSSIAN, and the defaults of nms_thresh, sigma and the voting IoU (sigma and the voting IoU, like
# min_score = the image's threshold, are PROVISIONAL: their effect on mAP has not been measured on a dataset)
DETECT_POST_MODES = ("hard", "soft_linear", "soft_gaussian")
DETECT_POST_DEFAULTS = (0.5, 0.5, 0.5)

SCALE_VERSION = 1               # include/ext/frcnn_hip_scale.h FRCNN_SCALE_VERSION
SCALE_SIGNATURES = {
    "frcnn_scale_version": (I, []),
    "frcnn_downscale_u8": (I, [P, ctypes.c_longlong, I, P, I, I, P, ctypes.c_longlong, I, I, P]),
}
SCALE_MAX_RATIO = 16            # ... FRCNN_SCALE_MAX_RATIO: a source side is at most this many times the output's

TRACK_LOOKBACK_VERSION = 1      # include/ext/frcnn_hip_track_lookback.h FRCNN_TRACK_LOOKBACK_VERSION
TRACK_LOOKBACK_SIGNATURES = {
    "frcnn_track_lookback_version": (I, []),
    "frcnn_track_lookback_state_bytes": (c_size_t, [I, I, I, I, I, I]),
    "frcnn_track_lookback": (I, [P, P, ctypes.c_longlong, P, ctypes.c_longlong, I, P, I, I, I, I, I, I, I, I, P, ctypes.c_longlong, P,
                                 ctypes.c_longlong, P, P]),
}
# the frames a new track is chained back over: (smallest, largest, the default) (FRCNN_TRACK_LOOKBACK_MAX)
TRACK_LOOKBACK = (1, 16, 8)
TRACK_LOOKBACK_MAX_BACK = 128   # ... FRCNN_TRACK_LOOKBACK_MAX_BACK: back-filled rows a full frame can still take, at most
TRACK_LOOKBACK_HEADER = 32      # ... FRCNN_TRACK_LOOKBACK_HEADER: bytes in front of a window's cells

TRACK_BACKTRACK_VERSION = 1     # include/ext/frcnn_hip_track_backtrack.h FRCNN_TRACK_BACKTRACK_VERSION
TRACK_BACKTRACK_SIGNATURES = {
    "frcnn_track_backtrack_version": (I, []),
    "frcnn_track_backtrack": (I, [P, P, ctypes.c_longlong, P, ctypes.c_longlong, I, P, I, I, I, I, I, I, I, I, I, P, ctypes.c_longlong, P,
                                  ctypes.c_longlong, P, P]),
}


class ConvDesc(ctypes.Structure):
    """frcnn_conv_desc (include/frcnn_hip.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in (
        "n", "h", "w", "cin", "cout", "kh", "kw", "stride", "pad_top", "pad_left", "ho", "wo",
        "act", "ldy", "ldres", "tile", "layout")]


class PackJob(ctypes.Structure):
    """frcnn_pack_job (include/frcnn_hip.h)."""
    _fields_ = [(k, c_void_p) for k in ("w_hwio", "packed", "packed_dgrad", "bias", "scale", "shift_const", "shift")] + \
               [(k, ctypes.c_int32) for k in ("kh", "kw", "cin", "cout")]


class WgradJob(ctypes.Structure):
    """frcnn_wgrad_job (include/frcnn_hip.h)."""
    _fields_ = [("d", ConvDesc)] + [(k, c_void_p) for k in ("x", "g", "scale", "dw")] + [(k, ctypes.c_int32) for k in ("in_bf16", "reserved")]


class X6Job(ctypes.Structure):
    """frcnn_x6_job (include/frcnn_hip.h)."""
    _fields_ = [("w_packed", c_void_p), ("planes_bf16", c_void_p), ("rows", ctypes.c_int32), ("kpad", ctypes.c_int32)]


H3_UNDER, H3_SATURATED, H3_NONFINITE = 1, 2, 4      # FRCNN_H3_* status bits (include/frcnn_hip.h)


class H3Planes(ctypes.Structure):
    """frcnn_h3_planes (include/frcnn_hip.h)."""
    _fields_ = [("planes", c_void_p), ("exponent", c_void_p), ("status", c_void_p)]


class ColsumJob(ctypes.Structure):
    """frcnn_colsum_job (include/frcnn_hip.h)."""
    _fields_ = [(k, c_void_p) for k in ("g", "scale", "out")] + [(k, ctypes.c_int32) for k in ("m", "cout", "g_is_bf16", "reserved")]


_lib = None


def load():
    """Load the shared library (once) and bind every declared symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FrcnnError(
            f"{LIB_PATH} is missing: build it with `python -m faster_rcnn_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    # torch bundles its own HIP runtime (same SONAME as /opt/rocm's).  The process must use
    # ONE runtime -- streams and device pointers are shared with torch -- so make sure
    # torch's copy is loaded first; ours then binds to it by SONAME.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in EXT_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in ROI_RES_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in POOL_EPILOGUE_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in ROWMAP_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in PNG_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in PNG_HUFF_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in JPEG_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in JPEG_OPT_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in JPEG_DEC_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in JPEG_DEC_BATCH_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in PNG_DEC_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in PNG_DEC_FULL_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in JPEG_DEC_FULL_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in Y4M_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in REDACT_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in TRACK_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_track_version() != TRACK_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_track_version()} of the tracking extension, this binding "
                         f"{TRACK_VERSION} (include/ext/frcnn_hip_track.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in TRACK_MOTION_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_track_motion_version() != TRACK_MOTION_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_track_motion_version()} of the tracker's motion extension, this binding "
                         f"{TRACK_MOTION_VERSION} (include/ext/frcnn_hip_track_motion.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in TRACK_LOOKBACK_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_track_lookback_version() != TRACK_LOOKBACK_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_track_lookback_version()} of the tracker's look-back extension, this binding "
                         f"{TRACK_LOOKBACK_VERSION} (include/ext/frcnn_hip_track_lookback.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in TRACK_BACKTRACK_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_track_backtrack.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_track_backtrack_version() != TRACK_BACKTRACK_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_track_backtrack_version()} of the tracker's back-track extension, this binding "
                         f"{TRACK_BACKTRACK_VERSION} (include/ext/frcnn_hip_track_backtrack.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in TRACK_INTERVAL_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_track_interval_version() != TRACK_INTERVAL_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_track_interval_version()} of the tracker's interval extension, this binding "
                         f"{TRACK_INTERVAL_VERSION} (include/ext/frcnn_hip_track_interval.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in TRACK_CUT_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_track_cut.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_track_cut_version() != TRACK_CUT_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_track_cut_version()} of the tracker's scene-cut extension, this binding "
                         f"{TRACK_CUT_VERSION} (include/ext/frcnn_hip_track_cut.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in TRACK_WEAK_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_track_weak.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_track_weak_version() != TRACK_WEAK_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_track_weak_version()} of the tracker's weak-row extension, this binding "
                         f"{TRACK_WEAK_VERSION} (include/ext/frcnn_hip_track_weak.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in TRACK_TRAILS_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_track_trails.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_track_trails_version() != TRACK_TRAILS_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_track_trails_version()} of the tracker's trail extension, this binding "
                         f"{TRACK_TRAILS_VERSION} (include/ext/frcnn_hip_track_trails.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in HEAT_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_heat.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_heat_version() != HEAT_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_heat_version()} of the heat-map extension, this binding "
                         f"{HEAT_VERSION} (include/ext/frcnn_hip_heat.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in COUNT_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_count.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_count_version() != COUNT_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_count_version()} of the line-count extension, this binding "
                         f"{COUNT_VERSION} (include/ext/frcnn_hip_count.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in ZONE_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_zone.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_zone_version() != ZONE_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_zone_version()} of the zone extension, this binding "
                         f"{ZONE_VERSION} (include/ext/frcnn_hip_zone.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in PLATE_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_plate.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_plate_version() != PLATE_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_plate_version()} of the background-plate extension, this binding "
                         f"{PLATE_VERSION} (include/ext/frcnn_hip_plate.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in TRACK_REID_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_track_reid.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_track_reid_version() != TRACK_REID_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_track_reid_version()} of the re-identify extension, this binding "
                         f"{TRACK_REID_VERSION} (include/ext/frcnn_hip_track_reid.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in DETECT_POST_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_detect_post.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_detect_post_version() != DETECT_POST_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_detect_post_version()} of the post-process extension, this binding "
                         f"{DETECT_POST_VERSION} (include/ext/frcnn_hip_detect_post.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in SCALE_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_scale.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_scale_version() != SCALE_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_scale_version()} of the scale extension, this binding "
                         f"{SCALE_VERSION} (include/ext/frcnn_hip_scale.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in REDACT_SHAPE_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_redact_shape.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_redact_shape_version() != REDACT_SHAPE_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_redact_shape_version()} of the shaped-redaction extension, this binding "
                         f"{REDACT_SHAPE_VERSION} (include/ext/frcnn_hip_redact_shape.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in REDACT_REGION_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_redact_region.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_redact_region_version() != REDACT_REGION_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_redact_region_version()} of the region-redaction extension, this binding "
                         f"{REDACT_REGION_VERSION} (include/ext/frcnn_hip_redact_region.h): rebuild with `python -m faster_rcnn_amd.build`")
    for name, (res, args) in REDACT_MOVING_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise FrcnnError(f"{LIB_PATH} has no {name} (include/ext/frcnn_hip_redact_moving.h): rebuild with `python -m faster_rcnn_amd.build`")
        fn.restype = res
        fn.argtypes = args
    if lib.frcnn_redact_moving_version() != REDACT_MOVING_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_redact_moving_version()} of the moving-redaction extension, this binding "
                         f"{REDACT_MOVING_VERSION} (include/ext/frcnn_hip_redact_moving.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_redact_version() != REDACT_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_redact_version()} of the redaction extension, this binding "
                         f"{REDACT_VERSION} (include/ext/frcnn_hip_redact.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_y4m_version() != Y4M_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_y4m_version()} of the YUV4MPEG2 extension, this binding "
                         f"{Y4M_VERSION} (include/ext/frcnn_hip_y4m.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_jpeg_dec_full_version() != JPEG_DEC_FULL_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_jpeg_dec_full_version()} of the JPEG decoder's progressive extension, this "
                         f"binding {JPEG_DEC_FULL_VERSION} (include/ext/frcnn_hip_jpeg_dec_full.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_png_dec_full_version() != PNG_DEC_FULL_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_png_dec_full_version()} of the PNG decoder's full-format extension, this "
                         f"binding {PNG_DEC_FULL_VERSION} (include/ext/frcnn_hip_png_dec_full.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_png_dec_version() != PNG_DEC_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_png_dec_version()} of the PNG decoder extension, this binding "
                         f"{PNG_DEC_VERSION} (include/ext/frcnn_hip_png_dec.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_jpeg_dec_batch_version() != JPEG_DEC_BATCH_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_jpeg_dec_batch_version()} of the JPEG decoder's batch extension, this binding "
                         f"{JPEG_DEC_BATCH_VERSION} (include/ext/frcnn_hip_jpeg_dec_batch.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_jpeg_dec_version() != JPEG_DEC_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_jpeg_dec_version()} of the JPEG decoder extension, this binding "
                         f"{JPEG_DEC_VERSION} (include/ext/frcnn_hip_jpeg_dec.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_jpeg_opt_version() != JPEG_OPT_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_jpeg_opt_version()} of the JPEG encoder's 4:2:0 / optimised-table extension, "
                         f"this binding {JPEG_OPT_VERSION} (include/ext/frcnn_hip_jpeg_opt.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_jpeg_version() != JPEG_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_jpeg_version()} of the JPEG encoder extension, this binding "
                         f"{JPEG_VERSION} (include/ext/frcnn_hip_jpeg.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_png_huff_version() != PNG_HUFF_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_png_huff_version()} of the PNG encoder's huffman extension, this binding "
                         f"{PNG_HUFF_VERSION} (include/ext/frcnn_hip_png_huff.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_png_version() != PNG_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_png_version()} of the PNG encoder extension, this binding "
                         f"{PNG_VERSION} (include/ext/frcnn_hip_png.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_roi_res_version() != ROI_RES_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_roi_res_version()} of the gathered-residual extension, this binding "
                         f"{ROI_RES_VERSION} (include/ext/frcnn_hip_roi_res.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_pool_epilogue_version() != POOL_EPILOGUE_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_pool_epilogue_version()} of the pooled-epilogue extension, this binding "
                         f"{POOL_EPILOGUE_VERSION} (include/ext/frcnn_hip_pool_epilogue.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_rowmap_version() != ROWMAP_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_rowmap_version()} of the row-map extension, this binding "
                         f"{ROWMAP_VERSION} (include/ext/frcnn_hip_rowmap.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_vgg_canvas_version() != VGG_CANVAS_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks revision {lib.frcnn_vgg_canvas_version()} of the VGG16 canvas extension, this binding "
                         f"{VGG_CANVAS_VERSION} (include/ext/frcnn_hip_vgg_canvas.h): rebuild with `python -m faster_rcnn_amd.build`")
    if lib.frcnn_version() != ABI_VERSION:
        raise FrcnnError(f"{LIB_PATH} speaks ABI revision {lib.frcnn_version()}, this binding {ABI_VERSION} (include/frcnn_hip.h "
                         "FRCNN_ABI_VERSION): rebuild with `python -m faster_rcnn_amd.build`")
    _lib = lib
    return lib


def check(code, what=""):
    if code != 0:
        msg = load().frcnn_last_error()
        raise FrcnnError(f"{what or 'frcnn call'} failed ({code}): {msg.decode() if msg else ''}")


def call(name, *args):
    """Call an int-returning entry point and raise FrcnnError on a non-zero status."""
    code = getattr(_lib or load(), name)(*args)
    if code != 0:
        check(code, name)
