"""ctypes binding of ``libawseg_hip.so`` (the C ABI declared in ``include/awseg.h`` and, for the input-restoration entry
points, in ``include/awseg_restore.h``).

This is the only door between the Python host code and the HIP kernels.  There is no CPU
fallback anywhere behind it: if the library is missing or a kernel is asked to run on
host tensors, the call raises.  (The CPU oracle lives in ``oracle/`` and is test
infrastructure; nothing in this package imports it.)
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import torch

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libawseg_hip.so"

U8, I64 = 0, 1
COMBINE_WEIGHTED, COMBINE_MAXCONF, COMBINE_MEAN = 0, 1, 2
LOSS_CE, LOSS_FOCAL = 0, 1
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
MAX_CLASSES = 32

c_i, c_i64, c_u64, c_f, c_d, c_p = C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_void_p

# numpy mirrors of the job structs in include/awseg.h (align=True == the C layout)
FOG_JOB = np.dtype([("image", "<i4"), ("_pad", "<i4"), ("beta", "<f8"), ("atmos", "<f8"), ("seed", "<u8")], align=True)
NIGHT_JOB = np.dtype([("image", "<i4"), ("_pad", "<i4"), ("brightness", "<f8"), ("intensity", "<f8"), ("seed", "<u8")], align=True)
PRIM_JOB = np.dtype([("image", "<i4"), ("prim_offset", "<i4"), ("prim_count", "<i4"), ("blur_ksize", "<i4"), ("intensity", "<f8")], align=True)
WEATHER_JOB = np.dtype([("kind", "<i4"), ("image", "<i4"), ("a", "<f8"), ("b", "<f8"), ("seed", "<u8"), ("prim_offset", "<i4"), ("prim_count", "<i4")], align=True)
WEATHER_CLEAN, WEATHER_FOG, WEATHER_RAIN, WEATHER_SNOW, WEATHER_NIGHT = 0, 1, 2, 3, 4
assert FOG_JOB.itemsize == 32 and NIGHT_JOB.itemsize == 32 and PRIM_JOB.itemsize == 24 and WEATHER_JOB.itemsize == 40

# name -> (restype, argtypes); every symbol include/awseg.h declares
SIGNATURES = {
    "awseg_abi_version": (c_i, []),
    "awseg_header_hash": (C.c_uint64, []),
    "awseg_error_string": (C.c_char_p, [c_i]),
    "awseg_device_count": (c_i, []),
    "awseg_metrics_workspace": (c_i64, [c_i64, c_i, c_i64]),
    "awseg_confusion_accumulate": (c_i, [c_p, c_i, c_p, c_i, c_i64, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    "awseg_argmax": (c_i, [c_p, c_i64, c_i, c_i64, c_p, c_i, c_p]),
    "awseg_combine_argmax_confusion": (c_i, [c_p, c_p, c_i64, c_i, c_i64, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_i, c_i,
                                            c_i, c_p, c_p, c_i, c_p, c_p, c_p]),
    "awseg_argmax_confusion": (c_i, [c_p, c_i64, c_i, c_i64, c_p, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_p]),
    "awseg_normalize": (c_i, [c_p, c_i64, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p]),
    "awseg_synthetic_depth": (c_i, [c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p]),
    "awseg_conv3x3_winograd_nhwc": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p]),
    "awseg_gemm_bias_act": (c_i, [c_p, c_p, c_p, c_p, c_i, c_p, c_i64, c_i, c_i, c_p, C.c_size_t, c_p]),
    "awseg_gemm_tune": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p, c_i64, c_i, c_i, c_p, C.c_size_t, c_p]),
    "awseg_gemm_split_weights": (c_i, [c_p, c_i, c_i, c_p, c_p]),
    "awseg_gemm_split_weight_halfs": (c_i64, [c_i, c_i]),
    "awseg_gemm_split_bias_act": (c_i, [c_p, c_p, c_p, c_p, c_i, c_p, c_i64, c_i, c_i, c_p]),
    "awseg_gemm_bf16_weights": (c_i, [c_p, c_i, c_i, c_p, c_p]),
    "awseg_gemm_bf16_weight_halfs": (c_i64, [c_i, c_i]),
    "awseg_gemm_bf16_bias_act": (c_i, [c_p, c_p, c_p, c_p, c_i, c_p, c_i64, c_i, c_i, c_p]),
    "awseg_conv3x3_winograd_bf16_nhwc": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p]),
    "awseg_attention_d32_bf16": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p]),
    "awseg_attention_d32_split_workspace": (c_i64, [c_i, c_i, c_i]),
    "awseg_attention_d32_split_ws": (c_i, [c_p, c_p, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_f, c_p, c_p]),
    "awseg_attention_d32_packed_kv": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_i, c_p]),
    "awseg_dwconv3x3_upcat_nhwc": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_i64, c_i, c_i, c_p, c_p, c_p]),
    "awseg_winograd_split_weight_halfs": (c_i64, [c_i, c_i]),
    "awseg_conv3x3_winograd_split_nhwc": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p]),
    "awseg_upconv_forms_floats": (c_i64, [c_i, c_i, c_i]),
    "awseg_upconv_forms": (c_i, [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p]),
    "awseg_depth_head_fused": (c_i, [c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p]),
    "awseg_im2col_nhwc": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p]),
    "awseg_attention_d32": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p]),
    "awseg_attention_d32_split": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p]),
    "awseg_depth_upsample_combine": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    "awseg_lut3_apply": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_p]),
    "awseg_local_contrast": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p]),
    "awseg_depth_estimate_workspace": (C.c_size_t, [c_i]),
    "awseg_depth_estimate": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "awseg_fog_apply": (c_i, [c_p, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "awseg_fog_fused": (c_i, [c_p, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "awseg_night_apply": (c_i, [c_p, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "awseg_rain_apply": (c_i, [c_p, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "awseg_snow_apply": (c_i, [c_p, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "awseg_weather_batch": (c_i, [c_p, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "awseg_streak_workspace": (c_i64, [c_i, c_i, c_i]),
    "awseg_fog_density_field": (c_i, [c_p, c_i, c_i64, c_u64, c_p, c_p, c_p]),
    "awseg_loss_partials": (c_i64, [c_i64, c_i64]),
    "awseg_fog_ce_forward": (c_i, [c_p, c_p, c_i, c_p, c_i64, c_i, c_i64, c_i, c_f, c_p, c_p, c_p, c_p, c_p]),
    "awseg_fog_ce_backward": (c_i, [c_p, c_p, c_i, c_p, c_i64, c_i, c_i64, c_i, c_f, c_p, c_p, c_p]),
    "awseg_density_workspace": (c_i64, [c_i64, c_i64]),
    "awseg_fog_density_from_depth": (c_i, [c_p, c_i64, c_i, c_i, c_p, c_p, c_p]),
    "awseg_segformer_head_fused": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p]),
    "awseg_segformer_head_fused_split": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p]),
    "awseg_upconv3x3_bn_relu": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_p]),
    "awseg_upconv3x3_linear": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_p]),
    "awseg_upconv3x3_adjoint": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_i, c_i, c_p, c_p]),
    "awseg_aspp_depthwise3": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_p, c_p]),
    "awseg_aspp_depthwise3_mean": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_p]),
    "awseg_dwconv3x3_nhwc": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_p, c_p]),
    "awseg_bias_act_nhwc": (c_i, [c_p, c_i64, c_i, c_p, c_p, c_i, c_p]),
    "awseg_layernorm_rows": (c_i, [c_p, c_i64, c_i, c_p, c_p, c_f, c_p, c_p]),
    "awseg_ensemble_eval_stats": (c_i, [c_p, c_p, c_i64, c_i, c_i64, c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_i, c_p, c_i, c_p, c_i,
                                       c_f, c_f, c_p, c_p]),
    "awseg_gemm_split_pieces_bias_act": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_i64, c_i, c_p]),
    "awseg_gemm_split_dual_bias_act": (c_i, [c_p, c_i, c_p, c_i, c_i64, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_i64, c_i, c_p]),
    "awseg_conv_gemm_split_bias_act": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_i, c_p]),
    "awseg_conv_rows_gemm_split_bias_act": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_i, c_p]),
    "awseg_bn_train_workspace": (c_i64, [c_i, c_i, c_i64]),
    "awseg_bn_train_stats": (c_i, [c_p, c_i, c_i, c_i64, c_p, c_p, c_p, c_p]),
    "awseg_bn_relu_dropout_forward": (c_i, [c_p, c_i, c_i, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "awseg_bn_relu_dropout_backward": (c_i, [c_p, c_p, c_i, c_i, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p]),
    "awseg_dwconv3x3_wgrad_workspace": (c_i64, [c_i64, c_i, c_i, c_i]),
    "awseg_dwconv3x3_wgrad_nhwc": (c_i, [c_p, c_p, c_i64, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    "awseg_mixffn_fused": (c_i, [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_f, c_p, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p]),
    "awseg_maxpool3x3s2_nhwc": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_p, c_p]),
    "awseg_maxpool3x3s2_bias_relu_nhwc": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_p, c_p, c_p]),
    "awseg_upsample_bilinear": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_i, c_i, c_p, c_p]),
    "awseg_stem_image": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i64, c_i64, c_i64, c_p, c_i, c_p]),
    "awseg_rowdot_sigmoid": (c_i, [c_p, c_i64, c_i, c_p, c_p, c_i, c_p, c_p]),
    "awseg_aspp_pool_branch_workspace": (c_i64, [c_i, c_i]),
    "awseg_aspp_pool_branch": (c_i, [c_p, c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_i, c_p, c_p, c_p]),
    "awseg_upsample_bilinear_strided": (c_i, [c_p, c_i64, c_i, c_i, c_i, c_i64, c_i64, c_i64, c_i64, c_i, c_i, c_i, c_p, c_p]),
    "awseg_combine_confusion_stats": (c_i, [c_p, c_p, c_i64, c_i, c_i64, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_i,
                                           c_p, c_i, c_p, c_i, c_f, c_f, c_p, c_p]),
    "awseg_combine_confusion_stats_pred": (c_i, [c_p, c_p, c_i64, c_i, c_i64, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_p, c_p,
                                                c_i, c_p, c_i, c_p, c_i, c_f, c_f, c_p, c_p, c_p]),
    "awseg_consistency_workspace": (c_i64, [c_i64, c_i, c_i64]),
    "awseg_prediction_consistency": (c_i, [c_p, c_p, c_i, c_i64, c_i64, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_p]),
    "awseg_ece_accumulate": (c_i, [c_p, c_i64, c_i, c_i64, c_p, c_i, c_p, c_p, c_i, c_p, c_i, c_p, c_p]),
    "awseg_temperature_grid_stats": (c_i, [c_p, c_i64, c_i, c_i64, c_p, c_i, c_p, c_p, c_i, c_p, c_i, c_p, c_i, c_p]),
    "awseg_ensemble_temperature_grid_stats": (c_i, [c_p, c_p, c_i64, c_i, c_i64, c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_i, c_p, c_i,
                                                   c_p, c_i, c_p]),
    "awseg_ensemble_weight_grid_stats": (c_i, [c_p, c_p, c_i64, c_i, c_i64, c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_i, c_p]),
    "awseg_depth_eval_stats": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_f, c_p, c_p, c_i, c_p]),
    "awseg_ensemble_failure_stats": (c_i, [c_p, c_p, c_p, c_i64, c_i, c_i64, c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_i, c_p]),
    "awseg_failure_stats": (c_i, [c_p, c_i64, c_i, c_i64, c_p, c_i, c_p, c_p, c_i, c_p]),
    "awseg_boundary_workspace": (c_i64, [c_i64, c_i, c_i, c_i, c_i]),
    "awseg_boundary_stats": (c_i, [c_p, c_p, c_i, c_i, c_i64, c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_i, c_p, c_p, c_p]),
    "awseg_segment_workspace": (c_i64, [c_i64, c_i, c_i]),
    "awseg_segment_stats": (c_i, [c_p, c_p, c_i, c_i, c_i64, c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p]),
    "awseg_frame_iou_workspace": (c_i64, [c_i64, c_i, c_i64]),
    "awseg_frame_iou_counts": (c_i, [c_p, c_p, c_i, c_i, c_i64, c_i64, c_i, c_p, c_p, c_i64, c_p, c_p, c_p]),
    "awseg_bootstrap_counts": (c_i, [c_p, c_p, c_i64, c_i64, c_i64, c_i64, c_u64, c_i64, c_i64, c_p, c_p, c_p]),
    "awseg_change_strata": (c_i, [c_p, c_p, c_i, c_i64, c_i, c_i64, c_p, c_p, c_p, c_i, c_p, c_p, c_p]),
    "awseg_strata_workspace": (c_i64, [c_i64, c_i, c_i64, c_i]),
    "awseg_stratified_stats": (c_i, [c_p, c_p, c_i, c_i, c_p, c_i, c_p, c_i, c_p, c_i64, c_i64, c_i, c_p, c_p, c_i, c_p, c_p, c_p]),
    "awseg_image_quality_workspace": (c_i64, [c_i64, c_i, c_i64, c_i64]),
    "awseg_image_quality": (c_i, [c_p, c_p, c_i, c_i64, c_i, c_i64, c_i64, c_p, c_p, c_p, c_p, c_f, c_f, c_p, c_p, c_i, c_p, c_p, c_p]),
}

# name -> (restype, argtypes); every symbol include/awseg_restore.h declares.  A table of its own, bound by lib() like the one above
# and called through the same call() / try_call(): the extension header is hashed on its own (awseg_restore_header_hash).
EXTENSION_SIGNATURES = {
    "awseg_restore_header_hash": (C.c_uint64, []),
    "awseg_dehaze_workspace": (c_i64, [c_i64, c_i64, c_i64]),
    "awseg_dehaze": (c_i, [c_p, c_i64, c_i, c_i64, c_i64, c_p, c_p, c_i, c_f, c_f, c_f, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p]),
    "awseg_dehaze_guided_workspace": (c_i64, [c_i64, c_i64, c_i64]),
    "awseg_dehaze_guided": (c_i, [c_p, c_i64, c_i, c_i64, c_i64, c_p, c_p, c_i, c_f, c_f, c_f, c_i, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_i,
                                  c_p, c_p]),
    "awseg_relight_workspace": (c_i64, [c_i64, c_i, c_i]),
    "awseg_relight": (c_i, [c_p, c_i64, c_i, c_i64, c_i64, c_p, c_p, c_i, c_i, c_f, c_f, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p]),
    "awseg_deocclude_workspace": (c_i64, [c_i64, c_i64, c_i64]),
    "awseg_deocclude": (c_i, [c_p, c_i64, c_i, c_i64, c_i64, c_p, c_p, c_i, c_f, c_f, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p]),
    "awseg_weather_estimate_workspace": (c_i64, [c_i64]),
    "awseg_weather_estimate": (c_i, [c_p, c_i64, c_i, c_i64, c_i64, c_p, c_p, c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_p, c_p, c_p, c_i,
                                     c_p, c_p]),
    "awseg_tta_view": (c_i, [c_p, c_i64, c_i, c_i64, c_i64, c_p, c_i64, c_i64, c_i, c_p]),
    "awseg_tta_accumulate": (c_i, [c_p, c_i64, c_i, c_i64, c_i64, c_p, c_i64, c_i64, c_i, c_f, c_i, c_p]),
}


class AwsegError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load libawseg_hip.so; raise (never fall back) if it is not built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise AwsegError(
                f"{LIB_PATH} is missing: build it with `python -m "
                "adverse_weather_semantic_segmentation_robustness_benchmark_amd.csrc.build` "
                "(there is no CPU fallback for the HIP hot path)")
        handle = C.CDLL(str(LIB_PATH))
        for table in (SIGNATURES, EXTENSION_SIGNATURES):
            for name, (res, args) in table.items():
                fn = getattr(handle, name)      # AttributeError here == header/library drift
                fn.restype, fn.argtypes = res, args
        # a library built from another state of include/awseg.h takes other arguments than these bindings pass: refuse it
        # (a stale .so next to newer sources is exactly how that happens; the symbols above may all still exist)
        header = LIB_PATH.parent.parent / "include" / "awseg.h"
        built = int(handle.awseg_header_hash())
        if built and header.exists():
            from .csrc.build import header_hash
            if built != header_hash():
                raise AwsegError(f"{LIB_PATH} was built from another include/awseg.h than the one beside it (ABI drift): rebuild it with "
                                 "`python -m adverse_weather_semantic_segmentation_robustness_benchmark_amd.csrc.build`")
        extension = header.with_name("awseg_restore.h")
        built = int(handle.awseg_restore_header_hash())
        if built and extension.exists():
            from .csrc.build import RESTORE_HEADER, header_hash
            if built != header_hash(RESTORE_HEADER):
                raise AwsegError(f"{LIB_PATH} was built from another include/awseg_restore.h than the one beside it (ABI drift): rebuild "
                                 "it with `python -m adverse_weather_semantic_segmentation_robustness_benchmark_amd.csrc.build`")
        _lib = handle
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().awseg_error_string(rc)
        raise AwsegError(f"{what} failed with code {rc}: {msg.decode() if msg else '?'}")


launch_hook = None     # bench.py installs a (name, thunk, args) -> rc wrapper to time launches with HIP events


def call(name: str, *args) -> None:
    """Invoke one C-ABI launcher and raise on a non-zero return code."""
    fn = getattr(lib(), name)
    rc = fn(*args) if launch_hook is None else launch_hook(name, lambda: fn(*args), args)
    check(rc, name)


def try_call(name: str, *args, allow=(-2,)) -> int:
    """call() for launchers that may decline a shape: return codes in `allow` (default AWSEG_ERANGE) are handed back to the
    caller, which then uses the general entry point; anything else non-zero raises."""
    fn = getattr(lib(), name)
    rc = fn(*args) if launch_hook is None else launch_hook(name, lambda: fn(*args), args)
    if rc != 0 and rc not in allow:
        check(rc, name)
    return rc


def ptr(t):
    """Device pointer of a CUDA tensor (None -> NULL).  Host tensors are refused."""
    if t is None:
        return None
    if not t.is_cuda:
        raise AwsegError("awseg kernels take device (HIP) tensors only; got a CPU tensor — no CPU fallback exists")
    if not t.is_contiguous():
        raise AwsegError("awseg kernels take contiguous tensors")
    return C.c_void_p(t.data_ptr())


def ptr_strided(t):
    """Device pointer of a CUDA tensor handed over together with its strides (entry points that take them)."""
    if not t.is_cuda:
        raise AwsegError("awseg kernels take device (HIP) tensors only; got a CPU tensor — no CPU fallback exists")
    return C.c_void_p(t.data_ptr())


def host(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def label_dtype(t: torch.Tensor) -> int:
    if t.dtype == torch.uint8:
        return U8
    if t.dtype == torch.int64:
        return I64
    raise AwsegError(f"label/prediction maps must be uint8 or int64, got {t.dtype}")


def host_jobs(arr: np.ndarray):
    """Structured numpy job array -> host pointer (the launcher copies jobs into kernel arguments)."""
    arr = np.ascontiguousarray(arr)
    p = arr.ctypes.data_as(C.c_void_p)
    p._keepalive = arr
    return p


class Workspace:
    """Grow-only per-device scratch buffers handed to the C ABI (which never allocates)."""

    def __init__(self):
        self._buf = {}

    def get(self, device, nbytes: int, tag: str = "ws") -> torch.Tensor:
        key = (str(device), tag)
        buf = self._buf.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
            self._buf[key] = buf
        return buf


workspace = Workspace()
