"""ctypes binding of libcrnerf_hip.so (the C ABI declared in the headers of include/).

The library is the product: if it is missing or fails to load, every call raises -- there is no
eager/CPU fallback behind these functions.
"""
import collections.abc
import ctypes
import itertools
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# CRNERF_LIB_PATH: a tuning build of the same library (tools/variants.py) -- never a different backend; a path that does not exist raises at load
LIB_PATH = os.environ.get("CRNERF_LIB_PATH") or os.path.join(_HERE, "libcrnerf_hip.so")

_c_fp = ctypes.c_void_p  # device float*


class RenderArgs(ctypes.Structure):
    """struct crnerf_render_args (include/crnerf.h)."""
    _fields_ = [
        ("packed_coarse", ctypes.c_void_p), ("packed_fine", ctypes.c_void_p),
        ("rays", _c_fp), ("view_dir", _c_fp), ("z_coarse", _c_fp), ("z_steps", _c_fp), ("u", _c_fp), ("u_stride", ctypes.c_int64),
        ("noise_coarse", _c_fp), ("noise_fine", _c_fp),
        ("noise_std", ctypes.c_float), ("use_disp", ctypes.c_int32),
        ("n_rays", ctypes.c_int64), ("n_samples", ctypes.c_int32), ("n_importance", ctypes.c_int32),
        ("weights_coarse", _c_fp), ("feature_coarse", _c_fp), ("depth_coarse", _c_fp),
        ("weights_fine", _c_fp), ("feature_fine", _c_fp), ("depth_fine", _c_fp), ("z_fine", _c_fp),
        ("rng_seed", ctypes.c_uint64), ("rng_ray_offset", ctypes.c_int64), ("rng_flags", ctypes.c_int32), ("perturb", ctypes.c_float),
        ("z_coarse_out", _c_fp), ("noise_coarse_out", _c_fp), ("noise_fine_out", _c_fp),
    ]


RNG_JITTER, RNG_U, RNG_NOISE = 1, 2, 4     # CRNERF_RNG_* (include/crnerf.h)
ERR_RANGE = -4                              # CRNERF_ERR_RANGE


class LossArgs(ctypes.Structure):
    """struct crnerf_loss_args (include/crnerf.h)."""
    _fields_ = [
        ("rgb_coarse", _c_fp), ("rgb_coarse_row_stride", ctypes.c_int64), ("rgb_coarse_chan_stride", ctypes.c_int64),
        ("rgb_fine", _c_fp), ("rgb_fine_row_stride", ctypes.c_int64), ("rgb_fine_chan_stride", ctypes.c_int64),
        ("targets", _c_fp), ("targets_row_stride", ctypes.c_int64), ("targets_chan_stride", ctypes.c_int64),
        ("mask", _c_fp),
        ("a_embedded", _c_fp), ("n_a", ctypes.c_int64),
        ("a_embedded_random", _c_fp), ("a_embedded_random_rec", _c_fp), ("n_rec", ctypes.c_int64),
        ("content_wo", _c_fp), ("content_with", _c_fp), ("n_content", ctypes.c_int64),
        ("n_rays", ctypes.c_int64),
        ("mse_on_appearance", ctypes.c_int32),
        ("coef", ctypes.c_float), ("weight_kl", ctypes.c_float), ("weight_rec_a", ctypes.c_float), ("weight_content", ctypes.c_float),
        ("mask_size_weight", ctypes.c_float), ("mask_digit_weight", ctypes.c_float),
    ]


class LossGrads(ctypes.Structure):
    """struct crnerf_loss_grads."""
    _fields_ = [(n, _c_fp) for n in ("d_rgb_coarse", "d_rgb_fine", "d_mask", "d_a_embedded", "d_a_embedded_random_rec",
                                     "d_content_wo", "d_content_with")]


class BatchArgs(ctypes.Structure):
    """struct crnerf_batch_args."""
    _fields_ = [
        ("all_rays", _c_fp), ("ray_stride", ctypes.c_int64), ("all_rgbs", _c_fp), ("row_offset", ctypes.c_int64),
        ("img_w", ctypes.c_int32), ("img_h", ctypes.c_int32), ("side", ctypes.c_int32),
        ("w_lin", _c_fp), ("h_lin", _c_fp),
        ("scale", ctypes.c_float), ("h_offset", ctypes.c_float), ("w_offset", ctypes.c_float),
        ("rays", _c_fp), ("ts", ctypes.c_void_p), ("rgbs", _c_fp), ("rgb_idx", ctypes.c_void_p), ("uv_sample", _c_fp),
    ]


class ImageMetricsArgs(ctypes.Structure):
    """struct crnerf_image_metrics_args."""
    _fields_ = [
        ("pred", _c_fp), ("pred_stride_c", ctypes.c_int64), ("pred_stride_y", ctypes.c_int64), ("pred_stride_x", ctypes.c_int64),
        ("gt", _c_fp), ("gt_stride_c", ctypes.c_int64), ("gt_stride_y", ctypes.c_int64), ("gt_stride_x", ctypes.c_int64),
        ("channels", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
        ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
        ("quantize_pred", ctypes.c_int32),
    ]


class LpipsArgs(ctypes.Structure):
    """struct crnerf_lpips_args."""
    _fields_ = [
        ("pred", _c_fp), ("pred_stride_c", ctypes.c_int64), ("pred_stride_y", ctypes.c_int64), ("pred_stride_x", ctypes.c_int64),
        ("gt", _c_fp), ("gt_stride_c", ctypes.c_int64), ("gt_stride_y", ctypes.c_int64), ("gt_stride_x", ctypes.c_int64),
        ("width", ctypes.c_int32), ("height", ctypes.c_int32),
        ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
        ("quantize_pred", ctypes.c_int32), ("normalize", ctypes.c_int32),
        ("conv_w", _c_fp * 5), ("conv_b", _c_fp * 5), ("lin", _c_fp * 5), ("shift", _c_fp), ("scale", _c_fp),
    ]


METRICS_TILE_H, METRICS_TILE_W = 16, 64     # CRNERF_METRICS_TILE_H / _W (include/crnerf.h)
LANCZOS_TILE_H, LANCZOS_TILE_W, LANCZOS_VBLOCK = 8, 32, 256     # CRNERF_LANCZOS_TILE_H / _W / _VBLOCK
LANCZOS_OUT = {"u8": 0, "rows": 1, "chw": 2, "chw_signed": 3}   # CRNERF_LANCZOS_OUT_*


RGBA_TILE_H, RGBA_TILE_W, RGBA_VBLOCK = 8, 32, 256     # CRNERF_RGBA_TILE_H / _W / _VBLOCK (include/crnerf_blender.h)
RGBA_MAX_RECTS = 16                                     # CRNERF_RGBA_MAX_RECTS
RGBA_OUT = {"u8": 0, "rows": 1, "chw": 2, "chw_signed": 3}      # CRNERF_RGBA_OUT_*


class RgbaPrepareArgs(ctypes.Structure):
    """struct crnerf_rgba_prepare_args (include/crnerf_blender.h)."""
    _fields_ = [
        ("src", ctypes.c_void_p), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
        ("kx", ctypes.c_void_p), ("bounds_x", ctypes.c_void_p), ("ky", ctypes.c_void_p), ("bounds_y", ctypes.c_void_p),
        ("ksize_x", ctypes.c_int32), ("ksize_y", ctypes.c_int32), ("n_rects", ctypes.c_int32), ("out_mode", ctypes.c_int32),
        ("rects", ctypes.c_void_p), ("colors", ctypes.c_void_p),          # HOST arrays
        ("lut", ctypes.c_void_p),
        ("dst", ctypes.c_void_p), ("valid_mask", ctypes.c_void_p), ("workspace", ctypes.c_void_p),
    ]


class ConvGeom(ctypes.Structure):
    """struct crnerf_conv_geom."""
    _fields_ = [(n, ctypes.c_int32) for n in ("cin", "cout", "H", "W", "k", "stride", "pad", "dil", "depthwise")]


class SweepDecodeArgs(ctypes.Structure):
    """struct crnerf_sweep_decode_args (include/crnerf_sweep.h)."""
    _fields_ = [
        ("content", _c_fp), ("HW", ctypes.c_int64), ("stats", _c_fp), ("style_HW", ctypes.c_int64),
        ("S", ctypes.c_int32), ("out_kind", ctypes.c_int32),
        ("weights", ctypes.POINTER(ctypes.c_void_p)), ("workspace", ctypes.c_void_p), ("out", ctypes.c_void_p),
        ("style_stride", ctypes.c_int64), ("plane_stride", ctypes.c_int64),
    ]


SWEEP_MAX_STYLES, SWEEP_STATS_FLOATS = 16, 1088          # CRNERF_SWEEP_MAX_STYLES, CRNERF_SWEEP_STATS_FLOATS
SWEEP_OUT_F32, SWEEP_OUT_U8 = 0, 1                       # CRNERF_SWEEP_OUT_*


# The ABI registry: one table per header of include/, in binding order; each table holds one row per prototype, name -> (restype, argtypes).
# Everything that needs the ABI reads it here: load() binds it, build() checks the library's exports against it, tests/test_host.py holds every
# table to its header parameter by parameter.  One spelling per C type, so that equal prototypes read equal.  A new header costs one entry.
i64, i32, u32, u64, f32, f64 = ctypes.c_int64, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float, ctypes.c_double      # i32: int / int32_t
usz, cstr, vp = ctypes.c_size_t, ctypes.c_char_p, ctypes.c_void_p
pp = ctypes.POINTER(ctypes.c_void_p)                     # a host array of pointers (every `T* const*`)
hf = ctypes.POINTER(ctypes.c_float)                      # a host float array (`*_host`)
ra = ctypes.POINTER(RenderArgs)
HEADER_SIGNATURES = {"crnerf.h": {
    "crnerf_abi_version": (i32, []),
    "crnerf_last_error": (cstr, []),
    "crnerf_packed_mlp_bytes": (usz, []),
    "crnerf_crossray_workspace_bytes": (usz, []),
    "crnerf_pack_mlp_weights": (i32, [pp, vp, vp]),
    "crnerf_packed_mlp_t_bytes": (usz, []),
    "crnerf_pack_mlp_weights_t": (i32, [pp, vp, vp]),
    "crnerf_mlp_train_acts_bytes": (usz, [i64]),
    "crnerf_mlp_train_scratch_bytes": (usz, [i64]),
    "crnerf_mlp_forward_train_f32": (i32, [vp, vp, vp, vp, i64, vp]),
    "crnerf_mlp_backward_f32": (i32, [vp, vp, vp, vp, vp, vp, pp, i64, vp]),
    "crnerf_mlp_backward_ex_f32": (i32, [vp, vp, vp, vp, vp, vp, pp, i64, i32, vp]),
    "crnerf_packed_mlp_mixed_bytes": (usz, []),
    "crnerf_pack_mlp_weights_mixed": (i32, [pp, vp, vp]),
    "crnerf_mlp_train_mixed_acts_bytes": (usz, [i64]),
    "crnerf_mlp_train_mixed_scratch_bytes": (usz, [i64]),
    "crnerf_mlp_forward_train_mixed_f32": (i32, [pp, vp, vp, vp, vp, i64, vp]),
    "crnerf_mlp_backward_mixed_f32": (i32, [pp, vp, vp, vp, vp, vp, vp, pp, i64, vp]),
    "crnerf_mlp_backward_mixed_ex_f32": (i32, [pp, vp, vp, vp, vp, vp, pp, i64, i32, vp]),
    "crnerf_posenc_f32": (i32, [vp, vp, i64, i32, vp]),
    "crnerf_embed_points_f32": (i32, [vp, vp, vp, vp, i64, i32, vp]),
    "crnerf_encoder_workspace_bytes": (usz, [i32, i32]),
    "crnerf_encoder_forward_f32": (i32, [vp, i32, i32, pp, vp, vp, vp]),
    "crnerf_ray_directions_f32": (i32, [i32, i32, f32, f32, f32, f32, vp, vp]),
    "crnerf_rays_from_directions_f32": (i32, [vp, hf, i64, vp, vp, vp]),
    "crnerf_generate_rays_f32": (i32, [hf, hf, i32, i32, f32, f32, vp, vp]),
    "crnerf_mlp_forward_f32": (i32, [vp, vp, vp, i64, i32, vp]),
    "crnerf_composite_f32": (i32, [vp, vp, vp, f32, vp, vp, vp, i64, i32, vp]),
    "crnerf_composite_backward_f32": (i32, [vp, vp, vp, f32, vp, vp, vp, vp, i64, i32, vp]),
    "crnerf_sample_pdf_merge_f32": (i32, [vp, vp, vp, i64, vp, vp, i64, i32, i32, vp]),
    "crnerf_render_rays_f32": (i32, [ra, vp]),
    "crnerf_render_rays_lean_f32": (i32, [ra, vp]),
    "crnerf_rng_fill_f32": (i32, [vp, i64, i32, u64, i32, i64, vp]),
    "crnerf_render_rays_train_f32": (i32, [ra, vp, vp, vp, vp, vp]),
    "crnerf_render_rays_train_bf16": (i32, [ra, vp, vp, vp, vp, vp]),
    "crnerf_render_rays_bf16": (i32, [ra, vp]),
    "crnerf_render_rays_bf16_fine": (i32, [ra, vp]),
    "crnerf_packed_mlp_h2_bytes": (usz, []),
    "crnerf_pack_mlp_weights_h2": (i32, [pp, vp, vp]),
    "crnerf_mlp_forward_f32h2": (i32, [vp, vp, vp, i64, i32, vp]),
    "crnerf_render_rays_f32h2": (i32, [ra, vp]),
    "crnerf_render_rays_f32x3_repair": (i32, [ra, vp]),
    "crnerf_mlp_forward_f32x3_repair": (i32, [vp, vp, vp, i64, i32, vp]),
    "crnerf_render_rays_train_f32h2": (i32, [ra, vp, vp, vp, vp, vp]),
    "crnerf_render_rays_train_f32x3_repair": (i32, [ra, vp, vp, vp, vp, vp]),
    "crnerf_packed_mlp_t_h2_bytes": (usz, []),
    "crnerf_pack_mlp_weights_t_h2": (i32, [pp, vp, vp]),
    "crnerf_mlp_backward_h2_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, pp, i64, i32, vp]),
    "crnerf_pack_mlp_weights_h2_async": (i32, [pp, vp, vp]),
    "crnerf_pack_h2_status": (i32, [vp, vp]),
    "crnerf_packed_mlp_x3_bytes": (usz, []),
    "crnerf_pack_mlp_weights_x3": (i32, [pp, vp, vp]),
    "crnerf_mlp_forward_f32x3": (i32, [vp, vp, vp, i64, i32, vp]),
    "crnerf_render_rays_f32x3": (i32, [ra, vp]),
    "crnerf_render_rays_train_f32x3": (i32, [ra, vp, vp, vp, vp, vp]),
    "crnerf_packed_mlp_t_x3_bytes": (usz, []),
    "crnerf_pack_mlp_weights_t_x3": (i32, [pp, vp, vp]),
    "crnerf_mlp_backward_x3_f32": (i32, [vp, vp, vp, vp, vp, vp, pp, i64, i32, vp]),
    "crnerf_packed_mlp_bf16_bytes": (usz, []),
    "crnerf_pack_mlp_weights_bf16": (i32, [pp, vp, vp]),
    "crnerf_mlp_forward_bf16": (i32, [vp, vp, vp, i64, i32, vp]),
    "crnerf_packed_mlp_f16_bytes": (usz, []),
    "crnerf_pack_mlp_weights_f16": (i32, [pp, vp, vp]),
    "crnerf_mlp_forward_f16": (i32, [vp, vp, vp, i64, i32, vp]),
    "crnerf_render_rays_f16": (i32, [ra, vp]),
    "crnerf_crossray_chansum_f32": (i32, [vp, i64, vp, vp, vp]),
    "crnerf_crossray_gram_f32": (i32, [vp, i64, vp, pp, vp, vp, vp]),
    "crnerf_crossray_matrix_f32": (i32, [vp, f64, vp, vp, vp, vp]),
    "crnerf_crossray_fold_f32": (i32, [vp, vp, vp, vp, pp, vp, vp]),
    "crnerf_crossray_apply_f32": (i32, [vp, i64, vp, vp, i64, vp]),
    "crnerf_crossray_backward_workspace_bytes": (usz, [i64, i64]),
    "crnerf_crossray_decode_backward_f32": (i32, [vp, i64, vp, i64, pp, vp, i64, vp, vp, vp, pp, vp]),
    "crnerf_crossray_decode_sharded_f32": (i32, [vp, i64, vp, i64, pp, i32, vp, f64, vp, vp, i64, vp]),
    "crnerf_crossray_decode_backward_sharded_f32": (i32, [vp, i64, vp, i64, pp, vp, i64, vp, vp, vp, pp, i32, vp, f64, vp, vp]),
    "crnerf_crossray_decode_f32": (i32, [vp, i64, vp, i64, pp, vp, vp, i64, vp]),
    "crnerf_decoder_content_backward_workspace_bytes": (usz, [i64]),
    "crnerf_decoder_content_backward_f32": (i32, [vp, i64, vp, vp, i64, vp, i64, vp, vp, vp, vp, vp]),
    "crnerf_encoder_train_saved_bytes": (usz, [i32, i32]),
    "crnerf_encoder_train_scratch_bytes": (usz, [i32, i32]),
    "crnerf_encoder_forward_train_f32": (i32, [vp, i32, i32, pp, vp, vp, vp]),
    "crnerf_encoder_backward_f32": (i32, [i32, i32, pp, vp, vp, vp, vp, pp, vp, vp]),
    "crnerf_encoder_train_band_saved_bytes": (usz, [i32, i32, i32]),
    "crnerf_encoder_train_band_scratch_bytes": (usz, [i32, i32, i32]),
    "crnerf_encoder_forward_train_band_f32": (i32, [vp, i32, i32, i32, i32, i32, i32, pp, vp, vp, vp]),
    "crnerf_encoder_backward_band_f32": (i32, [i32, i32, i32, i32, i32, i32, pp, vp, vp, vp, vp, pp, vp, vp]),
    "crnerf_loss_workspace_bytes": (usz, []),
    "crnerf_loss_f32": (i32, [ctypes.POINTER(LossArgs), vp, vp, vp]),
    "crnerf_loss_backward_f32": (i32, [ctypes.POINTER(LossArgs), vp, ctypes.POINTER(LossGrads), vp]),
    "crnerf_grid_sample_batch_f32": (i32, [ctypes.POINTER(BatchArgs), vp]),
    "crnerf_adam_max_tensors": (i32, []),
    "crnerf_adam_step_f32": (i32, [vp, vp, vp, vp, i32, pp, i32, f32, f64, f64, f32, f32, f32, vp]),
    "crnerf_conv2d_f32": (i32, [ctypes.POINTER(ConvGeom), vp, vp, vp, vp]),
    "crnerf_conv2d_backward_f32": (i32, [ctypes.POINTER(ConvGeom), vp, vp, vp, vp, vp, vp]),
    "crnerf_bn_prelu_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, f32, i32, vp]),
    "crnerf_bn_prelu_train_f32": (i32, [vp] * 11 + [f32, i32, i64, f32, vp]),
    "crnerf_bn_prelu_backward_f32": (i32, [vp] * 11 + [i32, i64, i32, vp]),
    "crnerf_avgpool3s2_f32": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "crnerf_fglo_f32": (i32, [vp] * 7 + [i32, i32, i64, vp]),
    "crnerf_fglo_backward_f32": (i32, [vp] * 11 + [i32, i32, i64, vp]),
    "crnerf_bilinear_gather_f32": (i32, [vp, i32, i32, i32, i32, vp, i64, i32, vp, vp]),
    "crnerf_bilinear_gather_backward_f32": (i32, [vp, vp, i32, i32, i32, i32, vp, i64, i32, vp, vp]),
    "crnerf_cgnet_param_count": (i32, []),
    "crnerf_cgnet_bn_count": (i32, []),
    "crnerf_cgnet_arena_bytes": (usz, [i32, i32, i32]),
    "crnerf_cgnet_forward_train_f32": (i32, [vp, i32, i32, i32, pp, pp, pp, pp, f32, f32, vp, vp, vp]),
    "crnerf_cgnet_backward_f32": (i32, [vp, i32, i32, i32, pp, vp, vp, vp, vp, pp, vp]),
    "crnerf_peer_window_bytes": (usz, []),
    "crnerf_peer_window_create": (i32, [pp, cstr]),
    "crnerf_peer_window_open": (i32, [cstr, pp]),
    "crnerf_peer_window_close": (i32, [vp]),
    "crnerf_peer_window_destroy": (i32, [vp]),
    "crnerf_peer_window_status": (i32, [vp, ctypes.POINTER(i32)]),
    "crnerf_peer_allreduce_f32": (i32, [vp, i32, pp, i32, i32, u32, i64, vp]),
    "crnerf_cus_per_xcd": (i32, []),
    "crnerf_stream_create_cu_share": (i32, [pp, i32, i32]),
    "crnerf_stream_destroy": (i32, [vp]),
    "crnerf_image_metrics_workspace_bytes": (usz, [i32, i32, i32]),
    "crnerf_image_metrics_f32": (i32, [ctypes.POINTER(ImageMetricsArgs), vp, vp, vp, vp]),
    "crnerf_lpips_workspace_bytes": (usz, [i32, i32]),
    "crnerf_lpips_f32": (i32, [ctypes.POINTER(LpipsArgs), vp, pp, vp, vp]),
    "crnerf_lanczos_workspace_bytes": (usz, [i32, i32, i32, i32]),
    "crnerf_lanczos_resize_u8": (i32, [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp]),
    "crnerf_scene_bounds_workspace_bytes": (usz, [i32, i32]),
    "crnerf_scene_bounds_f64": (i32, [vp, i32, vp, i32, f64, f64, vp, vp, vp, vp, vp]),
}, "crnerf_blender.h": {                # the Blender dataset path
    "crnerf_rgba_prepare_workspace_bytes": (usz, [i32, i32, i32, i32]),
    "crnerf_rgba_prepare_u8": (i32, [ctypes.POINTER(RgbaPrepareArgs), vp]),
    "crnerf_grid_sample_batch_round_f32": (i32, [ctypes.POINTER(BatchArgs), vp]),
    "crnerf_generate_rays_fmanorm_f32": (i32, [hf, hf, i32, i32, f32, f32, vp, vp]),
}, "crnerf_lean.h": {                   # the lean render on the pair core's two builds
    "crnerf_render_rays_lean_bf16": (i32, [ra, vp]),
    "crnerf_render_rays_lean_f16": (i32, [ra, vp]),
}, "crnerf_lean_composite.h": {         # the coarse-weights renders and the lean fine launch of the composite precisions
    "crnerf_render_coarse_weights_f32h2": (i32, [ra, vp]),
    "crnerf_render_coarse_weights_f32x3": (i32, [ra, vp]),
    "crnerf_render_coarse_weights_f32x3_repair": (i32, [ra, vp]),
    "crnerf_render_coarse_weights_f16": (i32, [ra, vp]),
    "crnerf_render_rays_lean_bf16_fine": (i32, [ra, vp]),
}, "crnerf_lean_x.h": {                 # the lean render on the two fp32-accurate split cores
    "crnerf_render_rays_lean_f32x3": (i32, [ra, vp]),
    "crnerf_render_rays_lean_f32h2": (i32, [ra, vp]),
    "crnerf_render_rays_lean_f32x3_repair": (i32, [ra, vp]),
}, "crnerf_sweep.h": {                  # the appearance sweep: S styles' statistics once, one content grid decoded under all of them
    "crnerf_crossray_style_stats_f32": (i32, [vp, i32, i64, i64, pp, vp, vp, vp]),
    "crnerf_crossray_decode_multi_f32": (i32, [ctypes.POINTER(SweepDecodeArgs), vp]),
}, "crnerf_geometry.h": {               # the density query: sigma at points or on a grid, trunk-only walk
    "crnerf_sigma_points_f32": (i32, [vp, vp, vp, i64, vp]),
    "crnerf_sigma_points_bf16": (i32, [vp, vp, vp, i64, vp]),
    "crnerf_sigma_grid_f32": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "crnerf_sigma_grid_bf16": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
}, "crnerf_mesh.h": {                   # the iso-surface of a density grid: count, then emit
    "crnerf_mesh_workspace_bytes": (usz, [i32, i32, i32]),
    "crnerf_mesh_count_f32": (i32, [vp, i32, i32, i32, f32, vp, vp, vp]),
    "crnerf_mesh_emit_f32": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, vp, i64, i64, vp, vp, vp, vp]),
}, "crnerf_mesh_parts.h": {             # the connected parts of an indexed mesh: label, sizes, select
    "crnerf_mesh_parts_workspace_bytes": (usz, [i64, i64]),
    "crnerf_mesh_parts_label_i32": (i32, [vp, i64, i64, vp, vp, vp, vp, vp]),
    "crnerf_mesh_parts_sizes_i32": (i32, [vp, vp, i64, i64, i64, vp, vp, vp]),
    "crnerf_mesh_parts_select_count": (i32, [vp, vp, i64, i64, i64, vp, vp, vp, vp]),
    "crnerf_mesh_parts_select_emit_f32": (i32, [vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, i64, i64, vp, vp, vp, vp]),
}}


class _AllSignatures(collections.abc.Mapping):
    """Every row of HEADER_SIGNATURES as one read-only mapping, in binding order.  It reads the registry on every access, so the two cannot
    fall out of step."""

    def __getitem__(self, name):
        return HEADER_SIGNATURES[header_of(name)][name]

    def __iter__(self):
        return itertools.chain.from_iterable(HEADER_SIGNATURES.values())

    def __len__(self):
        return sum(len(table) for table in HEADER_SIGNATURES.values())


def header_of(name):
    """The header whose table holds `name`; KeyError if none does."""
    for header, table in HEADER_SIGNATURES.items():
        if name in table:
            return header
    raise KeyError(name)


ALL_SIGNATURES = _AllSignatures()
EXPORTS = list(ALL_SIGNATURES)          # every symbol the library must export
if len(set(EXPORTS)) != len(EXPORTS):
    raise ImportError("crnerf_amd._lib: declared by more than one header: %s" % sorted({n for n in EXPORTS if EXPORTS.count(n) > 1}))

# Staged entries: headers that still live beside the sources (csrc/), one table per header in the registry's form.  load() binds them behind the
# registry loop; they are not counted by ALL_SIGNATURES / EXPORTS or by build()'s missing-symbol check until the header moves into include/ and
# its table into HEADER_SIGNATURES (tests/test_host.py pins those counts and is edited by that step).
STAGED_SIGNATURES = {"crnerf_point_features.h": {     # the point-feature query: 64 rgb features (and sigma) at points with a view direction, full walk
    "crnerf_feature_points_f32": (i32, [vp, vp, vp, vp, vp, i64, vp]),
    "crnerf_feature_points_bf16": (i32, [vp, vp, vp, vp, vp, i64, vp]),
}}
# A second staged mapping of the same form (tests/test_point_features_host.py pins the first to its one header): the mesh track's staged headers.
STAGED_MESH_SIGNATURES = {"crnerf_mesh_simplify.h": {   # mesh simplification by vertex clustering: count, then emit; the grid as nine scalars
    "crnerf_mesh_cluster_workspace_bytes": (usz, [i64, i64, i64]),
    "crnerf_mesh_cluster_count_f32": (i32, [vp, vp, i64, i64, f32, f32, f32, f32, f32, f32, i32, i32, i32, vp, vp, vp, vp]),
    "crnerf_mesh_cluster_emit_f32": (i32, [vp, vp, vp, vp, vp, i64, i64, f32, f32, f32, f32, f32, f32, i32, i32, i32, vp, i64, i64, vp, vp, vp, vp, vp]),
}}
STAGED_MAPPINGS = (STAGED_SIGNATURES, STAGED_MESH_SIGNATURES)      # what load() binds behind the registry, in this order
# A third staged mapping of the same form (tests/test_mesh_simplify_host.py pins the second to its one header and STAGED_MAPPINGS to its two
# mappings): load() binds it behind STAGED_MAPPINGS.
STAGED_SMOOTH_SIGNATURES = {"crnerf_mesh_smooth.h": {     # Taubin smoothing and face-derived vertex normals: adjacency, then smooth; the box as four scalars
    "crnerf_mesh_smooth_workspace_bytes": (usz, [i64, i64]),
    "crnerf_mesh_adjacency_i32": (i32, [vp, i64, i64, vp, vp]),
    "crnerf_mesh_smooth_f32": (i32, [vp, i64, i64, f32, f32, f32, i32, i32, f64, f64, i32, vp, vp, vp]),
    "crnerf_mesh_vertex_normals_f32": (i32, [vp, vp, i64, i64, i32, vp, vp, vp]),
}}
# A fourth staged mapping of the same form (tests/test_mesh_smooth_host.py pins the third to its one header): load() binds it behind the third.
STAGED_PHOTO_SIGNATURES = {"crnerf_mesh_photo.h": {       # photo colours for meshes: a z-buffer per posed view, then project / test / sample / average
    "crnerf_mesh_zbuffer_f32": (i32, [vp, vp, i64, i64, vp, vp, vp, i64, i64, f64, vp, vp]),
    "crnerf_mesh_photo_colors_u8": (i32, [vp, vp, i64, vp, vp, vp, vp, vp, i64, i64, f64, f64, vp, vp, vp]),
}}
_STAGED_ALL = STAGED_MAPPINGS + (STAGED_SMOOTH_SIGNATURES, STAGED_PHOTO_SIGNATURES)      # every staged mapping, in binding order
_staged = [n for mapping in _STAGED_ALL for table in mapping.values() for n in table]
if len(set(_staged)) != len(_staged) or set(_staged) & set(EXPORTS):
    raise ImportError("crnerf_amd._lib: a staged entry is declared twice: %s" % sorted(n for n in _staged if _staged.count(n) > 1 or n in EXPORTS))


_lib = None
_lock = threading.Lock()


def load():
    """Load (once) and return the ctypes handle; raises RuntimeError if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "crnerf_amd: %s not found -- build it with `python cr-nerf-pytorch_amd/build.py` "
                "(or __graft_entry__.build()); there is no fallback path." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in ALL_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise AttributeError("crnerf_amd: %s does not export %s, which include/%s declares: the library does not match that header"
                                     % (LIB_PATH, name, header_of(name))) from None
            fn.restype = res
            fn.argtypes = args
        for header, table in itertools.chain.from_iterable(mapping.items() for mapping in _STAGED_ALL):
            for name, (res, args) in table.items():
                try:
                    fn = getattr(lib, name)
                except AttributeError:
                    raise AttributeError("crnerf_amd: %s does not export %s, which csrc/%s declares: the library does not match that header"
                                         % (LIB_PATH, name, header)) from None
                fn.restype = res
                fn.argtypes = args
        _lib = lib
    return _lib


def check(code, what):
    if code != 0:
        msg = load().crnerf_last_error()
        raise RuntimeError("%s failed (code %d): %s" % (what, code, msg.decode() if msg else "?"))


# Host cost matters at the reference's 1,024-ray training batch (~450 launches per step, the step is host-bound): these helpers run once per
# pointer / launch, so they use torch's raw accessors -- no Stream object per launch, no string formatting unless something is wrong.
_get_device = getattr(torch._C, "_cuda_getDevice", None)
_get_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _current_device():
    return _get_device() if _get_device is not None else torch.cuda.current_device()


def stream_ptr():
    if _get_raw_stream is not None:
        return ctypes.c_void_p(_get_raw_stream(_current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bad_tensor(t, name, dtype):
    if not t.is_cuda:
        return RuntimeError("crnerf_amd: %s must live on the GPU (got %s); the HIP path has no CPU fallback" % (name, t.device))
    if t.device.index != _current_device():
        # kernels are enqueued on the CURRENT device's stream (stream_ptr): a tensor of another GPU would be reached through peer
        # access, unordered with its producers -- one process drives one GPU (torch.cuda.set_device(LOCAL_RANK) first)
        return RuntimeError("crnerf_amd: %s lives on cuda:%d but the current device is cuda:%d; call torch.cuda.set_device(%d) "
                            "(or wrap the call in torch.cuda.device) before using the HIP path"
                            % (name, t.device.index, _current_device(), t.device.index))
    if t.dtype != dtype:
        return TypeError("crnerf_amd: %s must be %s, got %s" % (name, dtype, t.dtype))
    return ValueError("crnerf_amd: %s must be contiguous" % name)


def dev_ptr(t, name="tensor", dtype=torch.float32):
    """Pointer of a contiguous device tensor; None -> NULL."""
    if t is None:
        return None
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.device.index != _current_device():
        raise _bad_tensor(t, name, dtype)
    return ctypes.c_void_p(t.data_ptr())


_PTR_ARRAYS = {}      # tuple of device addresses -> the ctypes array that holds them


def ptr_array(tensors, name):
    """HOST array of the tensors' device pointers (every `const float* const*` of the ABI).  A training step builds ~40 of them, mostly for the
    same parameter lists (their addresses are stable: optim.FlatAdam keeps p.data a view of one flat buffer) and for gradient lists the caching
    allocator hands back at the same addresses step after step: the arrays are kept by address tuple (round 6: 13 us -> 3 us per call; the
    1,024-ray step is host-bound).  The tensors are validated when an array is built; a hit means the same addresses passed that before."""
    key = tuple([t.data_ptr() for t in tensors])
    arr = _PTR_ARRAYS.get(key)
    if arr is not None:
        return arr
    arr = (ctypes.c_void_p * len(tensors))()
    dev = _current_device()
    for i, t in enumerate(tensors):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.device.index != dev:
            raise _bad_tensor(t, "%s[%d]" % (name, i), torch.float32)
        arr[i] = t.data_ptr()
    if len(_PTR_ARRAYS) >= 4096:
        _PTR_ARRAYS.clear()
    _PTR_ARRAYS[key] = arr
    return arr
