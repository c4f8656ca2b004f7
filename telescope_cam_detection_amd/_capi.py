"""ctypes binding of libmi355rtdetr.so (include/rtdetr_mi355.h).  No compute happens in Python.

The library is required: if it cannot be built / loaded this module raises - there is no CPU or
PyTorch fallback for the hot path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import build as _build
from .arch import Arch

RTD_OK, RTD_E_INVALID, RTD_E_OOM, RTD_E_HIP, RTD_E_WEIGHTS, RTD_E_STATE = range(6)
PREC_BF16, PREC_FP32, PREC_F16X3 = 0, 1, 2
DT_BF16, DT_F32, DT_F16X2 = 0, 1, 4
DEC_METHODS = {"default": 0, "discrete": 1}      # Arch.dec_method -> RTD_DEC_*
SPLIT_GROUP = 32      # channels per [hi | lo] group of a F16X2 tensor (csrc/common.h)


def precision_code(name) -> int:
    """'f16x3' (default engine: hi/lo fp16 pairs, three MFMAs per product - meets the reference tolerance), 'bf16', 'fp32'."""
    if isinstance(name, int):
        return name
    s = str(name).lower()
    if s in ("f16x3", "fp16x3", "pair"):
        return PREC_F16X3
    if s in ("fp32", "f32", "float32"):
        return PREC_FP32
    if s in ("bf16", "bfloat16"):
        return PREC_BF16
    raise ValueError(f"unknown precision {name!r} (f16x3 | bf16 | fp32)")


def to_split(x: np.ndarray) -> np.ndarray:
    """fp32 [..., C] (C % 32 == 0) -> F16X2 storage as uint16 [..., 2C]: per 32-channel group [32 hi | 32 lo],
    hi = fp16_rne(x), lo = fp16_rne(x - hi) (subnormals kept, +-65504 saturation).  Host-side mirror of csrc/common.h
    split_store8 (tests / tools)."""
    x = np.clip(np.ascontiguousarray(x, np.float32), -65504.0, 65504.0)
    C_ = x.shape[-1]
    assert C_ % SPLIT_GROUP == 0
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    g = x.shape[:-1] + (C_ // SPLIT_GROUP, SPLIT_GROUP)
    out = np.stack([hi.view(np.uint16).reshape(g), lo.view(np.uint16).reshape(g)], axis=-2)          # [..., groups, 2, 32]
    return np.ascontiguousarray(out.reshape(x.shape[:-1] + (2 * C_,)))


def from_split(s: np.ndarray) -> np.ndarray:
    """F16X2 storage (uint16 [..., 2C]) -> fp32 [..., C] (hi + lo, exact in fp32)."""
    s = np.ascontiguousarray(s, np.uint16)
    C_ = s.shape[-1] // 2
    g = s.reshape(s.shape[:-1] + (C_ // SPLIT_GROUP, 2, SPLIT_GROUP))
    f = g.view(np.float16).astype(np.float32)
    return np.ascontiguousarray((f[..., 0, :] + f[..., 1, :]).reshape(s.shape[:-1] + (C_,)))


ACT = {"none": 0, "relu": 1, "silu": 2, "gelu": 3, "lrelu": 4}


class RtdConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("device", C.c_int32), ("precision", C.c_int32), ("max_batch", C.c_int32),
        ("input_h", C.c_int32), ("input_w", C.c_int32), ("use_graph", C.c_int32),
        ("layer_type", C.c_int32), ("depths", C.c_int32 * 4), ("hidden_sizes", C.c_int32 * 4),
        ("embedding_size", C.c_int32),
        ("enc_dim", C.c_int32), ("enc_ffn", C.c_int32), ("enc_heads", C.c_int32), ("csp_hidden", C.c_int32),
        ("d_model", C.c_int32), ("dec_ffn", C.c_int32), ("dec_heads", C.c_int32), ("dec_layers", C.c_int32),
        ("num_queries", C.c_int32), ("num_classes", C.c_int32), ("n_levels", C.c_int32), ("n_points", C.c_int32),
        ("offset_scale", C.c_float), ("profile", C.c_int32), ("dec_method", C.c_int32),
    ]


class RtdDet(C.Structure):
    _fields_ = [("class_id", C.c_int32), ("score", C.c_float), ("x1", C.c_float), ("y1", C.c_float),
                ("x2", C.c_float), ("y2", C.c_float)]


class RtdStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("last_error_code", C.c_int32), ("stream_capture_status", C.c_int32), ("in_flight", C.c_int32),
                ("plans", C.c_int64), ("graphs", C.c_int64), ("graph_nodes", C.c_int64), ("graph_launches", C.c_int64),
                ("eager_passes", C.c_int64), ("submits", C.c_int64), ("collects", C.c_int64), ("failed_calls", C.c_int64),
                ("saturated_values", C.c_int64), ("max_abs_filter", C.c_float), ("reserved", C.c_int32)]


class RtdCheckReport(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rows", C.c_int32), ("rows_matched", C.c_int32), ("worst_score_err", C.c_float),
                ("worst_box_err_px", C.c_float), ("score_tol", C.c_float), ("box_tol_px", C.c_float), ("max_abs_filter", C.c_float),
                ("saturated_values", C.c_int64), ("max_abs_filter_name", C.c_char * 64)]


class RtdLayerTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("kernel", C.c_char * 24), ("ms", C.c_float), ("flops", C.c_double),
                ("bytes", C.c_double)]


class RtdEnhanceParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("clip_limit", C.c_float), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("bilateral_d", C.c_int32), ("sigma_color", C.c_float), ("sigma_space", C.c_float)]


class RtdEsrganConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("precision", C.c_int32), ("num_feat", C.c_int32),
                ("num_grow_ch", C.c_int32), ("num_block", C.c_int32), ("tile", C.c_int32), ("tile_pad", C.c_int32)]


class RtdEvaConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "device", "precision", "max_batch", "img", "patch", "dim", "depth", "heads", "hidden",
                                         "classes", "ref_feat", "scale_attn_inner", "scale_mlp", "pool", "reserved0")]


class RtdYuvFrame(C.Structure):
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("y_pitch", C.c_int32), ("c_pitch", C.c_int32), ("layout", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32),
                ("reserved0", C.c_int32)]


class RtdBgrFrame(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("pitch", C.c_int32), ("reserved0", C.c_int32)]


class RtdFaceRect(C.Structure):
    _fields_ = [("frame", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("style", C.c_int32),
                ("k_or_blocks", C.c_int32), ("reserved0", C.c_int32)]


class RtdYoloxPostConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "device", "num_classes", "max_batch", "max_anchors", "max_candidates")]


class RtdYoloxPostParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("conf_threshold", C.c_float), ("nms_threshold", C.c_float), ("decode", C.c_int32),
                ("in_h", C.c_int32), ("in_w", C.c_int32), ("class_keep", C.POINTER(C.c_uint32))]


class RtdYoloxNetConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "device", "precision", "num_classes", "base_channels", "depth", "max_batch", "reserved0")]


DET_DTYPE = np.dtype([("class_id", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])

_lib: Optional[C.CDLL] = None

# every symbol include/rtdetr_mi355.h declares: the product C ABI (what a reference-side binding uses)
EXPORTS = [
    "rtd_version", "rtd_create", "rtd_load_weights", "rtd_infer", "rtd_infer_raw", "rtd_infer_async", "rtd_collect", "rtd_prepare",
    "rtd_result_block", "rtd_sync", "rtd_stream", "rtd_wait_stream", "rtd_signal_stream", "rtd_get_stats", "rtd_arena_bytes", "rtd_destroy",
    "rtd_last_error", "rtd_crop_resize_batch", "rtd_self_check", "rtd_preprocess",
    "rtd_motion_create", "rtd_motion_check", "rtd_motion_reset", "rtd_motion_wait_stream", "rtd_motion_last_error", "rtd_motion_destroy",
    "rtd_mog2_create", "rtd_mog2_configure", "rtd_mog2_apply", "rtd_mog2_wait_stream", "rtd_mog2_last_error", "rtd_mog2_destroy",
    "rtd_jpeg_create", "rtd_jpeg_encode", "rtd_jpeg_wait_stream", "rtd_jpeg_last_error", "rtd_jpeg_destroy",
    "rtd_overlay_create", "rtd_overlay_draw", "rtd_overlay_wait_stream", "rtd_overlay_last_error", "rtd_overlay_destroy",
    "rtd_enhance_create", "rtd_enhance_layout", "rtd_enhance_crops", "rtd_enhance_last_error", "rtd_enhance_destroy",
    "rtd_esrgan_create", "rtd_esrgan_layout", "rtd_esrgan_upscale", "rtd_esrgan_arena_bytes", "rtd_esrgan_last_error", "rtd_esrgan_destroy",
    "rtd_ingest_create", "rtd_ingest_convert", "rtd_ingest_convert_resize", "rtd_ingest_resize", "rtd_ingest_wait_stream", "rtd_ingest_last_error", "rtd_ingest_destroy",
    "rtd_facemask_create", "rtd_facemask_apply", "rtd_facemask_gray", "rtd_facemask_wait_stream", "rtd_facemask_last_error", "rtd_facemask_destroy",
    "rtd_eva_create", "rtd_eva_forward", "rtd_eva_self_check", "rtd_eva_arena_bytes", "rtd_eva_last_error", "rtd_eva_close",
    "rtd_yolox_anchors", "rtd_yolox_post_create", "rtd_yolox_post_run", "rtd_yolox_post_last_error", "rtd_yolox_post_destroy",
    "rtd_yolox_net_create", "rtd_yolox_net_run", "rtd_yolox_net_run_frames", "rtd_yolox_net_arena_bytes", "rtd_yolox_net_last_error", "rtd_yolox_net_destroy",
]
# every symbol include/rtdetr_mi355_test.h declares: kernel-level test / bench / debug entry points (csrc/testapi.hip)
TEST_EXPORTS = [
    "rtd_debug_tensor", "rtd_debug_force_topk", "rtd_profile", "rtd_debug_option", "rtd_op_conv", "rtd_op_conv_dual", "rtd_op_conv_next",
    "rtd_op_layernorm", "rtd_op_attention", "rtd_op_msdeform", "rtd_op_topk", "rtd_op_resize", "rtd_op_pool", "rtd_bench_conv", "rtd_bench_conv_pair",
    "rtd_bench_mfma_rate", "rtd_debug_motion_state", "rtd_debug_mog2_model", "rtd_debug_mog2_fg_bits",
    "rtd_debug_jpeg_coefficients", "rtd_debug_overlay_tiles", "rtd_debug_enhance_stage",
    "rtd_op_conv_view", "rtd_bench_conv_act", "rtd_debug_esrgan_tensor",
    "rtd_op_msdeform_view", "rtd_op_select_score", "rtd_op_gather_ln", "rtd_op_split_convert", "rtd_op_set_rows", "rtd_op_rowmax",
    "rtd_op_gather_rows", "rtd_op_boxes", "rtd_op_add", "rtd_op_postprocess", "rtd_op_msdeform_discrete_view",
    "rtd_op_conv_avg", "rtd_op_conv_pool", "rtd_debug_conv_choice", "rtd_debug_last_conv", "rtd_debug_conv_instantiations",
    "rtd_debug_ingest_info", "rtd_debug_resize_table", "rtd_op_stem0_u8", "rtd_debug_facemask_plan",
    "rtd_op_eva_patchify", "rtd_op_eva_rope", "rtd_op_eva_layernorm", "rtd_op_eva_attention", "rtd_debug_eva_tensor",
    "rtd_op_yolox_focus", "rtd_op_yolox_focus_u8", "rtd_op_yolox_spp", "rtd_op_yolox_head_emit", "rtd_debug_yolox_tensor",
    "rtd_op_conv_views", "rtd_debug_conv_choice_views",
    "rtd_debug_yolox_plan_convs", "rtd_debug_eva_plan_convs", "rtd_debug_esrgan_plan_convs",
]
CONV_INFO_FIELDS = ("family", "stages", "bn", "mt", "bm", "smallc", "wsq", "sx", "cog", "S", "grid", "ntn")   # info[12] of the conv-choice calls


def lib() -> C.CDLL:
    """Load (building first if stale) the HIP library.  Raises if that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB_PATH
    override = os.environ.get("RTD_LIB_PATH")   # tools only (tools/ab_lib.sh): A/B an older build of the library on the same box
    if override:
        if not os.path.exists(override):
            raise RuntimeError(f"RTD_LIB_PATH={override} does not exist")
        path = override
    elif _build.needs_build():
        try:
            path = _build.build(verbose=False)
        except Exception as e:  # no hipcc on this box: use the prebuilt library if it is there
            if not os.path.exists(path):
                raise RuntimeError(f"libmi355rtdetr.so is missing and cannot be built: {e}") from e
    # PyTorch-ROCm bundles its own libamdhip64: load it FIRST so that this library's libamdhip64.so.7 dependency resolves
    # to the same runtime instance.  Loaded the other way round (this library, then torch) the process holds two HIP runtimes
    # and the second to touch the GPU reports "no ROCm-capable device" (seen with build() followed by smoke() in one process).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(path)
    vp, i32, f32, i64 = C.c_void_p, C.c_int32, C.c_float, C.c_int64
    L.rtd_version.restype = C.c_char_p
    L.rtd_last_error.restype = C.c_char_p
    L.rtd_last_error.argtypes = [vp]
    L.rtd_create.argtypes = [C.POINTER(RtdConfig), C.POINTER(vp)]
    L.rtd_load_weights.argtypes = [vp, vp, C.c_size_t]
    L.rtd_infer.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), i32, f32, i32, vp, C.POINTER(i32)]
    L.rtd_infer_raw.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), i32, vp, vp, vp]
    L.rtd_infer_async.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), i32]
    L.rtd_collect.argtypes = [vp, f32, i32, vp, C.POINTER(i32)]
    L.rtd_prepare.argtypes = [vp, i32]
    L.rtd_wait_stream.argtypes = [vp, vp]
    L.rtd_signal_stream.argtypes = [vp, vp]
    L.rtd_get_stats.argtypes = [vp, C.POINTER(RtdStats)]
    if hasattr(L, "rtd_self_check") or not override:     # (an OLDER build under RTD_LIB_PATH, tools/ab_lib.sh, may predate these two)
        L.rtd_self_check.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(RtdCheckReport)]
        L.rtd_self_check.restype = C.c_int
        L.rtd_preprocess.argtypes = [vp, vp, i32, i32, i32, vp]
        L.rtd_preprocess.restype = C.c_int
    L.rtd_result_block.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    L.rtd_sync.argtypes = [vp]
    L.rtd_stream.argtypes = [vp]
    L.rtd_stream.restype = vp
    L.rtd_destroy.argtypes = [vp]
    L.rtd_destroy.restype = None
    L.rtd_debug_tensor.argtypes = [vp, C.c_char_p, vp, i64, C.POINTER(i64)]
    L.rtd_debug_force_topk.argtypes = [vp, vp, i32]
    L.rtd_profile.argtypes = [vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.rtd_arena_bytes.argtypes = [vp]
    L.rtd_arena_bytes.restype = i64
    L.rtd_debug_option.argtypes = [C.c_char_p, i32]
    L.rtd_op_conv.argtypes = [i32, vp, vp, vp, vp, vp] + [i32] * 12
    L.rtd_op_conv_dual.argtypes = [i32, vp, vp, vp, vp, vp, vp] + [i32] * 13
    L.rtd_op_conv_next.argtypes = [i32] + [vp] * 9 + [i32] * 10
    L.rtd_op_layernorm.argtypes = [i32, vp, vp, vp, vp, vp, i32, i32, i32]
    L.rtd_op_attention.argtypes = [i32, vp, vp, vp, i32, i32, i32, i32]
    L.rtd_op_msdeform.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, C.POINTER(i32), i32, f32]
    L.rtd_op_topk.argtypes = [vp, i32, i32, i32, vp, vp]
    L.rtd_op_resize.argtypes = [vp, i32, i32, vp, i32, i32, i32]
    if hasattr(L, "rtd_op_pool"):              # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_op_pool.argtypes = [i32, i32, vp, vp] + [i32] * 6
    L.rtd_bench_conv.argtypes = [i32] * 12 + [C.POINTER(f32)]
    L.rtd_bench_conv_pair.argtypes = [C.POINTER(i32), C.POINTER(i32), i32, C.POINTER(f32)]
    if hasattr(L, "rtd_bench_mfma_rate"):      # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_bench_mfma_rate.argtypes = [i32, i32, C.POINTER(f32)]
    L.rtd_crop_resize_batch.argtypes = [i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), i32, C.POINTER(f32), C.POINTER(f32), vp, vp]
    if hasattr(L, "rtd_motion_create"):        # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_motion_create.argtypes = [i32, i32, C.POINTER(vp)]
        L.rtd_motion_check.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), i32, C.POINTER(i32), i32, C.POINTER(i64)]
        L.rtd_motion_reset.argtypes = [vp, i32]
        L.rtd_motion_wait_stream.argtypes = [vp, vp]
        L.rtd_motion_last_error.argtypes = [vp]
        L.rtd_motion_last_error.restype = C.c_char_p
        L.rtd_motion_destroy.argtypes = [vp]
        L.rtd_motion_destroy.restype = None
        L.rtd_debug_motion_state.argtypes = [vp, i32, vp, C.c_size_t]
    if hasattr(L, "rtd_mog2_create"):          # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_mog2_create.argtypes = [i32, i32, C.c_double, i32, C.POINTER(vp)]
        L.rtd_mog2_configure.argtypes = [vp, i32, C.c_double, i32]
        L.rtd_mog2_apply.argtypes = [vp, vp, C.POINTER(i32), i32, i32, C.POINTER(i32), i32, C.POINTER(i64)]
        L.rtd_mog2_wait_stream.argtypes = [vp, vp]
        L.rtd_mog2_last_error.argtypes = [vp]
        L.rtd_mog2_last_error.restype = C.c_char_p
        L.rtd_mog2_destroy.argtypes = [vp]
        L.rtd_mog2_destroy.restype = None
        L.rtd_debug_mog2_model.argtypes = [vp, C.POINTER(i32), C.POINTER(i64), vp, vp, vp, vp, C.c_size_t]
        L.rtd_debug_mog2_fg_bits.argtypes = [vp, vp, C.c_size_t]
    if hasattr(L, "rtd_jpeg_create"):          # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_jpeg_create.argtypes = [i32, C.POINTER(vp)]
        L.rtd_jpeg_encode.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), i32, i32, vp, i64, C.POINTER(i64)]
        L.rtd_jpeg_wait_stream.argtypes = [vp, vp]
        L.rtd_jpeg_last_error.argtypes = [vp]
        L.rtd_jpeg_last_error.restype = C.c_char_p
        L.rtd_jpeg_destroy.argtypes = [vp]
        L.rtd_jpeg_destroy.restype = None
        L.rtd_debug_jpeg_coefficients.argtypes = [vp, vp, i64, C.POINTER(i64)]
    if hasattr(L, "rtd_overlay_create"):       # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_overlay_create.argtypes = [i32, C.POINTER(vp)]
        L.rtd_overlay_draw.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), i32, C.POINTER(i32), vp, vp, i64, C.POINTER(vp)]
        L.rtd_overlay_wait_stream.argtypes = [vp, vp]
        L.rtd_overlay_last_error.argtypes = [vp]
        L.rtd_overlay_last_error.restype = C.c_char_p
        L.rtd_overlay_destroy.argtypes = [vp]
        L.rtd_overlay_destroy.restype = None
        L.rtd_debug_overlay_tiles.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    if hasattr(L, "rtd_enhance_create"):       # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_enhance_create.argtypes = [i32, C.POINTER(RtdEnhanceParams), C.POINTER(vp)]
        L.rtd_enhance_layout.argtypes = [i32, C.POINTER(i32), C.POINTER(i64)]
        L.rtd_enhance_crops.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), vp, i64, vp]
        L.rtd_enhance_last_error.argtypes = [vp]
        L.rtd_enhance_last_error.restype = C.c_char_p
        L.rtd_enhance_destroy.argtypes = [vp]
        L.rtd_enhance_destroy.restype = None
        L.rtd_debug_enhance_stage.argtypes = [vp, i32, i32, vp, C.c_size_t]
    if hasattr(L, "rtd_esrgan_create"):        # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_esrgan_create.argtypes = [C.POINTER(RtdEsrganConfig), vp, C.c_size_t, C.POINTER(vp)]
        L.rtd_esrgan_layout.argtypes = [i32, C.POINTER(i32), C.POINTER(i64)]
        L.rtd_esrgan_upscale.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), vp, i64, vp]
        L.rtd_esrgan_arena_bytes.argtypes = [vp]
        L.rtd_esrgan_arena_bytes.restype = i64
        L.rtd_esrgan_last_error.argtypes = [vp]
        L.rtd_esrgan_last_error.restype = C.c_char_p
        L.rtd_esrgan_destroy.argtypes = [vp]
        L.rtd_esrgan_destroy.restype = None
        L.rtd_debug_esrgan_tensor.argtypes = [vp, C.c_char_p, vp, i64, C.POINTER(i64)]
        L.rtd_op_conv_view.argtypes = [i32, vp, i32, vp, vp, vp, i32, vp, i32] + [i32] * 10
        L.rtd_bench_conv_act.argtypes = [i32] * 13 + [C.POINTER(f32)]
    if hasattr(L, "rtd_op_select_score"):      # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_op_msdeform_view.argtypes = [i32, vp, i32, i32, vp, vp, vp] + [i32] * 6 + [C.POINTER(i32), f32]
        L.rtd_op_select_score.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32]
        L.rtd_op_gather_ln.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, vp, i32]
        L.rtd_op_split_convert.argtypes = [i32, vp, vp, i64, i32, i64, i64]
        L.rtd_op_set_rows.argtypes = [i32, vp, i32, i32, vp, i32, i32, vp, i32]
        L.rtd_op_rowmax.argtypes = [vp, i32, i32, i32, vp]
        L.rtd_op_gather_rows.argtypes = [i32, vp, i32, i32, vp, i32, i32, i32, vp, i32]
        L.rtd_op_boxes.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp]
        L.rtd_op_add.argtypes = [i32, i32, i32, vp, vp, vp, i32, i32, i32, i32]
        L.rtd_op_postprocess.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp]
    if hasattr(L, "rtd_op_msdeform_discrete_view"):      # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_op_msdeform_discrete_view.argtypes = L.rtd_op_msdeform_view.argtypes
    if hasattr(L, "rtd_debug_conv_choice"):
        L.rtd_op_conv_avg.argtypes = [vp] * 9 + [i32] * 10
        L.rtd_op_conv_pool.argtypes = [vp, vp, vp, vp, i32, i32, i32]
        L.rtd_debug_conv_choice.argtypes = [i32] * 16 + [C.c_char_p, i32, C.POINTER(i32)]
        L.rtd_debug_last_conv.argtypes = [C.c_char_p, i32, C.POINTER(i32)]
        L.rtd_debug_conv_instantiations.argtypes = [C.c_char_p, i64, C.POINTER(i64)]
    if hasattr(L, "rtd_op_conv_views"):        # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_op_conv_views.argtypes = [i32, vp, i32, vp, i32, i32, vp, vp, vp, i32, vp, i32] + [i32] * 12
        L.rtd_debug_conv_choice_views.argtypes = [i32] * 17 + [C.c_char_p, i32, C.POINTER(i32)]
    if hasattr(L, "rtd_ingest_create"):        # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_ingest_create.argtypes = [i32, C.POINTER(vp)]
        L.rtd_ingest_convert.argtypes = [vp, i32, C.POINTER(RtdYuvFrame), i32, C.POINTER(vp)]
        L.rtd_ingest_wait_stream.argtypes = [vp, vp]
        L.rtd_ingest_last_error.argtypes = [vp]
        L.rtd_ingest_last_error.restype = C.c_char_p
        L.rtd_ingest_destroy.argtypes = [vp]
        L.rtd_ingest_destroy.restype = None
        L.rtd_debug_ingest_info.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), i32, C.POINTER(RtdYuvFrame), C.POINTER(i64)]
    if hasattr(L, "rtd_ingest_resize"):        # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_ingest_convert_resize.argtypes = [vp, i32, C.POINTER(RtdYuvFrame), i32, C.POINTER(i32), C.POINTER(vp), C.POINTER(vp)]
        L.rtd_ingest_resize.argtypes = [vp, i32, C.POINTER(RtdBgrFrame), i32, C.POINTER(i32), C.POINTER(vp)]
        L.rtd_debug_resize_table.argtypes = [i32, i32, i32, C.POINTER(i32), i32, i32, C.POINTER(i32), C.POINTER(i32)]
    if hasattr(L, "rtd_op_stem0_u8"):          # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_op_stem0_u8.argtypes = [C.POINTER(vp), i32, i32, i32, vp, vp, vp, i32]
    if hasattr(L, "rtd_facemask_create"):      # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_facemask_create.argtypes = [i32, C.POINTER(vp)]
        L.rtd_facemask_apply.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), i32, i32, C.POINTER(RtdFaceRect)]
        L.rtd_facemask_gray.argtypes = [vp, vp, i32, i32, vp]
        L.rtd_facemask_wait_stream.argtypes = [vp, vp]
        L.rtd_facemask_last_error.argtypes = [vp]
        L.rtd_facemask_last_error.restype = C.c_char_p
        L.rtd_facemask_destroy.argtypes = [vp]
        L.rtd_facemask_destroy.restype = None
        L.rtd_debug_facemask_plan.argtypes = [i32, C.POINTER(i32), i32, C.POINTER(RtdFaceRect), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32),
                                              C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), i32, C.POINTER(C.c_uint16)]
    if hasattr(L, "rtd_eva_create"):           # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_eva_create.argtypes = [C.POINTER(RtdEvaConfig), vp, C.c_size_t, C.POINTER(vp)]
        L.rtd_eva_forward.argtypes = [vp, vp, i32, vp, vp]
        L.rtd_eva_self_check.argtypes = [vp, C.POINTER(i64)]
        L.rtd_eva_arena_bytes.argtypes = [vp]
        L.rtd_eva_arena_bytes.restype = i64
        L.rtd_eva_last_error.argtypes = [vp]
        L.rtd_eva_last_error.restype = C.c_char_p
        L.rtd_eva_close.argtypes = [vp]
        L.rtd_eva_close.restype = None
        L.rtd_debug_eva_tensor.argtypes = [vp, C.c_char_p, vp, i64, C.POINTER(i64)]
        L.rtd_op_eva_patchify.argtypes = [i32, vp, vp, i32, i32, i32]
        L.rtd_op_eva_rope.argtypes = [i32, vp, vp, vp, i32, i32, i32]
        L.rtd_op_eva_layernorm.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32]
        L.rtd_op_eva_attention.argtypes = [i32, vp, vp, i32, i32, i32]
    if hasattr(L, "rtd_yolox_post_create"):    # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_yolox_anchors.argtypes = [i32, i32, C.POINTER(i32)]
        L.rtd_yolox_post_create.argtypes = [C.POINTER(RtdYoloxPostConfig), C.POINTER(vp)]
        L.rtd_yolox_post_run.argtypes = [vp, i32, vp, i32, C.POINTER(RtdYoloxPostParams), vp, vp, vp]
        L.rtd_yolox_post_last_error.argtypes = [vp]
        L.rtd_yolox_post_last_error.restype = C.c_char_p
        L.rtd_yolox_post_destroy.argtypes = [vp]
        L.rtd_yolox_post_destroy.restype = None
    if hasattr(L, "rtd_yolox_net_create"):     # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_yolox_net_create.argtypes = [C.POINTER(RtdYoloxNetConfig), vp, C.c_size_t, C.POINTER(vp)]
        L.rtd_yolox_net_run.argtypes = [vp, i32, vp, i32, i32, vp, vp]
        L.rtd_yolox_net_arena_bytes.argtypes = [vp]
        L.rtd_yolox_net_arena_bytes.restype = i64
        L.rtd_yolox_net_last_error.argtypes = [vp]
        L.rtd_yolox_net_last_error.restype = C.c_char_p
        L.rtd_yolox_net_destroy.argtypes = [vp]
        L.rtd_yolox_net_destroy.restype = None
        L.rtd_debug_yolox_tensor.argtypes = [vp, C.c_char_p, vp, i64, C.POINTER(i64)]
        L.rtd_op_yolox_focus.argtypes = [i32, vp, vp, i32, i32, i32]
        L.rtd_op_yolox_spp.argtypes = [i32, vp, i32, i32, i32, i32]
        L.rtd_op_yolox_head_emit.argtypes = [C.POINTER(vp), C.POINTER(vp), i32, i32, i32, i32, i32, i32, vp]
    if hasattr(L, "rtd_yolox_net_run_frames"):    # (absent from older builds loaded through RTD_LIB_PATH)
        L.rtd_yolox_net_run_frames.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), i32, i32, vp, vp]
        L.rtd_op_yolox_focus_u8.argtypes = [i32, C.POINTER(vp), C.POINTER(i32), i32, i32, i32, vp]
    if hasattr(L, "rtd_debug_yolox_plan_convs"):  # (absent from older builds loaded through RTD_LIB_PATH)
        for fn in (L.rtd_debug_yolox_plan_convs, L.rtd_debug_eva_plan_convs, L.rtd_debug_esrgan_plan_convs):
            fn.argtypes = [vp, C.c_char_p, i64, C.POINTER(i64)]
    _lib = L
    return L


def debug_option(name: str, value: int) -> None:
    rc = lib().rtd_debug_option(name.encode(), int(value))
    if rc != RTD_OK:
        raise ValueError(f"unknown debug option {name!r}")


def _conv_report(call, *args):
    key, info = C.create_string_buffer(64), (C.c_int32 * 12)()
    rc = call(*args, key, 64, info)
    if rc != RTD_OK:
        return None
    return dict(zip(CONV_INFO_FIELDS, info), key=key.value.decode())


def conv_choice(dtype: int, B: int, H: int, W: int, Cin: int, Cout: int, k: int = 1, stride: int = 1, pad: int = 0, res_mode: int = 0,
                out_f32: int = 0, C2: int = 0, x_up2: int = 0, Cnext: int = 0, avg: int = 0, pool: int = 0):
    """What launch_conv would launch for this launch under the debug options as they stand (rtd_debug_conv_choice: no GPU needed):
    {'key': ..., 'family': ..., 'S': ..., 'grid': ...}, or None when the launchers refuse it."""
    return _conv_report(lib().rtd_debug_conv_choice, dtype, B, H, W, Cin, C2, Cout, k, stride, pad, res_mode, out_f32, x_up2, Cnext, avg, pool)


def conv_choice_views(dtype: int, B: int, H: int, W: int, Cin: int, Cout: int, ldx: int, ldy: int, k: int = 1, stride: int = 1, pad: int = 0,
                      res_mode: int = 0, ldres: int = 0, out_f32: int = 0, C2: int = 0, ldx2: int = 0, x_up2: int = 0):
    """conv_choice for the launch rtd_op_conv_views describes (rtd_debug_conv_choice_views): channel-slice views with pixel strides ld*."""
    return _conv_report(lib().rtd_debug_conv_choice_views, dtype, ldx, C2, ldx2, ldres, ldy, B, H, W, Cin, Cout, k, stride, pad, res_mode, out_f32, x_up2)


def last_conv():
    """What this thread's last launch_conv / launch_conv_pool launched (rtd_debug_last_conv); None before the first."""
    return _conv_report(lib().rtd_debug_last_conv)


PLAN_CONV_FIELDS = ("dtype", "B", "H", "W", "Cin", "Cout", "k", "stride", "pad", "act", "res_mode", "out_f32", "ldx", "ldy", "ldres")


def plan_convs(prefix: str, handle) -> list:
    """The conv launches of a network handle's last plan (rtd_debug_<yolox|eva|esrgan>_plan_convs; prefix: "yolox", "eva" or "esrgan"),
    in execution order: dicts of name, PLAN_CONV_FIELDS (codes as the C ABI has them), key, S and grid.  Raises RtdError before the first run."""
    call = getattr(lib(), f"rtd_debug_{prefix}_plan_convs")
    need = C.c_int64(0)
    rc = call(handle, None, 0, C.byref(need))
    buf = C.create_string_buffer(max(int(need.value), 1))
    rc = rc or call(handle, buf, need.value, None)
    if rc != RTD_OK:
        raise RtdError(rc, f"rtd_debug_{prefix}_plan_convs failed")
    out = []
    for line in buf.value.decode().splitlines():
        w = line.split()
        out.append(dict(zip(PLAN_CONV_FIELDS, (int(v) for v in w[1:16])), name=w[0], key=w[16], S=int(w[17]), grid=int(w[18])))
    return out


def conv_instantiations() -> list:
    """The key of every conv kernel instantiation the launchers can name (rtd_debug_conv_instantiations)."""
    need = C.c_int64(0)
    lib().rtd_debug_conv_instantiations(None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value)
    rc = lib().rtd_debug_conv_instantiations(buf, need.value, None)
    assert rc == RTD_OK, rc
    return buf.value.decode().split()


class RtdError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rtd error {code}: {msg}")
        self.code = code


def _stats_of(handle) -> dict:
    st = RtdStats()
    if not handle or lib().rtd_get_stats(handle, C.byref(st)) != RTD_OK:
        return {}
    return {k: (float(getattr(st, k)) if k == "max_abs_filter" else int(getattr(st, k))) for k, _ in RtdStats._fields_ if k not in ("struct_size", "reserved")}


def _raise_msg(code: int, what: str, msg: bytes, suffix: str = ""):
    msg = (msg or b"").decode(errors="replace") + suffix
    if code == RTD_E_OOM:
        import torch
        # the only exception the reference's degrade path reacts to (src/inference_engine_yolox.py:607)
        raise torch.cuda.OutOfMemoryError(f"HIP out of memory in {what}: {msg}")
    raise RtdError(code, msg)


def _raise(code: int, handle=None) -> None:
    """the handle-less form: the calling thread's last refused rtd_create / rtd_op_* / rtd_crop_resize_batch (a call on a handle
    raises through Handle._raise)"""
    assert handle is None
    _raise_msg(code, Engine._what, lib().rtd_last_error(None))


# ---- the twelve handles (the engine; motion, mog2, jpeg, overlay, enhance, esrgan, ingest, facemask, eva, yolox_post, yolox_net) ------------------------------------------------------
def device_index(device) -> int:
    """an int, None (torch's current device), a torch.device or a string like 'cuda:1' -> the device's index"""
    if isinstance(device, int):
        return device
    if device is None:
        import torch
        return torch.cuda.current_device() if torch.cuda.is_available() else 0
    if hasattr(device, "index"):                  # torch.device
        return device.index or 0
    s = str(device)
    return int(s.split(":")[1]) if ":" in s else 0


def frame_ptrs(frames, on_device: bool):
    """HxWxC uint8 frames (C-contiguous numpy arrays, or contiguous device tensors when on_device) -> (addresses, shapes)"""
    return ([f.data_ptr() if on_device else f.ctypes.data for f in frames],
            [(int(f.shape[0]), int(f.shape[1]), int(f.shape[2])) for f in frames])


def c_frames(ptrs, shapes):
    """(addresses, shapes) -> (n, void* [n], int32 hwc [n][3]) as the rtd_* calls take them; never zero-length arrays"""
    n = len(ptrs)
    return n, (C.c_void_p * max(n, 1))(*ptrs), (C.c_int32 * max(3 * n, 1))(*[int(v) for s in shapes for v in s])


class Handle:
    """One handle of the engine or of a stand-alone back end: rtd_<x>_create / _last_error / _destroy, and _wait_stream where the back end owns a
    stream.  A subclass names its functions' prefix and what the out-of-memory message calls it."""
    _prefix = ""          # "rtd_jpeg"
    _what = ""            # "the JPEG encoder"

    def _fn(self, name: str):
        return getattr(self._L, f"{self._prefix}_{name}")

    def _open(self, *args) -> None:
        """rtd_<x>_create(*args, &handle)"""
        self._L = lib()
        self._h = C.c_void_p()
        rc = self._fn("create")(*args, C.byref(self._h))
        if rc != RTD_OK:
            self._h = C.c_void_p()        # (the message of a refused create is the one rtd_<x>_last_error(NULL) reports)
            self._raise(rc)

    def _raise(self, rc: int):
        _raise_msg(rc, self._what, self._fn("last_error")(self._h))

    def _check(self, rc: int) -> None:
        if rc != RTD_OK:
            self._raise(rc)

    def wait_stream(self, producer_stream: int) -> None:
        """The handle's stream waits for everything enqueued so far on `producer_stream` (a raw hipStream_t value; 0 = the default
        stream)."""
        self._check(self._fn("wait_stream")(self._h, C.c_void_p(int(producer_stream) or None)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MAX_CROPS_PER_CALL = 64       # rtd_enhance_crops, rtd_esrgan_upscale


def crop_layout(prefix: str, rects) -> list:
    """rtd_<x>_layout: byte offsets of the crops (x1, y1, x2, y2) in the output buffer, plus its size.  Host arithmetic only."""
    n = len(rects)
    rc = (C.c_int32 * max(4 * n, 1))(*[int(v) for r in rects for v in r])
    offsets = (C.c_int64 * (n + 1))()
    code = getattr(lib(), prefix + "_layout")(n, rc, offsets)
    if code != RTD_OK:
        raise RtdError(code, (getattr(lib(), prefix + "_last_error")(None) or b"").decode(errors="replace"))
    return list(offsets)


class CropHandle(Handle):
    """A back end whose call takes crops of device-resident frames and writes them, packed by its layout, into one buffer on the
    caller's stream (enhance, esrgan)."""
    _timing = None

    def _crop_call(self, call: str, scale: int, frames, rects_per_frame):
        """frames: device uint8 HWC BGR tensors; rects_per_frame: per frame a list of (x1, y1, x2, y2).  Returns (buffer, offsets,
        shapes): one uint8 device tensor holding every output crop (frame-major order), crop i being buffer[offsets[i]:][:h * w * 3]
        viewed as (h, w, 3) with shapes[i] = (h, w), `scale` times the rectangle; offsets has one more entry, the buffer's size.
        Enqueued on torch's current stream: the buffer is ready when that stream reaches it."""
        import torch

        flat = [(f, tuple(int(v) for v in r)) for f, rects in zip(frames, rects_per_frame) for r in rects]
        dev = frames[0].device if len(frames) else torch.device("cuda", self.device)
        offsets = crop_layout(self._prefix, [r for _, r in flat])
        shapes = [(scale * (r[3] - r[1]), scale * (r[2] - r[0])) for _, r in flat]
        buf = torch.empty((offsets[-1],), dtype=torch.uint8, device=dev)
        if not flat:
            return buf, offsets, shapes
        stream = torch.cuda.current_stream(dev)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        for i0 in range(0, len(flat), MAX_CROPS_PER_CALL):
            part = flat[i0:i0 + MAX_CROPS_PER_CALL]
            k = len(part)
            ptrs = (C.c_void_p * k)()
            hw = (C.c_int32 * (2 * k))()
            rc = (C.c_int32 * (4 * k))()
            for i, (f, r) in enumerate(part):
                assert f.is_cuda and f.dtype == torch.uint8 and f.is_contiguous() and f.dim() == 3 and f.shape[2] == 3
                ptrs[i] = f.data_ptr()
                hw[2 * i], hw[2 * i + 1] = int(f.shape[0]), int(f.shape[1])
                rc[4 * i:4 * i + 4] = r
            # the offsets of a chunk are the layout's for the whole list, relative to the chunk's first crop
            self._check(self._fn(call)(self._h, k, ptrs, hw, rc, C.c_void_p(buf.data_ptr() + offsets[i0]), offsets[-1] - offsets[i0],
                                       C.c_void_p(stream.cuda_stream)))
        ev1.record(stream)
        self._timing = (ev0, ev1)
        return buf, offsets, shapes

    def last_call_ms(self) -> Optional[float]:
        """device time of the last crop call in milliseconds (waits for it); None before the first call"""
        if self._timing is None:
            return None
        ev0, ev1 = self._timing
        ev1.synchronize()
        return float(ev0.elapsed_time(ev1))


PROFILE_LATENCY, PROFILE_THROUGHPUT = 0, 1


def make_config(arch: Arch, device: int, precision: int, max_batch: int, input_size, use_graph: bool,
                profile: int = PROFILE_LATENCY) -> RtdConfig:
    c = RtdConfig()
    c.struct_size = C.sizeof(RtdConfig)
    c.device, c.precision, c.max_batch = device, precision, max_batch
    c.input_h, c.input_w = int(input_size[0]), int(input_size[1])
    c.use_graph = 1 if use_graph else 0
    c.layer_type = 1 if arch.layer_type == "bottleneck" else 0
    c.depths = (C.c_int32 * 4)(*arch.depths)
    c.hidden_sizes = (C.c_int32 * 4)(*arch.hidden_sizes)
    c.embedding_size = arch.embedding_size
    c.enc_dim, c.enc_ffn, c.enc_heads, c.csp_hidden = arch.enc_dim, arch.enc_ffn, arch.enc_heads, arch.csp_hidden
    c.d_model, c.dec_ffn, c.dec_heads, c.dec_layers = arch.d_model, arch.dec_ffn, arch.dec_heads, arch.dec_layers
    c.num_queries, c.num_classes, c.n_levels, c.n_points = arch.num_queries, arch.num_classes, arch.n_levels, arch.n_points
    c.offset_scale = arch.offset_scale
    c.profile = profile
    c.dec_method = DEC_METHODS[arch.dec_method]
    return c


def cfg_for(arch: Arch, device: int = 0, precision: int = PREC_F16X3, max_batch: int = 1, input_size=(640, 640), use_graph: bool = False,
            profile: int = PROFILE_LATENCY) -> RtdConfig:
    """the rtd_config of `arch` with plain defaults for everything else (tests, tools)"""
    return make_config(arch, device, precision, max_batch, input_size, use_graph, profile)


class Engine(Handle):
    """Thin RAII wrapper of one rtd_handle."""
    _prefix = "rtd"
    _what = "libmi355rtdetr"

    def __init__(self, arch: Arch, blob: bytes, device: int = 0, precision: int = PREC_BF16, max_batch: int = 8,
                 input_size=(640, 640), use_graph: bool = True, profile: int = PROFILE_LATENCY, prepare=()):
        self.arch = arch
        self.num_queries = arch.num_queries
        self.max_batch = max_batch
        self._open(C.byref(make_config(arch, device, precision, max_batch, input_size, use_graph, profile)))
        try:
            self._check(self._fn("load_weights")(self._h, (C.c_char * len(blob)).from_buffer_copy(blob), len(blob)))
            for n in sorted({int(b) for b in prepare}):    # plan + arena + hipGraph of every declared batch size: the serving path only replays
                self.prepare(n)
        except BaseException:
            self.close()
            raise

    def _raise(self, rc: int):
        st = self.stats()
        # a failure describes itself: what the handle had done when it happened, and whether its stream is in capture state
        suffix = " | handle: " + ", ".join(f"{k}={v}" for k, v in st.items()) if st else ""
        _raise_msg(rc, self._what, self._fn("last_error")(self._h), suffix)

    def prepare(self, n: int):
        self._check(self._fn("prepare")(self._h, int(n)))

    # ---- helpers
    @staticmethod
    def _frame_args(frames, on_device: bool):
        n = len(frames)
        ptrs = (C.c_void_p * n)()
        hw = (C.c_int32 * (2 * n))()
        keep = []
        for i, f in enumerate(frames):
            if on_device:
                assert f.dtype.__str__() == "torch.uint8" and f.is_contiguous() and f.dim() == 3 and f.shape[2] == 3
                ptrs[i] = f.data_ptr()
                hw[2 * i], hw[2 * i + 1] = int(f.shape[0]), int(f.shape[1])
            else:
                a = np.ascontiguousarray(f, dtype=np.uint8)
                assert a.ndim == 3 and a.shape[2] == 3, "frames must be HxWx3 uint8 BGR"
                keep.append(a)
                ptrs[i] = a.ctypes.data
                hw[2 * i], hw[2 * i + 1] = a.shape[0], a.shape[1]
        return n, ptrs, hw, keep

    def infer(self, frames, conf: float, wildlife_only: bool, on_device: bool = False):
        n, ptrs, hw, keep = self._frame_args(frames, on_device)
        out = np.zeros((n, self.num_queries), dtype=DET_DTYPE)
        counts = (C.c_int32 * n)()
        self._check(self._fn("infer")(self._h, n, ptrs, hw, int(on_device), float(conf), int(bool(wildlife_only)), out.ctypes.data, counts))
        return [out[i, : counts[i]] for i in range(n)]

    def infer_raw(self, frames, on_device: bool = False):
        n, ptrs, hw, keep = self._frame_args(frames, on_device)
        Q = self.num_queries
        labels = np.zeros((n, Q), np.int32)
        boxes = np.zeros((n, Q, 4), np.float32)
        scores = np.zeros((n, Q), np.float32)
        self._check(self._fn("infer_raw")(self._h, n, ptrs, hw, int(on_device), labels.ctypes.data, boxes.ctypes.data, scores.ctypes.data))
        return labels, boxes, scores

    def infer_async(self, frames, on_device: bool = True):
        """Enqueue one batch and return.  Host frames are staged inside the library (pinned buffer + one DMA): the arrays may be
        released at once; device frames must stay alive until collect() / sync()."""
        n, ptrs, hw, keep = self._frame_args(frames, on_device)
        self._check(self._fn("infer_async")(self._h, n, ptrs, hw, int(on_device)))
        return n

    def collect(self, conf: float, wildlife_only: bool):
        """Wait for the batch of the last infer_async and return what infer() returns for it."""
        out = np.zeros((self.max_batch, self.num_queries), dtype=DET_DTYPE)
        counts = (C.c_int32 * self.max_batch)()
        self._check(self._fn("collect")(self._h, float(conf), int(bool(wildlife_only)), out.ctypes.data, counts))
        return out, counts

    def make_async_args(self, frames_dev):
        """Pre-marshal (n, ptrs, hw) once so a benchmark loop does no Python work per step."""
        return self._frame_args(frames_dev, True)

    def infer_async_prepared(self, args):
        self._check(self._fn("infer_async")(self._h, args[0], args[1], args[2], 1))

    def wait_stream(self, producer_stream: int):
        """The engine's stream waits for everything enqueued so far on `producer_stream` (a raw hipStream_t value, e.g.
        torch.cuda.current_stream().cuda_stream; 0 = the default stream)."""
        self._check(self._fn("wait_stream")(self._h, C.c_void_p(int(producer_stream) or None)))

    def signal_stream(self, consumer_stream: int):
        """`consumer_stream` waits for everything enqueued so far on the engine's stream."""
        self._check(self._fn("signal_stream")(self._h, C.c_void_p(int(consumer_stream) or None)))

    def stats(self) -> dict:
        return _stats_of(self._h)

    def preprocess_into(self, frame, on_device: bool, out_ptr: int) -> None:
        """rtd_preprocess: one HWC uint8 BGR frame (numpy array, or a contiguous device tensor when on_device) -> [3, H, W] fp32 at out_ptr (device)."""
        h, w = int(frame.shape[0]), int(frame.shape[1])
        src = frame.data_ptr() if on_device else frame.ctypes.data
        self._check(self._fn("preprocess")(self._h, C.c_void_p(src), h, w, int(on_device), C.c_void_p(out_ptr)))

    def self_check(self, blob: bytes) -> dict:
        """rtd_self_check: this engine's arithmetic against the library's exact fp32 engine on one built-in frame, with the weights of
        `blob` (the container this engine was loaded from: the handle keeps no host copy)."""
        rep = RtdCheckReport()
        rep.struct_size = C.sizeof(RtdCheckReport)
        self._check(self._fn("self_check")(self._h, blob, len(blob), C.byref(rep)))
        return {"rows": rep.rows, "rows_matched": rep.rows_matched, "worst_score_err": rep.worst_score_err, "worst_box_err_px": rep.worst_box_err_px,
                "score_tol": rep.score_tol, "box_tol_px": rep.box_tol_px, "saturated_values": rep.saturated_values,
                "max_abs_filter": rep.max_abs_filter, "max_abs_filter_name": rep.max_abs_filter_name.decode(errors="replace")}

    def result_block(self):
        p = C.c_void_p()
        n = C.c_int64()
        self._check(self._fn("result_block")(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def sync(self):
        self._check(self._fn("sync")(self._h))

    def stream(self) -> int:
        return lib().rtd_stream(self._h) or 0

    def debug_tensor(self, name: str) -> np.ndarray:
        shape = (C.c_int64 * 4)()
        self._check(self._fn("debug_tensor")(self._h, name.encode(), None, 0, shape))
        out = np.zeros(tuple(shape), np.float32)
        self._check(self._fn("debug_tensor")(self._h, name.encode(), out.ctypes.data, out.size, shape))
        return out

    def force_topk(self, idx: Optional[np.ndarray]):
        a = None if idx is None else np.ascontiguousarray(idx, np.int32)
        self._check(self._fn("debug_force_topk")(self._h, None if a is None else a.ctypes.data, 0 if a is None else a.shape[0]))

    def profile(self, n: int, reps: int = 5):
        cnt = C.c_int32()
        self._check(self._fn("profile")(self._h, n, reps, None, 0, C.byref(cnt)))
        arr = (RtdLayerTime * cnt.value)()
        self._check(self._fn("profile")(self._h, n, reps, arr, cnt.value, C.byref(cnt)))
        return [dict(name=a.name.decode(), kernel=a.kernel.decode(), ms=a.ms, flops=a.flops, bytes=a.bytes) for a in arr]

    def arena_bytes(self) -> int:
        return lib().rtd_arena_bytes(self._h)
