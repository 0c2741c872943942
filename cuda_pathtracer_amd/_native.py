"""ctypes binding of libpt_amd.so (the C ABI declared in include/pt_amd.h and include/sc_amd.h).

The library is REQUIRED: there is no CPU fallback anywhere in this package.  If the shared object
is missing or fails to load, every entry point raises NativeLibraryError.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["PT_AMD_LIB"]) if os.environ.get("PT_AMD_LIB") else _PKG / "libpt_amd.so"


class NativeLibraryError(RuntimeError):
    pass


class PtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[pt error {code}] {msg}")
        self.code = code


# ---- C structs (same layout as include/pt_amd.h) -------------------------------------------
class Flags(C.Structure):
    _fields_ = [("russian_roulette", C.c_int32), ("use_bvh", C.c_int32), ("use_bbox", C.c_int32),
                ("sort_by_material", C.c_int32), ("use_thrust_partition", C.c_int32), ("ssaa", C.c_int32),
                ("dof", C.c_int32), ("aperture", C.c_float), ("focal_dist", C.c_float),
                ("single_albedo", C.c_int32), ("bvh_cull", C.c_int32), ("shared_gpu", C.c_int32),
                ("rng_key_pixel", C.c_int32)]


class Material(C.Structure):
    _fields_ = [("color", C.c_float * 3), ("spec_exponent", C.c_float), ("spec_color", C.c_float * 3),
                ("has_reflective", C.c_float), ("has_refractive", C.c_float), ("ior", C.c_float),
                ("emittance", C.c_float), ("texture_id", C.c_int32)]


class Geom(C.Structure):
    _fields_ = [("type", C.c_int32), ("material_id", C.c_int32), ("translation", C.c_float * 3),
                ("rotation", C.c_float * 3), ("scale", C.c_float * 3), ("transform", C.c_float * 16),
                ("inverse_transform", C.c_float * 16), ("inv_transpose", C.c_float * 16),
                ("tri_start", C.c_int32), ("tri_end", C.c_int32), ("bbox_idx", C.c_int32),
                ("min_bound", C.c_float * 3), ("max_bound", C.c_float * 3)]


class Camera(C.Structure):
    _fields_ = [("res", C.c_int32 * 2), ("position", C.c_float * 3), ("look_at", C.c_float * 3),
                ("view", C.c_float * 3), ("up", C.c_float * 3), ("right", C.c_float * 3),
                ("fov", C.c_float * 2), ("pixel_length", C.c_float * 2)]


class Triangle(C.Structure):
    _fields_ = [("id", C.c_int32), ("v", (C.c_float * 3) * 3), ("uv", (C.c_float * 2) * 3),
                ("n", (C.c_float * 3) * 3), ("bmin", C.c_float * 3), ("bmax", C.c_float * 3)]


class BvhNode(C.Structure):
    _fields_ = [("bmin", C.c_float * 3), ("bmax", C.c_float * 3), ("sub_areas", C.c_int32),
                ("axis", C.c_int32), ("first_area_idx", C.c_int32), ("rchild_idx", C.c_int32)]


class Shard(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("spp", C.c_int32), ("reserved", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("passes", C.c_uint64), ("bounce_live", C.c_uint64 * 64),
                ("emissive_hits", C.c_uint64), ("bounce_emit", C.c_uint64 * 64), ("device_error", C.c_uint32),
                ("bound_mismatch", C.c_uint32)]


class BoundInfo(C.Structure):
    """pt_bound_info: one geom's row of pt_scene_bound_info."""
    _fields_ = [("bkind", C.c_int32), ("slo", C.c_float * 3), ("shi", C.c_float * 3), ("wlo", C.c_float * 3),
                ("whi", C.c_float * 3), ("tight", C.c_float * 6), ("tslack", C.c_float), ("back", C.c_float),
                ("wback", C.c_float)]


class BoundsReport(C.Structure):
    """pt_bounds_report: what pt_selftest_bounds counts."""
    _fields_ = [("pairs", C.c_uint64 * 5), ("bad_tagged", C.c_uint64 * 5), ("bad_float", C.c_uint64 * 5),
                ("rays", C.c_uint64 * 6), ("skipped", C.c_uint64 * 6), ("has_first", C.c_uint32),
                ("first_geom", C.c_uint32), ("first_form", C.c_uint32), ("first_origin", C.c_uint32 * 3),
                ("first_dir", C.c_uint32 * 3), ("first_bound", C.c_uint32), ("first_t", C.c_uint32),
                ("pad_", C.c_uint32)]


class DenoiseParams(C.Structure):
    """pt_denoise_params; DenoiseParams.default() = pt_denoise_params_default."""
    _fields_ = [("levels", C.c_int32), ("sigma_c", C.c_float), ("sigma_n", C.c_float), ("sigma_p", C.c_float),
                ("demodulate", C.c_int32), ("reserved", C.c_int32 * 3)]

    @classmethod
    def default(cls) -> "DenoiseParams":
        p = cls()
        lib().pt_denoise_params_default(C.byref(p))
        return p


class DenoiseVarParams(C.Structure):
    """pt_denoise_var_params; DenoiseVarParams.default() = pt_denoise_var_params_default."""
    _fields_ = [("levels", C.c_int32), ("sigma_l", C.c_float), ("sigma_n", C.c_float), ("sigma_p", C.c_float),
                ("demodulate", C.c_int32), ("reserved", C.c_int32 * 3)]

    @classmethod
    def default(cls) -> "DenoiseVarParams":
        p = cls()
        lib().pt_denoise_var_params_default(C.byref(p))
        return p


class TemporalParams(C.Structure):
    """pt_temporal_params; TemporalParams.default() = pt_temporal_params_default."""
    _fields_ = [("max_history", C.c_float), ("min_ndot", C.c_float), ("plane_tol", C.c_float),
                ("demodulate", C.c_int32), ("min_frames", C.c_int32), ("reserved", C.c_int32 * 3)]

    @classmethod
    def default(cls) -> "TemporalParams":
        p = cls()
        lib().pt_temporal_params_default(C.byref(p))
        return p


class AdaptiveParams(C.Structure):
    """pt_adaptive_params; AdaptiveParams.default() = pt_adaptive_params_default."""
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("min_batches", C.c_int32), ("dilate", C.c_int32),
                ("reserved", C.c_int32 * 4)]

    @classmethod
    def default(cls) -> "AdaptiveParams":
        p = cls()
        lib().pt_adaptive_params_default(C.byref(p))
        return p


class JpegParams(C.Structure):
    """pt_jpeg_params; JpegParams.default() = pt_jpeg_params_default (quality 90, 4:2:0, no mirror)."""
    _fields_ = [("quality", C.c_int32), ("subsampling", C.c_int32), ("mirror_x", C.c_int32), ("reserved", C.c_int32 * 5)]

    @classmethod
    def default(cls) -> "JpegParams":
        p = cls()
        lib().pt_jpeg_params_default(C.byref(p))
        return p


JPEG_444, JPEG_420 = 0, 1   # PT_JPEG_*
assert C.sizeof(JpegParams) == 32


class PngParams(C.Structure):
    """pt_png_params; PngParams.default() = pt_png_params_default (adaptive filter, 32 KiB deflate blocks,
    the preview's conversion, no mirror)."""
    _fields_ = [("filter", C.c_int32), ("block_bytes", C.c_int32), ("conv", C.c_int32), ("mirror_x", C.c_int32),
                ("reserved", C.c_int32 * 4)]

    @classmethod
    def default(cls) -> "PngParams":
        p = cls()
        lib().pt_png_params_default(C.byref(p))
        return p


PNG_FILTER_ADAPTIVE = 5                  # PT_PNG_FILTER_ADAPTIVE
PNG_CONV_PREVIEW, PNG_CONV_SAVE = 0, 1   # PT_PNG_CONV_*
assert C.sizeof(PngParams) == 32


class HdrParams(C.Structure):
    """pt_hdr_params; HdrParams.default() = pt_hdr_params_default (no mirror)."""
    _fields_ = [("mirror_x", C.c_int32), ("reserved", C.c_int32 * 7)]

    @classmethod
    def default(cls) -> "HdrParams":
        p = cls()
        lib().pt_hdr_params_default(C.byref(p))
        return p


assert C.sizeof(HdrParams) == 32


class ExrParams(C.Structure):
    """pt_exr_params; ExrParams.default() = pt_exr_params_default (ZIP, 32 KiB deflate blocks, no mirror)."""
    _fields_ = [("compression", C.c_int32), ("block_bytes", C.c_int32), ("mirror_x", C.c_int32), ("reserved", C.c_int32 * 5)]

    @classmethod
    def default(cls) -> "ExrParams":
        p = cls()
        lib().pt_exr_params_default(C.byref(p))
        return p


class ExrChannel(C.Structure):
    """pt_exr_channel: a name of 1 to 31 bytes from [A-Za-z0-9_.] and EXR_UINT, EXR_HALF or EXR_FLOAT."""
    _fields_ = [("name", C.c_char * 32), ("type", C.c_int32)]

    def __init__(self, name="", type=2):
        super().__init__((name.encode() if isinstance(name, str) else bytes(name))[:32], int(type))


class ExrPlane(C.Structure):
    """pt_exr_plane: a device pointer, the floats between two pixels and the divisor."""
    _fields_ = [("d", C.c_void_p), ("stride", C.c_int32), ("divisor", C.c_float)]


EXR_UINT, EXR_HALF, EXR_FLOAT = 0, 1, 2   # PT_EXR_* pixel types
EXR_NONE, EXR_ZIPS, EXR_ZIP = 0, 2, 3     # PT_EXR_* compressions
EXR_BEAUTY, EXR_ALBEDO, EXR_NORMAL, EXR_POSITION, EXR_DEPTH, EXR_UV, EXR_ID = 1, 2, 4, 8, 16, 32, 64   # PT_EXR_* layers
EXR_ALL_LAYERS = 127
assert C.sizeof(ExrParams) == 32 and C.sizeof(ExrChannel) == 36 and C.sizeof(ExrPlane) == 16


class DisplayParams(C.Structure):
    """pt_display_params; DisplayParams.default() = pt_display_params_default (manual exposure 1, no curve,
    linear transfer, no mirror: pt_tonemap's conversion)."""
    _fields_ = [("exposure_mode", C.c_int32), ("exposure", C.c_float), ("key_value", C.c_float),
                ("compensation_ev", C.c_float), ("min_ev", C.c_float), ("max_ev", C.c_float), ("pct_lo", C.c_int32),
                ("pct_hi", C.c_int32), ("rate", C.c_int32), ("curve", C.c_int32), ("white", C.c_float),
                ("transfer", C.c_int32), ("mirror_x", C.c_int32), ("reserved", C.c_int32 * 3)]

    @classmethod
    def default(cls) -> "DisplayParams":
        p = cls()
        lib().pt_display_params_default(C.byref(p))
        return p


class EnvParams(C.Structure):
    """pt_env_params; EnvParams.default() = pt_env_params_default (scale 1, no rotation, size 0: derived)."""
    _fields_ = [("scale", C.c_float), ("rotate_deg", C.c_float * 3), ("size", C.c_int32)]

    @classmethod
    def default(cls) -> "EnvParams":
        p = cls()
        lib().pt_env_params_default(C.byref(p))
        return p


assert C.sizeof(EnvParams) == 20
DISPLAY_MANUAL, DISPLAY_AUTO = 0, 1                                      # PT_DISPLAY_* exposure modes
class BloomParams(C.Structure):
    """pt_bloom_params; BloomParams.default() = pt_bloom_params_default (threshold 1, strength 0.25, spread 0.75,
    clamp 65504, levels from the size)."""
    _fields_ = [("threshold", C.c_float), ("strength", C.c_float), ("spread", C.c_float), ("clamp", C.c_float),
                ("levels", C.c_int32), ("reserved", C.c_int32 * 3)]

    @classmethod
    def default(cls) -> "BloomParams":
        p = cls()
        lib().pt_bloom_params_default(C.byref(p))
        return p


DISPLAY_NONE, DISPLAY_REINHARD, DISPLAY_ACES, DISPLAY_HABLE = 0, 1, 2, 3  # curves
DISPLAY_LINEAR, DISPLAY_SRGB = 0, 1                                      # transfers
assert C.sizeof(DisplayParams) == 64 and C.sizeof(BloomParams) == 32
assert C.sizeof(DenoiseParams) == 32 and C.sizeof(DenoiseVarParams) == 32 and C.sizeof(TemporalParams) == 32
assert C.sizeof(AdaptiveParams) == 32
assert C.sizeof(Geom) == 272 and C.sizeof(Material) == 48 and C.sizeof(Triangle) == 124
assert C.sizeof(BvhNode) == 40

_P = C.c_void_p
_I = C.c_int32
_F = C.c_float
_FP = C.POINTER(C.c_float)
_IP = C.POINTER(C.c_int32)

# name -> (restype, argtypes).  Every function declared in include/*.h appears here.
SIGNATURES = {
    # sc_amd.h
    "sc_last_error": (C.c_char_p, []),
    "sc_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "sc_scan_exclusive_i32": (_I, [_P, _P, C.c_int64, _P, _P]),
    "sc_compact_i32": (_I, [_P, _P, C.c_int64, _P, _P, _P]),
    "sc_partition_i32": (_I, [_P, _P, C.c_int64, _P, _P, _P]),
    "sc_partition_indices": (_I, [_P, _P, C.c_int64, _P, _P, _P]),
    "sc_efficient_scan": (_I, [C.c_int, _P, _P]),
    "sc_efficient_compact": (_I, [C.c_int, _P, _P, _IP]),
    "sc_timer_gpu_ms": (C.c_float, []),
    "sc_cpu_scan": (_I, [C.c_int, _P, _P]),
    "sc_cpu_compact_without_scan": (_I, [C.c_int, _P, _P, _IP]),
    "sc_cpu_compact_with_scan": (_I, [C.c_int, _P, _P, _IP]),
    "sc_naive_scan_i32": (_I, [_P, _P, C.c_int64, _P, _P]),
    "sc_thrust_scan_i32": (_I, [_P, _P, C.c_int64, _P]),
    "sc_naive_scan": (_I, [C.c_int, _P, _P]),
    "sc_thrust_scan": (_I, [C.c_int, _P, _P]),
    "sc_set_tile_schedule": (_I, [_I]),
    "sc_workspace_check": (_I, [_P]),
    "sc_workspace_error_word": (_P, [_P]),
    # pt_amd.h
    "pt_last_error": (C.c_char_p, []),
    "pt_flags_default": (None, [C.POINTER(Flags)]),
    "pt_scene_load_json": (_I, [C.c_char_p, C.POINTER(_P)]),
    "pt_scene_load_json_ex": (_I, [C.c_char_p, C.c_uint32, C.POINTER(_P)]),
    "pt_scene_create": (_I, [C.POINTER(_P)]),
    "pt_scene_free": (None, [_P]),
    "pt_scene_add_material": (_I, [_P, C.POINTER(Material), _IP]),
    "pt_scene_add_texture": (_I, [_P, _I, _I, _I, _P, _IP]),
    "pt_scene_texture_path": (_I, [_P, _I, C.c_char_p, _I]),
    "pt_scene_set_texture_pixels": (_I, [_P, _I, _I, _I, _I, _P]),
    "pt_scene_add_geom": (_I, [_P, _I, _I, _FP, _FP, _FP, _IP]),
    "pt_scene_add_mesh": (_I, [_P, _I, _FP, _FP, _FP, _FP, _I, _FP, _I, _FP, _I, _IP, _I, _IP, _IP, _IP, _IP]),
    "pt_scene_set_camera": (_I, [_P, _I, _I, _F, _FP, _FP, _FP]),
    "pt_scene_set_render": (_I, [_P, _I, _I, C.c_char_p]),
    "pt_scene_finalize": (_I, [_P]),
    "pt_scene_set_bvh_builder": (_I, [_P, _I]),
    "pt_scene_bvh_build_info": (_I, [_P, _IP, C.POINTER(C.c_double)]),
    "pt_scene_counts": (_I, [_P, _IP, _IP, _IP, _IP, _IP]),
    "pt_scene_get_camera": (_I, [_P, C.POINTER(Camera)]),
    "pt_scene_get_render": (_I, [_P, _IP, _IP, C.c_char_p, _I]),
    "pt_scene_get_orbit": (_I, [_P, _FP, _FP, _FP]),
    "pt_scene_set_orbit": (_I, [_P, _F, _F, _F, _FP]),
    "pt_scene_get_geoms": (_I, [_P, C.POINTER(Geom), _I]),
    "pt_scene_get_materials": (_I, [_P, C.POINTER(Material), _I]),
    "pt_scene_get_triangles": (_I, [_P, C.POINTER(Triangle), _I]),
    "pt_scene_get_bvh": (_I, [_P, C.POINTER(BvhNode), _I]),
    "pt_scene_bvh_quads": (_I, [_P, _P, _I, _IP, _IP]),
    "pt_scene_bvh_tcull": (_I, [_P, C.POINTER(C.c_uint32), _I, C.POINTER(C.c_double)]),
    "pt_scene_room_info": (_I, [_P, C.POINTER(Flags), _IP, _IP, _FP, _FP]),
    "pt_scene_bound_info": (_I, [_P, C.POINTER(Flags), C.POINTER(BoundInfo), _I, C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), _IP, _FP, _FP]),
    "pt_create": (_I, [_P, C.POINTER(Flags), C.POINTER(Shard), C.POINTER(_P)]),
    "pt_destroy": (_I, [_P]),
    "pt_set_flags": (_I, [_P, C.POINTER(Flags)]),
    "pt_ctx_cmask_info": (_I, [_P, _IP, C.POINTER(C.c_double), _IP]),
    "pt_ctx_room_info": (_I, [_P, _IP, _IP, _FP, _FP]),
    "pt_ctx_depart_counts": (_I, [_P] + [C.POINTER(C.c_uint64)] * 3),
    "pt_ctx_exact_counts": (_I, [_P] + [C.POINTER(C.c_uint64)] * 2),
    "pt_ctx_counters": (_I, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pt_ctx_stream_info": (_I, [_P] + [C.POINTER(C.c_int32)] * 5),
    "pt_ctx_walk_info": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_double)]),
    "pt_ctx_walk_kind": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "pt_render_pass": (_I, [_P, _I, _P]),
    "pt_render_ahead": (_I, [_P, _I, _P]),
    "pt_host_register": (_I, [_P, C.c_uint64]),
    "pt_host_unregister": (_I, [_P]),
    "pt_stream_create": (_I, [C.POINTER(_P)]),
    "pt_stream_destroy": (_I, [_P]),
    "pt_preview_rgba": (_I, [_P, _I, _P, _P]),
    "pt_tile_info": (_I, [_P, _IP, _IP, _IP, _IP]),
    "pt_get_image": (_I, [_P, _P]),
    "pt_get_accum": (_I, [_P, _P]),
    "pt_render_iteration": (_I, [_P, _I, _P, _P]),
    "pt_copy_image": (_I, [_P, _P, _P]),
    "pt_reset_image": (_I, [_P, _P]),
    "pt_stats": (_I, [_P, C.POINTER(Stats)]),
    "pt_profile_enable": (_I, [_P, _I]),
    "pt_selftest_math": (_I, [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]),
    "pt_selftest_exact": (_I, [C.c_uint64, C.c_uint32] + [C.POINTER(C.c_uint64)] * 3),
    "pt_selftest_renorm": (_I, [C.c_uint32, C.c_uint32] + [C.POINTER(C.c_uint64)] * 3),
    "pt_unit_rnorm_host": (_I, [_P, C.c_int64, _P, _P]),
    "pt_selftest_bounds": (_I, [_P, C.POINTER(Flags), C.c_uint64, C.c_uint32, C.POINTER(BoundsReport)]),
    "pt_profile_read": (_I, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "pt_profile_read_busy": (_I, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "pt_profile_read_kinds": (_I, [_P, _I, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "pt_tonemap": (_I, [_P, _I, _I, _F, _P]),
    "pt_save_png": (_I, [C.c_char_p, _P, _I, _I, _F]),
    "pt_save_hdr": (_I, [C.c_char_p, _P, _I, _I, _F]),
    "pt_encode_hdr": (_I, [_P, _I, _I, _F, _P, C.c_int64, _P]),
    "pt_set_accum": (_I, [_P, _P]),
    "pt_decode_jpeg": (_I, [C.c_char_p, C.c_int64, _IP, _IP, _IP, _P, C.c_int64]),
    "pt_gbuffer": (_I, [_P, _P, _P, _P, _P, _P]),
    "pt_get_gbuffer": (_I, [_P, _P, _P, _P, _P]),
    "pt_denoise_params_default": (None, [C.POINTER(DenoiseParams)]),
    "pt_denoiser_create": (_I, [_I, _I, C.POINTER(_P)]),
    "pt_denoiser_destroy": (_I, [_P]),
    "pt_denoiser_run": (_I, [_P, _P, _F, _P, _P, _P, C.POINTER(DenoiseParams), _P, _P]),
    "pt_denoise_host": (_I, [_I, _I, _P, _F, _P, _P, _P, C.POINTER(DenoiseParams), _P]),
    "pt_denoise_image": (_I, [_P, _F, C.POINTER(DenoiseParams), _P]),
    "pt_moments_create": (_I, [_I, _I, C.POINTER(_P)]),
    "pt_moments_destroy": (_I, [_P]),
    "pt_moments_reset": (_I, [_P, _P, _P]),
    "pt_moments_update": (_I, [_P, _P, _F, _P, _P]),
    "pt_moments_info": (_I, [_P, _IP, _FP]),
    "pt_moments_variance": (_I, [_P, _F, _P, _P]),
    "pt_moments_get": (_I, [_P, _P, _P, _P]),
    "pt_denoise_var_params_default": (None, [C.POINTER(DenoiseVarParams)]),
    "pt_denoiser_run_var": (_I, [_P, _P, _F, _P, _P, _P, _P, C.POINTER(DenoiseVarParams), _P, _P, _P]),
    "pt_denoise_var_host": (_I, [_I, _I, _P, _F, _P, _P, _P, _P, C.POINTER(DenoiseVarParams), _P, _P]),
    "pt_track_variance": (_I, [_P, _I]),
    "pt_variance_update": (_I, [_P, _F, _I, _P]),
    "pt_variance_info": (_I, [_P, _IP, _IP, _FP]),
    "pt_get_variance": (_I, [_P, _F, _P]),
    "pt_denoise_image_var": (_I, [_P, _F, C.POINTER(DenoiseVarParams), _P]),
    "pt_temporal_params_default": (None, [C.POINTER(TemporalParams)]),
    "pt_temporal_create": (_I, [_I, _I, C.POINTER(TemporalParams), C.POINTER(_P)]),
    "pt_temporal_destroy": (_I, [_P]),
    "pt_temporal_reset": (_I, [_P]),
    "pt_temporal_info": (_I, [_P, _IP, _FP, _IP]),
    "pt_temporal_frame": (_I, [_P, C.POINTER(Camera), _P, _F, _P, _P, _P, _P]),
    "pt_temporal_resolve": (_I, [_P, _P, _P, _P, _P]),
    "pt_temporal_frame_host": (_I, [_P, C.POINTER(Camera), _P, _F, _P, _P, _P]),
    "pt_temporal_get": (_I, [_P, _P, _P, _P, _P, _P, _P]),
    "pt_temporal_frame_ctx": (_I, [_P, _P, _F, _P]),
    "pt_temporal_image": (_I, [_P, C.POINTER(DenoiseVarParams), _P, _P, _P]),
    "pt_adaptive_params_default": (None, [C.POINTER(AdaptiveParams)]),
    "pt_adaptive_obj_create": (_I, [_I, _I, C.POINTER(_P)]),
    "pt_adaptive_obj_destroy": (_I, [_P]),
    "pt_adaptive_obj_info": (_I, [_P, _IP, _IP, _FP]),
    "pt_adaptive_obj_reset": (_I, [_P, _P, _P]),
    "pt_adaptive_obj_update": (_I, [_P, _P, _F, _P, _P]),
    "pt_adaptive_obj_select": (_I, [_P, C.POINTER(AdaptiveParams), _P, _IP, _IP]),
    "pt_adaptive_obj_set_mask": (_I, [_P, _P, _I, _P]),
    "pt_adaptive_obj_apply": (_I, [_P, _P, _P, _P]),
    "pt_adaptive_obj_resolve": (_I, [_P, _P, _P, _P, _P]),
    "pt_adaptive_obj_get": (_I, [_P, _P, _P, _P, _P, _P, _P]),
    "pt_adaptive_enable": (_I, [_P, _I]),
    "pt_adaptive_update": (_I, [_P, _I, _P]),
    "pt_adaptive_select": (_I, [_P, C.POINTER(AdaptiveParams), _IP, _IP]),
    "pt_adaptive_set_mask": (_I, [_P, _P, _I]),
    "pt_adaptive_info": (_I, [_P, _IP, _IP, _IP, _IP, _FP]),
    "pt_adaptive_get": (_I, [_P, _P, _P, _P, _P, _P, _P]),
    "pt_adaptive_image": (_I, [_P, C.POINTER(DenoiseVarParams), _P, _P]),
    "pt_jpeg_params_default": (None, [C.POINTER(JpegParams)]),
    "pt_jpeg_enc_create": (_I, [_I, _I, C.POINTER(JpegParams), C.POINTER(_P)]),
    "pt_jpeg_enc_destroy": (_I, [_P]),
    "pt_jpeg_enc_bound": (C.c_int64, [_P]),
    "pt_jpeg_enc_header": (C.c_int64, [_P, _P, C.c_int64]),
    "pt_jpeg_enc_pixels": (_I, [_P, _P, _I, _P, C.c_int64, _P, _P]),
    "pt_jpeg_enc_accum": (_I, [_P, _P, _F, _P, C.c_int64, _P, _P]),
    "pt_jpeg_encode_host": (_I, [_I, _I, _P, _I, C.POINTER(JpegParams), _P, C.c_int64, C.POINTER(C.c_int64)]),
    "pt_preview_jpeg": (_I, [_P, _I, _P, _P, C.c_int64, _P, _P]),
    "pt_jpeg_enc_profile": (_I, [_P, _I]),
    "pt_jpeg_enc_profile_read": (_I, [_P, _FP]),
    "pt_png_params_default": (None, [C.POINTER(PngParams)]),
    "pt_png_enc_create": (_I, [_I, _I, C.POINTER(PngParams), C.POINTER(_P)]),
    "pt_png_enc_destroy": (_I, [_P]),
    "pt_png_enc_bound": (C.c_int64, [_P]),
    "pt_png_enc_pixels": (_I, [_P, _P, _I, _P, C.c_int64, _P, _P]),
    "pt_png_enc_accum": (_I, [_P, _P, _F, _P, C.c_int64, _P, _P]),
    "pt_png_encode_host": (_I, [_I, _I, _P, _I, C.POINTER(PngParams), _P, C.c_int64, C.POINTER(C.c_int64)]),
    "pt_preview_png": (_I, [_P, _I, _P, _P, C.c_int64, _P, _P]),
    "pt_png_enc_profile": (_I, [_P, _I]),
    "pt_png_enc_profile_read": (_I, [_P, _FP]),
    "pt_hdr_params_default": (None, [C.POINTER(HdrParams)]),
    "pt_hdr_enc_create": (_I, [_I, _I, C.POINTER(HdrParams), C.POINTER(_P)]),
    "pt_hdr_enc_destroy": (_I, [_P]),
    "pt_hdr_enc_bound": (C.c_int64, [_P]),
    "pt_hdr_enc_accum": (_I, [_P, _P, _F, _P, C.c_int64, _P, _P]),
    "pt_hdr_encode_host": (_I, [_I, _I, _P, _F, C.POINTER(HdrParams), _P, C.c_int64, C.POINTER(C.c_int64)]),
    "pt_preview_hdr": (_I, [_P, _I, _P, _P, C.c_int64, _P, _P]),
    "pt_hdr_enc_profile": (_I, [_P, _I]),
    "pt_hdr_enc_profile_read": (_I, [_P, _FP]),
    "pt_exr_params_default": (None, [C.POINTER(ExrParams)]),
    "pt_exr_enc_create": (_I, [_I, _I, C.POINTER(ExrChannel), _I, C.POINTER(ExrParams), C.POINTER(_P)]),
    "pt_exr_enc_destroy": (_I, [_P]),
    "pt_exr_enc_bound": (C.c_int64, [_P]),
    "pt_exr_enc_header": (C.c_int64, [_P, _P, C.c_int64]),
    "pt_exr_enc_planes": (_I, [_P, C.POINTER(ExrPlane), _P, C.c_int64, _P, _P]),
    "pt_exr_encode_host": (_I, [_I, _I, C.POINTER(ExrChannel), _I, C.POINTER(_P), _IP, _FP, C.POINTER(ExrParams), _P, C.c_int64,
                                C.POINTER(C.c_int64)]),
    "pt_exr_enc_profile": (_I, [_P, _I]),
    "pt_exr_enc_profile_read": (_I, [_P, _FP]),
    "pt_exr_ctx_channels": (_I, [_I, _I, C.POINTER(ExrChannel), _IP]),
    "pt_preview_exr": (_I, [_P, _I, _I, _P, _P, C.c_int64, _P, _P]),
    "pt_display_params_default": (None, [C.POINTER(DisplayParams)]),
    "pt_display_create": (_I, [_I, _I, C.POINTER(DisplayParams), C.POINTER(_P)]),
    "pt_display_destroy": (_I, [_P]),
    "pt_display_meter": (_I, [_P, _P, _F, _P]),
    "pt_display_apply": (_I, [_P, _P, _F, _P, _I, _P]),
    "pt_display_frame": (_I, [_P, _P, _F, _P, _I, _P]),
    "pt_display_reset": (_I, [_P, _P]),
    "pt_display_host": (_I, [_I, _I, _P, _F, C.POINTER(DisplayParams), _P, _I]),
    "pt_display_info": (_I, [_P, _P, _IP, _FP, _IP]),
    "pt_display_tables": (None, [_P, _P, _FP]),
    "pt_preview_display": (_I, [_P, _I, _P, _P, _I, _P]),
    "pt_bloom_params_default": (None, [C.POINTER(BloomParams)]),
    "pt_bloom_create": (_I, [_I, _I, C.POINTER(BloomParams), C.POINTER(_P)]),
    "pt_bloom_destroy": (_I, [_P]),
    "pt_bloom_apply": (_I, [_P, _P, _F, _P, _P]),
    "pt_bloom_host": (_I, [_I, _I, _P, _F, C.POINTER(BloomParams), _P]),
    "pt_bloom_info": (_I, [_P, _IP, _IP, _IP]),
    "pt_preview_bloom": (_I, [_P, _I, _P, _P, _P]),
    "pt_env_params_default": (None, [C.POINTER(EnvParams)]),
    "pt_scene_set_environment": (_I, [_P, _I, _I, _P, C.POINTER(EnvParams)]),
    "pt_scene_set_environment_octa": (_I, [_P, _I, _P, C.POINTER(EnvParams)]),
    "pt_scene_load_environment": (_I, [_P, C.c_char_p, C.POINTER(EnvParams)]),
    "pt_scene_clear_environment": (_I, [_P]),
    "pt_scene_get_environment": (_I, [_P, _IP, C.POINTER(EnvParams), _P, C.c_int64]),
    "pt_decode_hdr": (_I, [C.c_char_p, C.c_int64, _IP, _IP, _P, C.c_int64]),
    "pt_env_eval": (_I, [_P, C.c_int64, _P, _P, _P]),
    "pt_env_eval_host": (_I, [_P, C.c_int64, _P, _P]),
}

_lib = None


def _preload_torch() -> None:
    # torch ships its own libamdhip64.so.7; importing torch first makes this library bind to the
    # same HIP runtime instance (same SONAME), so device pointers and streams are shared.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except Exception:
            pass


# Entry points an older library may lack when PT_AMD_LIB times it beside this tree (the shipped
# library has them all; pt_ctx_room_info: the A/B against the build before the room bound;
# pt_scene_room_info: the A/B against the build before the host-only bounds unit; the
# variance entry points, pt_temporal_* and pt_adaptive_*: the A/B against the builds before them;
# pt_ctx_depart_counts: the A/B against the build before the room's departure claim;
# pt_ctx_exact_counts, pt_selftest_exact: the A/B against the build before the exact tests' single gate;
# pt_scene_bound_info, pt_selftest_bounds: the A/B against the build before the per-pair bound check;
# pt_selftest_renorm, pt_unit_rnorm_host: the A/B against the build before the unit renormalisation;
# pt_jpeg_*, pt_preview_jpeg: the A/B against the build before the JPEG encoder; pt_png_*, pt_preview_png: the
# A/B against the build before the PNG encoder; pt_hdr_*, pt_preview_hdr: the A/B against the build before the
# HDR encoder; pt_exr_*, pt_preview_exr: the A/B against the build before the OpenEXR encoder; pt_display_*, pt_preview_display: scripts/display_time.py's A/B against the build before the display
# transform; pt_env_*, pt_scene_*_environment*, pt_decode_hdr: the A/B against the build before the environment;
# pt_bloom_*, pt_preview_bloom: the A/B against the build before the bloom).
_OPTIONAL = {"pt_bloom_params_default", "pt_bloom_create", "pt_bloom_destroy", "pt_bloom_apply", "pt_bloom_host", "pt_bloom_info",
             "pt_preview_bloom",
             "pt_env_params_default", "pt_scene_set_environment", "pt_scene_set_environment_octa",
             "pt_scene_load_environment", "pt_scene_clear_environment", "pt_scene_get_environment", "pt_decode_hdr",
             "pt_env_eval", "pt_env_eval_host",
             "pt_selftest_math", "pt_profile_read_kinds", "pt_ctx_room_info", "pt_scene_room_info", "pt_ctx_depart_counts",
             "pt_ctx_exact_counts", "pt_ctx_walk_kind", "pt_selftest_exact", "pt_scene_bound_info", "pt_selftest_bounds", "pt_selftest_renorm", "pt_unit_rnorm_host",
             "pt_moments_create",
             "pt_moments_destroy", "pt_moments_reset", "pt_moments_update", "pt_moments_info", "pt_moments_variance",
             "pt_moments_get", "pt_denoise_var_params_default", "pt_denoiser_run_var", "pt_denoise_var_host",
             "pt_track_variance", "pt_variance_update", "pt_variance_info", "pt_get_variance", "pt_denoise_image_var",
             "pt_temporal_params_default", "pt_temporal_create", "pt_temporal_destroy", "pt_temporal_reset",
             "pt_temporal_info", "pt_temporal_frame", "pt_temporal_resolve", "pt_temporal_frame_host", "pt_temporal_get",
             "pt_temporal_frame_ctx", "pt_temporal_image",
             "pt_adaptive_params_default", "pt_adaptive_obj_create", "pt_adaptive_obj_destroy", "pt_adaptive_obj_info",
             "pt_adaptive_obj_reset", "pt_adaptive_obj_update", "pt_adaptive_obj_select", "pt_adaptive_obj_set_mask",
             "pt_adaptive_obj_apply", "pt_adaptive_obj_resolve", "pt_adaptive_obj_get", "pt_adaptive_enable",
             "pt_adaptive_update", "pt_adaptive_select", "pt_adaptive_set_mask", "pt_adaptive_info", "pt_adaptive_get",
             "pt_adaptive_image",
             "pt_jpeg_params_default", "pt_jpeg_enc_create", "pt_jpeg_enc_destroy", "pt_jpeg_enc_bound", "pt_jpeg_enc_header",
             "pt_jpeg_enc_pixels", "pt_jpeg_enc_accum", "pt_jpeg_encode_host", "pt_preview_jpeg", "pt_jpeg_enc_profile",
             "pt_jpeg_enc_profile_read",
             "pt_png_params_default", "pt_png_enc_create", "pt_png_enc_destroy", "pt_png_enc_bound", "pt_png_enc_pixels",
             "pt_png_enc_accum", "pt_png_encode_host", "pt_preview_png", "pt_png_enc_profile", "pt_png_enc_profile_read",
             "pt_hdr_params_default", "pt_hdr_enc_create", "pt_hdr_enc_destroy", "pt_hdr_enc_bound", "pt_hdr_enc_accum",
             "pt_hdr_encode_host", "pt_preview_hdr", "pt_hdr_enc_profile", "pt_hdr_enc_profile_read",
             "pt_exr_params_default", "pt_exr_enc_create", "pt_exr_enc_destroy", "pt_exr_enc_bound", "pt_exr_enc_header",
             "pt_exr_enc_planes", "pt_exr_encode_host", "pt_exr_enc_profile", "pt_exr_enc_profile_read", "pt_exr_ctx_channels",
             "pt_preview_exr",
             "pt_display_params_default", "pt_display_create", "pt_display_destroy", "pt_display_meter", "pt_display_apply",
             "pt_display_frame", "pt_display_reset", "pt_display_host", "pt_display_info", "pt_display_tables",
             "pt_preview_display"}


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise NativeLibraryError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)")
    if os.environ.get("PT_AMD_NO_TORCH", "0") != "1":
        _preload_torch()
    try:
        L = C.CDLL(str(LIB_PATH), mode=C.RTLD_GLOBAL)
    except OSError as e:
        raise NativeLibraryError(f"failed to load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        if name in _OPTIONAL and not hasattr(L, name):   # (an older build timed beside this one)
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check_pt(rc: int) -> None:
    if rc != 0:
        raise PtError(rc, lib().pt_last_error().decode())


def check_sc(rc: int) -> None:
    if rc != 0:
        raise PtError(rc, lib().sc_last_error().decode())


def f3(x) -> C.Array:
    return (C.c_float * 3)(*[float(v) for v in x])
