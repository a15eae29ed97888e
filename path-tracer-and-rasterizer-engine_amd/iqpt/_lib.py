"""ctypes mirror of include/iqpt.h and the loader of the in-tree libiqpt.so.

The product path is native: this module only binds the C ABI. If the library is missing or does
not load, importing the render API raises — there is no Python or CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libiqpt.so"

IQPT_OK = 0
STATUS_NAMES = {
    0: "IQPT_OK", 1: "IQPT_ERR_INVALID_ARG", 2: "IQPT_ERR_HIP", 3: "IQPT_ERR_OUT_OF_MEMORY",
    4: "IQPT_ERR_NO_DEVICE", 5: "IQPT_ERR_NOT_READY", 6: "IQPT_ERR_UNSUPPORTED",
}
MESH_TRIANGLES = 0
MESH_SPHERES = 1
DEFAULT_SEED = 1984
DEFAULT_MAX_DEPTH = 5
SPLIT_AUTO, SPLIT_OFF, SPLIT_ON, SPLIT_CHAIN, SPLIT_FAN, SPLIT_SPEC = -1, 0, 1, 2, 3, 4   # IQPT_SPLIT_* (iqpt_set_split;
# CHAIN and FAN are refused with IQPT_ERR_UNSUPPORTED since round 6)
OVERLAP_OFF, OVERLAP_AUTO = 0, 1               # IQPT_OVERLAP_* (iqpt_set_overlap)
COMM_ID_BYTES = 128                            # IQPT_COMM_ID_BYTES (iqpt_comm_unique_id)
GATHER_ACCUM = 1                               # IQPT_GATHER_ACCUM / IQPT_GATHER_FRAME (iqpt_gather_read_select)
GATHER_FRAME = 2


class IqptError(RuntimeError):
    """A non-zero iqpt_status, with the library's iqpt_last_error() detail."""

    def __init__(self, status: int, detail: str, call: str):
        super().__init__(f"{call} -> {STATUS_NAMES.get(status, status)}: {detail}")
        self.status = status
        self.detail = detail


class Vertex(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("normal", C.c_float * 3)]


class TriMesh(C.Structure):
    _fields_ = [("vertices", C.POINTER(Vertex)), ("indices", C.POINTER(C.c_uint32)),
                ("num_indices", C.c_uint32), ("num_vertices", C.c_uint32)]


class TriMeshDrawcall(C.Structure):
    _fields_ = [("transform", C.c_float * 16), ("mesh_id", C.c_uint32)]


class SphereDrawcall(C.Structure):
    _fields_ = [("center", C.c_float * 4), ("radius", C.c_float)]


class Material(C.Structure):
    """iqpt_material (include/iqpt.h): IQPT_MAT_EMISSIVE (param = strength) or IQPT_MAT_OREN_NAYAR
    (param = roughness sigma)."""
    _fields_ = [("type", C.c_uint32), ("albedo", C.c_float * 4), ("param", C.c_float)]


MAT_EMISSIVE = 0
MAT_OREN_NAYAR = 1


class PacketDesc(C.Structure):
    _fields_ = [("num_drawcalls", C.c_uint32 * 2), ("num_tri_meshes", C.c_uint32),
                ("tri_meshes", C.POINTER(TriMesh)), ("tri_mesh_dcs", C.POINTER(TriMeshDrawcall)),
                ("sphere_dcs", C.POINTER(SphereDrawcall)),
                ("materials", C.POINTER(Material)), ("num_materials", C.c_uint32),
                ("tri_dc_material", C.POINTER(C.c_uint32)), ("sphere_dc_material", C.POINTER(C.c_uint32))]


class Camera(C.Structure):
    _fields_ = [("width", C.c_uint16), ("height", C.c_uint16), ("fovh", C.c_float),
                ("position", C.c_float * 4), ("forward", C.c_float * 4),
                ("view", C.c_float * 16), ("projection", C.c_float * 16),
                ("inv_view", C.c_float * 16), ("inv_proj", C.c_float * 16)]


class PixelSet(C.Structure):
    _fields_ = [("x0", C.c_uint32), ("x1", C.c_uint32), ("y0", C.c_uint32),
                ("ystep", C.c_uint32), ("nrows", C.c_uint32)]


class DrawItem(C.Structure):
    """iqpt_draw_item (include/raster/iqpt_raster.h): one model in draw order, with its mesh data."""
    _fields_ = [("transform", C.c_float * 16), ("vertices", C.POINTER(Vertex)), ("indices", C.POINTER(C.c_uint32)),
                ("num_vertices", C.c_uint32), ("num_indices", C.c_uint32), ("albedo", C.c_float * 3),
                ("mesh_type", C.c_int32)]


RASTER_NO_PRIM = 0xFFFFFFFF                    # IQPT_RASTER_NO_PRIM
RASTER_MAX_DIM = 8192                          # IQPT_RASTER_MAX_DIM

# (name, restype, argtypes) of every entry point declared in include/iqpt.h
_P = C.c_void_p
_FP = C.POINTER(C.c_float)
SIGNATURES = [
    ("iqpt_camera_init", C.c_int, [C.POINTER(Camera), C.c_uint16, C.c_uint16, C.c_float, C.c_float, C.c_float, _FP, _FP]),
    ("iqpt_camera_align", C.c_int, [C.POINTER(Camera), C.POINTER(Camera)]),
    ("iqpt_create", C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(PixelSet), C.c_uint64, C.c_int, C.POINTER(_P)]),
    ("iqpt_destroy", C.c_int, [_P]),
    ("iqpt_set_camera", C.c_int, [_P, C.POINTER(Camera)]),
    ("iqpt_upload_packet", C.c_int, [_P, C.POINTER(PacketDesc)]),
    ("iqpt_render", C.c_int, [_P, C.c_uint32]),
    ("iqpt_sync", C.c_int, [_P]),
    ("iqpt_reset", C.c_int, [_P]),
    ("iqpt_read", C.c_int, [_P, _FP, C.POINTER(C.c_uint8)]),
    ("iqpt_read_rng", C.c_int, [_P, C.POINTER(C.c_uint32)]),
    ("iqpt_copy_accum_device", C.c_int, [_P, _P, C.c_size_t]),
    ("iqpt_copy_frame_device", C.c_int, [_P, _P, C.c_size_t]),
    ("iqpt_copy_frame_device_async", C.c_int, [_P, _P, C.c_size_t]),
    ("iqpt_stream", C.c_int, [_P, C.POINTER(C.c_void_p)]),
    ("iqpt_frame_stream", C.c_int, [_P, C.POINTER(C.c_void_p)]),
    ("iqpt_set_split", C.c_int, [_P, C.c_int]),
    ("iqpt_set_overlap", C.c_int, [_P, C.c_int]),
    ("iqpt_kernel_span", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("iqpt_prepare", C.c_int, [_P]),
    ("iqpt_num_pixels", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("iqpt_frame_count", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("iqpt_rays_traced", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("iqpt_kernel_time", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("iqpt_kernel_name", C.c_char_p, []),
    ("iqpt_checkpoint_save", C.c_int, [_P, C.c_char_p]),
    ("iqpt_checkpoint_load", C.c_int, [_P, C.c_char_p]),
    ("iqpt_write_ppm", C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8)]),
    ("iqpt_error_string", C.c_char_p, [C.c_int]),
    ("iqpt_last_error", C.c_char_p, []),
    ("iqpt_abi_version", C.c_int, []),
    ("iqpt_comm_unique_id", C.c_int, [_P, C.c_size_t]),
    ("iqpt_comm_init", C.c_int, [_P, C.c_int, C.c_int, _P, C.c_size_t]),
    ("iqpt_gather_frame_async", C.c_int, [_P, C.c_int, _P, C.c_size_t]),
    ("iqpt_gather_accum", C.c_int, [_P, C.c_int, _P, C.c_size_t]),
    ("iqpt_gather_read", C.c_int, [_P, C.c_int, _FP, C.POINTER(C.c_uint8)]),
    ("iqpt_gather_read_select", C.c_int, [_P, C.c_int, C.c_int, _FP, C.POINTER(C.c_uint8)]),
    ("iqpt_comm_stream", C.c_int, [_P, C.POINTER(C.c_void_p)]),
    ("iqpt_comm_time", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("iqpt_scene_create", C.c_int, [C.POINTER(_P)]),
    ("iqpt_scene_destroy", C.c_int, [_P]),
    ("iqpt_scene_add_mesh_tri", C.c_int, [_P, C.c_char_p]),
    ("iqpt_scene_add_mesh_quad", C.c_int, [_P, C.c_char_p]),
    ("iqpt_scene_add_mesh_reg_polygon", C.c_int, [_P, C.c_char_p, C.c_uint32]),
    ("iqpt_scene_add_mesh_cube", C.c_int, [_P, C.c_char_p]),
    ("iqpt_scene_add_mesh_uv_sphere", C.c_int, [_P, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_int]),
    ("iqpt_scene_add_mesh", C.c_int, [_P, C.c_char_p, C.c_int, C.POINTER(Vertex), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]),
    ("iqpt_scene_add_model", C.c_int, [_P, C.c_char_p, C.c_char_p, _FP, _FP, _FP]),
    ("iqpt_scene_num_meshes", C.c_int, [_P, C.POINTER(C.c_uint32)]),
    ("iqpt_scene_add_preset", C.c_int, [_P, C.c_char_p]),
    ("iqpt_scene_add_material", C.c_int, [_P, C.POINTER(Material), C.POINTER(C.c_uint32)]),
    ("iqpt_scene_set_model_material", C.c_int, [_P, C.c_char_p, C.c_uint32]),
    ("iqpt_scene_build_packet", C.c_int, [_P, C.POINTER(PacketDesc)]),
]
# the same for include/raster/iqpt_raster.h (the rasterizer's additions; IQPT_ABI_VERSION is unchanged by them)
RASTER_SIGNATURES = [
    ("iqpt_scene_draw_list", C.c_int, [_P, C.POINTER(DrawItem), C.c_uint32, C.POINTER(C.c_uint32)]),
    ("iqpt_raster_create", C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    ("iqpt_raster_destroy", C.c_int, [_P]),
    ("iqpt_raster_set_camera", C.c_int, [_P, C.POINTER(Camera)]),
    ("iqpt_raster_upload_scene", C.c_int, [_P, _P]),
    ("iqpt_raster_draw", C.c_int, [_P]),
    ("iqpt_raster_draw_clip", C.c_int, [_P, _FP, _FP, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]),
    ("iqpt_raster_read", C.c_int, [_P, C.POINTER(C.c_uint8), _FP, C.POINTER(C.c_uint32)]),
    ("iqpt_raster_copy_frame_device", C.c_int, [_P, _P, C.c_size_t]),
    ("iqpt_raster_sync", C.c_int, [_P]),
    ("iqpt_raster_time", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("iqpt_raster_stage_time", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("iqpt_raster_stats", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("iqpt_raster_gbuffer", C.c_int, [_P]),
    ("iqpt_raster_read_gbuffer", C.c_int, [_P, _FP, C.POINTER(C.c_uint32)]),
    ("iqpt_raster_gbuffer_device", C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("iqpt_raster_gbuffer_time", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
]


class DenoiseParams(C.Structure):
    """iqpt_denoise_params (include/denoise/iqpt_denoise.h)."""
    _fields_ = [("levels", C.c_uint32), ("normal_squarings", C.c_uint32), ("depth_sharpness", C.c_float),
                ("colour_sharpness", C.c_float)]


DENOISE_MAX_LEVELS = 8                         # IQPT_DENOISE_MAX_LEVELS
# the same for include/denoise/iqpt_denoise.h (the denoiser's additions)
DENOISE_SIGNATURES = [
    ("iqpt_denoise_default_params", C.c_int, [C.POINTER(DenoiseParams)]),
    ("iqpt_denoise_create", C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    ("iqpt_denoise_destroy", C.c_int, [_P]),
    ("iqpt_denoise_set_params", C.c_int, [_P, C.POINTER(DenoiseParams)]),
    ("iqpt_denoise_set_guides", C.c_int, [_P, _FP, C.POINTER(C.c_uint32)]),
    ("iqpt_denoise_set_guides_device", C.c_int, [_P, _P, _P]),
    ("iqpt_denoise_run", C.c_int, [_P, _FP]),
    ("iqpt_denoise_run_device", C.c_int, [_P, _P]),
    ("iqpt_denoise_frame", C.c_int, [_P, _P, _P]),
    ("iqpt_denoise_read", C.c_int, [_P, _FP, C.POINTER(C.c_uint8)]),
    ("iqpt_denoise_copy_frame_device", C.c_int, [_P, _P, C.c_size_t]),
    ("iqpt_denoise_sync", C.c_int, [_P]),
    ("iqpt_denoise_time", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
]



class TemporalParams(C.Structure):
    """iqpt_temporal_params (include/temporal/iqpt_temporal.h)."""
    _fields_ = [("normal_min", C.c_float), ("plane_tolerance", C.c_float), ("max_history", C.c_uint32)]


TEMPORAL_MAX_HISTORY = 1 << 24                 # IQPT_TEMPORAL_MAX_HISTORY
# the same for include/temporal/iqpt_temporal.h (temporal reprojection's additions)
TEMPORAL_SIGNATURES = [
    ("iqpt_temporal_default_params", C.c_int, [C.POINTER(TemporalParams)]),
    ("iqpt_temporal_create", C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    ("iqpt_temporal_destroy", C.c_int, [_P]),
    ("iqpt_temporal_set_params", C.c_int, [_P, C.POINTER(TemporalParams)]),
    ("iqpt_temporal_begin_view", C.c_int, [_P, C.POINTER(Camera), _FP, C.POINTER(C.c_uint32)]),
    ("iqpt_temporal_begin_view_device", C.c_int, [_P, C.POINTER(Camera), _P, _P]),
    ("iqpt_temporal_begin_view_raster", C.c_int, [_P, _P]),
    ("iqpt_temporal_clear", C.c_int, [_P]),
    ("iqpt_temporal_resolve", C.c_int, [_P, _FP, C.c_uint64]),
    ("iqpt_temporal_resolve_device", C.c_int, [_P, _P, C.c_uint64]),
    ("iqpt_temporal_resolve_ctx", C.c_int, [_P, _P]),
    ("iqpt_temporal_read", C.c_int, [_P, _FP, C.POINTER(C.c_uint8)]),
    ("iqpt_temporal_output_device", C.c_int, [_P, C.POINTER(C.c_void_p)]),
    ("iqpt_temporal_copy_frame_device", C.c_int, [_P, _P, C.c_size_t]),
    ("iqpt_temporal_sync", C.c_int, [_P]),
    ("iqpt_temporal_time", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double),
                                     C.POINTER(C.c_uint64)]),
    ("iqpt_temporal_stats", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
]


class MotionEntry(C.Structure):
    """iqpt_motion_entry (include/motion/iqpt_motion.h): 128 bytes."""
    _fields_ = [("back", C.c_float * 16), ("nback", C.c_float * 12), ("moved", C.c_uint32), ("reserved", C.c_uint32 * 3)]


MOTION_MAX_ENTRIES = 1 << 20                   # IQPT_MOTION_MAX_ENTRIES
_MEP = C.POINTER(MotionEntry)
# include/motion/iqpt_motion.h: moving-model reprojection, in libiqpt_motion.so (bound by load_motion, not load)
MOTION_SIGNATURES = [
    ("iqpt_motion_table", C.c_int, [C.POINTER(DrawItem), C.c_uint32, C.POINTER(DrawItem), C.c_uint32, _MEP]),
    ("iqpt_motion_default_params", C.c_int, [C.POINTER(TemporalParams)]),
    ("iqpt_motion_create", C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    ("iqpt_motion_destroy", C.c_int, [_P]),
    ("iqpt_motion_set_params", C.c_int, [_P, C.POINTER(TemporalParams)]),
    ("iqpt_motion_begin_view", C.c_int, [_P, C.POINTER(Camera), _FP, C.POINTER(C.c_uint32), _P, C.c_uint32]),
    ("iqpt_motion_begin_view_device", C.c_int, [_P, C.POINTER(Camera), _P, _P, _P, C.c_uint32]),
    ("iqpt_motion_begin_view_raster", C.c_int, [_P, _P, _P, C.c_uint32]),
    ("iqpt_motion_clear", C.c_int, [_P]),
    ("iqpt_motion_resolve", C.c_int, [_P, _FP, C.c_uint64]),
    ("iqpt_motion_resolve_device", C.c_int, [_P, _P, C.c_uint64]),
    ("iqpt_motion_resolve_ctx", C.c_int, [_P, _P]),
    ("iqpt_motion_read", C.c_int, [_P, _FP, C.POINTER(C.c_uint8)]),
    ("iqpt_motion_output_device", C.c_int, [_P, C.POINTER(C.c_void_p)]),
    ("iqpt_motion_copy_frame_device", C.c_int, [_P, _P, C.c_size_t]),
    ("iqpt_motion_sync", C.c_int, [_P]),
    ("iqpt_motion_time", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double),
                                   C.POINTER(C.c_uint64)]),
    ("iqpt_motion_stats", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint64)]),
]


class SvgfParams(C.Structure):
    """iqpt_svgf_params (include/svgf/iqpt_svgf.h)."""
    _fields_ = [("normal_min", C.c_float), ("plane_tolerance", C.c_float), ("max_history", C.c_uint32),
                ("min_history", C.c_uint32), ("levels", C.c_uint32), ("normal_squarings", C.c_uint32),
                ("depth_sharpness", C.c_float), ("colour_sigma", C.c_float), ("variance_floor", C.c_float)]


SVGF_MAX_LEVELS = 8                            # IQPT_SVGF_MAX_LEVELS
_DP = C.POINTER(C.c_double)
# the same for include/svgf/iqpt_svgf.h (variance-guided filtering's additions)
SVGF_SIGNATURES = [
    ("iqpt_svgf_default_params", C.c_int, [C.POINTER(SvgfParams)]),
    ("iqpt_svgf_create", C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    ("iqpt_svgf_destroy", C.c_int, [_P]),
    ("iqpt_svgf_set_params", C.c_int, [_P, C.POINTER(SvgfParams)]),
    ("iqpt_svgf_begin_view", C.c_int, [_P, C.POINTER(Camera), _FP, C.POINTER(C.c_uint32)]),
    ("iqpt_svgf_begin_view_device", C.c_int, [_P, C.POINTER(Camera), _P, _P]),
    ("iqpt_svgf_begin_view_raster", C.c_int, [_P, _P]),
    ("iqpt_svgf_clear", C.c_int, [_P]),
    ("iqpt_svgf_resolve", C.c_int, [_P, _FP, C.c_uint64]),
    ("iqpt_svgf_resolve_device", C.c_int, [_P, _P, C.c_uint64]),
    ("iqpt_svgf_resolve_ctx", C.c_int, [_P, _P]),
    ("iqpt_svgf_read", C.c_int, [_P, _FP, C.POINTER(C.c_uint8)]),
    ("iqpt_svgf_read_stages", C.c_int, [_P, _FP, _FP]),
    ("iqpt_svgf_copy_frame_device", C.c_int, [_P, _P, C.c_size_t]),
    ("iqpt_svgf_sync", C.c_int, [_P]),
    ("iqpt_svgf_time", C.c_int, [_P, _DP, _DP, _DP, C.POINTER(C.c_uint64), _DP, _DP]),
    ("iqpt_svgf_stats", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
]


class UpscaleParams(C.Structure):
    """iqpt_upscale_params (include/upscale/iqpt_upscale.h)."""
    _fields_ = [("normal_squarings", C.c_uint32), ("depth_sharpness", C.c_float)]


_UP = C.POINTER(C.c_uint32)
_U64P = C.POINTER(C.c_uint64)
# the same for include/upscale/iqpt_upscale.h (guided upsampling's additions)
UPSCALE_SIGNATURES = [
    ("iqpt_upscale_default_params", C.c_int, [C.POINTER(UpscaleParams)]),
    ("iqpt_upscale_create", C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    ("iqpt_upscale_destroy", C.c_int, [_P]),
    ("iqpt_upscale_set_params", C.c_int, [_P, C.POINTER(UpscaleParams)]),
    ("iqpt_upscale_set_guides", C.c_int, [_P, _FP, _UP, _FP, _UP]),
    ("iqpt_upscale_set_guides_device", C.c_int, [_P, _P, _P, _P, _P]),
    ("iqpt_upscale_run", C.c_int, [_P, _FP]),
    ("iqpt_upscale_run_device", C.c_int, [_P, _P]),
    ("iqpt_upscale_frame", C.c_int, [_P, _P, _P, _P]),
    ("iqpt_upscale_read", C.c_int, [_P, _FP, C.POINTER(C.c_uint8)]),
    ("iqpt_upscale_output_device", C.c_int, [_P, C.POINTER(C.c_void_p)]),
    ("iqpt_upscale_copy_frame_device", C.c_int, [_P, _P, C.c_size_t]),
    ("iqpt_upscale_sync", C.c_int, [_P]),
    ("iqpt_upscale_time", C.c_int, [_P, C.POINTER(C.c_double), _U64P]),
    ("iqpt_upscale_stats", C.c_int, [_P, _U64P, _U64P, _U64P]),
]

# the kernel variant tables and the last launch's kernels (csrc/runtime/iq_debug.cpp; not part of include/iqpt.h):
# the variant census of tests/variant_cases.py reads both
VARIANT_TABLES = ("render", "fan", "sky", "anyhit", "spec", "stitch")     # iqpt_debug_variant_table's table numbers
_I32P = C.POINTER(C.c_int32)
DEBUG_SIGNATURES = [
    ("iqpt_debug_variant_table", C.c_int, [C.c_int, _I32P, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("iqpt_debug_last_launch", C.c_int, [_P, _I32P]),
]

_lib = None


ABI_VERSION = 6      # IQPT_ABI_VERSION of include/iqpt.h these bindings mirror
LOADED_ABI = None    # the ABI of the library load() bound (an A/B library may be older; bench.py reports it)


def load() -> C.CDLL:
    """Load libiqpt.so from the package directory (raises if it is absent: no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} is missing: run __graft_entry__.build() "
                          "(the HIP extension is required; there is no CPU fallback)")
    global LOADED_ABI
    lib = C.CDLL(str(LIB_PATH))
    # an A/B library of an earlier round (bench.py --lib, another path) may lack the newest entry points: those
    # are left unbound there; the package's own library must export every one. A library of a newer ABI than
    # these bindings is refused whatever its path (its signatures may differ from the ones bound here).
    own = LIB_PATH.resolve() == (_PKG / "libiqpt.so").resolve()
    abi = lib.iqpt_abi_version() if getattr(lib, "iqpt_abi_version", None) is not None else None
    if abi is not None and abi > ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI {abi}, newer than these bindings' {ABI_VERSION}")
    for name, res, args in SIGNATURES + RASTER_SIGNATURES + DENOISE_SIGNATURES + TEMPORAL_SIGNATURES + SVGF_SIGNATURES + \
            UPSCALE_SIGNATURES + DEBUG_SIGNATURES:
        fn = getattr(lib, name, None)
        if fn is None:
            if own:
                raise ImportError(f"{LIB_PATH} does not export {name}: rebuild with __graft_entry__.build()")
            continue
        fn.restype = res
        fn.argtypes = args
    if own and abi != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI {abi}, the bindings expect {ABI_VERSION}: "
                          "rebuild with __graft_entry__.build()")
    LOADED_ABI = abi
    _lib = lib
    return lib


MOTION_LIB_PATH = _PKG / "libiqpt_motion.so"
_motion_libs: dict = {}


def load_motion(path=None) -> C.CDLL:
    """Load libiqpt_motion.so (or another build of it, e.g. the A/B library with wave-uniform entry loads) on first use and bind
    MOTION_SIGNATURES; libiqpt.so is loaded first, the library links it. Raises if it is absent: no fallback."""
    load()
    path = Path(path) if path is not None else MOTION_LIB_PATH
    key = str(path.resolve())
    if key in _motion_libs:
        return _motion_libs[key]
    if not path.exists():
        raise ImportError(f"{path} is missing: run __graft_entry__.build() "
                          "(the HIP extension is required; there is no CPU fallback)")
    lib = C.CDLL(str(path))
    for name, res, args in MOTION_SIGNATURES:
        fn = getattr(lib, name, None)
        if fn is None:
            raise ImportError(f"{path} does not export {name}: rebuild with __graft_entry__.build()")
        fn.restype = res
        fn.argtypes = args
    _motion_libs[key] = lib
    return lib


def check(status: int, call: str) -> None:
    if status != IQPT_OK:
        lib = load()
        detail = lib.iqpt_last_error().decode(errors="replace")
        raise IqptError(status, detail, call)


def farr(values, n: int):
    arr = (C.c_float * n)(*[float(v) for v in values])
    return arr
