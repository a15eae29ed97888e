"""Motion binding: ``Motion`` owns one iqpt_motion (temporal reprojection whose history also follows the models,
DESIGN.md §15); ``motion_table`` makes the table of a scene change. The library (libiqpt_motion.so) is loaded on
first use."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Camera, MotionEntry, TemporalParams, check

# iqpt_motion_entry as a numpy record: 128 bytes
ENTRY_DTYPE = np.dtype([("back", np.float32, (16,)), ("nback", np.float32, (12,)), ("moved", np.uint32),
                        ("reserved", np.uint32, (3,))])
assert ENTRY_DTYPE.itemsize == C.sizeof(MotionEntry) == 128


def default_params() -> dict:
    """The parameters a new Motion starts with (iqpt_motion_default_params: temporal reprojection's)."""
    p = TemporalParams()
    check(_lib.load_motion().iqpt_motion_default_params(C.byref(p)), "iqpt_motion_default_params")
    return {"normal_min": p.normal_min, "plane_tolerance": p.plane_tolerance, "max_history": p.max_history}


def identity_table(n: int) -> np.ndarray:
    """n entries with moved = 0 and identity matrices."""
    t = np.zeros(n, ENTRY_DTYPE)
    t["back"][:, [0, 5, 10, 15]] = 1.0
    t["nback"][:, [0, 5, 10]] = 1.0
    return t


def _draw_items(lib, scene):
    n = C.c_uint32()
    check(lib.iqpt_scene_draw_list(scene._h, None, 0, C.byref(n)), "iqpt_scene_draw_list")
    items = (_lib.DrawItem * max(n.value, 1))()
    check(lib.iqpt_scene_draw_list(scene._h, items, n.value, C.byref(n)), "iqpt_scene_draw_list")
    return items, n.value


def motion_table(prev_scene, cur_scene) -> np.ndarray:
    """The motion table of two scenes with the same meshes and models (iqpt_motion_table over their draw lists):
    a structured array of ENTRY_DTYPE, one entry per draw index."""
    lib = _lib.load()
    prev, n_prev = _draw_items(lib, prev_scene)
    cur, n_cur = _draw_items(lib, cur_scene)
    out = np.zeros(max(n_cur, 1), ENTRY_DTYPE)
    check(_lib.load_motion().iqpt_motion_table(prev, n_prev, cur, n_cur, out.ctypes.data_as(C.POINTER(MotionEntry))),
          "iqpt_motion_table")
    return out[:n_cur]


def _table_args(motion):
    """(keep-alive array, pointer, n) of a begin_view's motion= argument: None, or an array of ENTRY_DTYPE."""
    if motion is None:
        return None, None, 0
    t = np.ascontiguousarray(motion)
    if t.dtype != ENTRY_DTYPE:
        raise ValueError("motion must be an array of iqpt.motion.ENTRY_DTYPE (iqpt.motion_table makes one)")
    t = t.reshape(-1)
    return t, (C.c_void_p(t.ctypes.data) if t.size else None), int(t.size)


class Motion:
    """Reprojection of the last result into every new view through each model's motion, and its blend with the
    accumulator (iqpt_motion_create .. iqpt_motion_destroy). Raises IqptError on failure. ``lib``: another build of
    libiqpt_motion.so (the A/B library with wave-uniform entry loads)."""

    def __init__(self, width: int, height: int, device: int = 0, lib=None):
        self._lib = _lib.load_motion(lib)
        h = C.c_void_p()
        check(self._lib.iqpt_motion_create(device, width, height, C.byref(h)), "iqpt_motion_create")
        self._h = h
        self.width, self.height = width, height

    def close(self):
        if getattr(self, "_h", None):
            self._lib.iqpt_motion_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_params(self, normal_min: float, plane_tolerance: float, max_history: int):
        p = TemporalParams(normal_min, plane_tolerance, max_history)
        check(self._lib.iqpt_motion_set_params(self._h, C.byref(p)), "iqpt_motion_set_params")

    def begin_view(self, cam: Camera, normal_z, ids, motion=None):
        """A new view: its camera, normal_z [H,W,4] float32 (n, z) and ids [H,W] uint32, as Rasterizer.gbuffer()
        returns them, and the motion table of the scene change before it (None: no model moved)."""
        n = np.ascontiguousarray(normal_z, dtype=np.float32)
        i = np.ascontiguousarray(ids, dtype=np.uint32)
        if n.size != self.width * self.height * 4 or i.size != self.width * self.height:
            raise ValueError("guides must have width*height entries")
        _keep, tp, tn = _table_args(motion)
        check(self._lib.iqpt_motion_begin_view(self._h, C.byref(cam), n.ctypes.data_as(C.POINTER(C.c_float)),
                                               i.ctypes.data_as(C.POINTER(C.c_uint32)), tp, tn), "iqpt_motion_begin_view")

    def begin_view_device(self, cam: Camera, normal_z_ptr: int, id_ptr: int, motion=None):
        _keep, tp, tn = _table_args(motion)
        check(self._lib.iqpt_motion_begin_view_device(self._h, C.byref(cam), C.c_void_p(normal_z_ptr), C.c_void_p(id_ptr),
                                                      tp, tn), "iqpt_motion_begin_view_device")

    def begin_view_raster(self, rasterizer, motion=None):
        """The rasterizer's G-buffer and the camera it was last given (iqpt_motion_begin_view_raster)."""
        _keep, tp, tn = _table_args(motion)
        check(self._lib.iqpt_motion_begin_view_raster(self._h, rasterizer.handle, tp, tn), "iqpt_motion_begin_view_raster")

    def clear(self):
        check(self._lib.iqpt_motion_clear(self._h), "iqpt_motion_clear")

    def resolve(self, colour, n: int):
        """Blend the view's history with colour [H,W,4] (or [H*W,4]) float32, the mean of n samples; the result is
        fetched with read()."""
        c = np.ascontiguousarray(colour, dtype=np.float32)
        if c.size != self.width * self.height * 4:
            raise ValueError("colour must have width*height float4 entries")
        check(self._lib.iqpt_motion_resolve(self._h, c.ctypes.data_as(C.POINTER(C.c_float)), n), "iqpt_motion_resolve")

    def resolve_device(self, colour_ptr: int, n: int):
        check(self._lib.iqpt_motion_resolve_device(self._h, C.c_void_p(colour_ptr), n), "iqpt_motion_resolve_device")

    def resolve_ctx(self, path_tracer):
        """The path tracer's accumulator and frame count (iqpt_motion_resolve_ctx)."""
        check(self._lib.iqpt_motion_resolve_ctx(self._h, path_tracer.handle), "iqpt_motion_resolve_ctx")

    def read(self) -> tuple[np.ndarray, np.ndarray]:
        """(lin [H,W,4] float32 with w = the samples behind the pixel, bgra [H,W,4] uint8) of the last resolve."""
        lin = np.empty((self.height, self.width, 4), dtype=np.float32)
        bgra = np.empty((self.height, self.width, 4), dtype=np.uint8)
        check(self._lib.iqpt_motion_read(self._h, lin.ctypes.data_as(C.POINTER(C.c_float)),
                                         bgra.ctypes.data_as(C.POINTER(C.c_uint8))), "iqpt_motion_read")
        return lin, bgra

    def output_device(self) -> int:
        """The device pointer of the float4 result (iqpt_motion_output_device), e.g. for Denoiser.run_device."""
        p = C.c_void_p()
        check(self._lib.iqpt_motion_output_device(self._h, C.byref(p)), "iqpt_motion_output_device")
        return int(p.value or 0)

    def copy_frame_device(self, dst_ptr: int, nbytes: int):
        check(self._lib.iqpt_motion_copy_frame_device(self._h, C.c_void_p(dst_ptr), nbytes), "iqpt_motion_copy_frame_device")

    def sync(self):
        check(self._lib.iqpt_motion_sync(self._h), "iqpt_motion_sync")

    def time(self) -> tuple[float, int, float, int]:
        """(view ms, views, resolve ms, resolves) since the last call (HIP events; iqpt_motion_time)."""
        vms, rms, nv, nr = C.c_double(), C.c_double(), C.c_uint64(), C.c_uint64()
        check(self._lib.iqpt_motion_time(self._h, C.byref(vms), C.byref(nv), C.byref(rms), C.byref(nr)), "iqpt_motion_time")
        return vms.value, nv.value, rms.value, nr.value

    def stats(self) -> tuple[int, int, int, int]:
        """(guided pixels, pixels with a valid history, pixels of moved models, those of them with a valid history)
        of the last begin_view (iqpt_motion_stats)."""
        g, v, m, mv = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self._lib.iqpt_motion_stats(self._h, C.byref(g), C.byref(v), C.byref(m), C.byref(mv)), "iqpt_motion_stats")
        return g.value, v.value, m.value, mv.value
