"""Rasterizer binding: ``Rasterizer`` owns one iqpt_raster (the engine's second renderer)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Camera, check
from .scene import Scene


class Rasterizer:
    """The headless HIP rasterizer (iqpt_raster_create .. iqpt_raster_destroy). Raises IqptError on failure."""

    def __init__(self, width: int, height: int, samples: int = 4, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.iqpt_raster_create(device, width, height, samples, C.byref(h)), "iqpt_raster_create")
        self._h = h
        self.width, self.height, self.samples = width, height, samples

    def close(self):
        if getattr(self, "_h", None):
            self._lib.iqpt_raster_destroy(self._h)
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

    def set_camera(self, cam: Camera):
        check(self._lib.iqpt_raster_set_camera(self._h, C.byref(cam)), "iqpt_raster_set_camera")

    def upload_scene(self, scene: Scene):
        check(self._lib.iqpt_raster_upload_scene(self._h, scene._h), "iqpt_raster_upload_scene")

    def draw(self):
        check(self._lib.iqpt_raster_draw(self._h), "iqpt_raster_draw")

    def draw_clip(self, clip_xyzw, normals, indices):
        """One frame from clip-space vertices [n,4], their world normals [n,3] and clockwise index triples."""
        c = np.ascontiguousarray(clip_xyzw, dtype=np.float32).reshape(-1, 4)
        n = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        if n.shape[0] != c.shape[0]:
            raise ValueError("one normal per vertex")
        fp = C.POINTER(C.c_float)
        check(self._lib.iqpt_raster_draw_clip(self._h, c.ctypes.data_as(fp), n.ctypes.data_as(fp), c.shape[0],
                                              i.ctypes.data_as(C.POINTER(C.c_uint32)), i.shape[0]),
              "iqpt_raster_draw_clip")

    def read(self, samples: bool = False):
        """bgra [H,W,4] uint8; with samples=True also depth [H,W,S] float32 and primitive index [H,W,S] uint32
        (RASTER_NO_PRIM where nothing was drawn)."""
        bgra = np.empty((self.height, self.width, 4), dtype=np.uint8)
        b = bgra.ctypes.data_as(C.POINTER(C.c_uint8))
        if not samples:
            check(self._lib.iqpt_raster_read(self._h, b, None, None), "iqpt_raster_read")
            return bgra
        depth = np.empty((self.height, self.width, self.samples), dtype=np.float32)
        prim = np.empty((self.height, self.width, self.samples), dtype=np.uint32)
        check(self._lib.iqpt_raster_read(self._h, b, depth.ctypes.data_as(C.POINTER(C.c_float)),
                                         prim.ctypes.data_as(C.POINTER(C.c_uint32))), "iqpt_raster_read")
        return bgra, depth, prim

    def gbuffer(self):
        """The G-buffer of the uploaded scene through the current camera: normal_z [H,W,4] float32
        (the normalised interpolated normal and the D32 depth) and id [H,W] uint32 (the draw index, RASTER_NO_PRIM
        where nothing was drawn). One sample per pixel and two-sided, whatever `samples` is."""
        check(self._lib.iqpt_raster_gbuffer(self._h), "iqpt_raster_gbuffer")
        nz = np.empty((self.height, self.width, 4), dtype=np.float32)
        ids = np.empty((self.height, self.width), dtype=np.uint32)
        check(self._lib.iqpt_raster_read_gbuffer(self._h, nz.ctypes.data_as(C.POINTER(C.c_float)),
                                                 ids.ctypes.data_as(C.POINTER(C.c_uint32))), "iqpt_raster_read_gbuffer")
        return nz, ids

    def gbuffer_device(self) -> tuple[int, int]:
        """Device pointers (normal_z, id) of the G-buffer, computed if need be (iqpt_raster_gbuffer_device)."""
        check(self._lib.iqpt_raster_gbuffer(self._h), "iqpt_raster_gbuffer")
        a, b = C.c_void_p(), C.c_void_p()
        check(self._lib.iqpt_raster_gbuffer_device(self._h, C.byref(a), C.byref(b)), "iqpt_raster_gbuffer_device")
        return a.value, b.value

    def gbuffer_time(self) -> tuple[float, int]:
        """(total ms, passes) of the G-buffer passes since the last call (iqpt_raster_gbuffer_time)."""
        ms, n = C.c_double(), C.c_uint64()
        check(self._lib.iqpt_raster_gbuffer_time(self._h, C.byref(ms), C.byref(n)), "iqpt_raster_gbuffer_time")
        return ms.value, n.value

    def copy_frame_device(self, dst_ptr: int, nbytes: int):
        check(self._lib.iqpt_raster_copy_frame_device(self._h, C.c_void_p(dst_ptr), nbytes),
              "iqpt_raster_copy_frame_device")

    def sync(self):
        check(self._lib.iqpt_raster_sync(self._h), "iqpt_raster_sync")

    def stage_time(self) -> list[float]:
        """ms per stage (vertex, setup, bin, sort, tiles) of the draws since the last time() call."""
        st = (C.c_double * 5)()
        check(self._lib.iqpt_raster_stage_time(self._h, st), "iqpt_raster_stage_time")
        return list(st)

    def time(self) -> tuple[float, int]:
        """(total ms, draws) since the last call (HIP events; iqpt_raster_time)."""
        ms, n = C.c_double(), C.c_uint64()
        check(self._lib.iqpt_raster_time(self._h, C.byref(ms), C.byref(n)), "iqpt_raster_time")
        return ms.value, n.value

    def stats(self) -> dict:
        c = (C.c_uint64 * 3)()
        check(self._lib.iqpt_raster_stats(self._h, c), "iqpt_raster_stats")
        return {"triangles": c[0], "records": c[1], "pairs": c[2]}
