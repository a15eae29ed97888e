"""Temporal binding: ``Temporal`` owns one iqpt_temporal (the history buffer that follows the camera)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Camera, TemporalParams, check


def default_params() -> dict:
    """The parameters a new Temporal starts with (iqpt_temporal_default_params)."""
    p = TemporalParams()
    check(_lib.load().iqpt_temporal_default_params(C.byref(p)), "iqpt_temporal_default_params")
    return {"normal_min": p.normal_min, "plane_tolerance": p.plane_tolerance, "max_history": p.max_history}


class Temporal:
    """Reprojection of the last result into every new view and its blend with the accumulator
    (iqpt_temporal_create .. iqpt_temporal_destroy). Raises IqptError on failure."""

    def __init__(self, width: int, height: int, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.iqpt_temporal_create(device, width, height, C.byref(h)), "iqpt_temporal_create")
        self._h = h
        self.width, self.height = width, height

    def close(self):
        if getattr(self, "_h", None):
            self._lib.iqpt_temporal_destroy(self._h)
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
        check(self._lib.iqpt_temporal_set_params(self._h, C.byref(p)), "iqpt_temporal_set_params")

    def begin_view(self, cam: Camera, normal_z, ids):
        """A new view: its camera, normal_z [H,W,4] float32 (n, z) and ids [H,W] uint32, as Rasterizer.gbuffer()
        returns them."""
        n = np.ascontiguousarray(normal_z, dtype=np.float32)
        i = np.ascontiguousarray(ids, dtype=np.uint32)
        if n.size != self.width * self.height * 4 or i.size != self.width * self.height:
            raise ValueError("guides must have width*height entries")
        check(self._lib.iqpt_temporal_begin_view(self._h, C.byref(cam), n.ctypes.data_as(C.POINTER(C.c_float)),
                                                 i.ctypes.data_as(C.POINTER(C.c_uint32))), "iqpt_temporal_begin_view")

    def begin_view_device(self, cam: Camera, normal_z_ptr: int, id_ptr: int):
        check(self._lib.iqpt_temporal_begin_view_device(self._h, C.byref(cam), C.c_void_p(normal_z_ptr),
                                                        C.c_void_p(id_ptr)), "iqpt_temporal_begin_view_device")

    def begin_view_raster(self, rasterizer):
        """The rasterizer's G-buffer and the camera it was last given (iqpt_temporal_begin_view_raster)."""
        check(self._lib.iqpt_temporal_begin_view_raster(self._h, rasterizer.handle), "iqpt_temporal_begin_view_raster")

    def clear(self):
        check(self._lib.iqpt_temporal_clear(self._h), "iqpt_temporal_clear")

    def resolve(self, colour, n: int):
        """Blend the view's history with colour [H,W,4] (or [H*W,4]) float32, the mean of n samples; the result is
        fetched with read()."""
        c = np.ascontiguousarray(colour, dtype=np.float32)
        if c.size != self.width * self.height * 4:
            raise ValueError("colour must have width*height float4 entries")
        check(self._lib.iqpt_temporal_resolve(self._h, c.ctypes.data_as(C.POINTER(C.c_float)), n), "iqpt_temporal_resolve")

    def resolve_device(self, colour_ptr: int, n: int):
        check(self._lib.iqpt_temporal_resolve_device(self._h, C.c_void_p(colour_ptr), n), "iqpt_temporal_resolve_device")

    def resolve_ctx(self, path_tracer):
        """The path tracer's accumulator and frame count (iqpt_temporal_resolve_ctx)."""
        check(self._lib.iqpt_temporal_resolve_ctx(self._h, path_tracer.handle), "iqpt_temporal_resolve_ctx")

    def read(self) -> tuple[np.ndarray, np.ndarray]:
        """(lin [H,W,4] float32 with w = the samples behind the pixel, bgra [H,W,4] uint8) of the last resolve."""
        lin = np.empty((self.height, self.width, 4), dtype=np.float32)
        bgra = np.empty((self.height, self.width, 4), dtype=np.uint8)
        check(self._lib.iqpt_temporal_read(self._h, lin.ctypes.data_as(C.POINTER(C.c_float)),
                                           bgra.ctypes.data_as(C.POINTER(C.c_uint8))), "iqpt_temporal_read")
        return lin, bgra

    def output_device(self) -> int:
        """The device pointer of the float4 result (iqpt_temporal_output_device), e.g. for Denoiser.run_device."""
        p = C.c_void_p()
        check(self._lib.iqpt_temporal_output_device(self._h, C.byref(p)), "iqpt_temporal_output_device")
        return int(p.value or 0)

    def copy_frame_device(self, dst_ptr: int, nbytes: int):
        check(self._lib.iqpt_temporal_copy_frame_device(self._h, C.c_void_p(dst_ptr), nbytes),
              "iqpt_temporal_copy_frame_device")

    def sync(self):
        check(self._lib.iqpt_temporal_sync(self._h), "iqpt_temporal_sync")

    def time(self) -> tuple[float, int, float, int]:
        """(view ms, views, resolve ms, resolves) since the last call (HIP events; iqpt_temporal_time)."""
        vms, rms, nv, nr = C.c_double(), C.c_double(), C.c_uint64(), C.c_uint64()
        check(self._lib.iqpt_temporal_time(self._h, C.byref(vms), C.byref(nv), C.byref(rms), C.byref(nr)),
              "iqpt_temporal_time")
        return vms.value, nv.value, rms.value, nr.value

    def stats(self) -> tuple[int, int]:
        """(guided pixels, pixels with a valid history) of the last begin_view (iqpt_temporal_stats)."""
        g, v = C.c_uint64(), C.c_uint64()
        check(self._lib.iqpt_temporal_stats(self._h, C.byref(g), C.byref(v)), "iqpt_temporal_stats")
        return g.value, v.value
