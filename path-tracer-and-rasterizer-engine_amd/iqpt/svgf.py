"""Variance-guided filtering binding: ``Svgf`` owns one iqpt_svgf (two temporal histories, the per-pixel variance
estimate and the à-trous filter it guides)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Camera, SvgfParams, check

PARAM_NAMES = tuple(name for name, _ in SvgfParams._fields_)


def default_params() -> dict:
    """The parameters a new Svgf starts with (iqpt_svgf_default_params)."""
    p = SvgfParams()
    check(_lib.load().iqpt_svgf_default_params(C.byref(p)), "iqpt_svgf_default_params")
    return {name: getattr(p, name) for name in PARAM_NAMES}


class Svgf:
    """Both histories, the variance estimate and the filter of one frame size (iqpt_svgf_create ..
    iqpt_svgf_destroy). Raises IqptError on failure."""

    def __init__(self, width: int, height: int, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.iqpt_svgf_create(device, width, height, C.byref(h)), "iqpt_svgf_create")
        self._h = h
        self.width, self.height = width, height

    def close(self):
        if getattr(self, "_h", None):
            self._lib.iqpt_svgf_destroy(self._h)
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

    def set_params(self, normal_min: float, plane_tolerance: float, max_history: int, min_history: int, levels: int,
                   normal_squarings: int, depth_sharpness: float, colour_sigma: float, variance_floor: float):
        p = SvgfParams(normal_min, plane_tolerance, max_history, min_history, levels, normal_squarings, depth_sharpness,
                       colour_sigma, variance_floor)
        check(self._lib.iqpt_svgf_set_params(self._h, C.byref(p)), "iqpt_svgf_set_params")

    def begin_view(self, cam: Camera, normal_z, ids):
        """A new view: its camera, normal_z [H,W,4] float32 (n, z) and ids [H,W] uint32, as Rasterizer.gbuffer()
        returns them."""
        n = np.ascontiguousarray(normal_z, dtype=np.float32)
        i = np.ascontiguousarray(ids, dtype=np.uint32)
        if n.size != self.width * self.height * 4 or i.size != self.width * self.height:
            raise ValueError("guides must have width*height entries")
        check(self._lib.iqpt_svgf_begin_view(self._h, C.byref(cam), n.ctypes.data_as(C.POINTER(C.c_float)),
                                             i.ctypes.data_as(C.POINTER(C.c_uint32))), "iqpt_svgf_begin_view")

    def begin_view_device(self, cam: Camera, normal_z_ptr: int, id_ptr: int):
        check(self._lib.iqpt_svgf_begin_view_device(self._h, C.byref(cam), C.c_void_p(normal_z_ptr), C.c_void_p(id_ptr)),
              "iqpt_svgf_begin_view_device")

    def begin_view_raster(self, rasterizer):
        """The rasterizer's G-buffer and the camera it was last given (iqpt_svgf_begin_view_raster)."""
        check(self._lib.iqpt_svgf_begin_view_raster(self._h, rasterizer.handle), "iqpt_svgf_begin_view_raster")

    def clear(self):
        check(self._lib.iqpt_svgf_clear(self._h), "iqpt_svgf_clear")

    def resolve(self, colour, n: int):
        """The whole chain for colour [H,W,4] (or [H*W,4]) float32, the mean of n samples; the result is fetched
        with read()."""
        c = np.ascontiguousarray(colour, dtype=np.float32)
        if c.size != self.width * self.height * 4:
            raise ValueError("colour must have width*height float4 entries")
        check(self._lib.iqpt_svgf_resolve(self._h, c.ctypes.data_as(C.POINTER(C.c_float)), n), "iqpt_svgf_resolve")

    def resolve_device(self, colour_ptr: int, n: int):
        check(self._lib.iqpt_svgf_resolve_device(self._h, C.c_void_p(colour_ptr), n), "iqpt_svgf_resolve_device")

    def resolve_ctx(self, path_tracer):
        """The path tracer's accumulator and frame count (iqpt_svgf_resolve_ctx)."""
        check(self._lib.iqpt_svgf_resolve_ctx(self._h, path_tracer.handle), "iqpt_svgf_resolve_ctx")

    def read(self) -> tuple[np.ndarray, np.ndarray]:
        """(lin [H,W,4] float32 with w = the filtered variance, bgra [H,W,4] uint8) of the last resolve."""
        lin = np.empty((self.height, self.width, 4), dtype=np.float32)
        bgra = np.empty((self.height, self.width, 4), dtype=np.uint8)
        check(self._lib.iqpt_svgf_read(self._h, lin.ctypes.data_as(C.POINTER(C.c_float)),
                                       bgra.ctypes.data_as(C.POINTER(C.c_uint8))), "iqpt_svgf_read")
        return lin, bgra

    def read_stages(self) -> tuple[np.ndarray, np.ndarray]:
        """(the colour history's result, c_0 = that colour with w = the variance estimate), [H,W,4] float32 each."""
        t = np.empty((self.height, self.width, 4), dtype=np.float32)
        v = np.empty((self.height, self.width, 4), dtype=np.float32)
        check(self._lib.iqpt_svgf_read_stages(self._h, t.ctypes.data_as(C.POINTER(C.c_float)),
                                              v.ctypes.data_as(C.POINTER(C.c_float))), "iqpt_svgf_read_stages")
        return t, v

    def copy_frame_device(self, dst_ptr: int, nbytes: int):
        check(self._lib.iqpt_svgf_copy_frame_device(self._h, C.c_void_p(dst_ptr), nbytes), "iqpt_svgf_copy_frame_device")

    def sync(self):
        check(self._lib.iqpt_svgf_sync(self._h), "iqpt_svgf_sync")

    def time(self) -> dict:
        """HIP-event sums since the last call (iqpt_svgf_time): moments_ms, variance_ms, level_ms [8], resolves,
        view_ms and history_resolve_ms ([colour history, moments history] each)."""
        mom, var, n = C.c_double(), C.c_double(), C.c_uint64()
        lev, view, res = (C.c_double * 8)(), (C.c_double * 2)(), (C.c_double * 2)()
        check(self._lib.iqpt_svgf_time(self._h, C.byref(mom), C.byref(var), lev, C.byref(n), view, res), "iqpt_svgf_time")
        return {"moments_ms": mom.value, "variance_ms": var.value, "level_ms": list(lev), "resolves": n.value,
                "view_ms": list(view), "history_resolve_ms": list(res)}

    def stats(self) -> tuple[int, int, int]:
        """(guided pixels, pixels with a valid history, pixels that took the spatial estimate at the last resolve)."""
        g, v, s = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self._lib.iqpt_svgf_stats(self._h, C.byref(g), C.byref(v), C.byref(s)), "iqpt_svgf_stats")
        return g.value, v.value, s.value
