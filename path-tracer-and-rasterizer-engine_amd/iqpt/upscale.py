"""Upscaler binding: ``Upscaler`` owns one iqpt_upscale (guided upsampling of a frame traced at 1/f size,
DESIGN.md §14)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import UpscaleParams, check


def default_params() -> dict:
    """The parameters a new Upscaler starts with (iqpt_upscale_default_params)."""
    p = UpscaleParams()
    check(_lib.load().iqpt_upscale_default_params(C.byref(p)), "iqpt_upscale_default_params")
    return {"normal_squarings": p.normal_squarings, "depth_sharpness": p.depth_sharpness}


class Upscaler:
    """Joint bilateral upsampling of a (width / factor) x (height / factor) float4 frame to width x height, guided
    by the G-buffers of both sizes (iqpt_upscale_create .. iqpt_upscale_destroy). Raises IqptError on failure."""

    def __init__(self, width: int, height: int, factor: int, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.iqpt_upscale_create(device, width, height, factor, C.byref(h)), "iqpt_upscale_create")
        self._h = h
        self.width, self.height, self.factor = width, height, factor
        self.lo_width, self.lo_height = width // factor, height // factor

    def close(self):
        if getattr(self, "_h", None):
            self._lib.iqpt_upscale_destroy(self._h)
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

    def set_params(self, normal_squarings: int, depth_sharpness: float):
        p = UpscaleParams(normal_squarings, depth_sharpness)
        check(self._lib.iqpt_upscale_set_params(self._h, C.byref(p)), "iqpt_upscale_set_params")

    def set_guides(self, normal_z_lo, ids_lo, normal_z_hi, ids_hi):
        """normal_z [h,w,4] float32 (n, z) and ids [h,w] uint32 of the lo size, then the same of the hi size, as
        Rasterizer.gbuffer() returns them."""
        planes = []
        for nz, ids, n in ((normal_z_lo, ids_lo, self.lo_width * self.lo_height), (normal_z_hi, ids_hi, self.width * self.height)):
            a = np.ascontiguousarray(nz, dtype=np.float32)
            i = np.ascontiguousarray(ids, dtype=np.uint32)
            if a.size != n * 4 or i.size != n:
                raise ValueError("guides must have one entry per pixel of their frame")
            planes += [a, i]
        check(self._lib.iqpt_upscale_set_guides(self._h, planes[0].ctypes.data_as(C.POINTER(C.c_float)),
                                                planes[1].ctypes.data_as(C.POINTER(C.c_uint32)),
                                                planes[2].ctypes.data_as(C.POINTER(C.c_float)),
                                                planes[3].ctypes.data_as(C.POINTER(C.c_uint32))), "iqpt_upscale_set_guides")

    def set_guides_device(self, normal_z_lo_ptr: int, id_lo_ptr: int, normal_z_hi_ptr: int, id_hi_ptr: int):
        check(self._lib.iqpt_upscale_set_guides_device(self._h, C.c_void_p(normal_z_lo_ptr), C.c_void_p(id_lo_ptr),
                                                       C.c_void_p(normal_z_hi_ptr), C.c_void_p(id_hi_ptr)),
              "iqpt_upscale_set_guides_device")

    def run(self, colour_lo):
        """Upsample colour_lo [h,w,4] (or [h*w,4]) float32 of the lo size; the result is fetched with read()."""
        c = np.ascontiguousarray(colour_lo, dtype=np.float32)
        if c.size != self.lo_width * self.lo_height * 4:
            raise ValueError("colour must have one float4 per pixel of the lo frame")
        check(self._lib.iqpt_upscale_run(self._h, c.ctypes.data_as(C.POINTER(C.c_float))), "iqpt_upscale_run")

    def run_device(self, colour_lo_ptr: int):
        check(self._lib.iqpt_upscale_run_device(self._h, C.c_void_p(colour_lo_ptr)), "iqpt_upscale_run_device")

    def frame(self, path_tracer, rasterizer_lo, rasterizer_hi):
        """The lo path tracer's accumulator under the two rasterizers' G-buffers (iqpt_upscale_frame)."""
        check(self._lib.iqpt_upscale_frame(self._h, path_tracer.handle, rasterizer_lo.handle, rasterizer_hi.handle),
              "iqpt_upscale_frame")

    def read(self) -> tuple[np.ndarray, np.ndarray]:
        """(lin [H,W,4] float32 with w = the pixel's class, bgra [H,W,4] uint8) of the last run."""
        lin = np.empty((self.height, self.width, 4), dtype=np.float32)
        bgra = np.empty((self.height, self.width, 4), dtype=np.uint8)
        check(self._lib.iqpt_upscale_read(self._h, lin.ctypes.data_as(C.POINTER(C.c_float)),
                                          bgra.ctypes.data_as(C.POINTER(C.c_uint8))), "iqpt_upscale_read")
        return lin, bgra

    @property
    def output_ptr(self) -> int:
        """The float4 result on the device, complete (iqpt_upscale_output_device): what Denoiser.run_device or
        Temporal.resolve_device of the full size takes."""
        p = C.c_void_p()
        check(self._lib.iqpt_upscale_output_device(self._h, C.byref(p)), "iqpt_upscale_output_device")
        return p.value

    def copy_frame_device(self, dst_ptr: int, nbytes: int):
        check(self._lib.iqpt_upscale_copy_frame_device(self._h, C.c_void_p(dst_ptr), nbytes),
              "iqpt_upscale_copy_frame_device")

    def sync(self):
        check(self._lib.iqpt_upscale_sync(self._h), "iqpt_upscale_sync")

    def time(self) -> tuple[float, int]:
        """(kernel ms summed over the runs, runs) since the last call (HIP events; iqpt_upscale_time)."""
        ms, n = C.c_double(), C.c_uint64()
        check(self._lib.iqpt_upscale_time(self._h, C.byref(ms), C.byref(n)), "iqpt_upscale_time")
        return ms.value, n.value

    def stats(self) -> tuple[int, int, int]:
        """(guided, widened, unguided): the hi pixels of each class in the last run (iqpt_upscale_stats)."""
        g, w, u = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self._lib.iqpt_upscale_stats(self._h, C.byref(g), C.byref(w), C.byref(u)), "iqpt_upscale_stats")
        return g.value, w.value, u.value
