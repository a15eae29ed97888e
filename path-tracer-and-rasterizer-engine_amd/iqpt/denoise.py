"""Denoiser binding: ``Denoiser`` owns one iqpt_denoise (the rasterizer-guided à-trous filter)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import DenoiseParams, check


def default_params() -> dict:
    """The parameters a new Denoiser starts with (iqpt_denoise_default_params)."""
    p = DenoiseParams()
    check(_lib.load().iqpt_denoise_default_params(C.byref(p)), "iqpt_denoise_default_params")
    return {"levels": p.levels, "normal_squarings": p.normal_squarings, "depth_sharpness": p.depth_sharpness,
            "colour_sharpness": p.colour_sharpness}


class Denoiser:
    """The edge-avoiding à-trous filter over a float4 frame, guided by a G-buffer (iqpt_denoise_create ..
    iqpt_denoise_destroy). Raises IqptError on failure."""

    def __init__(self, width: int, height: int, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.iqpt_denoise_create(device, width, height, C.byref(h)), "iqpt_denoise_create")
        self._h = h
        self.width, self.height = width, height

    def close(self):
        if getattr(self, "_h", None):
            self._lib.iqpt_denoise_destroy(self._h)
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

    def set_params(self, levels: int, normal_squarings: int, depth_sharpness: float, colour_sharpness: float):
        p = DenoiseParams(levels, normal_squarings, depth_sharpness, colour_sharpness)
        check(self._lib.iqpt_denoise_set_params(self._h, C.byref(p)), "iqpt_denoise_set_params")

    def set_guides(self, normal_z, ids):
        """normal_z [H,W,4] float32 (n, z) and ids [H,W] uint32, as Rasterizer.gbuffer() returns them."""
        n = np.ascontiguousarray(normal_z, dtype=np.float32)
        i = np.ascontiguousarray(ids, dtype=np.uint32)
        if n.size != self.width * self.height * 4 or i.size != self.width * self.height:
            raise ValueError("guides must have width*height entries")
        check(self._lib.iqpt_denoise_set_guides(self._h, n.ctypes.data_as(C.POINTER(C.c_float)),
                                                i.ctypes.data_as(C.POINTER(C.c_uint32))), "iqpt_denoise_set_guides")

    def set_guides_device(self, normal_z_ptr: int, id_ptr: int):
        check(self._lib.iqpt_denoise_set_guides_device(self._h, C.c_void_p(normal_z_ptr), C.c_void_p(id_ptr)),
              "iqpt_denoise_set_guides_device")

    def run(self, colour):
        """Filter colour [H,W,4] (or [H*W,4]) float32; the result is fetched with read()."""
        c = np.ascontiguousarray(colour, dtype=np.float32)
        if c.size != self.width * self.height * 4:
            raise ValueError("colour must have width*height float4 entries")
        check(self._lib.iqpt_denoise_run(self._h, c.ctypes.data_as(C.POINTER(C.c_float))), "iqpt_denoise_run")

    def run_device(self, colour_ptr: int):
        check(self._lib.iqpt_denoise_run_device(self._h, C.c_void_p(colour_ptr)), "iqpt_denoise_run_device")

    def frame(self, path_tracer, rasterizer):
        """The path tracer's accumulator under the rasterizer's G-buffer (iqpt_denoise_frame)."""
        check(self._lib.iqpt_denoise_frame(self._h, path_tracer.handle, rasterizer.handle), "iqpt_denoise_frame")

    def read(self) -> tuple[np.ndarray, np.ndarray]:
        """(lin [H,W,4] float32, bgra [H,W,4] uint8) of the last run."""
        lin = np.empty((self.height, self.width, 4), dtype=np.float32)
        bgra = np.empty((self.height, self.width, 4), dtype=np.uint8)
        check(self._lib.iqpt_denoise_read(self._h, lin.ctypes.data_as(C.POINTER(C.c_float)),
                                          bgra.ctypes.data_as(C.POINTER(C.c_uint8))), "iqpt_denoise_read")
        return lin, bgra

    def copy_frame_device(self, dst_ptr: int, nbytes: int):
        check(self._lib.iqpt_denoise_copy_frame_device(self._h, C.c_void_p(dst_ptr), nbytes),
              "iqpt_denoise_copy_frame_device")

    def sync(self):
        check(self._lib.iqpt_denoise_sync(self._h), "iqpt_denoise_sync")

    def time(self) -> tuple[float, list[float], int]:
        """(total ms, ms per level [8], runs) since the last call (HIP events; iqpt_denoise_time)."""
        ms, n = C.c_double(), C.c_uint64()
        lv = (C.c_double * _lib.DENOISE_MAX_LEVELS)()
        check(self._lib.iqpt_denoise_time(self._h, C.byref(ms), lv, C.byref(n)), "iqpt_denoise_time")
        return ms.value, list(lv), n.value
