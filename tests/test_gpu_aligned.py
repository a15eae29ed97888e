"""Aligned cameras (iqpt_camera_align) through the path tracer's camera paths, on the GPU.

An aligned camera has inv_proj[12] and inv_proj[13] non-zero with inv_proj[3] = inv_proj[7] = 0: kOptCamConst still
sees a constant w, cam_axis_constants still accepts a pitch-only camera, and the proofs' interval bundle carries the
two entries through dot_col like any other. No camera of iqpt_camera_init has that combination. Here cornell and
app_default, in a frame smaller than three tiles and in one of 8 x 5 tiles, under the aligned default camera and an
aligned camera of another pitch, rendered with the short camera transform forced on and off and with the certain-miss
sky kernel on and off: accumulator, BGRA8, XORWOW states and ray counts equal the oracle's bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import compare, scene_for
from iqpt import PathTracer, _lib, align_camera, make_camera
from test_camera_axis import cam_axis, pitch_camera

pytestmark = pytest.mark.gpu

K_OPT_CAM_AXIS = 1 << 14
SPP, DEPTH = 2, 5


def cameras(w, h):
    return {"default": align_camera(make_camera(w, h)),
            "pitch": align_camera(pitch_camera(w, h, 0.2, (0.0, 0.3, -2.5), fovh=60.0))}


_oracle = {}


def oracle_frame(preset, w, h, cname):
    """The oracle's frame of a case, rendered once and shared by the four switch settings."""
    key = (preset, w, h, cname)
    if key not in _oracle:
        sc, pk = scene_for(preset)
        fr = oracle.OracleFrame(w, h, max_depth=DEPTH)
        fr.render(pk, cameras(w, h)[cname], SPP)
        for a in (fr.lin, fr.bgra, fr.states, fr.rays):
            a.setflags(write=False)
        _oracle[key] = fr
    return _oracle[key]


@pytest.mark.parametrize("sky", [True, False])
@pytest.mark.parametrize("axis", [True, False])
@pytest.mark.parametrize("cname", ["default", "pitch"])
@pytest.mark.parametrize("w,h", [(17, 13), (64, 40)])
@pytest.mark.parametrize("preset", ["cornell", "app_default"])
def test_aligned_camera_frames_match_the_oracle(require_gpu, preset, w, h, cname, axis, sky):
    lb = _lib.load()
    lb.iqpt_debug_set_kernel_options.argtypes = [C.c_void_p, C.c_int]
    lb.iqpt_debug_last_options.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lb.iqpt_debug_set_sky.argtypes = [C.c_void_p, C.c_int]
    lb.iqpt_debug_sky_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    cam = cameras(w, h)[cname]
    assert cam.inv_proj[12] != 0.0 and cam.inv_proj[13] != 0.0 and cam_axis(cam)[0]
    sc, pk = scene_for(preset)
    with PathTracer(w, h, max_depth=DEPTH) as pt:
        pt.set_split(_lib.SPLIT_OFF)                     # plain launches: the ones that hand pixels to the sky kernel
        # (a fixed option set: the runtime adds the short transform by itself only where none was given)
        opt = lb.iqpt_debug_default_options() | (K_OPT_CAM_AXIS if axis else 0)
        _lib.check(lb.iqpt_debug_set_kernel_options(pt.handle, opt), "iqpt_debug_set_kernel_options")
        _lib.check(lb.iqpt_debug_set_sky(pt.handle, 1 if sky else 0), "iqpt_debug_set_sky")
        pt.set_camera(cam)
        pt.upload_packet(pk)
        pt.render(SPP)
        lin, bgra = pt.read()
        used = C.c_int(0)
        _lib.check(lb.iqpt_debug_last_options(pt.handle, C.byref(used)), "iqpt_debug_last_options")
        px, tiles = C.c_uint32(0), C.c_uint32(0)
        _lib.check(lb.iqpt_debug_sky_info(pt.handle, C.byref(px), C.byref(tiles)), "iqpt_debug_sky_info")
        fr = oracle_frame(preset, w, h, cname)
        c = compare(lin, fr.lin)
        assert c["bitexact"] == c["npix"], c
        assert np.array_equal(bgra, fr.bgra)
        assert np.array_equal(pt.read_rng(), fr.states)
        assert pt.rays() == int(fr.rays.sum())
    assert bool(used.value & K_OPT_CAM_AXIS) == axis
    if sky and preset == "cornell" and (w, h) == (64, 40):
        assert px.value > 0                              # open sky beside and below the box: certain misses
