"""The camera-ray proofs on the device, on seeded random geometry.

(a) Every mask the proof kernels write — iqpt_bin_kernel's tile masks, iqpt_certain_kernel's certain-hit and
certain-miss masks, the candidate lists with their offsets, iqpt_pixel_mask_kernel's per-pixel words — equals, word
for word, what the host build of csrc/iq_interval.h computes from the primitives the device arrays hold
(tests/proof_masks.py; the any-hit certain bit, which the kernel computes for a subset of a pixel's triangles, is
checked for soundness). tests/test_cull.py and tests/test_certain.py check the host build against the oracle's
intersection routines, ray by ray.

(b) Every random scene, rendered in launches of 1 and 3 samples, equals the oracle bit for bit: accumulator, BGRA8,
XORWOW states and ray counts. Four scene families with placements built from the camera's own corner rays (a shared
edge through pixel corners, a vertex on and a sphere tangent to a tile-corner ray, the camera inside a sphere, a
sphere behind the camera, triangles straddling t_min, at t ~ 999.99, edge-on, covering the frame, of zero area),
five cameras (the default, pitched and yawed, 5 and 120 degree fields of view, 1e4 units from the origin), three
frames (40 x 24, a ragged 37 x 19, a ragged row share with ystep 2), depths 2 and 8. One context and one oracle
frame serve a case's ten scenes (two seeds per camera), so the masks are rebuilt for each and the pixel state runs on.
Every case runs twice: on the five cameras and on the aligned form of each (iqpt_camera_align), with
scenes of their own and the same coverage asked of both.

The coverage each family must produce is asserted from the read-back masks over a case's scenes together."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import compare
from iqpt import PathTracer, _lib, pixel_set
from proof_masks import N_PLAIN, cameras, check_masks, random_scene, read_proofs

pytestmark = pytest.mark.gpu

FAMILIES = ["resident", "tris", "tris_spheres", "materials"]
# name: (width, height, pixel_set arguments after (w, h) or None, max_depth)
FRAMES = {
    "40x24": (40, 24, None, 8),
    "37x19": (37, 19, None, 2),
    "rows": (40, 48, (3, 40, 1, 2, 23), 8),          # columns 3..39 of rows 1, 3, .., 45: 37 x 23 owned pixels
}
LAUNCHES = [1, 3]
REPS = 2                     # scenes per camera and case: 10 scenes share a context
GROUPS = (0, 1)              # proof_masks.cameras: the five cameras, their aligned forms


def seed_of(family, frame, k, rep=0, group=0):
    return 1000 * FAMILIES.index(family) + 100 * list(FRAMES).index(frame) + 10 * rep + k + N_PLAIN * group


def last_options(pt):
    lb = _lib.load()
    lb.iqpt_debug_last_options.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    o = C.c_int(0)
    _lib.check(lb.iqpt_debug_last_options(pt._h, C.byref(o)), "iqpt_debug_last_options")
    return o.value


def pixel_mask_info(pt):
    lb = _lib.load()
    lb.iqpt_debug_pixel_mask_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int),
                                              C.POINTER(C.c_uint32)]
    n, every = C.c_uint32(0), C.c_int(0)
    _lib.check(lb.iqpt_debug_pixel_mask_info(pt._h, C.byref(n), C.byref(every), None), "iqpt_debug_pixel_mask_info")
    return n.value, bool(every.value)


def run_case(family, frame, mode=2, group=0):
    w, h, psargs, depth = FRAMES[frame]
    ps = pixel_set(w, h, *psargs) if psargs else pixel_set(w, h)
    mats = family == "materials"
    pt = PathTracer(w, h, pixels=ps, max_depth=depth)
    lb = _lib.load()
    lb.iqpt_debug_set_pixel_masks.argtypes = [C.c_void_p, C.c_int]
    _lib.check(lb.iqpt_debug_set_pixel_masks(pt._h, mode), "iqpt_debug_set_pixel_masks")
    fr = oracle.OracleFrame(w, h, pixels=ps, max_depth=depth)
    tot = dict(hit=0, miss=0, mixed_tiles=0, cleared_tiles=0, pm_tiles=0, anyhit=0, certain_scenes=0, list_scenes=0)
    cams = cameras(w, h)[N_PLAIN * group:N_PLAIN * (group + 1)]
    for rep, (k, (cname, cam)) in ((r, kc) for r in range(REPS) for kc in enumerate(cams)):
        sc = random_scene(family, seed_of(family, frame, k, rep, group), k, cam, ps)
        pk = sc.build_packet()
        pt.set_camera(cam)
        pt.upload_packet(pk)
        for i, s in enumerate(LAUNCHES):
            pt.render(s)
            fr.render(pk, cam, s)
            anyk = bool(last_options(pt) & (1 << 29))
            if i == 0:
                # (a) the masks of this scene and camera, after the first launch
                dev = read_proofs(pt)
                cov = check_masks(cam, ps, dev, mats, mode)
                for key in ("hit", "miss", "mixed_tiles", "cleared_tiles", "pm_tiles"):
                    tot[key] += cov[key]
                tot["certain_scenes"] += dev["have_certain"]
                tot["list_scenes"] += dev["have_lists"]
                ntiles, every = pixel_mask_info(pt)
                assert ntiles == cov["pm_tiles"]
                if dev["have_pmask"]:
                    assert every == cov["any_ok"]
            tot["anyhit"] += anyk
        # (b) the frame so far against the oracle
        lin, bgra = pt.read()
        c = compare(lin, fr.lin)
        assert c["bitexact"] == c["npix"], (cname, rep, c)
        assert np.array_equal(bgra, fr.bgra), cname
        assert np.array_equal(pt.read_rng(), fr.states), cname
        assert pt.rays() == int(fr.rays.sum()), cname
        sc.close()
    pt.close()
    return tot


@pytest.mark.parametrize("frame", list(FRAMES))
def test_resident_scenes(require_gpu, frame):
    """Tens of random triangles and a few spheres under the reference's materials: the certain-hit fold, the sky
    kernel and the tile masks together."""
    for group in GROUPS:
        tot = run_case("resident", frame, group=group)
        assert tot["certain_scenes"] == 5 * REPS
        assert tot["hit"] > 20 and tot["miss"] > 20 and tot["mixed_tiles"] > 5, tot


@pytest.mark.parametrize("mode", [2, 1])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_triangle_only_scenes(require_gpu, frame, mode):
    """More than 512 triangles and no sphere (cull_stride > 8): the candidate lists, the per-pixel masks and, in
    mode 2 for the streamed scenes (two balls), iqpt_anyhit_kernel. The one-ball scenes are resident and have certain
    masks as well; in frames of 5 x 3 tiles nearly every tile keeps more than the 96 candidate pairs the certain
    proofs take, so those masks are compared but no count of certain pixels is asked of this family."""
    for group in GROUPS:
        tot = run_case("tris", frame, mode, group=group)
        assert tot["list_scenes"] == 5 * REPS and tot["certain_scenes"] == 3 * REPS
        assert tot["pm_tiles"] > 20 and tot["cleared_tiles"] > 20, tot
        assert (tot["anyhit"] > 0) == (mode == 2), tot


@pytest.mark.parametrize("frame", list(FRAMES))
def test_triangle_and_sphere_scenes(require_gpu, frame):
    """More than 512 triangles plus spheres: the plain kernel walks the lists through the per-pixel masks."""
    for group in GROUPS:
        tot = run_case("tris_spheres", frame, group=group)
        assert tot["list_scenes"] == 5 * REPS and tot["anyhit"] == 0
        assert tot["pm_tiles"] > 20 and tot["cleared_tiles"] > 20, tot


@pytest.mark.parametrize("frame", list(FRAMES))
def test_scenes_with_a_material_table(require_gpu, frame):
    """A material table: no certain masks are built; the tile masks are, and the frame is still exact."""
    for group in GROUPS:
        tot = run_case("materials", frame, group=group)
        assert tot["certain_scenes"] == 0 and tot["hit"] == 0 and tot["miss"] == 0
