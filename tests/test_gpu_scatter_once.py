"""One Oren-Nayar scatter per iteration of the two-ray kernel (kOptPipe): ray a's terminal hits fold
first, then a single scatter serves ray a's sphere hits and the promoted ray b's sphere hits together, then the
promoted rays' terminal hits and the scatters that reached max_depth fold. Every case compares accumulator bits,
BGRA8, the six XORWOW words and the ray count with the oracle, and asserts that the launches carried kOptPipe.

The crops must contain the situations the three stages separate. That is checked from the oracle alone, before the
GPU result is looked at: from the oracle's per-sample ray counts (one sample at a time) the case's samples must hold
  * a pixel with a 1-ray sample (the path ends at once: stage 1, promotion or need_a) and a sample of 2 or more rays
    (a scatter) — both lane groups and terminal rays in one wave;
  * a pixel with a sample of 3 or more rays (a scatter after a scatter: ray b is dropped and made again).
A sample traces at most max_depth rays, so at max_depth 1 and 2 the counts are taken at depth 8 for the same pixels
and samples: the scatters are there, the depth limit only ends them in stage 3."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from helpers import scene_for
from iqpt import PathTracer, _lib, make_camera
from iqpt.render import pixel_set

pytestmark = pytest.mark.gpu

K_OPT_PIPE = 1 << 21
K_OPT_OVERLAP = 1 << 19

W, H = 1920, 1080
# where the left sphere faces the right one: 64 x 16 pixels, eight tiles (two- and three-scatter samples, silhouette)
CROP_FACING = (872, 936, 624, 1, 16)
# across the top edge of the right sphere: pixels that always miss, silhouette pixels, and three-ray samples
CROP_EDGE = (1112, 1176, 552, 1, 16)
# a band through both spheres, large enough (>= 64 blocks of 256 pixels) for overlapped launches
CROP_BAND = (720, 1200, 600, 1, 40)


def last_options(pt):
    lb = _lib.load()
    lb.iqpt_debug_last_options.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    o = C.c_int(0)
    _lib.check(lb.iqpt_debug_last_options(pt._h, C.byref(o)), "iqpt_debug_last_options")
    return o.value


def set_two_ray(pt, on):
    lb = _lib.load()
    lb.iqpt_debug_set_two_ray.argtypes = [C.c_void_p, C.c_int]
    _lib.check(lb.iqpt_debug_set_two_ray(pt._h, 1 if on else 0), "iqpt_debug_set_two_ray")


def run(preset, w, h, launches, depth=8, crop=None, two_ray=True, overlap=True):
    _sc, pk = scene_for(preset)
    cam = make_camera(w, h)
    pt = PathTracer(w, h, pixels=pixel_set(w, h, *crop) if crop else None, max_depth=depth)
    pt.set_split(_lib.SPLIT_OFF)
    pt.set_overlap(_lib.OVERLAP_AUTO if overlap else _lib.OVERLAP_OFF)
    set_two_ray(pt, two_ray)
    pt.set_camera(cam)
    pt.upload_packet(pk)
    opts = []
    for s in launches:
        pt.render(s)
        opts.append(last_options(pt))
    pt.sync()
    lin, bgra = pt.read()
    out = (lin, bgra, pt.read_rng(), pt.rays())
    pt.close()
    return out, opts


@functools.lru_cache(maxsize=None)
def oracle_steps(preset, w, h, crop, total, depth):
    """The oracle frame after `total` samples, rendered one sample at a time (consecutive reference launches, so
    the same frame as any grouping into launches), and the rays of every sample and pixel, [total, npix]. Computed
    once per (frame, samples, depth) and shared; the tests do not change it."""
    _sc, pk = scene_for(preset)
    fr = oracle.OracleFrame(w, h, pixels=pixel_set(w, h, *crop) if crop else None, max_depth=depth)
    cam = make_camera(w, h)
    per_sample = np.zeros((total, fr.npix), dtype=np.int64)
    for k in range(total):
        before = fr.rays.copy()
        fr.render(pk, cam, 1)
        per_sample[k] = (fr.rays - before).astype(np.int64)
    per_sample.setflags(write=False)
    return fr, per_sample


def check_inputs(preset, w, h, crop, total, depth, twice=True):
    """The condition on the inputs (module docstring), from the oracle alone."""
    _, c = oracle_steps(preset, w, h, crop, total, depth if depth >= 3 else 8)
    ends_and_scatters = int(((c == 1).any(axis=0) & (c >= 2).any(axis=0)).sum())
    scatters_twice = int((c >= 3).any(axis=0).sum())
    print(f"{preset} {crop} {total} samples depth {depth}: {ends_and_scatters} pixels with a 1-ray and a >= 2-ray "
          f"sample, {scatters_twice} with a >= 3-ray sample")
    assert ends_and_scatters >= 1
    assert scatters_twice >= 1 or not twice


def same_as_oracle(out, fr):
    lin, bgra, rng, rays = out
    a, b = lin[:, :3], fr.lin[:, :3]
    both_nan = np.isnan(a) & np.isnan(b)
    assert np.all((a.view(np.uint32) == b.view(np.uint32)) | both_nan)
    assert np.array_equal(bgra, fr.bgra)
    assert np.array_equal(rng, fr.states)
    assert rays == int(fr.rays.sum())


def same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2])
    assert a[3] == b[3]


def check_case(preset, w, h, launches, depth=8, crop=None, overlap=True, twice=True):
    check_inputs(preset, w, h, crop, sum(launches), depth, twice)
    out, opts = run(preset, w, h, launches, depth=depth, crop=crop, overlap=overlap)
    assert all(o & K_OPT_PIPE for o in opts), [hex(o) for o in opts]
    same_as_oracle(out, oracle_steps(preset, w, h, crop, sum(launches), depth)[0])
    return out, opts


@pytest.mark.parametrize("overlap", [True, False])
def test_both_scatter_groups(require_gpu, overlap):
    """Case 1: the facing crop, launches of 1, 2, 5 and 64 samples. Ray a's own scatters and promoted ray b's in
    one wave, with terminal promoted rays beside them; the 5-sample launch is the short-launch situation."""
    check_case("cornell", W, H, [1, 2, 5, 64], crop=CROP_FACING, overlap=overlap)


def test_overlapped_launches(require_gpu):
    """Beside case 1: its crop is too small for the runtime to overlap launches (fewer than 64 blocks of pixels), so
    a band of 480 x 40 pixels through both spheres takes the same launches with the overlapped variant really
    launched (a tile waits for the previous launch's pixel stores, which either fold now issues)."""
    _, opts = check_case("cornell", W, H, [1, 2, 5, 64], crop=CROP_BAND)
    assert any(o & K_OPT_OVERLAP for o in opts), [hex(o) for o in opts]


def test_silhouette_misses(require_gpu):
    """Case 2: a crop across a sphere's outer edge. Samples that miss: stage 3 without a stage-2 lane, then need_a."""
    check_case("cornell", W, H, [3, 4], crop=CROP_EDGE)


@pytest.mark.parametrize("depth", [1, 2, 3, 16])
def test_depths(require_gpu, depth):
    """Case 3: max_depth 1 ends every promoted scatter in stage 3; 2 ends ray a's second scatter there while other
    lanes promote; 3; 16 (the MAXD-16 variant)."""
    check_case("cornell", W, H, [5, 7], depth=depth, crop=CROP_FACING)


@pytest.mark.parametrize("launches", [[1, 1, 1], [2]])
def test_last_sample_has_no_ray_b(require_gpu, launches):
    """Case 4: has_b is false on a launch's last sample: no promotion, stage 3 empty."""
    check_case("cornell", W, H, launches, crop=CROP_FACING)


@pytest.mark.parametrize("preset,size,depth", [("app_default", (317, 181), 5), ("c1_plumbing", (250, 250), 2)])
def test_ragged_frames(require_gpu, preset, size, depth):
    """Case 5: ragged frames, partial tiles and partial waves. The C1 scene has a single sphere, and
    a ray that leaves a sphere cannot meet the same one again: no path of it scatters twice at any depth (0 pixels
    with a 3-ray sample in the oracle's 250 x 250 x 7 samples at depth 8), so only the first input condition is
    asked of it; the crops and the application scene meet both."""
    check_case(preset, size[0], size[1], [3, 4], depth=depth, twice=preset != "c1_plumbing")


def test_two_ray_equals_one_ray(require_gpu):
    """Case 6: the two-ray output equals the one-ray kernel's (iqpt_debug_set_two_ray 0) and the oracle's, overlap on."""
    on, _ = check_case("cornell", W, H, [64, 16], crop=CROP_FACING)
    off, o0 = run("cornell", W, H, [64, 16], crop=CROP_FACING, two_ray=False)
    assert not any(o & K_OPT_PIPE for o in o0)
    same(on, off)
