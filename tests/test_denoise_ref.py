"""The denoiser's numpy reference (tests/denoise_ref.py) against the properties the
definitions imply, the entry points' argument checks that need no device, and the quality of the filter on the
CPU oracle's frames."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import iqpt
import oracle
from iqpt import Scene, _lib, make_camera

F = np.float32
NO = dr.NO_PRIM


def guides(h, w, seed=7, ids=None):
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(h, w, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=2, keepdims=True).astype(np.float32)
    nz = np.concatenate([n, rng.random((h, w, 1), dtype=np.float32)], axis=2).astype(np.float32)
    if ids is None:
        ids = rng.integers(0, 3, size=(h, w)).astype(np.uint32)
    return nz, ids


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_zero_levels_is_the_identity():
    rng = np.random.default_rng(1)
    c = rng.random((9, 13, 4), dtype=np.float32)
    c[2, 3] = [np.nan, -0.0, np.inf, 5.0]
    nz, ids = guides(9, 13)
    out, bgra = dr.denoise(c, nz, ids, 0, 5, 1024.0, 2.0)
    assert np.array_equal(bits(out), bits(c))
    assert np.array_equal(bgra, dr.encode_bgra(c))
    assert tuple(bgra[2, 3]) == (255, 0, 0, 255)             # inf saturates, -0 and NaN give 0


@pytest.mark.parametrize("value", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("params", [(3, 5, 1024.0, 2.0), (5, 0, 0.0, 0.0)])
def test_constant_frame_comes_back_exactly(value, params):
    c = np.full((11, 19, 4), value, np.float32)
    c[..., 3] = 0
    nz, ids = guides(11, 19, ids=np.zeros((11, 19), np.uint32))
    out, _ = dr.denoise(c, nz, ids, *params)
    assert np.array_equal(bits(out), bits(c))


def test_nothing_leaks_across_ids():
    ids = np.zeros((12, 20), np.uint32)
    ids[:, 9:] = 4
    c = np.zeros((12, 20, 4), np.float32)
    c[:, 9:, :3] = 1.0
    nz, _ = guides(12, 20)
    nz[..., :3] = [0, 0, 1]
    out, _ = dr.denoise(c, nz, ids, 4, 0, 0.0, 0.0)           # every weight but the id test switched off
    assert np.array_equal(bits(out), bits(c))


def test_nan_pixel_keeps_its_bits_and_is_a_removed_tap():
    rng = np.random.default_rng(3)
    c = rng.random((9, 9, 4), dtype=np.float32)
    nz, ids = guides(9, 9, ids=np.zeros((9, 9), np.uint32))
    bad = c.copy()
    bad[4, 4] = [0.25, np.nan, 0.5, 7.0]
    args = (0, 2, 16.0, 1.5)
    got = dr.level(bad, nz, ids, *args)
    assert np.array_equal(bits(got[4, 4]), bits(bad[4, 4]))
    want = dr.level(c, nz, ids, *args, skip_tap=(4, 4))       # the clean frame with that tap treated as out of frame
    mask = np.ones((9, 9), bool)
    mask[4, 4] = False
    assert np.array_equal(bits(got)[mask], bits(want)[mask])
    assert not np.array_equal(bits(got)[mask], bits(dr.level(c, nz, ids, *args))[mask])


def test_no_prim_pixels_are_unchanged():
    rng = np.random.default_rng(5)
    c = rng.random((10, 14, 4), dtype=np.float32)
    nz, ids = guides(10, 14)
    ids[rng.random((10, 14)) < 0.4] = NO
    out, _ = dr.denoise(c, nz, ids, 3, 5, 1024.0, 2.0)
    assert np.array_equal(bits(out)[ids == NO], bits(c)[ids == NO])
    assert not np.array_equal(bits(out)[ids != NO], bits(c)[ids != NO])
    assert np.all(out[ids != NO][:, 3] == 0)


def inside_cube():
    """A camera at the centre of a cube of side 4: every pixel sees a face from behind."""
    sc = Scene()
    sc.add_mesh_cube("box")
    sc.add_model("room", "box", scale=4.0)
    cam = make_camera(48, 27, position=[0.0, 0.0, 0.0, 0.0], forward=[0.3, -0.2, 1.0, 0.0])
    return sc, cam


def test_guides_are_two_sided():
    import raster_ref as rr
    sc, cam = inside_cube()
    nz, ids = dr.gbuffer_scene(sc.draw_list(), cam, 48, 27)
    assert np.all(ids == 0) and np.all(nz[..., 3] < 1.0)
    lens = np.linalg.norm(nz[..., :3].astype(np.float64), axis=2)
    assert np.allclose(lens, 1.0, atol=1e-6)
    _, _, prim = rr.render_scene(sc.draw_list(), cam, 48, 27, 1)
    assert np.all(prim == NO)                                  # CULL_BACK alone sees nothing from inside


def test_argument_checks():
    lib = _lib.load()
    h = C.c_void_p()
    for w, hh in ((0, 4), (4, 0), (8193, 4), (4, 8193)):
        assert lib.iqpt_denoise_create(0, w, hh, C.byref(h)) == 1 and not h.value     # IQPT_ERR_INVALID_ARG
    assert lib.iqpt_denoise_create(0, 4, 4, None) == 1
    good = _lib.DenoiseParams(3, 5, 1024.0, 2.0)
    for bad in (_lib.DenoiseParams(9, 5, 1.0, 1.0), _lib.DenoiseParams(3, 8, 1.0, 1.0),
                _lib.DenoiseParams(3, 5, -1.0, 1.0), _lib.DenoiseParams(3, 5, 1.0, float("nan"))):
        assert lib.iqpt_denoise_set_params(None, C.byref(bad)) == 1
        assert b"must be" in lib.iqpt_last_error()
    assert lib.iqpt_denoise_set_params(None, C.byref(good)) == 1 and b"NULL" in lib.iqpt_last_error()
    assert lib.iqpt_denoise_set_params(None, None) == 1
    for call in (lambda: lib.iqpt_denoise_set_guides(None, None, None), lambda: lib.iqpt_denoise_run(None, None),
                 lambda: lib.iqpt_denoise_run_device(None, None), lambda: lib.iqpt_denoise_frame(None, None, None),
                 lambda: lib.iqpt_denoise_read(None, None, None), lambda: lib.iqpt_denoise_sync(None),
                 lambda: lib.iqpt_denoise_copy_frame_device(None, None, 0),
                 lambda: lib.iqpt_denoise_time(None, None, None, None),
                 lambda: lib.iqpt_raster_gbuffer(None), lambda: lib.iqpt_raster_read_gbuffer(None, None, None),
                 lambda: lib.iqpt_raster_gbuffer_device(None, None, None)):
        assert call() == 1
    assert lib.iqpt_denoise_destroy(None) == 0
    for bad in ((9, 5, 1.0, 1.0), (3, 8, 1.0, 1.0), (3, 5, -1.0, 1.0)):
        with pytest.raises(ValueError):
            dr.check_params(*bad)


# r measured with this reference (DESIGN.md §10 "Quality"); the test asks for half of that gain
R_MEASURED = 0.3815     # raw RMSE 0.0937, denoised 0.0357


def test_quality_on_the_oracle_frames():
    """cornell_lit, 96x54, depth 8, seed 1984: RMSE over xyz against the oracle's 2048-spp frame, the 4-spp frame
    filtered with L = 3, q = 5, s_z = 1024, s_c = 2 over the raw 4-spp frame."""
    w, h = 96, 54
    sc = Scene()
    sc.add_preset("cornell_lit")
    pk = sc.build_packet()
    cam = make_camera(w, h)
    fr = oracle.OracleFrame(w, h, max_depth=8, seed=1984)
    fr.render(pk, cam, 4)
    noisy = fr.lin.copy().reshape(h, w, 4)
    fr.render(pk, cam, 2044)
    ref = fr.lin.reshape(h, w, 4)[..., :3].astype(np.float64)
    nz, ids = dr.gbuffer_scene(sc.draw_list(), cam, w, h)
    out, _ = dr.denoise(noisy, nz, ids, 3, 5, 1024.0, 2.0)

    def rmse(a):
        return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref) ** 2)))

    raw, den = rmse(noisy), rmse(out)
    r = den / raw
    print(f"raw RMSE {raw:.4f} denoised {den:.4f} r = {r:.4f} guided pixels {np.mean(ids != NO):.3f}")
    assert r <= (1 + R_MEASURED) / 2


# the edge figure under the two camera pairings, measured with tests/edge_quality.py
EDGE_ONE_CAMERA, EDGE_ALIGNED = 0.08503, 0.07449


def test_edge_quality_with_the_aligned_camera():
    """The frames of the test above with the path tracer under the aligned camera, its own 2048-spp frame as the
    truth, RMSE over the pixels within one pixel of an id edge (14.5 % of the frame): at most the midpoint of the two
    measured figures, the form of the assertion above. Over the whole frame 0.0357 becomes 0.0319."""
    import edge_quality as eq
    fig = eq.denoise_figures(iqpt.align_camera)
    print(eq.show("denoise, aligned", fig))
    assert fig["out_edge"] <= (EDGE_ONE_CAMERA + EDGE_ALIGNED) / 2
