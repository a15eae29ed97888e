"""Variance-guided filtering's numpy reference (tests/svgf_ref.py) against the properties the
definition implies, the entry points' argument checks that need no device, and the quality of the filter on the CPU
oracle's frames."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as dr
import iqpt
import oracle
import svgf_ref as sr
import temporal_ref as tr
from iqpt import Scene, _lib, make_camera

F = np.float32
NO = sr.NO_PRIM
TEMPORAL = (0.9, 0.01, 256)
INVALID, NOT_READY = 1, 5
W0, H0 = 12, 7
PIX = (3, 5)


def params(min_history=4, levels=3, sigma=4.0, floor=1e-6):
    return TEMPORAL + (min_history, levels, 5, 1024.0, sigma, floor)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def flat_planes(h=H0, w=W0, z=0.998, normal=(0.0, 0.0, -1.0), ident=3):
    nz = np.empty((h, w, 4), np.float32)
    nz[..., :3] = np.array(normal, np.float32)
    nz[..., 3] = F(z)
    return nz, np.full((h, w), ident, np.uint32)


def colours(h=H0, w=W0, seed=1):
    c = np.random.default_rng(seed).random((h, w, 4), dtype=np.float32)
    c[..., 3] = 0
    return c


def finite_nonnegative(s):
    for k, c in enumerate(s.stages):
        v = c[..., 3]
        assert np.all(np.isfinite(v)) and np.all(v >= 0) and not np.any(np.signbit(v)), f"stage {k}"


def test_stage_one_is_the_temporal_reference():
    """Over a sequence with a camera move, a speckled id plane and several resolves per view, the colour stage is
    temporal_ref.Temporal's out, bit for bit, and so are its counts."""
    cams = [make_camera(W0, H0), make_camera(W0, H0, position=[0.0, 0.8, -4.8, 0.0], forward=[0.0, -0.5, 3.0, 0.0]),
            make_camera(W0, H0)]
    s = sr.Svgf(W0, H0, *params(min_history=1))
    t = tr.Temporal(W0, H0, *TEMPORAL)
    for k, cam in enumerate(cams):
        nz, ids = flat_planes()
        ids[k, 2 * k] = NO
        s.begin_view(cam, nz, ids)
        t.begin_view(cam, nz, ids)
        for n in (0, 1, 3):
            c = colours(seed=10 * k + n)
            c[1, 1] = [np.nan, 0.5, 0.25, 9.0]
            s.resolve(c, n)
            want, _ = t.resolve(c, n)
            assert np.array_equal(bits(s.temporal_out), bits(want)), (k, n)
            assert np.array_equal(bits(s.c0[..., :3]), bits(want[..., :3]))
            assert s.stats()[:2] == t.stats()
            finite_nonnegative(s)


@pytest.mark.parametrize("grey", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("min_history", [1, 4])
def test_constant_frames_come_back_exactly(grey, min_history):
    cam = make_camera(W0, H0)
    nz, ids = flat_planes()
    c = np.full((H0, W0, 4), grey, np.float32)
    c[..., 3] = 0
    s = sr.Svgf(W0, H0, *params(min_history=min_history, levels=4))
    for _ in range(3):
        s.begin_view(cam, nz, ids)
        out, bgra = s.resolve(c, 1)
        assert np.array_equal(bits(out[..., :3]), bits(c[..., :3]))
        for stage in s.stages:
            assert not bits(stage[..., 3]).any()               # v == +0 at every level
        assert np.array_equal(bgra, dr.encode_bgra(c))


def test_levels_zero_returns_the_variance_plane():
    cam = make_camera(W0, H0)
    nz, ids = flat_planes()
    s = sr.Svgf(W0, H0, *params(levels=0))
    s.begin_view(cam, nz, ids)
    out, bgra = s.resolve(colours(), 2)
    assert np.array_equal(bits(out), bits(s.c0)) and len(s.stages) == 1
    assert np.array_equal(bgra, dr.encode_bgra(s.c0)) and np.any(s.c0[..., 3] > 0)


def test_which_estimate_runs():
    """A first view has no history: every guided pixel with a finite colour takes the spatial estimate, and the
    counter says so. With min_history = 1 or 2 a second view takes the temporal one; with 4 it does not. The moments'
    w counts the current view's samples too, so min_history = 1 is met by a first view already (its estimate is the
    spread of one sample, +0): the degenerate end of the range."""
    cam = make_camera(W0, H0)
    nz, ids = flat_planes()
    ids[0, 0] = NO
    everyone = W0 * H0 - 1
    for min_history, first, second, preview in ((1, 0, 0, 0), (2, everyone, 0, everyone), (4, everyone, everyone, everyone)):
        s = sr.Svgf(W0, H0, *params(min_history=min_history))
        s.begin_view(cam, nz, ids)
        assert s.stats() == (everyone, 0, 0)                      # no resolve yet
        s.resolve(colours(seed=1), 1)
        assert s.stats() == (everyone, 0, first)
        if first:
            assert np.array_equal(s.spatial, ids != NO)
        s.begin_view(cam, nz, ids)
        s.resolve(colours(seed=2), 1)
        assert s.stats() == (everyone, everyone, second)
        # the preview (n = 0) counts views of one sample against the history alone, which holds one
        s.resolve(colours(seed=2), 0)
        assert s.stats()[2] == preview
    # samples, not views: a history of one 8-sample view is not min_history = 2 views of the current 8 samples,
    # but it is two views' worth of 4
    s = sr.Svgf(W0, H0, *params(min_history=2))
    s.begin_view(cam, nz, ids)
    s.resolve(colours(seed=1), 8)
    s.begin_view(cam, nz, ids)
    s.resolve(colours(seed=2), 8)
    assert s.stats()[2] == 0                                      # 8 + 8 >= 2 * 8
    s.resolve(colours(seed=2), 16)
    assert s.stats()[2] == W0 * H0 - 1                            # 8 + 16 < 2 * 16


def test_two_grey_levels_give_the_formulas_variance():
    """Two views of constant grey a then b, one sample each, min_history = 1: the temporal estimate, step by step in
    float32. And a first view of two grey halves: the spatial estimate of a pixel whose window spans both."""
    a, b = F(0.25), F(0.75)
    cam = make_camera(W0, H0)
    nz, ids = flat_planes()
    s = sr.Svgf(W0, H0, *params(min_history=1, levels=0))
    for g in (a, b):
        c = np.full((H0, W0, 4), g, np.float32)
        s.begin_view(cam, nz, ids)
        out, _ = s.resolve(c, 1)
    la, lb = [F(F(F(0.2126) * g + F(0.7152) * g) + F(0.0722) * g) for g in (a, b)]
    m1 = F(F(F(la * F(1)) + F(lb * F(1))) / F(2))
    m2 = F(F(F(F(la * la) * F(1)) + F(F(lb * lb) * F(1))) / F(2))
    want = F(F(m2 - F(m1 * m1)) * F(F(1) / F(2)))                 # ne / o.w = 1 / 2: the variance of the two-sample mean
    assert want > 0 and abs(float(want) - 0.03125) < 1e-6           # ((b - a) / 2)^2 / 2 for these values
    assert np.all(bits(out[..., 3]) == bits(want))
    assert np.array_equal(bits(s.mu[..., 0]), np.full((H0, W0), bits(m1))) and s.stats()[2] == 0
    # spatial: columns 0..5 grey a, 6..11 grey b, one view
    c = np.full((H0, W0, 4), a, np.float32)
    c[:, 6:] = b
    s = sr.Svgf(W0, H0, *params(levels=0))
    s.begin_view(cam, nz, ids)
    out, _ = s.resolve(c, 1)
    y, x = 3, 5                                                   # window columns 2..8 and rows 0..6: 28 taps of a, 21 of b
    s1 = s2 = F(0)
    for _dy in range(7):
        for dx in range(7):
            lum = la if x - 3 + dx < 6 else lb
            s1 = F(s1 + lum)
            s2 = F(s2 + F(lum * lum))
    mean = F(s1 / F(49))
    want = F(F(s2 / F(49)) - F(mean * mean))
    assert bits(out[y, x, 3]) == bits(want) and want > 0
    assert out[3, 1, 3] == 0 and out[0, 0, 3] == 0                # windows of one grey, clipped at the corner too


@pytest.mark.parametrize("bad", [[np.nan, 0.5, 0.25], [0.5, np.inf, 0.5], [-np.inf, 0.1, 0.2]])
@pytest.mark.parametrize("min_history", [1, 4])
def test_non_finite_colour_is_a_removed_tap(bad, min_history):
    """A NaN or an inf colour. In a second view the pixel falls back on both histories (case B), so it stays an
    ordinary finite pixel and neither history takes the colour in. In a first view it has nothing to fall back on:
    it passes through with v = +0, counts no sample, and every other pixel equals the result with that tap removed
    from every window."""
    cam = make_camera(W0, H0)
    nz, ids = flat_planes()
    c2 = colours(seed=2)
    c2[PIX][:3] = bad
    s = sr.Svgf(W0, H0, *params(min_history=min_history))
    s.begin_view(cam, nz, ids)
    s.resolve(colours(seed=1), 1)
    before = s.temporal_out[PIX].copy(), s.mu[PIX].copy()
    s.begin_view(cam, nz, ids)
    s.resolve(c2, 1)
    finite_nonnegative(s)
    assert np.all(np.isfinite(s.mu)) and np.all(np.isfinite(s.temporal_out))
    assert np.array_equal(bits(s.temporal_out[PIX]), bits(before[0])) and np.array_equal(bits(s.mu[PIX]), bits(before[1]))
    others = np.ones((H0, W0), bool)
    others[PIX] = False
    first = []
    for skip in (None, PIX):
        s.clear()
        s.begin_view(cam, nz, ids)
        out, _ = s.resolve(c2, 1, skip_tap=skip)
        finite_nonnegative(s)
        assert np.array_equal(bits(out[PIX][:3]), bits(c2[PIX][:3])) and bits(out[PIX][3]) == 0
        assert s.moments.out[PIX][3] == 0 and s.colour.out[PIX][3] == 0      # case C: no sample counted
        first.append(out.copy())
        nxt = s.colour.begin_view(cam, nz, ids), s.moments.begin_view(cam, nz, ids)
        assert np.all(np.isfinite(nxt[0])) and np.all(np.isfinite(nxt[1])) and not bits(nxt[1][PIX]).any()
    assert np.array_equal(bits(first[0][others]), bits(first[1][others]))


def test_luminance_overflow_never_reaches_a_variance():
    """A finite colour whose L L overflows: the colour history takes it (it is finite), the moments history skips
    that view as §11's case B does, and no variance and no history is non-finite, under either estimate. The
    pixel is still a tap of its neighbours' 7x7 windows (the tap rule asks for a finite colour only): their sums
    overflow and their estimate is the replaced +0, so the removed-tap equality of the non-finite colours does not
    hold here and is not asserted."""
    cam = make_camera(W0, H0)
    nz, ids = flat_planes()
    c2 = colours(seed=2)
    c2[PIX][:3] = [3e19, 3e19, 3e19]
    assert np.isfinite(sr.luminance(c2)[PIX]) and np.isinf(sr.moments(c2)[PIX][1])
    for min_history in (1, 4):
        s = sr.Svgf(W0, H0, *params(min_history=min_history))
        s.begin_view(cam, nz, ids)
        s.resolve(colours(seed=1), 1)
        hist_before = s.moments.out[PIX].copy()
        s.begin_view(cam, nz, ids)
        s.resolve(c2, 1)
        finite_nonnegative(s)
        assert np.all(np.isfinite(s.mu)) and np.array_equal(bits(s.mu[PIX]), bits(hist_before))   # case B
        assert s.temporal_out[PIX][3] == 2 and np.all(np.isfinite(s.temporal_out))
        nxt = s.moments.begin_view(cam, nz, ids)
        assert np.all(np.isfinite(nxt)) and nxt[PIX][3] == 1
    # on a first view the moments pixel is case C with w = +0 and a non-finite second moment: still no such variance
    s = sr.Svgf(W0, H0, *params())
    s.begin_view(cam, nz, ids)
    s.resolve(c2, 1)
    finite_nonnegative(s)
    assert np.isinf(s.mu[PIX][1]) and s.mu[PIX][3] == 0
    assert not bits(s.moments.begin_view(cam, nz, ids)[PIX]).any()


def test_nothing_leaks_across_ids():
    """Two models side by side, one black and one white with a noisy pixel each: no colour and no variance crosses."""
    cam = make_camera(W0, H0)
    nz, ids = flat_planes()
    ids[:, 6:] = 4
    c = np.zeros((H0, W0, 4), np.float32)
    c[:, 6:, :3] = 1.0
    for min_history in (1, 4):
        s = sr.Svgf(W0, H0, *params(min_history=min_history, levels=4, sigma=0.0))
        for _ in range(2):
            s.begin_view(cam, nz, ids)
            out, _ = s.resolve(c, 1)
        assert np.array_equal(bits(out[..., :3]), bits(c[..., :3])) and not bits(out[..., 3]).any()
    # a noisy right half leaves the left half's variance at +0 and its colour alone
    c2 = c.copy()
    c2[:, 6:, :3] = np.random.default_rng(4).random((H0, W0 - 6, 3), dtype=np.float32)
    s = sr.Svgf(W0, H0, *params(levels=4, sigma=0.0))
    s.begin_view(cam, nz, ids)
    out, _ = s.resolve(c2, 1)
    assert not bits(out[:, :6]).any() and np.all(out[:, 6:, 3] > 0)
    finite_nonnegative(s)


def test_no_prim_pixels_keep_all_four_components():
    cam = make_camera(W0, H0)
    nz, ids = flat_planes()
    ids[2:4, 3:9] = NO
    s = sr.Svgf(W0, H0, *params(min_history=1, levels=4))
    for k in range(2):
        c = colours(seed=k)
        s.begin_view(cam, nz, ids)
        out, _ = s.resolve(c, 1)
        sky = ids == NO
        assert np.array_equal(bits(out[sky][:, :3]), bits(c[sky][:, :3])) and not bits(out[sky][:, 3]).any()
        for a, b in zip(s.stages, s.stages[1:]):
            assert np.array_equal(bits(a[sky]), bits(b[sky]))
        # a pass-through pixel carries whatever fourth component it has through a level, bit for bit
        odd = s.c0.copy()
        odd[sky, 3] = F(7.5)
        assert np.array_equal(bits(sr.level(odd, nz, ids, 0, 5, 1024.0, 4.0, 1e-6)[sky]), bits(odd[sky]))
        finite_nonnegative(s)


def test_variance_is_finite_and_non_negative_on_hostile_input():
    rng = np.random.default_rng(11)
    h, w = 17, 13
    cam = make_camera(w, h)
    special = np.array([0.0, -0.0, 1e-40, -3e-42, np.nan, np.inf, -np.inf, 1.5, 37.0, 1e-38, 3e19, -3e19], np.float32)
    for min_history in (1, 4):
        s = sr.Svgf(w, h, *params(min_history=min_history, levels=5))
        for k in range(3):
            nz, ids = flat_planes(h, w)
            ids[rng.random((h, w)) < 0.2] = 5
            ids[rng.random((h, w)) < 0.1] = NO
            c = rng.random((h, w, 4), dtype=np.float32)
            pick = rng.random((h, w, 4)) < 0.1
            c[pick] = rng.choice(special, size=int(pick.sum()))
            s.begin_view(cam, nz, ids)
            for n in (0, 1, 1 << 24):
                s.resolve(c, n)
                finite_nonnegative(s)
                # a second moment can overflow in §11's blend (4e37 times a history length): the temporal estimate
                # refuses a non-finite moment and the next view's gather refuses it as a history, so no NaN arises
                for t in (s.colour, s.moments):
                    assert np.all(np.isfinite(t.hist)) and not np.any(np.isnan(t.out[t.out[..., 3] > 0]))


# ------------------------------------------------------------------------------------------------ the library
def test_header_is_the_signature_table():
    text = (Path(__file__).resolve().parent.parent / "include" / "svgf" / "iqpt_svgf.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(iqpt_[a-z0-9_]+)\s*\(", text))
    lib = iqpt.load()
    assert len(names) == 17
    for n in names:
        assert hasattr(lib, n), n
    assert names == {s[0] for s in _lib.SVGF_SIGNATURES}
    assert lib.iqpt_abi_version() == 6                      # additions only
    assert iqpt.Svgf is iqpt.svgf.Svgf


def test_argument_checks():
    lib = _lib.load()
    h = C.c_void_p()
    for w, hh in ((0, 4), (4, 0), (8193, 4), (4, 8193)):
        assert lib.iqpt_svgf_create(0, w, hh, C.byref(h)) == INVALID and not h.value
    assert lib.iqpt_svgf_create(0, 4, 4, None) == INVALID
    good = (0.9, 0.01, 256, 4, 4, 5, 1024.0, 4.0, 1e-6)
    nan, inf, big = float("nan"), float("inf"), (1 << 24) + 1
    bad_values = {0: (nan, inf), 1: (-0.5, nan), 2: (0, big), 3: (0, big), 4: (9,), 5: (8,), 6: (-1.0, nan, inf),
                  7: (-1.0, nan, inf), 8: (0.0, -1.0, nan, inf)}
    for field, values in bad_values.items():
        for v in values:
            args = list(good)
            args[field] = v
            assert lib.iqpt_svgf_set_params(None, C.byref(_lib.SvgfParams(*args))) == INVALID, (field, v)
            assert b"must be" in lib.iqpt_last_error()
            with pytest.raises(ValueError):
                sr.check_params(*args)
    assert lib.iqpt_svgf_set_params(None, C.byref(_lib.SvgfParams(*good))) == INVALID and b"NULL" in lib.iqpt_last_error()
    assert lib.iqpt_svgf_set_params(None, None) == INVALID
    sr.check_params(*good)
    for edge in ((0.9, 0.0, 1, 1, 0, 0, 0.0, 0.0, 1e-30), (-1.0, 1e9, 1 << 24, 1 << 24, 8, 7, 1e30, 1e9, 1e30)):
        sr.check_params(*edge)
        assert lib.iqpt_svgf_set_params(None, C.byref(_lib.SvgfParams(*edge))) == INVALID and b"NULL" in lib.iqpt_last_error()
    for call in (lambda: lib.iqpt_svgf_default_params(None), lambda: lib.iqpt_svgf_begin_view(None, None, None, None),
                 lambda: lib.iqpt_svgf_begin_view_device(None, None, None, None),
                 lambda: lib.iqpt_svgf_begin_view_raster(None, None), lambda: lib.iqpt_svgf_clear(None),
                 lambda: lib.iqpt_svgf_resolve(None, None, 1), lambda: lib.iqpt_svgf_resolve_device(None, None, 1),
                 lambda: lib.iqpt_svgf_resolve_ctx(None, None), lambda: lib.iqpt_svgf_read(None, None, None),
                 lambda: lib.iqpt_svgf_read_stages(None, None, None),
                 lambda: lib.iqpt_svgf_copy_frame_device(None, None, 0), lambda: lib.iqpt_svgf_sync(None),
                 lambda: lib.iqpt_svgf_time(None, None, None, None, None, None, None),
                 lambda: lib.iqpt_svgf_stats(None, None, None, None)):
        assert call() == INVALID
    assert lib.iqpt_svgf_destroy(None) == 0
    p = _lib.SvgfParams()
    assert lib.iqpt_svgf_default_params(C.byref(p)) == 0
    sr.check_params(*[getattr(p, name) for name, _ in _lib.SvgfParams._fields_])
    assert iqpt.svgf.default_params()["min_history"] == p.min_history
    s = sr.Svgf(W0, H0, *good)
    with pytest.raises(RuntimeError):
        s.resolve(colours(), 1)


# ------------------------------------------------------------------------------------------------ quality
# measured with this reference and the library's defaults (DESIGN.md §12.4 "Quality"): (a) raw 0.2309, (b) temporal
# 0.0954, (c) temporal through the fixed default filter 0.0531, (d) this feature 0.0489
RATIO_MEASURED = 0.5126     # d / b


@functools.lru_cache(maxsize=None)
def quality_figures():
    """§11.4's setup: cornell_lit, 96x54, depth 8, seed 1984, one OracleFrame with reset() between 8 views of 1 spp,
    view k at (0.05 k, 0.5, -3) looking along (-0.02 k, -0.5, 3), against a 1024-spp frame of the last view from
    another seed; RMSE over xyz of the guided pixels. Svgf runs the library's default filter parameters, the fixed
    filter its own; the histories run 0.9 / 0.01 / 256. The static frames are one view of the last camera, 1 and 16
    samples of a third seed, through a first view (no history) and through the fixed filter."""
    w, h, views = 96, 54, 8
    sc = Scene()
    sc.add_preset("cornell_lit")
    pk = sc.build_packet()
    items = sc.draw_list()
    fr = oracle.OracleFrame(w, h, max_depth=8, seed=1984)
    p = iqpt.svgf.default_params()
    svgf_args = (0.9, 0.01, 256, p["min_history"], p["levels"], p["normal_squarings"], p["depth_sharpness"],
                 p["colour_sigma"], p["variance_floor"])
    s = sr.Svgf(w, h, *svgf_args)
    for k in range(views):
        cam = make_camera(w, h, position=[0.05 * k, 0.5, -3.0, 0.0], forward=[-0.02 * k, -0.5, 3.0, 0.0])
        nz, ids = dr.gbuffer_scene(items, cam, w, h)
        fr.reset()
        fr.render(pk, cam, 1)
        s.begin_view(cam, nz, ids)
        out, _ = s.resolve(fr.lin, 1)
    raw = fr.lin.copy().reshape(h, w, 4)
    guided = ids != NO
    truth = oracle.OracleFrame(w, h, max_depth=8, seed=77)
    truth.render(pk, cam, 1024)
    ref = truth.lin.reshape(h, w, 4)[..., :3].astype(np.float64)

    def rmse(a):
        return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref)[guided] ** 2)))

    d = iqpt.denoise.default_params()
    fixed = (d["levels"], d["normal_squarings"], d["depth_sharpness"], d["colour_sharpness"])
    fig = {"a": rmse(raw), "b": rmse(s.temporal_out), "c": rmse(dr.denoise(s.temporal_out, nz, ids, *fixed)[0]),
           "d": rmse(out), "spatial_share": s.stats()[2] / s.stats()[0]}
    one = oracle.OracleFrame(w, h, max_depth=8, seed=5)
    for spp, more in ((1, 1), (16, 15)):
        one.render(pk, cam, more)
        lin = one.lin.copy().reshape(h, w, 4)
        v = sr.Svgf(w, h, *svgf_args)
        v.begin_view(cam, nz, ids)
        fig[f"raw{spp}"], fig[f"fixed{spp}"] = rmse(lin), rmse(dr.denoise(lin, nz, ids, *fixed)[0])
        fig[f"svgf{spp}"] = rmse(v.resolve(lin, spp)[0])
    print(" ".join(f"{k} {v:.4f}" for k, v in fig.items()))
    return fig


def test_quality_on_the_oracle_frames():
    """Half of the measured gain over the temporal result, the margin of §10.4 and §11.4 (the run is deterministic,
    so it only guards against later edits of the reference), and the order against the fixed filter on the same
    temporal result: (d) 0.0489 against (c) 0.0531, a gap of 7.9 % of the larger figure.

    The two static-view orders are not asserted: on one first view of 1 sample the feature comes out at 0.0610
    against the fixed default's 0.0624 (raw 0.2400), at 16 samples at 0.0484 against 0.0485 (raw 0.0597), gaps of
    2.2 % and 0.2 %, under the 5 % an order needs to be asserted."""
    fig = quality_figures()
    assert fig["d"] / fig["b"] <= (1 + RATIO_MEASURED) / 2
    assert fig["d"] <= fig["c"]
    assert fig["b"] < fig["a"] and fig["svgf1"] < fig["raw1"] and fig["svgf16"] < fig["raw16"]


# the edge figure under the two camera pairings, measured with tests/edge_quality.py
EDGE_ONE_CAMERA, EDGE_ALIGNED = 0.10151, 0.08793


def test_edge_quality_with_the_aligned_camera():
    """The eight views of the test above with the path tracer under the aligned camera of each view, its own 1024-spp
    frame as the truth, RMSE of the filtered result over the guided pixels within one pixel of an id edge (11.2 % of
    the frame): at most the midpoint of the two measured figures. Over all guided pixels 0.0489 becomes 0.0435. The
    temporal result of the same run does not move at the edges, 0.1282 under both pairings: it blends
    along time only, so it gets no assertion."""
    import edge_quality as eq
    temporal, svgf = eq.history_figures(iqpt.align_camera)
    print(eq.show("temporal, aligned", temporal))
    print(eq.show("svgf, aligned", svgf))
    assert svgf["out_edge"] <= (EDGE_ONE_CAMERA + EDGE_ALIGNED) / 2
