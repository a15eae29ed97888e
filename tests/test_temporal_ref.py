"""Temporal reprojection's numpy reference (tests/temporal_ref.py) against the properties the
definition implies, the entry points' argument checks that need no device, and the quality of the history on the
CPU oracle's frames."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as dr
import iqpt
import oracle
import temporal_ref as tr
from iqpt import Scene, _lib, make_camera

F = np.float32
NO = tr.NO_PRIM
PARAMS = (0.9, 0.01, 256)
INVALID, NOT_READY = 1, 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def flat_planes(h, w, z=0.998, normal=(0.0, 0.0, -1.0), ident=3):
    """One surface of constant D32 depth (about 5 units away with the default near and far planes), every pixel
    guided."""
    nz = np.empty((h, w, 4), np.float32)
    nz[..., :3] = np.array(normal, np.float32)
    nz[..., 3] = F(z)
    return nz, np.full((h, w), ident, np.uint32)


def colours(h, w, seed=1):
    c = np.random.default_rng(seed).random((h, w, 4), dtype=np.float32)
    c[..., 3] = 0
    return c


W0, H0 = 12, 7


def two_views(change=None, cam2=None, n1=3, colour1=None, params=PARAMS, change1=None):
    """View 1 of the flat planes (after change1(nz, ids)) resolved with n1 samples, then view 2 (the same camera and
    planes unless cam2 / change(nz, ids) say otherwise). Returns the Temporal after the second begin_view."""
    cam = make_camera(W0, H0)
    nz, ids = flat_planes(H0, W0)
    if change1 is not None:
        change1(nz, ids)
    t = tr.Temporal(W0, H0, *params)
    t.begin_view(cam, nz, ids)
    t.resolve(colours(H0, W0) if colour1 is None else colour1, n1)
    nz2, ids2 = nz.copy(), ids.copy()
    if change is not None:
        change(nz2, ids2)
    t.first_out = t.out.copy()
    t.begin_view(cam2 if cam2 is not None else cam, nz2, ids2)
    return t


def test_first_view_is_the_accumulator():
    cam = make_camera(W0, H0)
    nz, ids = flat_planes(H0, W0)
    ids[2, 3] = NO
    c = colours(H0, W0)
    c[1, 1] = [np.nan, 0.5, 0.25, 9.0]
    c[..., 3] = 5.0                                         # the accumulator's w is never used
    t = tr.Temporal(W0, H0, *PARAMS)
    assert np.all(bits(t.begin_view(cam, nz, ids)) == 0)
    out, bgra = t.resolve(c, 4)
    assert np.array_equal(bits(out[..., :3]), bits(c[..., :3]))
    want_w = np.full((H0, W0), 4.0, np.float32)
    want_w[1, 1] = 0.0                                      # a non-finite colour counts no sample
    assert np.array_equal(bits(out[..., 3]), bits(want_w))
    assert np.array_equal(bgra, dr.encode_bgra(c))
    assert t.stats() == (W0 * H0 - 1, 0)


def test_same_camera_twice_carries_everything():
    t = two_views(n1=3)
    assert np.all(t.reasons["valid"])
    assert np.array_equal(t.reasons["qx"], np.tile(np.arange(W0), (H0, 1)))
    assert np.array_equal(t.reasons["qy"], np.tile(np.arange(H0)[:, None], (1, W0)))
    assert np.array_equal(bits(t.hist), bits(t.first_out))
    assert t.stats() == (W0 * H0, W0 * H0)
    # and the blend is the mean of both views' samples
    c2 = colours(H0, W0, seed=2)
    out, _ = t.resolve(c2, 1)
    want = ((t.first_out[..., :3] * F(3)) + (c2[..., :3] * F(1))) / F(4)
    assert np.array_equal(bits(out[..., :3]), bits(want)) and np.all(out[..., 3] == 4)


def test_same_camera_twice_on_a_scene():
    w, h = 48, 27
    sc = Scene()
    sc.add_preset("cornell_lit")
    cam = make_camera(w, h)
    nz, ids = dr.gbuffer_scene(sc.draw_list(), cam, w, h)
    t = tr.Temporal(w, h, 0.9, 0.01, 2)
    t.begin_view(cam, nz, ids)
    first, _ = t.resolve(colours(h, w), 3)
    hist = t.begin_view(cam, nz, ids)
    guided = ids != NO
    assert 0.25 < guided.mean() < 1.0
    assert np.array_equal(t.reasons["valid"], guided) and t.stats() == (int(guided.sum()), int(guided.sum()))
    assert np.array_equal(bits(hist[guided][:, :3]), bits(first[guided][:, :3]))
    assert np.all(hist[guided][:, 3] == 2)                  # 3 samples, capped at max_history = 2
    assert np.all(bits(hist[~guided]) == 0)                 # a NO_PRIM pixel never has history


PIX = (3, 5)


def only_pixel_fails(t, condition):
    r = t.reasons
    want = np.ones((H0, W0), bool)
    want[PIX] = False
    assert np.array_equal(r["valid"], want)
    for name in ("guided", "inside", "same_id", "normal_ok", "plane_ok", "hist_ok"):
        assert bool(r[name][PIX]) == (name != condition), name
    assert np.all(bits(t.hist[PIX]) == 0) and np.all(t.hist[want][:, 3] > 0)


def test_reject_no_prim():
    def change(nz, ids):
        ids[PIX] = NO
    only_pixel_fails(two_views(change, change1=change), "guided")      # even where the old pixel had none either
    t = two_views(change)
    assert not t.reasons["valid"][PIX] and t.reasons["valid"].sum() == W0 * H0 - 1


def test_reject_id_mismatch():
    def change(nz, ids):
        ids[PIX] = 4
    only_pixel_fails(two_views(change), "same_id")


def test_reject_normal():
    def change(nz, ids):
        nz[PIX][:3] = [0.6, 0.0, -0.8]                      # n_p . n_q = 0.8 < 0.9; D = 0, so the plane test holds
    only_pixel_fails(two_views(change), "normal_ok")
    t = two_views(change, params=(0.75, 0.01, 256))
    assert np.all(t.reasons["valid"])


def test_reject_plane_distance():
    def change(nz, ids):
        nz[PIX][3] = F(0.5)                                 # the same ray, another depth: q = p, far off the plane
    only_pixel_fails(two_views(change), "plane_ok")
    t = two_views(change, params=(0.9, 1e9, 256))
    assert np.all(t.reasons["valid"])


def test_reject_nan_depth():
    def change(nz, ids):
        nz[PIX][3] = np.nan                                 # a NaN position fails the frame test already
    t = two_views(change)
    assert not t.reasons["valid"][PIX] and not t.reasons["inside"][PIX] and np.all(bits(t.hist[PIX]) == 0)
    assert int(t.reasons["valid"].sum()) == W0 * H0 - 1


def test_reject_behind_the_previous_camera():
    """The new camera stands at the same place and looks the other way: every point it sees lies behind the
    previous camera (c.w <= 0). The plane tolerance is out of the way, so nothing else refuses the taps."""
    cam = make_camera(W0, H0, position=[0.0, 0.5, -3.0, 0.0], forward=[0.0, -0.5, 3.0, 0.0])
    back = make_camera(W0, H0, position=[0.0, 0.5, -3.0, 0.0], forward=[0.0, 0.5, -3.0, 0.0])
    nz, ids = flat_planes(H0, W0)
    t = tr.Temporal(W0, H0, 0.9, 1e9, 256)
    t.begin_view(cam, nz, ids)
    t.resolve(colours(H0, W0), 2)
    t.begin_view(back, nz, ids)
    assert np.all(t.reasons["cw"] <= 0) and not np.any(t.reasons["inside"]) and np.all(bits(t.hist) == 0)
    assert np.all(t.reasons["same_id"] & t.reasons["normal_ok"] & t.reasons["hist_ok"])


def test_reject_off_frame():
    """A camera moved back sees more than the previous one did: the border reprojects off the old frame on all four
    sides with c.w > 0, the middle stays valid."""
    cam2 = make_camera(W0, H0, position=[0.0, 0.8, -4.8, 0.0], forward=[0.0, -0.5, 3.0, 0.0])
    t = two_views(cam2=cam2, params=(0.9, 1e9, 256))
    r = t.reasons
    assert np.all(r["cw"] > 0)
    assert np.any(r["xs"] < 0) and np.any(r["xs"] >= W0) and np.any(r["ys"] < 0) and np.any(r["ys"] >= H0)
    assert np.array_equal(r["valid"], r["inside"]) and 0 < r["valid"].sum() < W0 * H0
    assert np.all(bits(t.hist[~r["inside"]]) == 0)


def test_reject_empty_and_non_finite_history():
    c = colours(H0, W0)
    c[PIX] = [0.5, np.inf, 0.5, 0.0]
    t = two_views(colour1=c)                                # case C with a non-finite colour: out.w = +0
    assert t.first_out[PIX][3] == 0 and np.isinf(t.first_out[PIX][1])
    only_pixel_fails(t, "hist_ok")
    t = two_views(n1=0)                                     # case D everywhere: nothing to carry
    assert not np.any(t.reasons["hist_ok"]) and np.all(bits(t.hist) == 0)
    # a non-finite colour under a positive length cannot come out of a resolve; the tap test refuses it all the same
    cam = make_camera(W0, H0)
    nz, ids = flat_planes(H0, W0)
    t = tr.Temporal(W0, H0, *PARAMS)
    t.begin_view(cam, nz, ids)
    t.resolve(colours(H0, W0), 2)
    t.out[PIX][0] = -np.inf
    t.begin_view(cam, nz, ids)
    only_pixel_fails(t, "hist_ok")


def test_nan_colour_never_enters_a_history():
    t = two_views(n1=3)
    c2 = colours(H0, W0, seed=2)
    c2[PIX] = [0.1, np.nan, 0.2, 0.0]
    hist = t.hist.copy()
    out, _ = t.resolve(c2, 5)
    assert np.array_equal(bits(out[PIX]), bits(hist[PIX]))  # case B: the history, bit for bit
    assert np.all(np.isfinite(out)) and out[0, 0, 3] == 8
    nxt = t.begin_view(make_camera(W0, H0), *flat_planes(H0, W0))
    assert np.all(np.isfinite(nxt)) and nxt[PIX][3] == 3


def test_max_history_caps_the_length():
    t = two_views(n1=1000, params=(0.9, 0.01, 16))
    assert np.all(t.first_out[..., 3] == 1000) and np.all(t.hist[..., 3] == 16)
    out, _ = t.resolve(colours(H0, W0, seed=3), 1 << 30)    # n is clamped to 2^24
    assert np.all(out[..., 3] == F(16) + F(1 << 24))


def test_no_samples_returns_the_history_and_resolve_is_idempotent():
    t = two_views(n1=3)
    hist = t.hist.copy()
    out, bgra = t.resolve(colours(H0, W0, seed=4), 0)
    assert np.array_equal(bits(out), bits(hist)) and np.array_equal(bgra, dr.encode_bgra(hist))
    c = colours(H0, W0, seed=5)
    a, a8 = t.resolve(c, 2)
    b, b8 = t.resolve(c, 2)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(a8, b8) and np.array_equal(bits(t.hist), bits(hist))
    assert np.all(a[..., 3] == 5)                           # 3 + 2, not 3 + 2 + 2


def test_begin_view_invalidates_the_result_and_clear_forgets():
    t = two_views(n1=3)
    assert t.out is None
    assert np.all(bits(t.begin_view(make_camera(W0, H0), *flat_planes(H0, W0))) == 0)    # no result in between
    t.resolve(colours(H0, W0), 1)
    t.clear()
    with pytest.raises(RuntimeError):
        t.resolve(colours(H0, W0), 1)
    assert np.all(bits(t.begin_view(make_camera(W0, H0), *flat_planes(H0, W0))) == 0)


# ------------------------------------------------------------------------------------------------ the library
def test_header_is_the_signature_table():
    text = (Path(__file__).resolve().parent.parent / "include" / "temporal" / "iqpt_temporal.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(iqpt_[a-z0-9_]+)\s*\(", text))
    lib = iqpt.load()
    assert len(names) == 17
    for n in names:
        assert hasattr(lib, n), n
    assert names == {s[0] for s in _lib.TEMPORAL_SIGNATURES}
    assert lib.iqpt_abi_version() == 6                      # additions only


def test_argument_checks():
    lib = _lib.load()
    h = C.c_void_p()
    for w, hh in ((0, 4), (4, 0), (8193, 4), (4, 8193)):
        assert lib.iqpt_temporal_create(0, w, hh, C.byref(h)) == INVALID and not h.value
    assert lib.iqpt_temporal_create(0, 4, 4, None) == INVALID
    good = _lib.TemporalParams(0.9, 0.01, 256)
    for bad in (_lib.TemporalParams(float("nan"), 0.01, 256), _lib.TemporalParams(float("inf"), 0.01, 256),
                _lib.TemporalParams(0.9, -0.5, 256), _lib.TemporalParams(0.9, float("nan"), 256),
                _lib.TemporalParams(0.9, 0.01, 0), _lib.TemporalParams(0.9, 0.01, (1 << 24) + 1)):
        assert lib.iqpt_temporal_set_params(None, C.byref(bad)) == INVALID
        assert b"must be" in lib.iqpt_last_error()
    assert lib.iqpt_temporal_set_params(None, C.byref(good)) == INVALID and b"NULL" in lib.iqpt_last_error()
    assert lib.iqpt_temporal_set_params(None, None) == INVALID
    for call in (lambda: lib.iqpt_temporal_default_params(None),
                 lambda: lib.iqpt_temporal_begin_view(None, None, None, None),
                 lambda: lib.iqpt_temporal_begin_view_device(None, None, None, None),
                 lambda: lib.iqpt_temporal_begin_view_raster(None, None), lambda: lib.iqpt_temporal_clear(None),
                 lambda: lib.iqpt_temporal_resolve(None, None, 1), lambda: lib.iqpt_temporal_resolve_device(None, None, 1),
                 lambda: lib.iqpt_temporal_resolve_ctx(None, None), lambda: lib.iqpt_temporal_read(None, None, None),
                 lambda: lib.iqpt_temporal_output_device(None, None),
                 lambda: lib.iqpt_temporal_copy_frame_device(None, None, 0), lambda: lib.iqpt_temporal_sync(None),
                 lambda: lib.iqpt_temporal_time(None, None, None, None, None),
                 lambda: lib.iqpt_temporal_stats(None, None, None)):
        assert call() == INVALID
    assert lib.iqpt_temporal_destroy(None) == 0
    p = _lib.TemporalParams()
    assert lib.iqpt_temporal_default_params(C.byref(p)) == 0 and 1 <= p.max_history <= 1 << 24
    for bad in ((float("nan"), 0.01, 256), (0.9, -1.0, 256), (0.9, 0.01, 0), (0.9, 0.01, (1 << 24) + 1)):
        with pytest.raises(ValueError):
            tr.check_params(*bad)


# ------------------------------------------------------------------------------------------------ quality
# r measured with this reference (DESIGN.md §11 "Quality"); the test asks for half of that gain
R_MEASURED = 0.4130     # raw RMSE 0.2309, temporal 0.0954; valid share 0.983, mean history length 7.55


def test_quality_on_the_oracle_frames():
    """cornell_lit, 96x54, depth 8, seed 1984, one OracleFrame with reset() between 8 views of 1 spp, view k at
    (0.05 k, 0.5, -3) looking along (-0.02 k, -0.5, 3); parameters 0.9 / 0.01 / 256. RMSE over xyz of the guided
    pixels of the last view against a 1024-spp frame of another seed."""
    w, h, views = 96, 54, 8
    sc = Scene()
    sc.add_preset("cornell_lit")
    pk = sc.build_packet()
    items = sc.draw_list()
    fr = oracle.OracleFrame(w, h, max_depth=8, seed=1984)
    t = tr.Temporal(w, h, 0.9, 0.01, 256)
    for k in range(views):
        cam = make_camera(w, h, position=[0.05 * k, 0.5, -3.0, 0.0], forward=[-0.02 * k, -0.5, 3.0, 0.0])
        nz, ids = dr.gbuffer_scene(items, cam, w, h)
        fr.reset()
        fr.render(pk, cam, 1)
        t.begin_view(cam, nz, ids)
        out, _ = t.resolve(fr.lin, 1)
    raw = fr.lin.copy().reshape(h, w, 4)
    guided = ids != NO
    n_guided, n_valid = t.stats()
    share = n_valid / n_guided
    truth = oracle.OracleFrame(w, h, max_depth=8, seed=77)
    truth.render(pk, cam, 1024)
    ref = truth.lin.reshape(h, w, 4)[..., :3].astype(np.float64)

    def rmse(a):
        return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref)[guided] ** 2)))

    e_raw, e_tmp = rmse(raw), rmse(out)
    r = e_tmp / e_raw
    p = iqpt.denoise.default_params()
    args = (p["levels"], p["normal_squarings"], p["depth_sharpness"], p["colour_sharpness"])
    d_raw, d_tmp = rmse(dr.denoise(raw, nz, ids, *args)[0]), rmse(dr.denoise(out, nz, ids, *args)[0])
    print(f"valid share {share:.4f} mean history {float(out[guided][:, 3].mean()):.2f} raw RMSE {e_raw:.4f} "
          f"temporal {e_tmp:.4f} r = {r:.4f}; denoised raw {d_raw:.4f} denoised temporal {d_tmp:.4f}")
    assert share >= 0.95
    assert r <= (1 + R_MEASURED) / 2
    assert d_tmp < d_raw
