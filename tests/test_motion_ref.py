"""Moving-model reprojection's numpy reference (tests/motion_ref.py) against the properties the
definition implies, the host-only table helper (iqpt_motion_table) against float64, the entry points' argument
checks that need no device, and the float64 truth of where a moved model's pixels came from."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_ref as dr
import iqpt
import motion_cases as mc
import motion_ref as mr
import raster_ref as rr
import temporal_ref as tr
import truth
from iqpt import Scene, _lib, make_camera

F = np.float32
NO = mr.NO_PRIM
PARAMS = (0.9, 0.01, 256)
INVALID, NOT_READY = 1, 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ equivalence
@pytest.mark.parametrize("layout", mc.LAYOUTS)
@pytest.mark.parametrize("table", ["none", "static"])
def test_no_motion_is_temporal_reprojection(layout, table):
    """n == 0 and all-static tables: the object equals temporal_ref.Temporal bit for bit, on seeded planes with
    special colours and depths."""
    w, h, n = 33, 9, 3
    m, t = mr.Motion(w, h, *mc.PARAMS), tr.Temporal(w, h, *mc.PARAMS)
    valid = 0
    for cam, nz, ids, colour, samples, _ in mc.synthetic_views(w, h, n, layout, seed=5):
        ids = np.where(ids == NO, NO, ids % n).astype(np.uint32)      # every id inside the table
        hist = m.begin_view(cam, nz, ids, None if table == "none" else mr.identity_table(n))
        assert np.array_equal(bits(hist), bits(t.begin_view(cam, nz, ids)))
        assert m.stats() == t.stats() + (0, 0)
        valid += m.stats()[1]
        got, want = m.resolve(colour, samples), t.resolve(colour, samples)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    assert valid > 0


def wall_pair(w=24, h=14, n_ids=1):
    """One wall seen twice by the same camera: (cam, nz, ids, colour)."""
    cam = mc.camera_at(w, h, mc.POS_A)
    nz = np.empty((h, w, 4), np.float32)
    nz[..., :3] = (-mc.FWD_UNIT).astype(np.float32)
    nz[..., 3] = mc.wall_depth(cam)
    ids = np.zeros((h, w), np.uint32)
    colour = np.random.default_rng(2).random((h, w, 4), dtype=np.float32)
    return cam, nz, ids, colour


def second_view(cam, nz, ids, colour, table, ids2=None, nz2=None):
    m = mr.Motion(ids.shape[1], ids.shape[0], *PARAMS)
    m.begin_view(cam, nz, ids)
    m.first_out = m.resolve(colour, 3)[0].copy()
    m.begin_view(cam, nz if nz2 is None else nz2, ids if ids2 is None else ids2, table)
    return m


def test_a_moved_identity_renormalises_the_normal():
    """moved == 1 with identity matrices is not the static path: nm is n_p * (1 / sqrt(n_p . n_p)), which differs from
    n_p in some pixel's bits; the history is the same wherever the tests still pass."""
    cam, nz, ids, colour = wall_pair()
    rng = np.random.default_rng(11)
    n = rng.normal(size=nz.shape[:2] + (3,))
    n = (0.15 * n / np.linalg.norm(n, axis=-1, keepdims=True) - mc.FWD_UNIT)
    nz[..., :3] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)      # unit to float32 rounding
    ident = mr.identity_table(1)
    ident["moved"] = 1
    a = second_view(cam, nz, ids, colour, ident)
    b = second_view(cam, nz, ids, colour, mr.identity_table(1))
    nm = a.reasons["moved_reasons"]["nm"]
    assert np.any(bits(nm) != bits(nz[..., :3]))
    assert np.allclose(nm, nz[..., :3], atol=3e-7)
    assert np.array_equal(bits(a.reasons["moved_reasons"]["Pm"]), bits(a.view[2]))       # the point is not touched
    both = (a.hist[..., 3] > 0) & (b.hist[..., 3] > 0)
    assert both.sum() > 0.9 * both.size
    assert np.array_equal(bits(a.hist[both]), bits(b.hist[both]))
    assert a.stats() == (ids.size, int((a.hist[..., 3] > 0).sum()), ids.size, int((a.hist[..., 3] > 0).sum()))
    assert b.stats()[2:] == (0, 0)


# ------------------------------------------------------------------------------------------------ rigid motion
def test_rigid_motion_against_an_integer_map():
    """A plane of points (the wall) carried by a known rotation about its normal and a translation in its plane, the
    camera fixed: view 2's pixel (x, y) shows the point that view 1 showed at the pixel an explicit float64 map gives,
    and inherits exactly that pixel's result."""
    w, h = 40, 24
    cam, nz, ids, colour = wall_pair(w, h)
    angle, shift = 0.06, np.array([0.21, 0.0, 0.0])
    k = mc.FWD_UNIT
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).T
    forward = mc._about_centre(R) @ mc._translate(shift)           # where the model's points go (row vectors)
    back = np.linalg.inv(forward)
    table = np.array([mr.entry(back)])
    m = second_view(cam, nz, ids, colour, table)
    # the explicit map, in float64 and without any of the restatement's steps: pixel centre -> world point on the
    # wall -> back -> screen
    py, px = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    world = truth.unproject_point(cam, px, py, float(nz[0, 0, 3]))
    was = (np.concatenate([world, np.ones((h, w, 1))], axis=-1) @ back)[..., :3]
    sx, sy, _, cw = truth.project(cam, was)
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h) & (cw > 0)
    clear = inside & (np.abs(sx - np.round(sx)) > 1e-3) & (np.abs(sy - np.round(sy)) > 1e-3)    # not on a pixel edge
    qx, qy = np.floor(sx).astype(int), np.floor(sy).astype(int)
    assert clear.sum() > 0.7 * w * h and np.any(qx[clear] != np.arange(w)[None, :].repeat(h, 0)[clear])
    assert np.all(m.hist[clear][:, 3] == 3)
    assert np.array_equal(bits(m.hist[clear][:, :3]), bits(m.first_out[qy[clear], qx[clear]][:, :3]))
    assert not np.any(m.hist[~inside][:, 3] > 0)                   # came from beyond the old frame
    assert m.stats() == (w * h, int((m.hist[..., 3] > 0).sum()), w * h, int((m.hist[..., 3] > 0).sum()))


def test_disocclusion_and_static_neighbours():
    """A model (id 1) covers the wall's (id 0) left part, then moves two pixels to the left: the wall pixels it
    uncovered start empty (the pixel they reproject to showed the model), the model's pixels follow it, and every
    other wall pixel keeps §11's history exactly."""
    w, h = 32, 10
    cam, nz, ids, colour = wall_pair(w, h)
    ids[:, 4:12] = 1
    ids2 = np.zeros_like(ids)
    ids2[:, 2:10] = 1
    table = mr.identity_table(2)
    table[1] = mc.kind_entry("translate", cam, w)                  # back: two pixels along +x, on the screen too
    m = second_view(cam, nz, ids, colour, table, ids2=ids2)
    s = tr.Temporal(w, h, *PARAMS)
    s.begin_view(cam, nz, ids)
    s.resolve(colour, 3)
    s.begin_view(cam, nz, ids2)
    step = 2
    assert np.all(m.reasons["moved_reasons"]["qx"][:, 2:10] == np.arange(2 + step, 10 + step)[None, :])
    model = ids2 == 1
    uncovered = (ids == 1) & ~model
    assert uncovered.any() and np.all(bits(m.hist[uncovered]) == 0)
    assert np.all(m.hist[model][:, 3] == 3)                        # every pixel of the model was visible before
    xs = np.flatnonzero(model[0])
    assert np.array_equal(bits(m.hist[:, xs, :3]), bits(m.first_out[:, xs + step, :3]))
    assert np.array_equal(bits(m.hist[~model]), bits(s.hist[~model]))
    still = ~model & ~uncovered
    assert np.all(m.hist[still][:, 3] == 3)


def test_a_poisoned_draw_harms_nobody_else():
    w, h = 32, 10
    cam, nz, ids, colour = wall_pair(w, h)
    ids[:, 10:20] = 1
    ids[:, 20:] = 2
    good = mr.identity_table(3)
    good[2] = mc.kind_entry("translate", cam, w)
    for poison in ("nan", "inf"):
        bad = good.copy()
        bad[1] = mc.kind_entry("nan", cam, w)
        if poison == "inf":
            bad[1]["back"][:] = np.inf
            bad[1]["nback"][:] = -np.inf
        a, b = second_view(cam, nz, ids, colour, bad), second_view(cam, nz, ids, colour, good)
        assert np.all(bits(a.hist[ids == 1]) == 0) and np.all(b.hist[ids == 1][:, 3] == 3)
        assert np.array_equal(bits(a.hist[ids != 1]), bits(b.hist[ids != 1]))
        assert a.stats()[3] > 0 and a.stats()[3] == b.stats()[3]


def test_ids_beyond_the_table_start_empty():
    w, h = 32, 10
    cam, nz, ids, colour = wall_pair(w, h)
    ids[:, 10:20] = 1
    ids[:, 20:] = 7
    m = second_view(cam, nz, ids, colour, mr.identity_table(2))
    assert np.all(bits(m.hist[ids == 7]) == 0) and np.all(m.hist[ids < 2][:, 3] == 3)
    assert np.all(second_view(cam, nz, ids, colour, None).hist[..., 3] == 3)          # n == 0: no bound at all
    assert m.stats() == (w * h, int((ids < 2).sum()), 0, 0)


# ------------------------------------------------------------------------------------------------ arguments
def test_reference_table_checks():
    t = mr.identity_table(2)
    for field, value in (("moved", 2), ("moved", 0xFFFFFFFF), ("reserved", 1)):
        bad = t.copy()
        bad[field][1] = value
        with pytest.raises(ValueError):
            mr.check_table(bad)
    with pytest.raises(ValueError):
        mr.check_table(np.zeros(3, np.float32))
    assert mr.check_table(None)[1] == 0 and mr.check_table(t)[1] == 2


def test_argument_checks_without_a_device():
    lib = _lib.load_motion()
    p = _lib.TemporalParams()
    assert lib.iqpt_motion_default_params(None) == INVALID
    assert lib.iqpt_motion_default_params(C.byref(p)) == 0
    assert (p.normal_min, p.plane_tolerance, p.max_history) == tuple(iqpt.temporal.default_params().values())
    assert iqpt.motion.default_params() == iqpt.temporal.default_params()
    h = C.c_void_p()
    for w, hh in ((0, 4), (4, 0), (8193, 4), (4, 8193)):
        assert lib.iqpt_motion_create(0, w, hh, C.byref(h)) == INVALID and not h.value
    assert lib.iqpt_motion_create(0, 4, 4, None) == INVALID
    assert lib.iqpt_motion_destroy(None) == 0
    assert lib.iqpt_motion_set_params(None, C.byref(p)) == INVALID
    for bad in ((np.nan, 0.01, 256), (0.9, -1.0, 256), (0.9, 0.01, 0), (0.9, 0.01, (1 << 24) + 1)):
        assert lib.iqpt_motion_set_params(None, C.byref(_lib.TemporalParams(*bad))) == INVALID
    cam = make_camera(4, 4)
    assert lib.iqpt_motion_begin_view(None, C.byref(cam), None, None, None, 0) == INVALID
    assert lib.iqpt_motion_begin_view_device(None, C.byref(cam), None, None, None, 0) == INVALID
    assert lib.iqpt_motion_begin_view_raster(None, None, None, 0) == INVALID
    for fn in (lib.iqpt_motion_clear, lib.iqpt_motion_sync):
        assert fn(None) == INVALID
    assert lib.iqpt_motion_resolve(None, None, 1) == INVALID
    assert lib.iqpt_motion_resolve_device(None, None, 1) == INVALID
    assert lib.iqpt_motion_resolve_ctx(None, None) == INVALID
    assert lib.iqpt_motion_read(None, None, None) == INVALID
    assert lib.iqpt_motion_output_device(None, None) == INVALID
    assert lib.iqpt_motion_copy_frame_device(None, None, 0) == INVALID
    assert lib.iqpt_motion_time(None, None, None, None, None) == INVALID
    assert lib.iqpt_motion_stats(None, None, None, None, None) == INVALID
    assert C.sizeof(_lib.MotionEntry) == iqpt.motion.ENTRY_DTYPE.itemsize == mr.ENTRY_DTYPE.itemsize == 128
    assert iqpt.motion.ENTRY_DTYPE == mr.ENTRY_DTYPE


# ------------------------------------------------------------------------------------------------ iqpt_motion_table
def scene_of(models):
    """A scene of cubes (and one quad) with the given (scale, rotation, translation) per model, in draw order."""
    sc = Scene()
    for i, (s, r, t) in enumerate(models):
        name = f"m{i:02d}"
        (sc.add_mesh_quad if i == 0 else sc.add_mesh_cube)(name)
        sc.add_model(name, name, scale=s, rotation=r, translation=t)
    return sc


TABLE_PREV = [(1.0, [0, 0, 0, 0], [0, 0, 0, 0]),                       # stays
              (0.5, [0, 0, 0, 0], [0.3, -0.2, 0.1, 0]),                # translated
              (1.0, [0.2, 0.0, 0.0, 0], [0, 0, 0, 0]),                 # rotated about each axis in turn
              (1.0, [0.0, 0.3, 0.0, 0], [1, 0.5, 0, 0]),
              (1.0, [0.0, 0.0, 1.1, 0], [-1, 0.5, 0, 0]),
              (0.35, [0, 0, 0, 0], [-0.4, -0.15, 0.2, 0]),             # uniform scale
              ([2.0, 2.0, 1.0, 1.0], [np.pi / 2, 0, 0, 0], [0, -0.5, 0, 0]),      # non-uniform, as the presets' walls
              (10.0, [np.pi / 2, 0, 0, 0], [0, -10.0, 0, 0]),          # the presets' largest magnitudes
              (1.0, [0, 0, 0, 0], [0, 0, 0, 0]),                       # becomes singular
              (0.4, [0.1, 0.2, 0.3, 0], [0.2, 0.1, -0.4, 0])]          # stays, with a general transform
TABLE_CUR = [TABLE_PREV[0],
             (0.5, [0, 0, 0, 0], [0.4, -0.2, 0.35, 0]),
             (1.0, [0.9, 0.0, 0.0, 0], [0, 0, 0, 0]),
             (1.0, [0.0, -0.5, 0.0, 0], [1, 0.5, 0.2, 0]),
             (1.0, [0.3, 0.2, 1.4, 0], [-1, 0.7, 0, 0]),
             (0.7, [0, 0.1, 0, 0], [-0.4, -0.1, 0.2, 0]),
             ([2.5, 1.5, 1.0, 1.0], [np.pi / 2, 0.2, 0, 0], [0.1, -0.5, 0, 0]),
             (10.0, [np.pi / 2, 0.05, 0, 0], [0.5, -10.0, -0.25, 0]),
             ([1.0, 0.0, 1.0, 1.0], [0, 0, 0, 0], [0, 0, 0, 0]),
             TABLE_PREV[9]]
SINGULAR = 8
# The largest |back - float64 inv(cur) @ prev| over TABLE_PREV -> TABLE_CUR's moved, regular draws, relative to the
# largest word of the float64 matrix, as iqpt_motion_table computes it (deterministic host arithmetic); the
# assertion allows four times it, a margin against later edits of the helper alone.
BACK_ERROR_MEASURED = 1.2e-7


def test_motion_table_against_float64():
    prev, cur = scene_of(TABLE_PREV), scene_of(TABLE_CUR)
    t = iqpt.motion_table(prev, cur)
    dp, dc = prev.draw_list(), cur.draw_list()
    assert t.dtype == mr.ENTRY_DTYPE and len(t) == len(dp) == len(TABLE_PREV)
    assert not t["reserved"].any()
    ident = mr.identity_table(1)[0]
    worst = 0.0
    for i, (e, a, b) in enumerate(zip(t, dp, dc)):
        same = np.array_equal(bits(a["transform"]), bits(b["transform"]))
        assert same == (i in (0, 9)) and e["moved"] == (0 if same else 1)
        if same:
            assert e.tobytes() == ident.tobytes()
            continue
        back = e["back"].reshape(4, 4)
        nb = e["nback"].reshape(3, 4)
        assert np.array_equal(bits(nb[:, :3]), bits(rr.normal_matrix(back))) and not bits(nb[:, 3]).any()
        if i == SINGULAR:
            assert not np.any(np.isfinite(back[:3, :3])) and not np.any(np.isfinite(nb[:, :3]))
            continue
        want = np.linalg.inv(b["transform"].astype(np.float64)) @ a["transform"].astype(np.float64)
        err = float(np.abs(back - want).max() / np.abs(want).max())
        print(f"draw {i}: |back - float64| / max|float64| = {err:.3e}")
        worst = max(worst, err)
        # the normal matrix of back sends a normal of the current scene to the previous scene's, up to length
        nrm = np.array([0.3, -0.5, 0.8])
        n_prev = nrm @ np.linalg.inv(a["transform"].astype(np.float64)[:3, :3].T)
        n_cur = nrm @ np.linalg.inv(b["transform"].astype(np.float64)[:3, :3].T)
        got = n_cur @ nb[:, :3].astype(np.float64)
        assert np.allclose(got / np.linalg.norm(got), n_prev / np.linalg.norm(n_prev), atol=1e-5)
    print(f"largest: {worst:.3e}")
    assert 0 < worst <= 4 * BACK_ERROR_MEASURED
    # a poisoned (singular) draw has no history in the restatement
    assert not np.isfinite(t[SINGULAR]["back"]).all()


def test_motion_table_refuses_other_scenes():
    prev = scene_of(TABLE_PREV[:3])
    with pytest.raises(iqpt.IqptError) as e:
        iqpt.motion_table(prev, scene_of(TABLE_PREV[:2]))
    assert e.value.status == INVALID
    other = Scene()
    for i in range(3):
        other.add_mesh_cube(f"m{i:02d}")                           # draw 0 is a cube here and a quad there
        other.add_model(f"m{i:02d}", f"m{i:02d}")
    with pytest.raises(iqpt.IqptError) as e:
        iqpt.motion_table(prev, other)
    assert e.value.status == INVALID
    assert len(iqpt.motion_table(Scene(), Scene())) == 0
    t = iqpt.motion_table(prev, prev)
    assert not t["moved"].any() and t.tobytes() == mr.identity_table(3).tobytes()


# ------------------------------------------------------------------------------------------------ truth
TRUTH_FRAMES = [(17, 13), (48, 27)]
OFFSETS = np.array([[0.0, 0.0], [-1, -1], [-1, 1], [1, -1], [1, 1]]) / 128.0
# The largest distance, in pixels of the previous view, between the restatement's (xs, ys) of a decided pixel of the
# moved cube and the float64 hit point sent through float64 inv(cur) @ prev and the previous camera, over both
# frames and both moves; the assertion allows twice it. It must stay below 0.05 px.
TRUTH_DISTANCE_MEASURED = 9.7e-4


@functools.lru_cache(maxsize=None)
def movers_view(k, w, h):
    sc = mc.movers(k)
    dl = sc.draw_list()
    cam = mc.movers_camera(w, h)
    nz, ids = dr.gbuffer_scene(dl, cam, w, h)
    return sc, dl, cam, nz, ids


@pytest.mark.parametrize("w,h", TRUTH_FRAMES)
@pytest.mark.parametrize("k", [1, 2])
def test_truth_moved_pixels_come_from_where_float64_says(k, w, h):
    """Independent of the restatement: tests/truth.py's float64 triangles and caster on the movers scene, views k - 1
    and k. Every decided pixel (§9.6: the centre and the four points around it hit the same draw) of the moved cube in
    view k: its float64 hit point through float64 inv(cur) @ prev and the previous camera lands where the
    restatement's (xs, ys) says, within twice the measured distance."""
    sp, dlp, cam, nzp, idsp = movers_view(k - 1, w, h)
    sc, dlc, _, nzc, idsc = movers_view(k, w, h)
    tris = truth.world_triangles(dlc)
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    sx, sy = px[..., None] + 0.5 + OFFSETS[:, 0], py[..., None] + 0.5 + OFFSETS[:, 1]
    o, d = truth.unproject(cam, sx, sy)
    hit = truth.cast(tris, o.reshape(-1, 3), d.reshape(-1, 3))
    draw = hit["draw"].reshape(h, w, 5)
    decided = np.all(draw == draw[..., :1], axis=-1)
    undecided = 1.0 - float(decided.mean())
    assert undecided <= 0.02, undecided
    on_mover = decided & (draw[..., 0] == mc.MOVER)
    assert on_mover.sum() >= 4 and np.array_equal(idsc[on_mover], np.full(int(on_mover.sum()), mc.MOVER, np.uint32))
    # float64 truth of where the point was
    Mp, Mc = dlp[mc.MOVER]["transform"].astype(np.float64), dlc[mc.MOVER]["transform"].astype(np.float64)
    point = hit["point"].reshape(h, w, 5, 3)[..., 0, :]
    was = (np.concatenate([point, np.ones((h, w, 1))], axis=-1) @ (np.linalg.inv(Mc) @ Mp))[..., :3]
    tx, ty, _, tw = truth.project(cam, was)
    # the restatement, with iqpt_motion_table's entry
    table = iqpt.motion_table(sp, sc)
    assert list(table["moved"]) == [0, 0, 1]
    m = mr.Motion(w, h, *PARAMS)
    m.begin_view(cam, nzp, idsp)
    m.resolve(np.ones((h, w, 4), np.float32), 1)
    m.begin_view(cam, nzc, idsc, table)
    r = m.reasons["moved_reasons"]
    dist = np.hypot(r["xs"].astype(np.float64) - tx, r["ys"].astype(np.float64) - ty)[on_mover]
    print(f"view {k} {w}x{h}: undecided {100 * undecided:.2f} %, {int(on_mover.sum())} decided pixels on the mover, "
          f"largest distance {dist.max():.3e} px, with history {int((m.hist[on_mover][:, 3] > 0).sum())}")
    assert np.all(tw[on_mover] > 0)
    assert TRUTH_DISTANCE_MEASURED < 0.05 and dist.max() <= 2 * TRUTH_DISTANCE_MEASURED
    # and the pixel it names showed the mover where float64 says so too, away from pixel edges
    assert (m.hist[on_mover][:, 3] > 0).sum() >= on_mover.sum() // 2


# ------------------------------------------------------------------------------------------------ quality
# measured with this reference, on the moved cube's pixels with a valid history in the last view;
# the test asks for half of that gain (§10.4's rule)
R_MEASURED = 0.6415     # mover: raw RMSE 0.0638, clear-on-change 0.0638, motion 0.0409; valid share 0.939 (139 of 148), mean
                        # history 14.2. Whole frame: 0.0515, 0.0515, 0.0293


def test_quality_on_the_oracle_frames():
    """The movers scene, 96x54, depth 8, seed 1984, the aligned camera, one OracleFrame with reset() between K = 4
    views of 4 spp, the cube moving one step (a quarter of its width along x and 10 degrees about y) per view;
    parameters 0.9 / 0.01 / 256. RMSE over xyz against a 2048-spp frame of the last scene (another seed): (a) the raw
    4-spp last view, (b) clear-on-change, §11 with iqpt_temporal_clear at every scene change, (c) this feature.
    Lighting that changed with the move (the cube's shadow and bounce light on the ground) stays in the history:
    the whole-frame figures are printed, not asserted."""
    import oracle
    from iqpt import align_camera
    w, h, views, spp = 96, 54, 4, 4
    cam = mc.movers_camera(w, h)
    acam = align_camera(cam)
    fr = oracle.OracleFrame(w, h, max_depth=8, seed=1984)
    m, c = mr.Motion(w, h, *PARAMS), tr.Temporal(w, h, *PARAMS)
    prev = None
    for k in range(views):
        sc = mc.movers(k)
        pk = sc.build_packet()
        nz, ids = dr.gbuffer_scene(sc.draw_list(), cam, w, h)
        fr.reset()
        fr.render(pk, acam, spp)
        m.begin_view(cam, nz, ids, iqpt.motion_table(prev, sc) if prev is not None else None)
        out_m, _ = m.resolve(fr.lin, spp)
        c.clear()                                           # "ids are not comparable across packets"
        c.begin_view(cam, nz, ids)
        out_c, _ = c.resolve(fr.lin, spp)
        prev = sc
    raw = fr.lin.copy().reshape(h, w, 4)
    truth_frame = oracle.OracleFrame(w, h, max_depth=8, seed=77)
    truth_frame.render(pk, acam, 2048)
    ref = truth_frame.lin.reshape(h, w, 4)[..., :3].astype(np.float64)

    def rmse(a, mask):
        return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref)[mask] ** 2)))

    mover = ids == mc.MOVER
    carried = mover & (m.hist[..., 3] > 0)
    share = carried.sum() / mover.sum()
    whole = np.ones((h, w), bool)
    fig = {name: (rmse(raw, mask), rmse(out_c, mask), rmse(out_m, mask)) for name, mask in (("frame", whole), ("mover", carried))}
    for name, (a, b, cc) in fig.items():
        print(f"{name}: (a) raw {a:.4f} (b) clear-on-change {b:.4f} (c) motion {cc:.4f} c/a = {cc / a:.4f}")
    print(f"mover pixels {int(mover.sum())}, with a valid history {int(carried.sum())} ({share:.4f}), "
          f"mean history there {float(out_m[carried][:, 3].mean()):.2f}; stats {m.stats()}")
    assert m.stats()[2:] == (int(mover.sum()), int(carried.sum()))
    assert share >= 0.5
    a, b, cc = fig["mover"]
    assert b == a                                           # clear-on-change keeps nothing: every view changed the scene
    assert cc / a <= (1 + R_MEASURED) / 2
