"""CPU tests of the rasterizer: the numpy reference's own properties (tests/raster_ref.py) and
the argument validation of the iqpt_raster_* entry points, which needs no device."""
import ctypes as C

import numpy as np
import pytest

import iqpt
import raster_ref as rr
from iqpt import _lib

W = H = 16


def screen_pieces(tris):
    """Set-up pieces from integer screen coordinates (1/256 pixel) [T,3,2], flat shading data."""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3, 2)
    n = t.shape[0]
    sx, sy = t[:, :, 0], t[:, :, 1]
    area = (sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0]) - (sx[:, 2] - sx[:, 0]) * (sy[:, 1] - sy[:, 0])
    assert np.all(area > 0), "test triangles are clockwise (y down)"
    return {"sx": sx, "sy": sy, "z": np.full((n, 3), 0.5, np.float32), "rw": np.ones((n, 3), np.float32),
            "n": np.tile(np.array([0, 1, 0], np.float32), (n, 3, 1)), "tri": np.arange(n),
            "piece": np.zeros(n, np.int64), "area": area}


def coverage(tri, samples):
    _, _, prim = rr.rasterize(screen_pieces([tri]), W, H, samples)
    return prim != rr.NO_PRIM


def to_clip(px, py, z=0.5, w=1.0):
    """Clip coordinates of the screen position (px, py) pixels on the W x H frame (exact for these sizes)."""
    return [(px / W * 2 - 1) * w, (1 - py / H * 2) * w, z * w, w]


@pytest.mark.parametrize("samples", [1, 4])
def test_shared_edge_samples_are_covered_exactly_once(samples):
    """A convex quad split along a diagonal: every sample of the quad belongs to exactly one of the two triangles,
    the samples exactly on the shared edge included (vertices on the per-axis lattice of the sample coordinates,
    half pixels for pixel centres and quarter pixels plus 1/8 for the 4x pattern, so that edges pass through many
    sample positions)."""
    rng = np.random.default_rng(7)
    on_edge_seen = 0
    grid, first = (2, 0) if samples == 1 else (4, 32)
    for _ in range(240):
        # four points around a centre, clockwise with y down (angles ascending), on the grid
        ang = np.sort(rng.uniform(0, 2 * np.pi, 4))
        if np.min(np.diff(np.concatenate([ang, [ang[0] + 2 * np.pi]]))) < 0.3:
            continue
        rad = rng.uniform(3, 7, 4)
        pts = np.stack([8 + rad * np.cos(ang), 8 + rad * np.sin(ang)], axis=1)
        pts = (np.rint(pts * grid) * (256 // grid)).astype(np.int64) + first
        a, b, c, d = pts
        cross = lambda p, q, r: (q[0] - p[0]) * (r[1] - p[1]) - (r[0] - p[0]) * (q[1] - p[1])
        if min(cross(a, b, c), cross(b, c, d), cross(c, d, a), cross(d, a, b), cross(a, c, d)) <= 0:
            continue                                                      # not strictly convex after snapping
        c1, c2 = coverage([a, b, c], samples), coverage([a, c, d], samples)
        both = rr.rasterize(screen_pieces([[a, b, c], [a, c, d]]), W, H, samples)[2] != rr.NO_PRIM
        assert not np.any(c1 & c2), "a sample on the shared edge is covered twice"
        # the quad itself, as four half-planes with the same top-left rule
        ox, oy = rr.OFFSETS[samples]
        py, px, sm = np.meshgrid(np.arange(H), np.arange(W), np.arange(samples), indexing="ij")
        X, Y = px * 256 + 128 + ox[sm], py * 256 + 128 + oy[sm]
        quad = np.ones_like(X, bool)
        for p, q in ((a, b), (b, c), (c, d), (d, a)):
            dx, dy = q[0] - p[0], q[1] - p[1]
            e = dx * (Y - p[1]) - dy * (X - p[0])
            quad &= (e > 0) | ((e == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
        assert np.array_equal(c1 | c2, quad), "a sample of the quad is covered by neither triangle"
        assert np.array_equal(both, quad)
        diag = (c[0] - a[0]) * (Y - a[1]) - (c[1] - a[1]) * (X - a[0])
        on_edge_seen += int(np.sum((diag == 0) & quad))
    print("samples on the shared edge:", on_edge_seen)
    assert on_edge_seen > 20, "the cases must put samples exactly on the shared edge"


@pytest.mark.parametrize("samples", [1, 4])
def test_rectangle_on_sample_positions_keeps_left_and_top(samples):
    """Sides exactly on sample coordinates: the left and top samples are in, the right and bottom ones out."""
    off = 0.5 if samples == 1 else 0.125       # 0.125: x of sample 2 and y of sample 0 of the 4x pattern
    l, r, t, b = 2 + off, 6 + off, 3 + off, 7 + off
    clip = np.array([to_clip(l, t), to_clip(r, t), to_clip(r, b), to_clip(l, b)], np.float32)
    nrm = np.tile(np.array([0, 1, 0], np.float32), (4, 1))
    _, _, prim = rr.render_clip(clip, nrm, [0, 1, 2, 0, 2, 3], W, H, samples)
    ox, oy = rr.OFFSETS[samples]
    py, px, sm = np.meshgrid(np.arange(H), np.arange(W), np.arange(samples), indexing="ij")
    X, Y = px + 0.5 + ox[sm] / 256, py + 0.5 + oy[sm] / 256
    want = (X >= l) & (X < r) & (Y >= t) & (Y < b)
    assert np.array_equal(prim != rr.NO_PRIM, want)
    assert np.any((X == l) & want) and np.any((Y == t) & want)            # left and top samples kept
    assert np.any((X == r) & (Y >= t) & (Y < b)) and np.any((Y == b) & (X >= l) & (X < r))   # those lost exist


def random_inside_triangles(rng, n):
    clip, idx = [], []
    while len(idx) < 3 * n:
        p = rng.uniform(-1, W + 1, (3, 2))
        if (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[2, 0] - p[0, 0]) * (p[1, 1] - p[0, 1]) <= 0:
            p = p[::-1]
        for q in p:
            w = rng.uniform(0.5, 3.0)
            idx.append(len(clip))
            clip.append(to_clip(q[0], q[1], z=rng.uniform(0.05, 0.95), w=w))
    clip = np.array(clip, np.float32)
    nrm = rng.normal(size=(clip.shape[0], 3)).astype(np.float32)
    return clip, nrm, np.array(idx)


@pytest.mark.parametrize("samples", [1, 4])
def test_clipper_leaves_triangles_inside_every_plane_unchanged(samples):
    """Triangles inside all six planes: their clipped pieces cover exactly the samples of the unclipped triangle
    (same owner, depth and colour per sample)."""
    clip, nrm, idx = random_inside_triangles(np.random.default_rng(3), 24)
    assert np.all(rr.plane_dist(clip) >= 0)
    a = rr.render_clip(clip, nrm, idx, W, H, samples)
    b = rr.render_clip(clip, nrm, idx, W, H, samples, force_clip=True)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    assert np.sum(a[2] != rr.NO_PRIM) > 100


@pytest.mark.parametrize("samples", [1, 4])
def test_bounding_box_drop_changes_nothing(samples):
    """Dropping triangles whose snapped box holds no sample coordinate is invisible: small triangles, many of
    them between samples, render the same with and without it."""
    rng = np.random.default_rng(11)
    clip, idx = [], []
    for _ in range(300):
        c = rng.uniform(0, W, 2)
        p = c + rng.uniform(-0.4, 0.4, (3, 2))
        if (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[2, 0] - p[0, 0]) * (p[1, 1] - p[0, 1]) <= 0:
            p = p[::-1]
        for q in p:
            idx.append(len(clip))
            clip.append(to_clip(q[0], q[1], z=rng.uniform(0.1, 0.9)))
    clip = np.array(clip, np.float32)
    nrm = np.tile(np.array([0, 1, 0], np.float32), (clip.shape[0], 1))
    kept = len(rr.setup(clip, nrm, idx, W, H, samples)["tri"])
    assert kept < len(rr.setup(clip, nrm, idx, W, H, samples, prefilter=False)["tri"])
    a = rr.render_clip(clip, nrm, idx, W, H, samples)
    b = rr.render_clip(clip, nrm, idx, W, H, samples, prefilter=False)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))


def test_clear_colour_and_resolve():
    bgra, depth, prim = rr.render_clip(np.zeros((0, 4)), np.zeros((0, 3)), [], 5, 3, 4)
    assert np.all(bgra == rr.CLEAR_BGRA) and np.all(depth == 1.0) and np.all(prim == rr.NO_PRIM)


# ------------------------------------------------------------------ argument validation (no device needed)
INVALID, NO_DEVICE, NOT_READY = 1, 4, 5


def test_every_declared_raster_symbol_is_exported_and_bound():
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parent.parent / "include" / "raster" / "iqpt_raster.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(iqpt_[a-z0-9_]+)\s*\(", text))
    lib = iqpt.load()
    assert len(names) >= 13
    for n in names:
        assert hasattr(lib, n), n
    assert names == {s[0] for s in _lib.RASTER_SIGNATURES}
    assert lib.iqpt_abi_version() == 6                                      # additions only


def test_raster_create_validates_arguments_before_touching_the_device():
    lib = iqpt.load()
    h = C.c_void_p()
    assert lib.iqpt_raster_create(0, 16, 16, 4, None) == INVALID
    for w, hh in ((0, 16), (16, 0), (_lib.RASTER_MAX_DIM + 1, 16), (16, _lib.RASTER_MAX_DIM + 1)):
        assert lib.iqpt_raster_create(0, w, hh, 4, C.byref(h)) == INVALID
        assert h.value is None
    for s in (0, 2, 3, 8):
        assert lib.iqpt_raster_create(0, 16, 16, s, C.byref(h)) == INVALID
    assert b"samples" in lib.iqpt_last_error()
    assert lib.iqpt_raster_create(1 << 20, 16, 16, 4, C.byref(h)) == NO_DEVICE     # no such device anywhere
    assert lib.iqpt_raster_create(-1, 16, 16, 4, C.byref(h)) == NO_DEVICE
    with pytest.raises(iqpt.IqptError):
        iqpt.Rasterizer(16, 16, samples=2)


def test_raster_entry_points_reject_null():
    lib = iqpt.load()
    cam = iqpt.make_camera(16, 16)
    assert lib.iqpt_raster_set_camera(None, C.byref(cam)) == INVALID
    assert lib.iqpt_raster_upload_scene(None, None) == INVALID
    assert lib.iqpt_raster_draw(None) == INVALID
    assert lib.iqpt_raster_draw_clip(None, None, None, 0, None, 0) == INVALID
    assert lib.iqpt_raster_read(None, None, None, None) == INVALID
    assert lib.iqpt_raster_copy_frame_device(None, None, 0) == INVALID
    assert lib.iqpt_raster_sync(None) == INVALID
    assert lib.iqpt_raster_time(None, None, None) == INVALID
    assert lib.iqpt_raster_destroy(None) == 0
    n = C.c_uint32()
    assert lib.iqpt_scene_draw_list(None, None, 0, C.byref(n)) == INVALID


def test_scene_draw_list_has_both_mesh_types_in_packet_order():
    sc = iqpt.Scene()
    sc.add_preset("app_default")
    red = sc.add_material(iqpt.MAT_OREN_NAYAR, [0.1, 0.2, 0.3], 0.5)
    sc.set_model_material("sph", red)
    dl = sc.draw_list()
    # by mesh name ("cube" < "sphere"), then insertion ("ground" before "sph")
    assert [d["mesh_type"] for d in dl] == [iqpt.MESH_TRIANGLES, iqpt.MESH_SPHERES, iqpt.MESH_SPHERES]
    assert [d["indices"].size // 3 for d in dl] == [12, 16128, 16128]
    assert np.allclose(dl[1]["transform"][3, :3], [0, -10, 0]) and np.allclose(dl[2]["transform"][3, :3], [0, 0.5, 0])
    assert np.array_equal(dl[0]["albedo"], np.array([1, 0, 0], np.float32))
    assert np.allclose(dl[2]["albedo"], [0.1, 0.2, 0.3])
    pk = sc.build_packet()
    assert np.array_equal(np.array(pk.tri_mesh_dcs[0].transform, np.float32).reshape(4, 4), dl[0]["transform"])
