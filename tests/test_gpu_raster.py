"""The HIP rasterizer against its numpy reference (tests/raster_ref.py): the BGRA bytes, the
per-sample depth bits and the per-sample primitive indices are compared for equality."""
import numpy as np
import pytest

import iqpt
import raster_ref as rr
from iqpt import Rasterizer, Scene, make_camera

pytestmark = pytest.mark.gpu

def to_clip(px, py, width, height, z=0.5, w=1.0):
    return [(px / width * 2 - 1) * w, (1 - py / height * 2) * w, z * w, w]


def tri_list(points, width, height):
    """Clip vertices, normals and indices of screen-space triangles [(x, y, z, w) * 3, ...], one normal each."""
    clip, nrm, idx = [], [], []
    for k, t in enumerate(points):
        for (x, y, z, w) in t:
            idx.append(len(clip))
            clip.append(to_clip(x, y, width, height, z, w))
            nrm.append([0.3 * np.sin(k + 1.0), 0.2 + 0.8 * np.cos(0.37 * k) ** 2, 0.1 * k])
    return (np.array(clip, np.float32).reshape(-1, 4), np.array(nrm, np.float32).reshape(-1, 3),
            np.array(idx, np.uint32))


def assert_same(got, want, what=""):
    bgra, depth, prim = got
    rb, rd, rp = want
    assert np.array_equal(prim, rp), f"{what}: {int(np.sum(prim != rp))} samples owned by another primitive"
    assert np.array_equal(depth.view(np.uint32), rd.view(np.uint32)), f"{what}: depth bits differ"
    assert np.array_equal(bgra, rb), f"{what}: {int(np.sum(np.any(bgra != rb, axis=2)))} pixels differ"


def draw_and_check(r, clip, nrm, idx, what=""):
    r.draw_clip(clip, nrm, idx)
    got = r.read(samples=True)
    want = rr.render_clip(clip, nrm, idx, r.width, r.height, r.samples)
    assert_same(got, want, what)
    assert np.array_equal(r.read(), got[0])
    return got


@pytest.fixture(scope="module", params=[1, 4])
def r16(request, require_gpu):
    with Rasterizer(16, 16, samples=request.param) as r:
        yield r


# ------------------------------------------------------------------------------------------------ 1. rules
def test_rule_shared_edge_and_top_left(r16):
    s = r16.samples
    first = 128 if s == 1 else 32
    # a quad on the sample lattice split along its diagonal: the shared edge runs through sample positions
    q = [((2 * 256 + first) / 256, (1 * 256 + first) / 256), ((13 * 256 + first) / 256, (3 * 256 + first) / 256),
         ((11 * 256 + first) / 256, (14 * 256 + first) / 256), ((1 * 256 + first) / 256, (9 * 256 + first) / 256)]
    v = [(x, y, 0.5, 1.0) for x, y in q]
    clip, nrm, idx = tri_list([(v[0], v[1], v[2]), (v[0], v[2], v[3])], 16, 16)
    _, _, prim = draw_and_check(r16, clip, nrm, idx, "shared edge")
    assert set(np.unique(prim)) == {0, 1, rr.NO_PRIM}
    # a rectangle whose sides lie exactly on sample positions keeps left and top, loses right and bottom
    off = 0.5 if s == 1 else 0.125
    l, rt, t, b = 2 + off, 6 + off, 3 + off, 7 + off
    v = [(l, t, 0.5, 1.0), (rt, t, 0.5, 1.0), (rt, b, 0.5, 1.0), (l, b, 0.5, 1.0)]
    clip, nrm, idx = tri_list([(v[0], v[1], v[2]), (v[0], v[2], v[3])], 16, 16)
    _, _, prim = draw_and_check(r16, clip, nrm, idx, "rectangle")
    ox, oy = rr.OFFSETS[s]
    py, px, sm = np.meshgrid(np.arange(16), np.arange(16), np.arange(s), indexing="ij")
    X, Y = px + 0.5 + ox[sm] / 256, py + 0.5 + oy[sm] / 256
    assert np.array_equal(prim != rr.NO_PRIM, (X >= l) & (X < rt) & (Y >= t) & (Y < b))


def test_rule_depth_order(r16):
    a = [(1, 1, 0.5, 1.0), (14, 2, 0.5, 1.0), (3, 13, 0.5, 1.0)]
    b = [(4, 0.5, 0.5, 1.0), (15, 8, 0.5, 1.0), (2, 15, 0.5, 1.0)]
    # equal depths: the first submission wins wherever both cover
    _, _, prim = draw_and_check(r16, *tri_list([a, b], 16, 16), "equal depth")
    only_a = draw_and_check(r16, *tri_list([a], 16, 16), "first alone")[2] == 0
    assert np.all(prim[only_a] == 0) and np.any(prim == 1)
    # LESS against a nearer and a farther triangle, in both orders
    near = [(x, y, 0.25, w) for x, y, _, w in b]
    far = [(x, y, 0.75, w) for x, y, _, w in b]
    for second, winner in ((near, 1), (far, 0)):
        _, _, prim = draw_and_check(r16, *tri_list([a, second], 16, 16), "a then b")
        both = only_a & (draw_and_check(r16, *tri_list([second], 16, 16))[2] == 0)
        assert np.any(both) and np.all(prim[both] == winner)
        _, _, prim = draw_and_check(r16, *tri_list([second, a], 16, 16), "b then a")
        assert np.all(prim[both] == 1 - winner)
    # slanted depths that cross inside the overlap
    c = [(1, 1, 0.1, 1.0), (14, 2, 0.9, 2.0), (3, 13, 0.5, 0.7)]
    d = [(4, 0.5, 0.9, 1.5), (15, 8, 0.2, 1.0), (2, 15, 0.6, 3.0)]
    draw_and_check(r16, *tri_list([c, d, a], 16, 16), "crossing depths")


def test_rule_culling(r16):
    front = [(2, 2, 0.5, 1.0), (12, 3, 0.5, 1.0), (5, 12, 0.5, 1.0)]
    back = [front[0], front[2], front[1]]                                  # counter-clockwise: culled
    flat = [(1, 1, 0.2, 1.0), (8, 8, 0.2, 1.0), (15, 15, 0.2, 1.0)]      # zero area
    point = [(4, 4, 0.1, 1.0)] * 3
    _, _, prim = draw_and_check(r16, *tri_list([back, flat, point, front], 16, 16), "culling")
    assert set(np.unique(prim)) == {3, rr.NO_PRIM}
    bgra, _, prim = draw_and_check(r16, *tri_list([back, flat], 16, 16), "all culled")
    assert np.all(prim == rr.NO_PRIM) and np.all(bgra == rr.CLEAR_BGRA)


def test_rule_uncovered_centre_is_extrapolated(require_gpu):
    # a sliver around sample 0 of pixel (5, 5), at (5.375, 5.125): the centre (5.5, 5.5) is outside it, the
    # attributes there are extrapolated; normals and w differ per vertex so the extrapolation shows
    t = [(5.30, 5.05, 0.4, 1.0), (5.45, 5.10, 0.5, 2.5), (5.36, 5.20, 0.6, 0.6)]
    clip, _, idx = tri_list([t], 16, 16)
    nrm = np.array([[0.2, 0.9, 0.1], [0.1, 0.2, 0.9], [0.9, 0.4, 0.0]], np.float32)
    with Rasterizer(16, 16, samples=4) as r:
        bgra, _, prim = draw_and_check(r, clip, nrm, idx, "extrapolated")
    assert list(prim[5, 5]) == [0, rr.NO_PRIM, rr.NO_PRIM, rr.NO_PRIM]
    assert np.sum(prim != rr.NO_PRIM) == 1 and not np.array_equal(bgra[5, 5], rr.CLEAR_BGRA)


# ------------------------------------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("size", [(1, 1), (17, 13), (65, 33)])
def test_shapes_edge_tiles(require_gpu, size, samples):
    w, h = size
    with Rasterizer(w, h, samples=samples) as r:
        # an empty scene: the clear colour only
        bgra, depth, prim = draw_and_check(r, np.zeros((0, 4)), np.zeros((0, 3)), np.zeros(0, np.uint32), "empty")
        assert np.all(bgra == rr.CLEAR_BGRA) and np.all(depth == 1.0) and np.all(prim == rr.NO_PRIM)
        # one triangle across every tile, a slanted one through it, and triangles wholly off-screen
        big = [(-1, -1, 0.6, 1.0), (2 * w + 2, -1, 0.6, 2.0), (-1, 2 * h + 2, 0.6, 0.5)]
        slant = [(0.2 * w, -2, 0.1, 1.0), (1.1 * w, 0.6 * h, 0.9, 1.0), (-0.3 * w, 1.2 * h, 0.5, 1.0)]
        off = [[(w + 3, 1, 0.5, 1.0), (w + 9, 2, 0.5, 1.0), (w + 4, 7, 0.5, 1.0)],
               [(1, -9, 0.5, 1.0), (5, -3, 0.5, 1.0), (0, -2, 0.5, 1.0)],
               [(-30, h + 2, 0.5, 1.0), (-2, h + 3, 0.5, 1.0), (-20, h + 40, 0.5, 1.0)]]
        _, _, prim = draw_and_check(r, *tri_list([big, slant] + off, w, h), "across every tile")
        assert np.all(prim != rr.NO_PRIM) and set(np.unique(prim)) <= {0, 1}
        bgra, _, _ = draw_and_check(r, *tri_list(off, w, h), "off-screen")
        assert np.all(bgra == rr.CLEAR_BGRA)


@pytest.mark.parametrize("samples", [1, 4])
def test_shapes_many_triangles_in_one_tile(require_gpu, samples):
    """300 small triangles inside one 8x8 tile of a 17x13 frame: a list longer than one 64-entry chunk."""
    rng = np.random.default_rng(5)
    tris = []
    for _ in range(300):
        c = rng.uniform([8.5, 0.5], [15.5, 7.5])
        p = c + rng.uniform(-1.2, 1.2, (3, 2))
        p = np.clip(p, [8.05, 0.05], [15.95, 7.95])
        if (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[2, 0] - p[0, 0]) * (p[1, 1] - p[0, 1]) <= 0:
            p = p[::-1]
        z = rng.choice([0.2, 0.4, 0.4, 0.6])                               # many equal depths
        tris.append([(q[0], q[1], z, rng.uniform(0.5, 2.0)) for q in p])
    with Rasterizer(17, 13, samples=samples) as r:
        _, _, prim = draw_and_check(r, *tri_list(tris, 17, 13), "300 in one tile")
        assert len(np.unique(prim)) > 30
        assert r.stats()["pairs"] == r.stats()["records"] > 200             # every record in the one tile


def test_shapes_stacked_layers(require_gpu):
    """3,000 full-frame layers over 64x64: every tile's list is 3,000 long, the record buffer has to grow past
    its first size, depths repeat so the submission order decides."""
    rng = np.random.default_rng(9)
    zs = rng.choice(np.linspace(0.05, 0.95, 40), 3000)
    tris = [[(-2, -2, z, 1.0), (140, -2, z, 1.0), (-2, 140, z, 1.0)] for z in zs]
    with Rasterizer(64, 64, samples=4) as r:
        _, _, prim = draw_and_check(r, *tri_list(tris, 64, 64), "3000 layers")
        assert np.all(prim == np.argmin(zs))                                # argmin: the first of the nearest
        assert r.stats() == {"triangles": 3000, "records": 3000, "pairs": 3000 * 64}


# ------------------------------------------------------------------------------------------------ 3. clipping
CLIP_CASES = {
    # clip-space vertices (x, y, z, w)
    "near plane": [(-0.6, -0.5, 0.3, 1.0), (0.1, 0.8, -0.4, 0.2), (0.7, -0.6, 0.5, 1.2)],
    "far plane": [(-0.6, -0.5, 0.3, 1.0), (0.2, 1.5, 2.6, 2.0), (0.7, -0.6, 0.5, 1.2)],
    "near and far": [(-1.5, -1.0, -0.5, 1.0), (0.0, 3.0, 4.0, 3.0), (1.5, -1.0, 1.3, 1.2)],
    "guard band": [(-0.8, 0.7, 0.5, 1.0), (2000.0, 0.9, 0.5, 1.0), (-0.7, -2000.0, 0.5, 1.0)],
    "guard band, far w": [(-800.0, 900.0, 0.5, 2.0), (1500.0, -100.0, 0.2, 1.0), (-900.0, -2400.0, 0.9, 1.5)],
    "behind the camera": [(-0.5, -0.5, -0.3, -1.0), (0.0, 0.5, -0.2, -0.5), (0.5, -0.5, -0.1, -2.0)],
    "w = 0 vertex": [(-0.6, -0.5, 0.3, 1.0), (0.3, 0.9, -0.01, 0.0), (0.7, -0.6, 0.5, 1.2)],
    "origin vertex": [(-0.6, -0.5, 0.3, 1.0), (0.0, 0.0, 0.0, 0.0), (0.7, -0.6, 0.5, 1.2)],
    "not finite": [(-0.6, -0.5, 0.3, 1.0), (np.inf, 0.9, 0.5, 1.0), (0.7, np.nan, 0.5, 1.2)],
}


@pytest.mark.parametrize("samples", [1, 4])
def test_clipping(require_gpu, samples):
    w, h = 24, 16
    nrm = np.array([[0.1, 0.9, 0.2], [0.7, 0.5, 0.1], [0.0, 0.3, 0.9]], np.float32)
    idx = np.arange(3, dtype=np.uint32)
    cases = CLIP_CASES
    drawn = {}
    with Rasterizer(w, h, samples=samples) as r:
        for name, verts in cases.items():
            for order in ((0, 1, 2), (0, 2, 1)):                           # one of the two windings faces the camera
                clip = np.array([verts[k] for k in order], np.float32)
                _, _, prim = draw_and_check(r, clip, nrm, idx, name)
                drawn[name] = drawn.get(name, 0) + int(np.sum(prim == 0))
        # every case at once, behind a far full-frame triangle
        clip = np.array([v for verts in cases.values() for v in verts] +
                        [(-3.0, 3.0, 0.99, 1.0), (3.0, 3.0, 0.99, 1.0), (-3.0, -3.0, 0.99, 1.0)], np.float32)
        nn = np.tile(nrm, (len(cases) + 1, 1))
        draw_and_check(r, clip, nn, np.arange(clip.shape[0], dtype=np.uint32), "all clipping cases")
    for name in ("near plane", "far plane", "near and far", "guard band", "guard band, far w", "w = 0 vertex"):
        assert drawn[name] > 0, f"{name}: nothing was drawn"
    for name in ("behind the camera", "origin vertex", "not finite"):
        assert drawn[name] == 0, name


# ------------------------------------------------------------------------------------------------ 4. scenes
def material_scene():
    sc = Scene()
    sc.add_preset("cornell")
    sc.set_model_material("left", sc.add_material(iqpt.MAT_OREN_NAYAR, [0.65, 0.05, 0.05], 0.5))
    sc.set_model_material("right", sc.add_material(iqpt.MAT_OREN_NAYAR, [0.12, 0.45, 0.15], 0.5))
    sc.set_model_material("sphere_big", sc.add_material(iqpt.MAT_EMISSIVE, [0.9, 0.8, 2.0], 3.0))
    return sc


def preset_scene(name):
    sc = Scene()
    sc.add_preset(name)
    return sc


SCENES = {"cornell": lambda: preset_scene("cornell"), "app_default": lambda: preset_scene("app_default"),
          "materials": material_scene}
_scene_refs = {}


def scene_ref(name, samples):
    """The reference frame of a scene at 96x54, computed once and shared."""
    key = (name, samples)
    if key not in _scene_refs:
        out = rr.render_scene(SCENES[name]().draw_list(), make_camera(96, 54), 96, 54, samples)
        for a in out:
            a.setflags(write=False)
        _scene_refs[key] = out
    return _scene_refs[key]


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("name", ["cornell", "app_default", "materials"])
def test_scenes(require_gpu, name, samples):
    sc = SCENES[name]()
    with Rasterizer(96, 54, samples=samples) as r:
        r.set_camera(make_camera(96, 54))
        r.upload_scene(sc)
        r.draw()
        got = r.read(samples=True)
    want = scene_ref(name, samples)
    assert_same(got, want, name)
    assert np.mean(got[2] != rr.NO_PRIM) > 0.25
    if name == "materials":
        plain = scene_ref("cornell", samples)
        assert np.array_equal(got[2], plain[2]) and not np.array_equal(got[0], plain[0])   # same geometry, other colours


# ------------------------------------------------------------------------------------------------ 6. state
def test_determinism_and_state(require_gpu):
    cam_a = make_camera(96, 54)
    cam_b = make_camera(96, 54, position=[0.8, 1.0, -2.5, 0.0], forward=[-0.3, -0.4, 1.0, 0.0])

    def fresh(scene_name, cam):
        with Rasterizer(96, 54) as q:
            q.set_camera(cam)
            q.upload_scene(SCENES[scene_name]())
            q.draw()
            return q.read(samples=True)

    with Rasterizer(96, 54) as r:
        r.set_camera(cam_a)
        r.upload_scene(SCENES["cornell"]())
        r.draw()
        first = r.read(samples=True)
        r.draw()
        assert_same(r.read(samples=True), first, "second draw")
        assert_same(first, scene_ref("cornell", 4), "cornell")
        r.set_camera(cam_b)
        r.draw()
        moved = r.read(samples=True)
        assert not np.array_equal(moved[0], first[0])
        assert_same(moved, fresh("cornell", cam_b), "after set_camera")
        r.upload_scene(SCENES["app_default"]())
        r.draw()
        assert_same(r.read(samples=True), fresh("app_default", cam_b), "after a second upload_scene")
        # a draw_clip in between leaves the uploaded scene in place
        r.draw_clip(np.zeros((0, 4)), np.zeros((0, 3)), np.zeros(0, np.uint32))
        assert np.all(r.read() == rr.CLEAR_BGRA)
        r.draw()
        assert_same(r.read(samples=True), fresh("app_default", cam_b), "after draw_clip")
        ms, n = r.time()
        assert n == 6 and ms > 0.0


def test_not_ready_and_frame_copy(require_gpu):
    import torch
    with Rasterizer(16, 16) as r:
        with pytest.raises(iqpt.IqptError) as e:
            r.draw()
        assert e.value.status == 5                                          # IQPT_ERR_NOT_READY
        with pytest.raises(iqpt.IqptError):
            r.read()
        r.draw_clip(*tri_list([[(1, 1, 0.5, 1.0), (14, 2, 0.5, 1.0), (3, 13, 0.5, 1.0)]], 16, 16))
        dst = torch.zeros(16 * 16, dtype=torch.int32, device="cuda")
        r.copy_frame_device(dst.data_ptr(), 16 * 16 * 4)
        assert np.array_equal(dst.cpu().numpy().view(np.uint8).reshape(16, 16, 4), r.read())
