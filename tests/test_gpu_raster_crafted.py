"""The rasterizer's scene path on a crafted scene, bit for bit against tests/denoise_ref.py (G-buffer) and
tests/raster_ref.py (draw). The preset scenes have at most a dozen models and reach iqr_setup_kernel<true> and
iqr_guide_tile_kernel at 96x54 only; here:

  77 models, so that find_draw searches a long table in the vertex and in the set-up kernel;
  one cube mesh shared by 66 of them, a custom pyramid mesh shared by 10, and between the two (in mesh-name order,
  which is draw order) an empty mesh with a model of its own: the id of a pixel is the model's position in
  Scene.draw_list(), not in the table of the models that have triangles;
  rotations about all three axes and non-uniform scales; one model with a singular transform (a cube scaled by 0 in y);
  every model inside a scaled cube, the first of the draw list, which only the two-sided G-buffer sees from inside;
  two cameras, one of them among the models with its near plane at 0.6, which cuts many of their triangles;
  frames of 1x1, 17x13 and 65x33: smaller than a tile, ragged tiles, more than one block of tiles."""
import numpy as np
import pytest

import denoise_ref as dr
import raster_ref as rr
from iqpt import Rasterizer, Scene, make_camera

NO = dr.NO_PRIM
FRAMES = [(1, 1), (17, 13), (65, 33)]
CAMERAS = {
    "outside": dict(),
    "among": dict(fovh=70.0, znear=0.6, zfar=40.0, position=[0.1, 0.2, -0.9, 0.0], forward=[0.15, -0.3, 1.0, 0.0]),
}
N_MODELS = 77


def crafted():
    sc = Scene()
    sc.add_mesh_cube("a_cube")
    empty = True
    try:
        sc.add_mesh("b_empty", np.zeros((0, 6), np.float32), np.zeros(0, np.uint32))
    except Exception:
        empty = False                    # the builder refuses an empty mesh: the scene goes without one
    apex, base = (0.0, 1.0, 0.0), [(-1.0, 0.0, -1.0), (1.0, 0.0, -1.0), (1.0, 0.0, 1.0), (-1.0, 0.0, 1.0)]
    v, idx = [], []
    for k in range(4):                   # four flat sides, clockwise seen from outside, and no floor
        a, b = np.array(base[k]), np.array(base[(k + 1) % 4])
        n = np.cross(np.array(apex) - a, b - a)
        n = n / np.linalg.norm(n)
        n = n if np.dot(n, (a + b) / 2) > 0 else -n
        for p in (apex, b, a):
            v.append([*p, *n])
        idx += [3 * k, 3 * k + 1, 3 * k + 2]
    sc.add_mesh("c_pyramid", np.array(v, np.float32), np.array(idx, np.uint32))
    sc.add_model("room", "a_cube", scale=(7.0, 4.0, 9.0, 0.0), rotation=(0.0, 0.2, 0.0, 0.0))
    for k in range(2):
        for j in range(4):
            for i in range(8):
                sc.add_model(f"box{k}{j}{i}", "a_cube", scale=(0.12 + 0.01 * i, 0.08 + 0.02 * j, 0.15, 0.0),
                             rotation=(0.3 * i, 0.2 * j, 0.5 * k + 0.1, 0.0),
                             translation=(-1.75 + 0.5 * i, -0.75 + 0.5 * j, 0.6 * k, 0.0))
    sc.add_model("flat", "a_cube", scale=(0.5, 0.0, 0.5, 0.0), translation=(0.0, 1.0, 0.3, 0.0))
    if empty:
        sc.add_model("hole", "b_empty", scale=1.0)
    for i in range(10):
        sc.add_model(f"spire{i}", "c_pyramid", scale=(0.1, 0.2 + 0.02 * i, 0.1, 0.0), rotation=(0.0, 0.4 * i, 0.05 * i, 0.0),
                     translation=(-1.3 + 0.28 * i, -0.45, -1.2, 0.0))
    return sc, empty


_refs = {}


def reference(name, w, h):
    """(the scene, G-buffer reference, draw reference at 1 sample) of a camera and frame, computed once and shared."""
    key = (name, w, h)
    if key not in _refs:
        sc, empty = crafted()
        items = sc.draw_list()
        cam = make_camera(w, h, **CAMERAS[name])
        g = dr.gbuffer_scene(items, cam, w, h)
        d = rr.render_scene(items, cam, w, h, 1)
        for a in g + d:
            a.setflags(write=False)
        _refs[key] = (sc, empty, items, cam, g, d)
    return _refs[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_the_scene_is_what_it_says():
    """No GPU: the draw list's order and the references' coverage, so that the GPU test below compares what it means to."""
    sc, empty, items, cam, (nz, ids), (_, _, prim) = reference("outside", 65, 33)
    assert len(items) == N_MODELS - (0 if empty else 1)
    counts = [d["indices"].size // 3 for d in items]
    assert counts[0] == 12 and counts[-1] == 4 and counts[:66] == [12] * 66
    if empty:
        assert counts[66] == 0 and counts[67:] == [4] * 10
    seen = set(np.unique(ids).tolist())
    assert 0 in seen and len(items) - 1 in seen and NO not in seen       # the room closes the view
    assert len(seen) > 40
    assert not (empty and 66 in seen)
    draw_of_tri = np.concatenate([np.full(n, k) for k, n in enumerate(counts)])
    drawn = set(np.unique(draw_of_tri[prim[prim != rr.NO_PRIM]]).tolist())
    assert 0 not in drawn and len(items) - 1 in drawn and len(drawn) > 40   # CULL_BACK does not see the room from inside
    # the near plane of the camera among the models cuts triangles: pixels at depth 0 would be clamped ones; what
    # shows the cut is geometry on both sides of the plane
    _, _, items, cam, (nz, ids), _ = reference("among", 65, 33)
    view = np.array(cam.view, np.float64).reshape(4, 4)
    cut = 0
    for d in items:
        if d["indices"].size == 0:
            continue
        p = np.concatenate([d["vertices"][:, :3].astype(np.float64), np.ones((d["vertices"].shape[0], 1))], axis=1)
        z = (p @ d["transform"].astype(np.float64) @ view)[:, 2][d["indices"].reshape(-1, 3).astype(np.int64)]
        cut += int(np.sum((z.min(axis=1) < 0.6) & (z.max(axis=1) > 0.6)))
    assert cut >= 20
    assert len(np.unique(ids)) > 10


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", FRAMES)
@pytest.mark.parametrize("name", list(CAMERAS))
def test_crafted_scene(require_gpu, name, w, h):
    sc, empty, items, cam, want_g, want_d = reference(name, w, h)
    with Rasterizer(w, h, samples=1) as r:
        r.set_camera(cam)
        r.upload_scene(sc)
        nz, ids = r.gbuffer()
        r.draw()
        got = r.read(samples=True)
    assert np.array_equal(ids, want_g[1]), f"{int(np.sum(ids != want_g[1]))} ids differ"
    same = bits(nz) == bits(want_g[0])
    both_nan = np.isnan(nz) & np.isnan(want_g[0])          # the singular model's normals: any NaN is the NaN
    assert np.all(same | both_nan), f"{int(np.sum(~np.all(same | both_nan, axis=2)))} normal/depth pixels differ"
    assert np.array_equal(got[2], want_d[2]), f"{int(np.sum(got[2] != want_d[2]))} samples owned by another primitive"
    assert np.array_equal(got[1].view(np.uint32), want_d[1].view(np.uint32)), "depth bits differ"
    assert np.array_equal(got[0], want_d[0]), f"{int(np.sum(np.any(got[0] != want_d[0], axis=2)))} pixels differ"
    if (w, h) == (65, 33) and name == "outside":
        seen = set(np.unique(ids).tolist())
        assert 0 in seen and len(items) - 1 in seen


@pytest.mark.gpu
def test_crafted_scene_four_samples(require_gpu):
    """The draw at 4 samples per pixel (the G-buffer does not depend on the sample count)."""
    w, h = 17, 13
    sc, empty, items, cam, want_g, _ = reference("among", w, h)
    want = rr.render_scene(items, cam, w, h, 4)
    with Rasterizer(w, h, samples=4) as r:
        r.set_camera(cam)
        r.upload_scene(sc)
        r.draw()
        got = r.read(samples=True)
        nz, ids = r.gbuffer()
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(ids, want_g[1])
