"""Certain hits beside a sphere (iqpt_certain_kernel's third plane), on the host build of
csrc/iq_interval.h, no GPU. The rule is restated in tests/certain_beside.py from iqpt_debug_cull_tile and
iqpt_debug_certain_tile per pixel: a pixel of a tile WITH a sphere candidate is marked when the tile has at most 96
candidate pairs, the pixel's own bundle is ok and culls every sphere of the tile's candidate pairs, and some candidate
triangle is tri_certain on it.

* Soundness against the oracle's intersectors, on scenes placed from the camera's own rays, for test_cull.py's
  cameras: for every marked pixel, its four corner jitters (test_cull.state_with_outputs through corner_rays) and
  random jitters, iqo_sphere_intersect rejects every sphere and iqo_triangle_intersect (t_min 1e-6, t_max 999.99)
  accepts some triangle. Each class of placement must occur and yield what is stated below.
* Reach on the bench frame (C2, 1920 x 1080): the counts of marked pixels and of fully marked tiles.
* On a 16-spp oracle frame every marked pixel traced exactly one ray per sample and holds 1.0f in each channel."""
import functools

import numpy as np
import pytest

import oracle
from certain_beside import (MARKED, MISS, SEAM, SPHERE, beside_masks, beside_tile, folds, lane_pixels, packet_primitives,
                            tile_grid)
from iqpt import Scene, make_camera, pixel_set
from proof_masks import TILE
from test_certain import T_MAX, Footprint, W, H, as_v0e1e2, certain_tile, covering
from test_cull import CAMERAS, corner_rays, sph_hit, tile_rays, tri_hit

RADII = [1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3]
CLASSES = ["tangent_outside", "tangent_inside", "tiny_in_footprint", "camera_inside", "behind_camera", "before_seam"] + \
          [f"radius_{r:g}" for r in RADII]
N_RANDOM_JITTERS = 3


def reach(cls):
    """Tiles on each side of the target's that a class looks at: a pixel's bundle culls a sphere a few pixels wide
    only some tens of pixels from it (the angle of about sqrt(2 x the pixel's width))."""
    return 3 if cls == "before_seam" else 1


def neighbourhood(ps, x, y, k):
    """The (2 k + 1) x (2 k + 1) tiles around pixel (x, y) of a full frame."""
    _, ntx, _ = tile_grid(ps)
    tx, ty = x // TILE, y // TILE
    return [(ty + j) * ntx + tx + i for j in range(-k, k + 1) for i in range(-k, k + 1)]


def place(cls, cam, x, y, rng):
    """Triangles (vertex triples) and spheres (centre, radius) of one class around the target pixel (x, y)."""
    fp = Footprint(cam, x, x, y, y, 0, rng)
    m = TILE * reach(cls) + TILE
    fn = Footprint(cam, x - m, x + m, y - m, y + m, 0, rng)          # the neighbourhood's bundle
    a, b = fp.basis(fp.dc)
    _, rho1 = fp.on_plane(fp.oc + fp.dc, fp.dc)                      # the pixel's footprint radius at distance 1
    t = max(4.0, 4e-3 / rho1) if cls == "tiny_in_footprint" else 4.0
    c, rho = fp.on_plane(fp.oc + t * fp.dc, fp.dc)
    o, d = (v[:3].astype(np.float64) for v in corner_rays(cam, x, x, y, y, rng)[0])   # jitter (-0.5, -0.5)
    corner = o + (((c - o) @ fp.dc) / (d @ fp.dc)) * d               # the corner ray's point on the plane through c
    inward = (c - corner) - ((c - corner) @ d) / (d @ d) * d         # towards the pixel's centre, square to the ray
    inward /= np.linalg.norm(inward)
    wall_t = 2.0 * t
    if cls == "before_seam":
        # a quad of two triangles whose shared diagonal runs through the target pixel's central ray
        cw, rw = fn.on_plane(fp.oc + wall_t * fp.dc, fp.dc)
        p = [cw + 3.0 * rw * (sa * a + sb * b) for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        tris = [np.array([p[0], p[1], p[2]]), np.array([p[0], p[2], p[3]])]
        sph = [np.append(fp.oc + t * fp.dc, 3.0 * rho)]
    else:
        tris = [covering(fn, rng, wall_t, 2.0, max_tilt=20.0)]
        if cls == "tangent_outside":
            r = 40.0 * rho                                           # (wide: a pixel's cull is tight beside it)
            sph = [np.append(corner - r * inward, r)]
        elif cls == "tangent_inside":
            r = 0.3 * rho
            sph = [np.append(corner + r * inward, r)]
        elif cls == "tiny_in_footprint":
            sph = [np.append(c + 0.2 * rho * a, 1e-3)]
        elif cls == "camera_inside":
            sph = [np.append(fp.oc + 0.3 * 50.0 * a, 50.0)]
        elif cls == "behind_camera":
            sph = [np.append(fp.oc - 4.0 * 0.5 * fp.fwd, 0.5)]
        else:
            r = float(cls.split("_")[1])
            sph = [np.append(c + (r + 6.0 * rho) * a, r)]            # its silhouette six pixel radii from the pixel
    return tris, np.asarray(sph, np.float32).reshape(-1, 4)


def check_sound(cam, pixels, tris, sph4, rng):
    """Every ray of every marked pixel: no sphere accepted, some triangle accepted with the kernel's t range."""
    for x, y in pixels:
        for o, d in tile_rays(cam, x, x, y, y, N_RANDOM_JITTERS, rng):      # random jitters, then the four corners
            for s in sph4:
                assert not sph_hit(s[:3], s[3], o, d), ("a marked pixel's ray hits a sphere", (x, y), s)
            assert any(tri_hit(v[0], v[1], v[2], o, d, t_max=T_MAX) for v in tris), \
                ("a marked pixel's ray hits no triangle", (x, y))


@pytest.mark.parametrize("ci", range(len(CAMERAS)))
def test_marked_pixels_are_sound_and_classes_yield_what_they_should(ci):
    rng = np.random.default_rng(4100 + ci)
    cam = make_camera(W, H, **CAMERAS[ci])
    ps = pixel_set(W, H)
    seen = {}
    for k, cls in enumerate(CLASSES):
        x, y = TILE * (6 + 2 * k) + int(rng.integers(TILE)), TILE * (4 + k) + int(rng.integers(TILE))
        tris, sph4 = place(cls, cam, x, y, rng)
        tris32 = [np.asarray(v, np.float32) for v in tris]
        tris9 = np.stack([as_v0e1e2(v) for v in tris32])
        n = {MARKED: 0, SPHERE: 0, SEAM: 0, MISS: 0, "tiles": 0}
        marked, target = [], None
        for t in neighbourhood(ps, x, y, reach(cls)):
            r = beside_tile(cam, ps, t, tris9, sph4)
            if r is None:
                continue
            n["tiles"] += 1
            for kind in (MARKED, SPHERE, SEAM, MISS):
                n[kind] += int((r[1] == kind).sum())
            marked += lane_pixels(ps, t, r[0])
            if t == (y // TILE) * tile_grid(ps)[1] + x // TILE:
                target = int(r[1][(y % TILE) * TILE + x % TILE])
        assert len(marked) == n[MARKED]
        check_sound(cam, marked, tris32, sph4, rng)
        seen[cls] = n
        print(cls, (x, y), "target", target, n)
        if cls == "behind_camera":
            # culled for every tile's bundle: no tile is the rule's (they are the tile rule's, whose proof holds)
            assert n["tiles"] == 0 and certain_tile(cam, x, x, y, y, tris9)[1].any(), n
            continue
        assert target is not None, n                       # the target's tile keeps the sphere: the rule's domain
        if cls == "camera_inside":
            assert n["tiles"] == 9 and n[SPHERE] == 9 * TILE * TILE, n    # every ray hits it: no pixel is marked
        elif cls in ("tangent_inside", "tiny_in_footprint"):
            assert target == SPHERE, (target, n)           # the pixel that holds it (as the pixels around: see reach)
        elif cls == "tangent_outside":
            assert n[MARKED] > 0 and n[SPHERE] > 0, n
        elif cls == "before_seam":
            assert n[MARKED] > 0 and n[SPHERE] > 0 and n[SEAM] > 0, n
    radii = [seen[c] for c in CLASSES if c.startswith("radius_")]
    assert len(radii) == len(RADII) and all(r[SPHERE] > 0 for r in radii), radii
    assert sum(r[MARKED] for r in radii) > 0, radii
    assert seen["camera_inside"][MARKED] == 0 and seen["behind_camera"][MARKED] == 0


# ------------------------------------------------------------------ the bench frame

BENCH_W, BENCH_H = 1920, 1080
EXPECT_MARKED, EXPECT_FULL_TILES = 59903, 740
# of those, the pixels of the tiles that fold theirs (at least half a tile marked): what bench.py --full reports as
# certain pixels is the tile rule's 1,016,215 plus these
EXPECT_FOLDED, EXPECT_FOLDING_TILES = 58603, 962


@functools.lru_cache(maxsize=None)
def bench_marks():
    """C2's marked pixels over its sphere-candidate tiles: (scene, packet, camera, {tile: mask}, per-tile kinds)."""
    sc = Scene()
    sc.add_preset("cornell")
    pk = sc.build_packet()
    cam = make_camera(BENCH_W, BENCH_H)
    tris9, sph4 = packet_primitives(pk)
    plane, kinds = beside_masks(cam, pixel_set(BENCH_W, BENCH_H), tris9, sph4)
    plane.setflags(write=False)
    return sc, pk, cam, plane, kinds


def test_reach_on_the_bench_frame():
    _sc, _pk, _cam, plane, kinds = bench_marks()
    n = sum(bin(int(v)).count("1") for v in plane)
    full = sum(int(v) == (1 << 64) - 1 for v in plane)
    no_sphere = sum(not (k == SPHERE).any() for k in kinds.values())
    seam = sum(int((k == SEAM).sum()) for k in kinds.values())
    sphere = sum(int((k == SPHERE).sum()) for k in kinds.values())
    print(f"sphere-candidate tiles {len(kinds)}, marked pixels {n}, fully marked tiles {full}, tiles without a pixel "
          f"that can reach a sphere {no_sphere}, seam pixels {seam}, pixels that may reach a sphere {sphere}")
    folding = [int(v) for v in plane if int(v) and folds(v, 64)]
    nfold = sum(bin(v).count("1") for v in folding)
    print(f"tiles that fold their marked pixels {len(folding)}, holding {nfold} of them")
    assert len(kinds) == 2665
    assert n == EXPECT_MARKED and full == EXPECT_FULL_TILES
    assert nfold == EXPECT_FOLDED and len(folding) == EXPECT_FOLDING_TILES


def test_marked_pixels_of_the_bench_frame_are_one_ray_white_in_the_oracle():
    _sc, pk, cam, plane, kinds = bench_marks()
    ps_full = pixel_set(BENCH_W, BENCH_H)
    marked = np.array([p for t in kinds for p in lane_pixels(ps_full, t, plane[t])], np.int64)
    assert len(marked) > 0
    # the oracle over the marked pixels' bounding box only
    x0, x1 = int(marked[:, 0].min()), int(marked[:, 0].max()) + 1
    y0, y1 = int(marked[:, 1].min()), int(marked[:, 1].max()) + 1
    spp = 16
    fr = oracle.OracleFrame(BENCH_W, BENCH_H, pixels=pixel_set(BENCH_W, BENCH_H, x0, x1, y0, 1, y1 - y0), max_depth=8)
    fr.render(pk, cam, spp)
    idx = (marked[:, 1] - y0) * (x1 - x0) + (marked[:, 0] - x0)
    assert np.array_equal(np.asarray(fr.rays).reshape(-1)[idx], np.full(len(idx), spp))
    assert (fr.lin[idx, :3].view(np.uint32) == np.float32(1.0).view(np.uint32)).all()
