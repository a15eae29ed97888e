"""Soundness of the per-pixel camera-ray proofs on the host build of csrc/iq_interval.h (DESIGN.md §3.3, §3.12,
§3.15): tri_certain ("every camera ray of the bundle hits this triangle as a first hit") and tri_culled /
sphere_culled on single-pixel bundles (the certain-miss proof and the per-pixel candidate masks), against the
oracle's intersection routines.

Every ray set holds the bundle's corner rays: the corner pixels with the jitter pairs (-0.5 | +0.5, -0.5 | +0.5),
drawn from XORWOW states constructed so that their first two outputs are 0 or 2^32 - 1 (test_cull.corner_rays),
plus random pixels and jitters. Primitives are placed from the bundle's own rays, class by class, so that both
outcomes and the near misses occur; each test asserts the outcome counts of the classes that are meant to produce
one. tests/test_gpu_proofs.py then checks that the device build computes the same masks as this host build, word
for word."""
import ctypes as C

import numpy as np
import pytest

import oracle
from iqpt import _lib, make_camera
from test_cull import (CAMERAS, FP, M32, U8, UP, corner_rays, cull_tile, random_prims, sph_hit,
                       state_with_outputs, tile_rays, tri_hit)

T_MAX = np.float32(999.99)           # the kernel's kTMax: the closest hit a ray starts with (path_tracer.cu:241)
EPS = np.float32(0.000001)           # is_zero's bound on |det| (iqmath.h:28-31)
W, H = 320, 180
F32 = np.float32


def certain_tile(cam, xa, xb, ya, yb, tris9):
    lib = _lib.load()
    f = lib.iqpt_debug_certain_tile
    f.argtypes = [C.POINTER(type(cam)), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, FP, C.c_uint32, U8]
    f.restype = C.c_int
    tris9 = np.ascontiguousarray(tris9, dtype=np.float32).reshape(-1, 9)
    out = np.zeros(len(tris9), np.uint8)
    ok = f(C.byref(cam), xa, xb, ya, yb, tris9.ctypes.data_as(FP), len(tris9), out.ctypes.data_as(U8))
    assert ok >= 0, lib.iqpt_last_error()
    return ok == 1, out.astype(bool)


def camera(ci):
    """The three cameras of test_cull.py and a fourth whose cam_constants take the non-constant path (w of the
    unprojected points varies over the frame). make_camera cannot produce one: the inverse of its perspective
    matrix always has inv_proj[3] == inv_proj[7] == 0, which is cam_constants' condition together with finite
    non-zero inv_proj[11], [15]. The fourth camera is the second with those two entries set by hand, to +10 % and
    -5 % of the far point's w at the frame's centre; the oracle's camera_get_ray divides by the w it computes, so
    it follows."""
    if ci < len(CAMERAS):
        cam = make_camera(W, H, **CAMERAS[ci])
        assert cam.inv_proj[3] == 0.0 and cam.inv_proj[7] == 0.0
        return cam
    cam = make_camera(W, H, **CAMERAS[1])
    wf = cam.inv_proj[11] + cam.inv_proj[15]
    cam.inv_proj[3] = 0.1 * wf
    cam.inv_proj[7] = -0.05 * wf
    return cam


NCAM = len(CAMERAS) + 1


def test_corner_states_give_the_extreme_jitters():
    """The constructed states' first two outputs are the chosen ones (checked with iqo_xorwow_next inside
    state_with_outputs) and random::real maps them to -0.5 and +0.5 exactly."""
    lib = oracle.load()
    rng = np.random.default_rng(5)
    for r1 in (0, M32, 12345):
        for r2 in (0, M32, 0x80000000):
            st = state_with_outputs(r1, r2, rng)
            a = lib.iqo_real(st.ctypes.data_as(UP), -0.5, 0.5)
            b = lib.iqo_real(st.ctypes.data_as(UP), -0.5, 0.5)
            for r, u in ((r1, a), (r2, b)):
                if r == 0:
                    assert u == -0.5
                elif r == M32:
                    assert u == 0.5
                else:
                    assert -0.5 < u < 0.5
    # a pixel's corner rays differ from each other and span its random rays' origins
    cam = camera(0)
    cr = corner_rays(cam, 17, 17, 40, 40, rng)
    assert len(cr) == 4 and len({tuple(d) for _, d in cr}) == 4
    assert len(corner_rays(cam, 8, 15, 16, 23, rng)) == 16


# ------------------------------------------------------------------ geometry from a bundle's own rays

class Footprint:
    """A bundle's rays (random ones plus the corner rays) and its footprint on a plane, in float64."""

    def __init__(self, cam, xa, xb, ya, yb, nrand, rng):
        self.box = (xa, xb, ya, yb)
        self.rays = tile_rays(cam, xa, xb, ya, yb, nrand, rng)
        cr = corner_rays(cam, xa, xb, ya, yb, rng)
        self.co = np.array([o[:3] for o, _ in cr], np.float64)
        self.cd = np.array([d[:3] for _, d in cr], np.float64)
        self.oc = self.co.mean(0)
        dc = self.cd.mean(0)
        self.dc = dc / np.linalg.norm(dc)
        f = np.array(cam.forward[:3], np.float64)
        self.fwd = f / np.linalg.norm(f)

    def basis(self, n):
        a = np.cross(n, [0.31, 0.95, 0.11])
        a /= np.linalg.norm(a)
        return a, np.cross(n, a)

    def on_plane(self, x0, n):
        """Where the central ray meets the plane (x0, n), and the largest distance of a corner ray's point from it."""
        s = ((x0 - self.co) @ n) / (self.cd @ n)
        p = self.co + s[:, None] * self.cd
        c = self.oc + (((x0 - self.oc) @ n) / (self.dc @ n)) * self.dc
        return c, float(np.max(np.linalg.norm(p - c, axis=1)))

    def tilted(self, rng, max_deg):
        """A unit normal within max_deg of the central ray."""
        a, b = self.basis(self.dc)
        th = np.radians(rng.uniform(0, max_deg))
        ph = rng.uniform(0, 2 * np.pi)
        return np.cos(th) * self.dc + np.sin(th) * (np.cos(ph) * a + np.sin(ph) * b)


def regular(c, n, inradius, rot, fp):
    a, b = fp.basis(n)
    r = 2.0 * inradius
    return np.array([c + r * (np.cos(rot + k * 2 * np.pi / 3) * a + np.sin(rot + k * 2 * np.pi / 3) * b)
                     for k in range(3)])


def loguni(rng, lo, hi):
    return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))


def covering(fp, rng, t, margin, max_tilt=50.0):
    """A triangle whose inscribed circle, seen from the camera, has `margin` times the footprint's radius."""
    n = fp.tilted(rng, max_tilt)
    c, rho = fp.on_plane(fp.oc + t * fp.dc, n)
    return regular(c, n, margin * rho / abs(n @ fp.dc), rng.uniform(0, 2 * np.pi), fp)


def edge_through(fp, rng):
    """One edge runs through the footprint; the triangle extends 15 footprint radii to one side of it."""
    n = fp.tilted(rng, 40.0)
    c, rho = fp.on_plane(fp.oc + loguni(rng, 0.05, 200.0) * fp.dc, n)
    a, b = fp.basis(n)
    ph, ps = rng.uniform(0, 2 * np.pi, 2)
    q = c + rng.uniform(0, 0.5) * rho * (np.cos(ph) * a + np.sin(ph) * b)
    e, m = np.cos(ps) * a + np.sin(ps) * b, -np.sin(ps) * a + np.cos(ps) * b
    return np.array([q - 15 * rho * e, q + 15 * rho * e, q + 15 * rho * m])


def vertex_inside(fp, rng):
    """One vertex lies inside the footprint; the triangle opens 60 degrees away from it."""
    n = fp.tilted(rng, 40.0)
    c, rho = fp.on_plane(fp.oc + loguni(rng, 0.05, 200.0) * fp.dc, n)
    a, b = fp.basis(n)
    ph, ps = rng.uniform(0, 2 * np.pi, 2)
    q = c + rng.uniform(0, 0.5) * rho * (np.cos(ph) * a + np.sin(ph) * b)
    e1 = np.cos(ps + np.pi / 6) * a + np.sin(ps + np.pi / 6) * b
    e2 = np.cos(ps - np.pi / 6) * a + np.sin(ps - np.pi / 6) * b
    return np.array([q, q + 20 * rho * e1, q + 20 * rho * e2])


def mt_det(vs, d):
    """The Möller–Trumbore determinant as the reference evaluates it (shape.cu:65-70), in binary32 steps."""
    e1, e2 = vs[1] - vs[0], vs[2] - vs[0]
    px = F32(F32(d[1] * e2[2]) - F32(d[2] * e2[1]))
    py = F32(F32(d[2] * e2[0]) - F32(d[0] * e2[2]))
    pz = F32(F32(d[0] * e2[1]) - F32(d[1] * e2[0]))
    return F32(F32(F32(e1[0] * px) + F32(e1[1] * py)) + F32(e1[2] * pz))


def land_det(vs, d, rel):
    """Scale the edge v0 -> v2 until |det| for the ray direction d is (1 + rel) * 1e-6, as closely as the
    vertices' own rounding allows. Returns the float32 vertices and the deviation reached, |det| / 1e-6 - 1."""
    vs = np.asarray(vs, np.float64)
    for _ in range(8):
        v32 = vs.astype(np.float32)
        det = float(abs(mt_det(v32, d)))
        if det == 0.0 or not np.isfinite(det):
            break
        vs[2] = vs[0] + (vs[2] - vs[0]) * (1e-6 * (1.0 + rel) / det)
    v32 = vs.astype(np.float32)

    def dev(v):
        return float(abs(mt_det(v, d))) / float(EPS) - 1.0

    # the vertices' rounding decides the last digits: step single coordinates of v1 and v2 by an ulp while it helps
    best = dev(v32)
    for _ in range(6):
        improved = False
        for k in (1, 2):
            for c in range(3):
                for to in (np.inf, -np.inf):
                    w = v32.copy()
                    w[k, c] = np.nextafter(w[k, c], F32(to))
                    x = dev(w)
                    if abs(x - rel) < abs(best - rel):
                        v32, best, improved = w, x, True
        if not improved:
            break
    return v32, best


DET_DEVIATIONS = [k * 2.0 ** -23 for k in (-3, -2, -1, 0, 1, 2, 3)] + [s * m for s in (-1, 1)
                                                                      for m in (1e-6, 1e-5, 1e-4, 1e-3)]


def small_face_on(fp, rng, rel):
    """|det| within a few ulps (or a chosen small fraction) of 1e-6 by area: a small triangle square to the central
    ray, close to the camera, covering the footprint where the footprint is small enough."""
    t = loguni(rng, 1e-4, 3e-3)
    c, rho = fp.on_plane(fp.oc + t * fp.dc, fp.dc)
    vs = regular(c, fp.dc, 0.00025, rng.uniform(0, 2 * np.pi), fp)     # area about 1e-6 / 1.5 before scaling
    return land_det(vs, fp.rays[0][1], rel)


def edge_on(fp, rng, rel):
    """|det| near 1e-6 by orientation: e1 almost along the central ray, e2 across it."""
    a, b = fp.basis(fp.dc)
    t = loguni(rng, 0.05, 20.0)
    l1, l2 = loguni(rng, 1e-4, 1.0), loguni(rng, 0.1, 2.0)
    e1 = l1 * fp.dc + (1e-6 / l2) * b
    e2 = l2 * a
    v0 = fp.oc + t * fp.dc - (e1 + e2) / 3.0
    return land_det(np.array([v0, v0 + e1, v0 + e2]), fp.rays[0][1], rel)


def facing_camera(fp, rng, t_axis, margin):
    """A covering triangle in a plane parallel to the near plane (the rays' origins lie on it), t_axis along the
    central ray from its origin: every ray of the bundle meets it at t = t_axis * (d_c . f) / (d . f)."""
    c, rho = fp.on_plane(fp.oc + t_axis * fp.dc, fp.fwd)
    return regular(c, fp.fwd, margin * max(rho, 1e-7) / abs(fp.fwd @ fp.dc), rng.uniform(0, 2 * np.pi), fp)


def signed_dev(rng, lo, hi):
    return float(rng.choice([-1.0, 1.0])) * loguni(rng, lo, hi)


def triangle_classes(fp, rng):
    """(class name, float32 vertices) for one bundle. The classes are the ones DESIGN.md §3.3 lists."""
    out = []
    for _ in range(8):
        out.append(("contains_with_room", covering(fp, rng, loguni(rng, 0.05, 200.0), rng.uniform(3.0, 8.0))))
    for _ in range(6):
        out.append(("edge_through_footprint", edge_through(fp, rng)))
        out.append(("vertex_in_footprint", vertex_inside(fp, rng)))
    for rel in rng.choice(DET_DEVIATIONS, 8, replace=False):
        vs, dev = small_face_on(fp, rng, float(rel))
        out.append(("det_near_eps_small", vs, dev))
    for rel in rng.choice(DET_DEVIATIONS, 4, replace=False):
        vs, dev = edge_on(fp, rng, float(rel))
        out.append(("det_near_eps_edge_on", vs, dev))
    for _ in range(4):
        out.append(("t_just_above_t_min", facing_camera(fp, rng, 1e-6 * (1.0 + loguni(rng, 1e-3, 4.0)), 6.0)))
        out.append(("t_just_below_t_min", facing_camera(fp, rng, 1e-6 * (1.0 - loguni(rng, 1e-3, 0.9)), 6.0)))
        out.append(("t_just_inside_t_max", facing_camera(fp, rng, 999.99 * (1.0 - loguni(rng, 1e-6, 0.3)), 6.0)))
        out.append(("t_just_beyond_t_max", facing_camera(fp, rng, 999.99 * (1.0 + loguni(rng, 1e-6, 0.3)), 6.0)))
    for _ in range(3):
        out.append(("behind_camera", covering(fp, rng, -loguni(rng, 0.5, 50.0), 8.0)))
        vs = covering(fp, rng, loguni(rng, 0.5, 50.0), 8.0)
        k, j = [(2, 0), (1, 0), (2, 1)][int(rng.integers(3))]      # e2 = 0, e1 = 0 or e1 = e2
        vs[k] = vs[j]
        out.append(("zero_area", vs))
    for bad in (np.nan, np.inf, -np.inf, np.nan):
        vs = covering(fp, rng, loguni(rng, 0.5, 50.0), 8.0)
        vs[rng.integers(3), rng.integers(3)] = bad
        out.append(("non_finite", vs))
    return [(c[0], np.asarray(c[1], np.float32)) + tuple(c[2:]) for c in out]


def as_v0e1e2(vs):
    with np.errstate(invalid="ignore"):
        return np.concatenate([vs[0], vs[1] - vs[0], vs[2] - vs[0]]).astype(np.float32)


def bundles(kind, rng):
    """Single-pixel bundles (the frame's corner pixels among them) or 8 x 8 tiles (a ragged one among them)."""
    if kind == "pixel":
        px = [(0, 0), (W - 1, H - 1), (W - 1, 0)] + [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(5)]
        return [(x, x, y, y) for x, y in px]
    tl = [(0, 0), (W - 8, H - 8)] + [(int(rng.integers(W - 8)), int(rng.integers(H - 8))) for _ in range(4)]
    return [(x, x + 7, y, y + 7) for x, y in tl] + [(W - 8, W - 1, 176, H - 1)]      # 8 x 4: the last tile row


NOT_CERTAIN = ("edge_through_footprint", "vertex_in_footprint", "det_near_eps_edge_on", "t_just_below_t_min",
               "t_just_beyond_t_max", "behind_camera", "zero_area", "non_finite")


@pytest.mark.parametrize("kind", ["pixel", "tile"])
@pytest.mark.parametrize("ci", range(NCAM))
def test_certain_triangles_are_accepted_by_every_ray(ci, kind):
    """Every triangle tri_certain reports is accepted by iqo_triangle_intersect with t_min = 1e-6, t_max = 999.99
    for every ray of the set, class by class."""
    rng = np.random.default_rng(300 + 10 * ci + (kind == "tile"))
    cam = camera(ci)
    n = {}
    straddled = landed = 0
    for box in bundles(kind, rng):
        fp = Footprint(cam, *box, 40 if kind == "tile" else 24, rng)
        cls = triangle_classes(fp, rng)
        ok, cert = certain_tile(cam, *box, np.stack([as_v0e1e2(c[1]) for c in cls]))
        assert ok
        for c, sure in zip(cls, cert):
            name, vs = c[0], c[1]
            if sure:
                for o, d in fp.rays:
                    assert tri_hit(vs[0], vs[1], vs[2], o, d, T_MAX), (name, box, vs.tolist())
            k = n.setdefault(name, [0, 0])
            k[1 if sure else 0] += 1
            if name in ("edge_through_footprint", "vertex_in_footprint"):
                hits = [bool(tri_hit(vs[0], vs[1], vs[2], o, d, T_MAX)) for o, d in fp.rays]
                straddled += any(hits) and not all(hits)
            if name.startswith("det_near_eps"):
                landed += abs(c[2]) <= 4 * 2.0 ** -23
    total = np.sum(list(n.values()), axis=0)
    # both outcomes occur, overall and in the classes meant to produce one
    assert total[1] > 20 and total[0] > 20, n
    assert n["contains_with_room"][1] > 20, n
    for name in NOT_CERTAIN:
        assert n[name][1] == 0, (name, n)
    assert sum(n[name][0] for name in NOT_CERTAIN) > 20, n
    assert n["edge_through_footprint"][0] + n["vertex_in_footprint"][0] > 20 and straddled > 20, (n, straddled)
    assert landed > 5, landed           # triangles whose |det| came within 4 ulps of 1e-6 for a ray of the bundle
    # the t bounds are probed from both sides: some triangle just inside each bound is certain
    assert n["t_just_inside_t_max"][1] > 0, n


def test_t_min_bound_between_the_outcomes():
    """Covering triangles square to the camera at t from 1e-6 to 1 in front of the rays' origins (the default
    camera). The interval of t is as wide as the pixel's footprint on the near plane lets it be (the origin's
    interval enters t through tvec x e1), so the proof fires only some way above t_min: both outcomes occur along
    the sweep, none below t_min, and what is reported certain is accepted by every ray."""
    rng = np.random.default_rng(41)
    cam = camera(0)
    sure = unsure = 0
    for box in bundles("pixel", rng):
        fp = Footprint(cam, *box, 16, rng)
        ts = [loguni(rng, 1e-6, 1.0) for _ in range(12)] + [1e-6 * (1.0 - loguni(rng, 1e-3, 0.9)) for _ in range(4)]
        tris = [facing_camera(fp, rng, t, 6.0).astype(np.float32) for t in ts]
        ok, cert = certain_tile(cam, *box, np.stack([as_v0e1e2(v) for v in tris]))
        assert ok
        for t, vs, s in zip(ts, tris, cert):
            assert not (s and t < 1e-6)
            unsure += not s
            if s:
                sure += 1
                for o, d in fp.rays:
                    assert tri_hit(vs[0], vs[1], vs[2], o, d, T_MAX)
    assert sure > 20 and unsure > 20, (sure, unsure)


@pytest.mark.parametrize("kind", ["pixel", "tile"])
@pytest.mark.parametrize("ci", range(NCAM))
def test_wide_triangles_are_certain(ci, kind):
    """Liveness: a triangle whose footprint exceeds the bundle's ten times in every direction, at mid-range t and
    tilted up to 40 degrees, is reported certain (a proof that never fires would be sound too)."""
    rng = np.random.default_rng(500 + 10 * ci + (kind == "tile"))
    cam = camera(ci)
    n = 0
    for box in bundles(kind, rng):
        fp = Footprint(cam, *box, 8, rng)
        tris = [covering(fp, rng, loguni(rng, 0.5, 50.0), 10.0, max_tilt=40.0).astype(np.float32) for _ in range(4)]
        ok, cert = certain_tile(cam, *box, np.stack([as_v0e1e2(v) for v in tris]))
        assert ok and cert.all(), (box, cert)
        for vs in tris:
            for o, d in fp.rays:
                assert tri_hit(vs[0], vs[1], vs[2], o, d, T_MAX)
        n += len(tris)
    assert n > 20


def test_unbounded_bundle_proves_nothing():
    """A bundle that is not ok (here: a camera whose inverse view matrix holds an infinity) reports no triangle
    certain and returns 0, whatever the triangle."""
    rng = np.random.default_rng(9)
    good = camera(0)
    fp = Footprint(good, 100, 100, 60, 60, 4, rng)
    tris = np.stack([as_v0e1e2(covering(fp, rng, 5.0, 10.0).astype(np.float32)) for _ in range(6)])
    ok, cert = certain_tile(good, 100, 100, 60, 60, tris)
    assert ok and cert.all()
    bad = camera(0)
    bad.inv_view[12] = np.inf
    ok, cert = certain_tile(bad, 100, 100, 60, 60, tris)
    assert not ok and not cert.any()
    ok, tc, _ = cull_tile(bad, 100, 100, 60, 60, tris, np.zeros((0, 4), np.float32))
    assert not ok and not tc.any()


# ------------------------------------------------------------------ tri_culled / sphere_culled, one pixel

def sphere_classes(fp, rng):
    """(class name, (cx, cy, cz, r)) grazing one pixel's ray cone; radii from 1e-3 to 1e3."""
    a, b = fp.basis(fp.dc)
    out = []
    for _ in range(10):
        # silhouette through or near the footprint: the central ray passes the centre at r + delta footprint
        # radii, |delta| from 0.05 to 1000 (the interval of the discriminant is wide where r or t is large)
        r, t = loguni(rng, 1e-3, 1e3), loguni(rng, 0.05, 100.0)
        c, rho = fp.on_plane(fp.oc + t * fp.dc, fp.dc)
        ph = rng.uniform(0, 2 * np.pi)
        off = (r + signed_dev(rng, 0.05, 1000.0) * rho) * (np.cos(ph) * a + np.sin(ph) * b)
        out.append(("silhouette", np.append(c + off, r)))
    for _ in range(4):
        r = loguni(rng, 1e-2, 1e3)
        v = rng.normal(0, 1, 3)
        out.append(("camera_inside", np.append(fp.oc + rng.uniform(0, 0.9) * r * v / np.linalg.norm(v), r)))
        r = loguni(rng, 1e-3, 1e3)
        out.append(("behind_camera", np.append(fp.oc - r * (1.0 + loguni(rng, 0.01, 3.0)) * fp.dc, r)))
        # the far root of the central ray at t_min (1 + dev): t2 = (c - o) . d + r
        r = loguni(rng, 1e-3, 1e3)
        t2 = 1e-6 * (1.0 + signed_dev(rng, 1e-3, 1.0))
        out.append(("far_root_near_t_min", np.append(fp.oc + (t2 - r) * fp.dc, r)))
    return [(name, np.asarray(s, np.float32)) for name, s in out]


@pytest.mark.parametrize("ci", range(NCAM))
def test_culled_primitives_are_rejected_by_every_pixel_ray(ci):
    """test_cull.py's soundness check on single-pixel bundles (xa == xb, ya == yb): what the certain-miss proof
    and the per-pixel candidate masks evaluate. Random primitives on and around the pixel's rays, the triangle
    classes above and spheres grazing the pixel's ray cone."""
    rng = np.random.default_rng(700 + ci)
    cam = camera(ci)
    n = {}
    for x, _, y, _ in bundles("pixel", rng) + bundles("pixel", rng):
        fp = Footprint(cam, x, x, y, y, 24, rng)
        tris, sphs = random_prims(fp.rays, rng, ntri=16, nsph=8)
        tl = [("random", t[0]) for t in tris] + [c[:2] for c in triangle_classes(fp, rng)]
        sl = [("random", s) for s in sphs] + sphere_classes(fp, rng)
        ok, tc, sc = cull_tile(cam, x, x, y, y, np.stack([as_v0e1e2(v) for _, v in tl]), np.stack([s for _, s in sl]))
        assert ok
        for (name, vs), culled in zip(tl, tc):
            if culled:
                for o, d in fp.rays:
                    assert not tri_hit(vs[0], vs[1], vs[2], o, d), ("culled triangle hit by a pixel ray", name, (x, y))
            n.setdefault("tri_" + name, [0, 0])[int(culled)] += 1
        for (name, s), culled in zip(sl, sc):
            if culled:
                for o, d in fp.rays:
                    assert not sph_hit(s[:3], s[3], o, d), ("culled sphere hit by a pixel ray", name, (x, y))
            n.setdefault("sph_" + name, [0, 0])[int(culled)] += 1
    for group in ("tri_", "sph_"):
        tot = np.sum([v for k, v in n.items() if k.startswith(group)], axis=0)
        assert tot[1] > 20 and tot[0] > 20, (group, n)
    # classes meant to produce one outcome
    assert n["tri_contains_with_room"][0] > 20 and n["tri_contains_with_room"][1] == 0, n
    assert n["tri_non_finite"][1] == 0, n              # the reference's comparisons all fail on NaN: a hit
    assert n["tri_behind_camera"][1] > 20, n
    assert n["sph_camera_inside"][0] > 20 and n["sph_camera_inside"][1] == 0, n
    assert n["sph_behind_camera"][1] > 20, n
    assert n["sph_silhouette"][0] > 20 and n["sph_silhouette"][1] > 20, n


@pytest.mark.parametrize("ci", range(NCAM))
def test_primitives_a_pixel_ray_hits_are_never_culled(ci):
    """The contrapositive on the grazing classes: a primitive that some ray of the pixel hits keeps its bit."""
    rng = np.random.default_rng(900 + ci)
    cam = camera(ci)
    hits = 0
    for x, _, y, _ in bundles("pixel", rng):
        fp = Footprint(cam, x, x, y, y, 16, rng)
        tl = [c[:2] for c in triangle_classes(fp, rng) if c[0] in ("edge_through_footprint", "vertex_in_footprint")]
        sl = [s for s in sphere_classes(fp, rng) if s[0] in ("silhouette", "far_root_near_t_min")]
        ok, tc, sc = cull_tile(cam, x, x, y, y, np.stack([as_v0e1e2(v) for _, v in tl]), np.stack([s for _, s in sl]))
        assert ok
        for (_, vs), culled in zip(tl, tc):
            if any(tri_hit(vs[0], vs[1], vs[2], o, d) for o, d in fp.rays):
                hits += 1
                assert not culled
        for (_, s), culled in zip(sl, sc):
            if any(sph_hit(s[:3], s[3], o, d) for o, d in fp.rays):
                hits += 1
                assert not culled
    assert hits > 20
