"""Shared by tests/test_gpu_proofs.py: the proof kernels' buffers read back from a context (iqpt_debug_read_proofs),
the same masks recomputed with the host build of csrc/iq_interval.h (iqpt_debug_cull_tile /
iqpt_debug_certain_tile) from the primitives the device holds, and seeded random scenes placed from the camera's
own rays. Nothing here restates a transform or a pair order: the primitives come from the device arrays."""
import ctypes as C

import numpy as np

from iqpt import MAT_EMISSIVE, MAT_OREN_NAYAR, Scene, _lib, align_camera, make_camera
from test_certain import Footprint, certain_tile, covering, facing_camera, loguni
from test_cull import corner_rays, cull_tile

TILE = 8
CERTAIN_MAX_PAIRS = 96        # iqpt_certain_kernel leaves tiles with more candidate pairs uncertain
PIX_MASK_MAX = 1024           # iqpt_pixel_mask_kernel: lists of up to this many entries
ANY_MAX_ENTRIES = 512         # iqpt_anyhit_kernel: lists of up to this many entries
RESIDENT_BYTES = 32 * 1024    # pair records that fit are resident in LDS: 80 B per triangle pair, 32 per sphere pair


# ------------------------------------------------------------------ read-back

def _read(pt, what, dtype=np.uint32):
    lib = _lib.load()
    f = lib.iqpt_debug_read_proofs
    f.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint64)]
    f.restype = C.c_int
    n = C.c_uint64(0)
    _lib.check(f(pt._h, what, None, 0, C.byref(n)), "iqpt_debug_read_proofs")
    out = np.zeros(n.value, np.uint32)
    if n.value:
        _lib.check(f(pt._h, what, out.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n)),
                   "iqpt_debug_read_proofs")
    return out.view(dtype)


def read_proofs(pt):
    """Everything iqpt_debug_read_proofs exposes, split into named arrays (None where a buffer was not built)."""
    g = _read(pt, 0)
    d = dict(ntx=int(g[0]), nty=int(g[1]), wt=int(g[2]), stride=int(g[3]), ntri=int(g[4]), nsph=int(g[5]),
             have_certain=bool(g[6]), have_lists=bool(g[7]), list_total=int(g[8]), have_pmask=bool(g[9]),
             pmask_words=int(g[10]))
    nt = d["ntx"] * d["nty"]
    d["cull"] = _read(pt, 1).reshape(nt, d["stride"])
    cert = _read(pt, 2)
    assert len(cert) == (4 * nt if d["have_certain"] else 0)
    d["hit"] = cert[:2 * nt].reshape(nt, 2) if d["have_certain"] else None
    d["miss"] = cert[2 * nt:].reshape(nt, 2) if d["have_certain"] else None
    ls = _read(pt, 3)
    assert len(ls) == (d["list_total"] + 2 * (nt + 1) if d["have_lists"] else 0)
    d["list"] = ls[:d["list_total"]] if d["have_lists"] else None
    d["off_tri"] = ls[d["list_total"]:d["list_total"] + nt + 1] if d["have_lists"] else None
    d["off_sph"] = ls[d["list_total"] + nt + 1:] if d["have_lists"] else None
    pm = _read(pt, 4)
    assert len(pm) == (nt + 1 + d["pmask_words"] + 2 * nt if d["have_pmask"] else 0)
    d["pm_off"] = pm[:nt + 1] if d["have_pmask"] else None
    d["pm"] = pm[nt + 1:nt + 1 + d["pmask_words"]] if d["have_pmask"] else None
    d["pm_certain"] = pm[nt + 1 + d["pmask_words"]:].reshape(nt, 2) if d["have_pmask"] else None
    d["tris"] = _read(pt, 5, np.float32).reshape(-1, 12)[:, :9].copy()
    d["sph"] = _read(pt, 6, np.float32).reshape(-1, 4).copy()
    assert len(d["tris"]) == d["ntri"] and len(d["sph"]) == d["nsph"]
    return d


# ------------------------------------------------------------------ the host build's masks

def _pack(bits):
    """Boolean rows -> 32-bit words, bit i of word w = entry 32 w + i."""
    bits = np.asarray(bits, bool)
    n = bits.shape[-1]
    pad = (-n) % 32
    b = np.concatenate([bits, np.zeros(bits.shape[:-1] + (pad,), bool)], axis=-1).reshape(bits.shape[:-1] + (-1, 32))
    return (b.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def _pairs(flags, n):
    """Per pair: both of its primitives flagged (a missing second one counts as flagged)."""
    p = np.ones(2 * ((n + 1) // 2), bool)
    p[:n] = flags
    return p[0::2] & p[1::2]


def host_masks(cam, ps, tris9, sph4, mats=False, lists=None):
    """What the proof kernels must write for this camera, pixel set and primitives, computed with the host build.
    lists: per tile the triangle candidate list in the device's order (None: ascending pair indices)."""
    ntri, nsph = len(tris9), len(sph4)
    ntp, nsp = (ntri + 1) // 2, (nsph + 1) // 2
    ncols, nrows = ps.x1 - ps.x0, ps.nrows
    ntx, nty = (ncols + TILE - 1) // TILE, (nrows + TILE - 1) // TILE
    nt = ntx * nty
    wt = (ntp + 31) // 32
    stride = wt + (nsp + 31) // 32
    e = dict(ntx=ntx, nty=nty, wt=wt, stride=stride, ntri=ntri, nsph=nsph)
    e["have_certain"] = (not mats) and nt > 0 and ntp * 80 + nsp * 32 <= RESIDENT_BYTES
    cull = np.zeros((nt, stride), np.uint32)
    hit = np.zeros(nt, np.uint64)
    miss = np.zeros(nt, np.uint64)
    pm_sure = []                       # per tile, per lane: some listed entry holds a tri_certain triangle
    pm_words = []
    cand_t, cand_s = [], []
    for t in range(nt):
        tx, ty = t % ntx, t // ntx
        c0, c1 = tx * TILE, min(tx * TILE + TILE, ncols) - 1
        k0, k1 = ty * TILE, min(ty * TILE + TILE, nrows) - 1
        ok, tc, sc = cull_tile(cam, ps.x0 + c0, ps.x0 + c1, ps.y0 + k0 * ps.ystep, ps.y0 + k1 * ps.ystep, tris9, sph4)
        keep_t = ~(_pairs(tc, ntri) & ok)
        keep_s = ~(_pairs(sc, nsph) & ok)
        if wt:
            cull[t, :wt] = _pack(keep_t)
        if stride > wt:
            cull[t, wt:] = _pack(keep_s)
        jt, js = np.flatnonzero(keep_t), np.flatnonzero(keep_s)
        cand_t.append(jt)
        cand_s.append(js)
        lst = jt if lists is None else np.asarray(lists[t], np.int64)
        ti = np.array([k for j in jt for k in (2 * j, 2 * j + 1) if k < ntri], np.int64)
        si = np.array([k for j in js for k in (2 * j, 2 * j + 1) if k < nsph], np.int64)
        small = len(jt) + len(js) <= CERTAIN_MAX_PAIRS
        tw, th = c1 - c0 + 1, k1 - k0 + 1
        li = np.concatenate([2 * lst, 2 * lst + 1])
        li = li[li < ntri]
        words = np.zeros(((len(lst) + 31) // 32, 64), np.uint32)
        sure = np.zeros(64, bool)
        for lane in range(tw * th):
            x, y = ps.x0 + c0 + lane % tw, ps.y0 + (k0 + lane // tw) * ps.ystep
            pok, ptc, psc = cull_tile(cam, x, x, y, y, tris9, sph4)
            pok2, pcert = certain_tile(cam, x, x, y, y, tris9)
            assert pok == pok2
            h = small and len(js) == 0 and pok and bool(pcert[ti].any())
            m = small and pok and not h and bool(ptc[ti].all()) and bool(psc[si].all())
            hit[t] |= np.uint64(int(h) << lane)
            miss[t] |= np.uint64(int(m) << lane)
            if len(lst):
                words[:, lane] = _pack(~(_pairs(ptc, ntri) & pok)[lst])
                sure[lane] = bool(pcert[li].any())
        pm_words.append(words)
        pm_sure.append(sure)
    e.update(cull=cull, hit=hit, miss=miss, cand_t=cand_t, cand_s=cand_s, pm_words=pm_words, pm_sure=pm_sure)
    total = sum(len(j) for j in cand_t) + sum(len(j) for j in cand_s)
    e["have_lists"] = stride > 8 and total > 0
    return e


def u64(words2):
    return words2[:, 0].astype(np.uint64) | (words2[:, 1].astype(np.uint64) << np.uint64(32))


def check_masks(cam, ps, dev, mats, pmask_mode):
    """Every mask the proof kernels wrote against the host build, word for word. Returns coverage figures."""
    nt = dev["ntx"] * dev["nty"]
    lists = None
    if dev["have_lists"]:
        lists = [dev["list"][dev["off_tri"][t]:dev["off_tri"][t + 1]] for t in range(nt)]
    e = host_masks(cam, ps, dev["tris"], dev["sph"], mats=mats, lists=lists)
    for k in ("ntx", "nty", "wt", "stride", "ntri", "nsph", "have_certain", "have_lists"):
        assert dev[k] == e[k], (k, dev[k], e[k])
    assert np.array_equal(dev["cull"], e["cull"]), np.argwhere(dev["cull"] != e["cull"])[:8]
    cov = dict(hit=0, miss=0, mixed_tiles=0, cleared_tiles=0, pm_tiles=0)
    if e["have_certain"]:
        dh, dm = u64(dev["hit"]), u64(dev["miss"])
        for name, got, want in (("hit", dh, e["hit"]), ("miss", dm, e["miss"])):
            bad = [(t, hex(a), hex(b)) for t, (a, b) in enumerate(zip(got, want)) if a != b]
            assert not bad, (name, bad[:4])
        ncols, nrows = ps.x1 - ps.x0, ps.nrows
        for t in range(nt):
            tx, ty = t % dev["ntx"], t // dev["ntx"]
            npt = min(TILE, ncols - tx * TILE) * min(TILE, nrows - ty * TILE)
            sure = int(dh[t] | dm[t])
            assert sure >> npt == 0 and int(dh[t] & dm[t]) == 0          # lanes outside a ragged tile are 0
            cov["mixed_tiles"] += sure != 0 and sure != (1 << npt) - 1
        cov["hit"] = sum(bin(int(v)).count("1") for v in dh)
        cov["miss"] = sum(bin(int(v)).count("1") for v in dm)
    if dev["have_lists"]:
        cnt_t = np.array([len(j) for j in e["cand_t"]])
        cnt_s = np.array([len(j) for j in e["cand_s"]])
        off = np.concatenate([[0], np.cumsum(cnt_t)])
        assert np.array_equal(dev["off_tri"], off)
        assert np.array_equal(dev["off_sph"], off[-1] + np.concatenate([[0], np.cumsum(cnt_s)]))
        for t in range(nt):
            assert np.array_equal(np.sort(lists[t]), e["cand_t"][t]), t      # the tile's candidates, in some order
            seg = dev["list"][dev["off_sph"][t]:dev["off_sph"][t + 1]]
            assert np.array_equal(seg, e["cand_s"][t]), t
        assert dev["have_pmask"] == (pmask_mode != 0)
    else:
        assert not dev["have_pmask"]
    if dev["have_pmask"]:
        masked = cnt_t <= PIX_MASK_MAX
        pm_off = np.concatenate([[0], np.cumsum(np.where(masked, 64 * ((cnt_t + 31) // 32), 0))])
        assert np.array_equal(dev["pm_off"], pm_off) and dev["pmask_words"] == pm_off[-1]
        dsure = u64(dev["pm_certain"])
        for t in range(nt):
            if not masked[t]:
                assert dsure[t] == 0
                continue
            w = dev["pm"][pm_off[t]:pm_off[t + 1]].reshape(-1, 64)
            assert np.array_equal(w, e["pm_words"][t]), t
            for lane in range(64):
                if (int(dsure[t]) >> lane) & 1:
                    assert e["pm_sure"][t][lane], (t, lane)                  # soundness of the any-hit certain bit
            if cnt_t[t]:
                tx, ty = t % dev["ntx"], t // dev["ntx"]
                npt = min(TILE, ps.x1 - ps.x0 - tx * TILE) * min(TILE, ps.nrows - ty * TILE)
                assert not w[:, npt:].any()                                  # lanes outside a ragged tile are 0
                cov["pm_tiles"] += 1
                cov["cleared_tiles"] += bool((w[:, :npt] != _pack(np.ones(cnt_t[t], bool))[:, None]).any())
        cov["any_ok"] = bool((cnt_t <= ANY_MAX_ENTRIES).all() and (cnt_s == 0).all())
    return cov


# ------------------------------------------------------------------ cameras, frames, scenes

def cameras(w, h):
    """The default camera; a 5 degree field of view; one pitched and yawed; a 120 degree field of view; one about
    1e4 units from the origin (the scenes are placed from the camera's rays, so they move along), where the
    intervals are wide. A tile's bundle is a box of directions about as wide as the tile, so it culls a small
    primitive only at an angle of about sqrt(2 x that width) from it: several tiles for the 45 and 70 degree cameras,
    more tiles than these frames have for the 5 degree one (whose masks stay full) and the 120 degree one (whose
    tiles span 24 degrees). Then the aligned form of each (iqpt_camera_align), in the same order:
    inv_proj[12] and inv_proj[13] are non-zero, which no camera of iqpt_camera_init has."""
    plain = [
        ("default", make_camera(w, h)),
        ("fov5", make_camera(w, h, fovh=5.0, position=(0.5, 0.2, -3.0, 0.0), forward=(0.1, 0.05, 1.0, 0.0))),
        ("pitched", make_camera(w, h, fovh=70.0, znear=0.05, zfar=50.0, position=(0.3, 1.2, -2.0, 0.0),
                                forward=(-0.1, -0.6, 1.0, 0.0))),
        ("fov120", make_camera(w, h, fovh=120.0, znear=0.02, position=(-0.4, 0.3, 0.5, 0.0),
                               forward=(0.7, -0.2, -0.6, 0.0))),
        ("far", make_camera(w, h, position=(8000.0, -2500.0, 5500.0, 0.0), forward=(0.3, -0.2, 1.0, 0.0))),
    ]
    return plain + [(name + "_aligned", align_camera(cam)) for name, cam in plain]


N_PLAIN = 5                # cameras(w, h)[k] and [N_PLAIN + k] are a camera and its aligned form


# (k below: the scene's index in its family, the camera's index within its group of N_PLAIN)
STREAMED = (1, 4)          # the scenes of the "tris" family with two balls (more than 32 KiB of pair records)
FILLED = 3                 # the scene that gets the triangle covering the frame and the sphere around the camera


def frame_footprint(cam, ps, rng):
    return Footprint(cam, ps.x0, ps.x1 - 1, ps.y0, ps.y0 + (ps.nrows - 1) * ps.ystep, 0, rng)


def _point(fr, rng, t, spread=0.9):
    """A point at distance t along the frame's central ray, moved sideways within the frame's footprint there."""
    a, b = fr.basis(fr.dc)
    c, rho = fr.on_plane(fr.oc + t * fr.dc, fr.dc)
    return c + spread * 0.7 * rho * (rng.uniform(-1, 1) * a + rng.uniform(-1, 1) * b), rho


def _add_triangle(sc, name, vs):
    """One world-space triangle: a mesh of its own under the identity transform."""
    v = np.zeros((3, 6), np.float32)
    v[:, :3] = np.asarray(vs, np.float32)
    v[:, 5] = 1.0
    sc.add_mesh(name + "_mesh", v, np.array([0, 1, 2], np.uint32))
    sc.add_model(name, name + "_mesh", 1.0, 0.0, 0.0)


def _pixel_corner_ray(cam, x, y, rng):
    o, d = corner_rays(cam, x, x, y, y, rng)[0]          # jitter (-0.5, -0.5): the pixel's corner
    return o[:3].astype(np.float64), d[:3].astype(np.float64)


def add_adversarial(sc, cam, ps, fr, rng, spheres, k):
    """Placements built from the camera's own corner rays (k: the scene's index in its family; the two placements
    that fill the frame go into one scene)."""
    a, b = fr.basis(fr.dc)
    ncols = ps.x1 - ps.x0

    def pixel():
        return ps.x0 + int(rng.integers(ncols)), ps.y0 + int(rng.integers(ps.nrows)) * ps.ystep

    def tile_corner(first_column=False):
        return (ps.x0 + TILE * (1 if first_column else int(rng.integers(1, (ncols + TILE - 1) // TILE))),
                ps.y0 + TILE * int(rng.integers(1, (ps.nrows + TILE - 1) // TILE)) * ps.ystep)

    t = loguni(rng, 2.0, 6.0)
    _, rho = fr.on_plane(fr.oc + t * fr.dc, fr.dc)
    # two triangles sharing an edge that runs through pixel corners
    (o1, d1), (o2, d2) = _pixel_corner_ray(cam, *pixel(), rng), _pixel_corner_ray(cam, *pixel(), rng)
    p, q = o1 + t * d1, o2 + t * d2
    m = np.cross(q - p, fr.dc)
    m = m / max(np.linalg.norm(m), 1e-30) * 0.3 * rho
    _add_triangle(sc, "adv_edge_a", [p, q, (p + q) / 2 + m])
    _add_triangle(sc, "adv_edge_b", [q, p, (p + q) / 2 - m])
    # a triangle with a vertex on a tile-corner ray
    o, d = _pixel_corner_ray(cam, *tile_corner(), rng)
    v0 = o + 0.8 * t * d
    _add_triangle(sc, "adv_vertex", [v0, v0 + 0.3 * rho * a, v0 + 0.3 * rho * b])
    # a triangle straddling t_min: two vertices in front of the rays' origins, one behind them
    (o1, d1), (o2, d2), (o3, d3) = (_pixel_corner_ray(cam, *pixel(), rng) for _ in range(3))
    _add_triangle(sc, "adv_t_min", [o1 + 0.3 * t * d1, o2 + 0.3 * t * d2, o3 - 0.3 * t * d3])
    # one at t ~ 999.99, square to the camera, a few pixels wide
    x, y = pixel()
    fp = Footprint(cam, x, x, y, y, 0, rng)
    _add_triangle(sc, "adv_t_max", facing_camera(fp, rng, 999.99 * (1.0 + rng.uniform(-1e-5, 1e-5)), 4.0))
    # one edge-on: e1 along a pixel's corner ray
    o, d = _pixel_corner_ray(cam, *pixel(), rng)
    v0 = o + 0.5 * t * d
    _add_triangle(sc, "adv_edge_on", [v0, v0 + 0.4 * t * d, v0 + 0.2 * rho * a])
    # a zero-area one
    v0, _ = _point(fr, rng, t)
    _add_triangle(sc, "adv_zero_area", [v0, v0 + 0.2 * rho * a, v0])
    if k == FILLED:
        _add_triangle(sc, "adv_whole_frame", covering(fr, rng, loguni(rng, 50.0, 200.0), 1.5, max_tilt=30.0))
    if spheres:
        # tangent to a tile-corner ray
        o, d = _pixel_corner_ray(cam, *tile_corner(True), rng)
        r = 0.05 * rho
        n = np.cross(d, a)
        sc.add_model("adv_tangent", "sphere", float(r), 0.0, tuple(o + t * d + r * n / np.linalg.norm(n)))
        # wholly behind the camera
        r = loguni(rng, 0.1, 1.0)
        sc.add_model("adv_behind", "sphere", float(r), 0.0, tuple(fr.oc - 4.0 * r * fr.fwd))
        if k == FILLED:
            r = loguni(rng, 20.0, 60.0)                   # the camera inside a sphere
            sc.add_model("adv_inside", "sphere", float(r), 0.0, tuple(fr.oc + 0.3 * r * a))


def random_scene(family, seed, k, cam, ps):
    """family: "resident" (tens of triangles, a few spheres, the reference's materials), "tris" (triangle-only, more
    than 512: one ball resident, two balls streamed), "tris_spheres" (more than 512 triangles plus spheres),
    "materials" (the resident family with a material table). Returns the Scene (keep it while its packet is used)."""
    rng = np.random.default_rng(seed)
    fr = frame_footprint(cam, ps, rng)
    sc = Scene()
    # (triangle meshes are named to sort before "sphere": a packet's mesh ids count every mesh name, scene.cu:167)
    sc.add_mesh_tri("a_tri")
    sc.add_mesh_quad("b_quad")
    sc.add_mesh_cube("cube")
    sc.add_mesh_uv_sphere("ball", False, 21, 15, _lib.MESH_TRIANGLES)        # 588 triangles
    sc.add_mesh_uv_sphere("sphere")
    spheres = family in ("resident", "tris_spheres", "materials")

    def place(name, mesh, size_lo, size_hi):
        t = loguni(rng, 1.5, 8.0)
        p, rho = _point(fr, rng, t)
        sc.add_model(name, mesh, float(rho * loguni(rng, size_lo, size_hi)), tuple(rng.uniform(0, 2 * np.pi, 3)),
                     tuple(p))

    if family in ("resident", "materials"):
        for i in range(int(rng.integers(7, 12))):
            place(f"m{i}", ["a_tri", "b_quad", "cube"][int(rng.integers(3))], 0.05, 0.4)
        # a wall in the frame's last columns, away from the spheres: pixels it covers with room to spare
        o, d = _pixel_corner_ray(cam, ps.x1 - 8, ps.y0 + (ps.nrows // 2) * ps.ystep, rng)
        t = loguni(rng, 3.0, 8.0)
        _, rho = fr.on_plane(fr.oc + t * fr.dc, fr.dc)
        sc.add_model("wall", "b_quad", float(0.5 * rho), tuple(rng.uniform(-0.4, 0.4, 3)), tuple(o + t * d))
    else:
        # balls a few pixels wide: the tiles away from a ball cull it, so their lists stay short (the certain proofs
        # take tiles of up to 96 candidate pairs, iqpt_anyhit_kernel lists of up to 512); two balls at the frame's
        # two ends make the scene streamed
        mid = ps.y0 + (ps.nrows // 2) * ps.ystep
        if family == "tris" and k in STREAMED:
            at = [(ps.x0 + 3, mid), (ps.x1 - 4, mid)]
        else:
            at = [(ps.x0 + int(rng.integers(ps.x1 - ps.x0)), ps.y0 + int(rng.integers(ps.nrows)) * ps.ystep)]
        for i, (x, y) in enumerate(at):
            fp = Footprint(cam, x, x, y, y, 0, rng)
            c, rpx = fp.on_plane(fp.oc + loguni(rng, 2.0, 6.0) * fp.dc, fp.dc)
            sc.add_model(f"ball{i}", "ball", float(rpx * rng.uniform(4.0, 7.0)), tuple(rng.uniform(0, 2 * np.pi, 3)),
                         tuple(c))
        for i in range(4):
            place(f"q{i}", "b_quad", 0.1, 0.6)
    if spheres:
        # (on rays of the frame's first columns: a tile's bundle is wide in so small a frame, a sphere is a candidate
        # of the tiles around its own, and the certain-hit proof needs tiles without a sphere candidate)
        for i in range(3):
            t = loguni(rng, 1.5, 8.0)
            o, d = _pixel_corner_ray(cam, ps.x0 + int(rng.integers(4)), ps.y0 + int(rng.integers(ps.nrows)) * ps.ystep,
                                     rng)
            _, rho = fr.on_plane(fr.oc + t * fr.dc, fr.dc)
            sc.add_model(f"s{i}", "sphere", float(rho * loguni(rng, 0.02, 0.08)), 0.0, tuple(o + t * d))
    add_adversarial(sc, cam, ps, fr, rng, spheres, k)
    if family == "materials":
        rough = sc.add_material(MAT_OREN_NAYAR, (0.8, 0.4, 0.2, 0.0), 0.6)
        lamp = sc.add_material(MAT_EMISSIVE, (1.0, 0.9, 0.7, 1.0), 4.0)
        sc.set_model_material("m0", rough)
        sc.set_model_material("m1", rough)
        sc.set_model_material("adv_edge_a", rough)
        sc.set_model_material("s0", lamp)
    return sc
