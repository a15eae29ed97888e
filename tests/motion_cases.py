"""What tests/test_motion_ref.py, tests/test_gpu_motion.py and tests/test_gpu_motion_facade.py share: the "movers"
scene, built with Scene's own calls, and the synthetic views of one wall whose ids are laid out by
wave (a wave of the view kernel is two rows of 32 pixels of a 32 x 8 block) with a motion table of every kind."""
from __future__ import annotations

import numpy as np

import motion_ref as mr
from iqpt import MAT_OREN_NAYAR, Scene, make_camera

F = np.float32
NO = mr.NO_PRIM
PARAMS = (0.9, 0.01, 16)

# ------------------------------------------------------------------------------------------------ the movers scene
GROUND, STATIC_CUBE, MOVER = 0, 1, 2          # draw indices: mesh names sort a_, b_, z_
MOVER_SCALE = 0.4
STEP_X = 0.25 * MOVER_SCALE                   # a quarter of the moving cube's width per view
STEP_ROT = np.deg2rad(10.0)                   # plus 10 degrees about y


def movers(k: int, materials: bool = True) -> Scene:
    """The scene of view k: a ground quad, a static cube and, in front of both, a cube at step k of its motion. All
    three Oren-Nayar, the sky the only light. materials=False: without the material table (what iqpt::scene, which
    has no call for one, builds in csrc/tools/test_motion_facade.cpp)."""
    sc = Scene()
    sc.add_mesh_quad("a_ground")
    sc.add_mesh_cube("b_cube")
    sc.add_mesh_cube("z_mover")
    sc.add_model("ground", "a_ground", scale=[4.0, 4.0, 1.0, 1.0], rotation=[np.pi / 2, 0.0, 0.0, 0.0],
                 translation=[0.0, -0.5, 0.0, 0.0])
    sc.add_model("box", "b_cube", scale=0.5, rotation=[0.0, 0.4, 0.0, 0.0], translation=[-0.6, -0.25, 0.6, 0.0])
    sc.add_model("mover", "z_mover", scale=MOVER_SCALE, rotation=[0.0, STEP_ROT * k, 0.0, 0.0],
                 translation=[0.15 + STEP_X * k, -0.3, -0.4, 0.0])
    if not materials:
        return sc
    for model, albedo, sigma in (("ground", (0.7, 0.7, 0.7), 0.5), ("box", (0.2, 0.5, 0.7), 0.5),
                                 ("mover", (0.8, 0.4, 0.2), 0.5)):
        sc.set_model_material(model, sc.add_material(MAT_OREN_NAYAR, albedo, sigma))
    return sc


def movers_camera(w, h):
    return make_camera(w, h)


# ------------------------------------------------------------------------------------------------ synthetic views
POS_A = np.array([0.0, 0.5, -3.0])
FWD = np.array([0.0, -0.5, 3.0])
FWD_UNIT = FWD / np.linalg.norm(FWD)
WALL = 5.0                       # the distance of the wall from camera A along its forward vector
CENTRE = POS_A + WALL * FWD_UNIT
KINDS = ("static", "translate", "rotate", "scale", "nan", "behind", "off")


def camera_at(w, h, pos, fwd=FWD):
    return make_camera(w, h, position=[*pos, 0.0], forward=[*fwd, 0.0])


def wall_depth(cam):
    p = np.array([[*CENTRE, 1.0]], np.float32)
    c = mr.rr.dot4(mr.rr.dot4(p, np.array(cam.view, np.float32)), np.array(cam.projection, np.float32))
    return F(c[0, 2] / c[0, 3])


def _translate(v):
    m = np.eye(4)
    m[3, :3] = v
    return m


def _about_centre(m3):
    m = np.eye(4)
    m[:3, :3] = m3
    return _translate(-CENTRE) @ m @ _translate(CENTRE)


def kind_entry(kind, cam, w):
    """The entry of one kind for the wall seen by cam: every motion but "behind" keeps the wall in its own plane."""
    if kind == "static":
        return mr.identity_table(1)[0]
    if kind == "translate":
        # two pixels along x (none on a frame too narrow for that): a pixel's world width on the wall is
        # 2 WALL / (P00 |right| w), the view matrix's right vector being as long as the reference's look_at leaves it
        right = float(np.linalg.norm(np.array(cam.view, np.float64).reshape(4, 4)[:3, 0]))
        px = 2.0 * WALL / (float(np.array(cam.projection, np.float32).reshape(4, 4)[0, 0]) * right * w)
        return mr.entry(_translate([2.0 * px if w >= 8 else 0.0, 0.0, 0.0]))
    if kind == "rotate":
        a, k = 0.04, FWD_UNIT
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return mr.entry(_about_centre((np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K).T))
    if kind == "scale":
        return mr.entry(_about_centre(np.diag([0.9, 1.0, 1.0])))
    if kind == "nan":
        e = mr.identity_table(1)[0]
        e["back"][:] = np.nan
        e["nback"][:] = np.nan
        e["back"][5], e["nback"][2] = np.inf, -np.inf
        e["moved"] = 1
        return e
    if kind == "behind":
        return mr.entry(_translate(-2.0 * WALL * FWD_UNIT))
    assert kind == "off"
    return mr.entry(_translate([100.0, 0.0, 0.0]))


def make_table(n, cam, w):
    """n entries: entry i of kind KINDS[i % 7]; a table of one entry holds a translation."""
    t = mr.identity_table(n)
    for i in range(n):
        t[i] = kind_entry("translate" if n == 1 else KINDS[i % len(KINDS)], cam, w)
    return t


LAYOUTS = ("waves", "checker", "foreign")


def id_plane(layout, w, h, n, rng):
    """ids [h, w] laid out by wave. "waves": one id per wave (with a few NO_PRIM lanes), in the order 0, n (beyond the
    table), a wave that is NO_PRIM alone, n + 1, a wave of id 0 (static where n >= 3) and NO_PRIM alone, then
    1 .. n - 1; "checker": two ids alternating pixel by pixel, both moved where the table has two moved entries;
    "foreign": one moved id per wave and a single lane of another, which cycles through the kinds of entry."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    wave = (y // 2) * ((w + 31) // 32) + x // 32
    a, b = (1, 2) if n >= 3 else (0, 1)
    if layout == "waves":
        seq = np.array([0, n, NO, n + 1, 0] + list(range(1, n)), np.uint32)
        cyc = wave % len(seq)
        ids = seq[cyc]
        ids[(cyc == 4) & ((x + y) % 3 == 0)] = NO
        ids[(cyc != 4) & (rng.random((h, w)) < 0.05)] = NO
        return ids
    if layout == "checker":
        return np.where((x + y) % 2 == 0, a, b).astype(np.uint32)
    assert layout == "foreign"
    ids = np.where(wave % 2 == 0, a, b).astype(np.uint32)
    lane = (x % 32 == 5) & (y % 2 == 1)
    other = 3 + wave % 4 if n >= 7 else np.where(wave % 2 == 0, b, a)
    ids[lane] = other[lane]
    return ids


def special_colours(rng, h, w):
    c = rng.random((h, w, 4), dtype=np.float32)
    special = np.array([0.0, -0.0, 1e-40, -3e-42, np.nan, np.inf, -np.inf, 1.5, 37.0, 1e-38], np.float32)
    pick = rng.random((h, w, 4)) < 0.06
    c[pick] = rng.choice(special, size=int(pick.sum()))
    return c


def synthetic_views(w, h, n, layout, seed):
    """Three views of one wall: (camera, normal_z, ids, colour, samples, table) each. 0: camera A, no table. 1: A
    again with the table: only the models move. 2: camera B, a little to the side, with the table again and speckles
    of another normal, other depths and NaN and +-inf depths: camera and models move."""
    rng = np.random.default_rng(seed)
    normal = (-FWD_UNIT).astype(np.float32)
    cams = [camera_at(w, h, POS_A), camera_at(w, h, POS_A), camera_at(w, h, POS_A + np.array([0.03, 0.0, 0.0]))]
    ids = id_plane(layout, w, h, n, rng)
    views = []
    for k, cam in enumerate(cams):
        nz = np.empty((h, w, 4), np.float32)
        nz[..., :3] = normal
        nz[..., 3] = wall_depth(cam)
        if k == 2:
            sp = rng.random((h, w))
            other = rng.normal(size=(h, w, 3)).astype(np.float32)
            other /= np.linalg.norm(other, axis=2, keepdims=True).astype(np.float32)
            m = sp < 0.06
            nz[m, :3] = other[m]
            m = (sp >= 0.06) & (sp < 0.12)
            nz[m, 3] = rng.random(int(m.sum()), dtype=np.float32)
            m = (sp >= 0.12) & (sp < 0.16)
            nz[m, 3] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, 1.0], np.float32), size=int(m.sum()))
            m = (sp >= 0.16) & (sp < 0.19)
            nz[m, :3] = rng.choice(np.array([0.0, 1e-6, -1e-6, np.nan], np.float32), size=(int(m.sum()), 3))
        views.append((cam, nz, ids, special_colours(rng, h, w), (3, 5, 1)[k], None if k == 0 else make_table(n, cam, w)))
    return views
