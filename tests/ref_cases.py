"""Inputs and runners shared by tests/test_ref_units.py, tests/test_ref_frames.py, tests/test_gpu_ref_golden.py and
tests/golden/make_ref_golden.py: the cases on which the oracle (oracle/iqpt_oracle.c), the scene builder
(csrc/iq_scene.cpp) and the HIP path tracer are compared with the reference's own source (oracle/ref/).

Every runner returns a flat dict of arrays ("routine.output"), so that two sides are compared key by key: floats as
uint32, flags, integers and generator states for equality. Nothing here needs the reference directory; the runners
of the reference side take an oracle/ref_oracle.py library.
"""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np

import oracle
from iqpt import Scene, _lib, make_camera

F32 = np.float32
FP = C.POINTER(C.c_float)
UP = C.POINTER(C.c_uint32)
TRI, SPH = _lib.MESH_TRIANGLES, _lib.MESH_SPHERES

N_LIVE = 4000       # seeded random cases per routine in the live comparison
N_RECORDED = 384    # the first of them that tests/golden/ref_units.npz records (plus every edge case)
T_MIN, T_MAX = F32(0.000001), F32(999.99)      # ray_color's bounds


def _v4(a, w=0.0):
    a = np.asarray(a, F32)
    out = np.full(a.shape[:-1] + (4,), w, F32)
    out[..., :a.shape[-1]] = a
    return out


def _unit(a):
    a = np.asarray(a, F32)
    return (a / np.sqrt((a.astype(np.float64) ** 2).sum(-1, keepdims=True))).astype(F32)


def _up(x, k=1):
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf))
    return x


def _states(rng, n):
    return rng.integers(0, 2 ** 32, size=(n, 6), dtype=np.uint64).astype(np.uint32)


def _stack(cases, keys):
    return {k: np.ascontiguousarray(np.stack([np.asarray(c[k], F32) for c in cases])) for k in keys}


# ------------------------------------------------------------------------------------------------ unit inputs
def triangle_inputs(n_random):
    rng = np.random.default_rng(101)
    n = n_random
    scale = (10.0 ** rng.uniform(-2, 1, size=(n, 1))).astype(F32)
    v = [_v4(rng.normal(size=(n, 3)) * scale, 1.0) for _ in range(3)]
    nr = [_v4(rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-1, 1, size=(n, 1)), 0.0) for _ in range(3)]
    o = _v4(rng.normal(size=(n, 3)) * 3.0, 1.0)
    bary = rng.dirichlet([1, 1, 1], size=n)
    target = sum(bary[:, k:k + 1] * v[k][:, :3] for k in range(3))
    toward = _unit(target - o[:, :3])
    anyway = _unit(rng.normal(size=(n, 3)))
    d = _v4(np.where(rng.random((n, 1)) < 0.7, toward, anyway), 0.0)
    t_min = np.full(n, T_MIN, F32)
    t_max = np.where(rng.random(n) < 0.8, T_MAX, (10.0 ** rng.uniform(-1, 1.5, size=n))).astype(F32)
    rnd = dict(v0=v[0], v1=v[1], v2=v[2], n0=nr[0], n1=nr[1], n2=nr[2], o=o, d=d, t_min=t_min, t_max=t_max)

    # edges on the unit right triangle of the z = 0 plane: |e1 x e2| = 1, so the determinant is -d.z
    A, B, Cc = (0, 0, 0, 1), (1, 0, 0, 1), (0, 1, 0, 1)
    nz = (0, 0, -1, 0)
    cases = []

    def add(v0=A, v1=B, v2=Cc, n0=nz, n1=nz, n2=nz, o=(0.2, 0.2, -1, 1), d=(0, 0, 1, 0), t_min=T_MIN, t_max=T_MAX):
        cases.append(dict(v0=v0, v1=v1, v2=v2, n0=n0, n1=n1, n2=n2, o=o, d=d, t_min=t_min, t_max=t_max))

    for vx in (A, B, Cc):                                              # through each vertex, head-on and oblique
        add(o=(vx[0], vx[1], -1, 1))
        add(o=(vx[0] - 1, vx[1] - 2, -2, 1), d=_v4(_unit([1, 2, 2])))
    for px in ((0.5, 0, 0), (0, 0.5, 0), (0.5, 0.5, 0)):              # a point on each edge
        add(o=(px[0], px[1], -1, 1))
    add(o=(-1, 0, 0, 1), d=(1, 0, 0, 0))                               # along the edge A-B, in the plane
    add(o=(0, -1, 0, 1), d=(0, 1, 0, 0))                               # along the edge A-C
    add(o=(2, -1, 0, 1), d=_v4(_unit([-1, 1, 0])))                     # along the edge B-C
    add(o=(0.2, 0.2, -1, 1), d=(1, 0, 0, 0))                           # parallel to the plane, off it
    eps = F32(0.000001)                                                # is_zero's epsilon
    for k in (-2, -1, 0, 1, 2):                                        # nearly parallel: |det| around the epsilon
        for sgn in (1, -1):
            dz = F32(sgn) * _up(eps, k)
            add(o=(0.2, 0.2, F32(-sgn) * F32(1e-7), 1), d=(1, 0, dz, 0))
            add(o=(0.2, 0.2, F32(-sgn) * F32(1e-7), 1), d=_v4(_unit([1, 0, dz])))
    add(o=(0.2, 0.2, 1, 1), d=(0, 0, -1, 0))                           # back-facing
    add(o=(0.2, 0.2, 1, 1), d=_v4(_unit([0.1, -0.1, -1])))
    for tm in (F32(1), _up(1, -1), _up(1, 1)):                         # t == 1 exactly against both bounds
        add(t_max=tm)
        add(t_min=tm)
    add(t_min=F32(1), t_max=F32(1))
    add(o=(0.2, 0.2, 1, 1))                                            # the plane is behind the origin
    add(o=(0.2, 0.2, 0, 1))                                            # origin on the plane (t = 0 < t_min)
    add(v1=Cc)                                                         # zero area: v1 == v2
    add(v1=A, v2=A)                                                    # a point
    add(v0=(0, 0, 0, 1), v1=(2, 0, 0, 1), v2=(1, 0, 0, 1))             # collinear
    for s in (1e18, 1e12, 1e-6, 1e-12, 1e-20):                         # very large and very small triangles
        add(v0=(0, 0, 0, 1), v1=(s, 0, 0, 1), v2=(0, s, 0, 1), o=(0.25 * s, 0.25 * s, -1, 1))
        add(v0=(0, 0, 0, 1), v1=(s, 0, 0, 1), v2=(0, s, 0, 1), o=(0.25 * s, 0.25 * s, -s, 1))
    zero = (0, 0, 0, 0)
    add(n0=zero, n1=zero, n2=zero)                                     # vertex normals: zero, partly zero,
    add(n0=zero)
    add(n0=(0, 0, -5e-6, 0), n1=(0, 0, -5e-6, 0), n2=(0, 0, -5e-6, 0))  # under is_null's 1e-5,
    add(n0=(0, 0, -2e-5, 0), n1=(0, 0, -2e-5, 0), n2=(0, 0, -2e-5, 0))  # just over it,
    add(n0=(0, 0, -300, 0), n1=(3, 0, -0.01, 0), n2=(0, 7, -2, 0))     # far from unit,
    add(n0=(0, 0, 1, 0), n1=(0, 0, -1, 0), n2=(0, 0, 1, 0), o=(0.5, 0.25, -1, 1))   # cancelling to zero,
    add(n0=(np.inf, 0, -1, 0), n1=nz, n2=nz)                           # and not finite
    add(n0=(0, 0, -1, 7), n1=(0, 0, -1, 7), n2=(0, 0, -1, 7))          # a w component is carried along
    keys = list(rnd)
    edge = _stack(cases, keys)
    return {k: np.concatenate([rnd[k], edge[k].reshape((-1,) + rnd[k].shape[1:])]) for k in keys}


def sphere_inputs(n_random):
    rng = np.random.default_rng(102)
    n = n_random
    c = _v4(rng.normal(size=(n, 3)) * 3.0, 0.0)
    r = (10.0 ** rng.uniform(-2, 1.5, size=n)).astype(F32)
    o = _v4(rng.normal(size=(n, 3)) * 4.0, 1.0)
    near = c[:, :3] + rng.normal(size=(n, 3)) * r[:, None] * 0.7
    d = _v4(np.where(rng.random((n, 1)) < 0.7, _unit(near - o[:, :3]), _unit(rng.normal(size=(n, 3)))), 0.0)
    t_min = np.full(n, T_MIN, F32)
    t_max = np.where(rng.random(n) < 0.8, T_MAX, (10.0 ** rng.uniform(-1, 1.5, size=n))).astype(F32)
    rnd = dict(c=c, r=r, o=o, d=d, t_min=t_min, t_max=t_max)
    cases = []

    def add(c=(0, 0, 0, 0), r=1.0, o=(0, 0, -3, 1), d=(0, 0, 1, 0), t_min=T_MIN, t_max=T_MAX):
        cases.append(dict(c=c, r=r, o=o, d=d, t_min=t_min, t_max=t_max))

    for k in (-2, -1, 0, 1, 2):                                        # tangent: discriminant 0 and a few ulps around
        add(o=(_up(1, k), 0, -3, 1))
        add(o=(0, _up(1, k), -3, 1))
        add(r=_up(1, k), o=(1, 0, -3, 1))
        add(c=(0, 0, 0, 0), r=_up(0.5, k), o=(0.3, 0.4, -2, 1))
    add(o=(0, 0, 0, 1))                                                # origin inside: the far root
    add(o=(0.3, -0.2, 0.5, 1), d=_v4(_unit([1, 2, -1])))
    add(o=(0, 0, 0, 1), t_max=F32(0.5))                                # ... which is not checked against t_max
    add(o=(0, 0, -1, 1))                                               # origin on the surface
    add(o=(0, 0, 1, 1))
    add(o=(0, 0, 3, 1))                                                # sphere behind the ray
    add(o=(0, 0, 3, 1), d=_v4(_unit([0.1, 0, 1])))
    for rad in (0.0, 1e-30, 1e-12, 1e4, 1e10, 1e19, 1e30):             # radius 0 ... huge (r*r overflows)
        add(r=rad, o=(0, 0, -3, 1))
        add(r=rad, o=(0, 0, 0, 1))
        add(c=(0, -rad, 0, 0), r=rad, o=(0, 1, -3, 1), d=_v4(_unit([0, -1, 3])))
    for tm in (F32(2), _up(2, -1), _up(2, 1)):                         # near root t == 2 against both bounds
        add(t_max=tm)
        add(t_min=tm)
    for tm in (F32(1), _up(1, -1), _up(1, 1)):                         # far root t == 1 against both bounds
        add(o=(0, 0, 0, 1), t_min=tm)
        add(o=(0, 0, 0, 1), t_max=tm)
    add(t_min=F32(2), t_max=F32(2))
    add(c=(0, 0, 0, 9), o=(0, 0, -3, 5))                               # w components are carried along
    edge = _stack(cases, list(rnd))
    return {k: np.concatenate([rnd[k], edge[k].reshape((-1,) + rnd[k].shape[1:])]) for k in rnd}


def onb_inputs(n_random):
    rng = np.random.default_rng(103)
    rnd = _v4(rng.normal(size=(n_random, 3)) * 10.0 ** rng.uniform(-3, 3, size=(n_random, 1)), 0.0)
    cases = []
    for ax in range(3):
        for s in (1.0, -1.0, 0.3, -250.0):
            e = [0.0, 0.0, 0.0]
            e[ax] = s
            cases.append(e)
    y = float(np.sqrt(1 - 0.81))
    for k in range(-3, 4):                                             # around the |x| > 0.9 switch of the basis
        for sgn in (1, -1):
            cases.append([sgn * _up(0.9, k), y, 0.0])
            cases.append([sgn * _up(0.9, k), 0.0, -y])
            cases.append([sgn * 9.0 * (1 + k * 1e-7), 0.0, 10 * y])    # not normalised on input
    cases += [[0, 0, 0], [5e-6, -5e-6, 5e-6], [2e-5, 0, 0], [0, 1e-5, 0], [1e20, 1e20, 0], [np.inf, 0, 0]]
    return {"n": np.concatenate([rnd, _v4(np.array(cases, F32), 0.0)])}


def real_inputs(n_random):
    rng = np.random.default_rng(104)
    lo = rng.uniform(-10, 10, size=n_random).astype(F32)
    hi = (lo + rng.uniform(0, 20, size=n_random)).astype(F32)
    pick = rng.integers(0, 4, size=n_random)
    lo = np.where(pick == 0, F32(-0.5), np.where(pick == 1, F32(0.0), lo)).astype(F32)
    hi = np.where(pick == 0, F32(0.5), np.where(pick == 1, F32(1.0), hi)).astype(F32)
    # edges: the smallest and largest draws (u = 0, and u = 1.0 exactly: (float)UINT32_MAX is 2^32) and the rounding
    # boundary below 2^32, over the two ranges the reference uses
    es = np.concatenate([_draw_states(x) for x in _EDGE_DRAWS] * 2)
    ne = len(_EDGE_DRAWS)
    return {"states": np.concatenate([_states(rng, n_random), es]),
            "lo": np.concatenate([lo, np.full(ne, -0.5, F32), np.zeros(ne, F32)]),
            "hi": np.concatenate([hi, np.full(ne, 0.5, F32), np.ones(ne, F32)])}


_WEYL = 362437
_EDGE_DRAWS = (0, 1, 127, 128, 129, 0x7fffffff, 0x80000000, 0xffffff00 - 129, 0xffffff00 - 128, 0xffffff7f,
               0xffffff80, 0xffffffff, 0xffffffff - _WEYL, 2 ** 32 - _WEYL)


def _draw_states(first):
    """A generator state (all-zero xorshift words, so only the Weyl counter moves) whose next draws are ``first``,
    ``first + 362437``, ..."""
    st = np.zeros((1, 6), np.uint32)
    st[0, 5] = (first - _WEYL) % 2 ** 32
    return st


def cosine_inputs(n_random):
    # edges: u1 = 0 and 1.0 (phi = 2 pi), u2 = 0 and 1.0 (z = 0), from crafted states
    es = np.concatenate([_draw_states(x) for x in _EDGE_DRAWS])
    return {"states": np.concatenate([_states(np.random.default_rng(105), n_random), es])}


def scatter_inputs(n_random):
    rng = np.random.default_rng(106)
    n = n_random
    p = _v4(rng.normal(size=(n, 3)) * 3.0, 1.0)
    nrm = _v4(_unit(rng.normal(size=(n, 3))), 0.0)
    d_in = _v4(_unit(rng.normal(size=(n, 3))), 0.0)
    cases = []
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), tuple(_unit([1, 2, 3])),
            tuple(_unit([0.9, np.sqrt(0.19), 0])), tuple(_unit([-0.95, 0.1, 0.2]))]
    for a in axes:
        a = np.array(a, F32)
        t = _unit(np.cross(a, [0.3, -0.5, 0.8]))
        cases.append((a, -a))                                          # head-on
        cases.append((a, a))                                           # the normal is opposite the ray's side
        cases.append((a, t))                                           # grazing: exactly perpendicular
        for g in (1e-3, 1e-5, 1e-7):
            cases.append((a, _unit(t - g * a)))                        # grazing from above
            cases.append((a, _unit(t + g * a)))                        # and from below
        cases.append((2.5 * a, -a))                                    # a normal that is not unit
        cases.append((1e-6 * a, -a))                                   # one under is_null's epsilon
    ne = np.array([c[0] for c in cases], F32)
    de = np.array([c[1] for c in cases], F32)
    pe = np.tile(np.array([[0.25, 1.0, -0.5]], F32), (len(cases), 1))
    nall = n + len(cases)
    return {"p": np.concatenate([p, _v4(pe, 1.0)]), "n": np.concatenate([nrm, _v4(ne, 0.0)]),
            "d": np.concatenate([d_in, _v4(de, 0.0)]), "states": _states(rng, nall)}


def matrix_inputs(n_random):
    rng = np.random.default_rng(107)
    mats = [np.eye(4)]
    for s in (2.0, 0.5, 0.03, 0.0216, 0.0215, 0.01, 1e-4, 50.0):       # uniform scales across the 1e-5 determinant quirk
        mats.append(np.diag([s, s, s, 1.0]))
    mats += [np.diag([2.0, 4.0, 8.0, 1.0]), np.diag([2.0, 2.0, 1.0, 1.0]), np.diag([0.6, 0.6, 1.0, 1.0]),
             np.diag([-1.0, 1.0, 1.0, 1.0]), np.diag([1.0, -3.0, 0.5, 1.0])]
    sc = Scene()
    sc.add_mesh_tri("t")
    rots = [(np.pi / 2, 0, 0), (-np.pi / 2, 0, 0), (0, np.pi / 2, 0), (0, -np.pi / 2, 0), (0, 0, np.pi / 3),
            (0.3, -1.1, 2.0), (3.0, 3.0, 3.0)]
    for i, r in enumerate(rots):                                       # rotations (with scale and translation)
        sc.add_model(f"m{i:02d}", "t", scale=[1 + i, 2.0, 0.5, 1.0], rotation=list(r) + [0.0],
                     translation=[0.5 * i, -1.0, 2.0, 0.0])
    mats += [it["transform"].astype(np.float64) for it in sc.draw_list()]
    z = np.eye(4)
    z[1, :3] = 0.0
    mats.append(z)                                                     # singular: a zero row
    z = np.eye(4)
    z[2, :3] = z[0, :3] * 2
    mats.append(z)                                                     # singular: dependent rows
    rnd = rng.normal(size=(n_random, 4, 4)) * 10.0 ** rng.uniform(-1.5, 1.5, size=(n_random, 1, 1))
    rnd[:, :3, 3] = 0.0
    rnd[:, 3, 3] = 1.0
    m = np.ascontiguousarray(np.concatenate([rnd, np.array(mats)]).astype(F32).reshape(-1, 16))
    p3 = np.ascontiguousarray((rng.normal(size=(len(m), 3)) * 2.0).astype(F32))
    return {"m": m, "p3": p3}


CAMERAS = {   # the default camera and the three others of tests/test_gpu_camera.py
    "default": {},
    "pitch_up": dict(position=(0.0, -2.0, 4.0, 0.0), forward=(0.0, 1.7, 3.0, 0.0), fovh=60.0),
    "origin": dict(position=(0.0, 0.0, 0.0, 0.0), forward=(0.0, 0.0, 3.0, 0.0)),
    "yawed": dict(position=(0.3, 0.5, -3.0, 0.0), forward=(-0.2, -0.5, 3.0, 0.0)),
}
FRAME_SIZES = ((1, 1), (16, 9), (1920, 1080), (3840, 2160))
RANDOM_PIXELS = 24


def camera_cases():
    """(key, camera kwargs, w, h, x, y, states): the four corners, the centre and seeded random pixels."""
    rng = np.random.default_rng(108)
    for cname, kw in CAMERAS.items():
        for w, h in FRAME_SIZES:
            xs = [0, w - 1, 0, w - 1, w // 2] + list(rng.integers(0, w, size=RANDOM_PIXELS))
            ys = [0, 0, h - 1, h - 1, h // 2] + list(rng.integers(0, h, size=RANDOM_PIXELS))
            yield (f"{cname}_{w}x{h}", kw, w, h, np.array(xs, np.uint32), np.array(ys, np.uint32),
                   _states(rng, len(xs)))


MESHES = ([("tri", 0, 0, TRI), ("quad", 0, 0, TRI), ("reg_polygon", 3, 0, TRI), ("reg_polygon", 4, 0, TRI),
           ("reg_polygon", 7, 0, TRI), ("cube", 0, 0, TRI)]
          + [("uv_sphere", s, r, t, flat) for (s, r) in ((4, 2), (16, 8), (32, 16), (128, 64)) for t in (TRI, SPH)
             for flat in (False, True)])


def mesh_key(spec):
    gen, a, b, t = spec[:4]
    flat = spec[4] if len(spec) > 4 else False
    return f"{gen}_{a}_{b}_{'tri' if t == TRI else 'sph'}{'_flat' if flat else ''}"


# ------------------------------------------------------------------------------------------------ scenes
PI_2 = float(F32(1.5707963267948966))


def _m(name, mesh, scale, rotation=(0, 0, 0, 0), translation=(0, 0, 0, 0)):
    s = [float(scale)] * 4 if np.isscalar(scale) else list(scale)
    return (name, mesh, [float(x) for x in s], [float(x) for x in rotation], [float(x) for x in translation])


_WALL = (2.0, 2.0, 1.0, 1.0)
SCENES = {   # plain descriptions of the project's presets (csrc/iq_scene.cpp) and of two scenes of the suite
    "app_default": dict(
        meshes=[("default", "tri", 0, 0, False, TRI), ("cube", "cube", 0, 0, False, TRI),
                ("sphere", "uv_sphere", 128, 64, False, SPH)],
        models=[_m("ground", "sphere", 10.0, (PI_2, 0, 0, 0), (0, -10, 0, 0)), _m("sph", "sphere", 0.5, translation=(0, 0.5, 0, 0)),
                _m("wall", "cube", 1.0, translation=(1, 0.5, 0, 0))]),
    "c1_plumbing": dict(
        meshes=[("light", "uv_sphere", 16, 8, False, TRI), ("sphere", "uv_sphere", 32, 16, False, SPH)],
        models=[_m("lamp", "light", 0.5, translation=(1, 1, 0, 0)), _m("ball", "sphere", 0.5, translation=(0, 0.5, 0, 0))]),
    "cornell": dict(
        meshes=[("quad", "quad", 0, 0, False, TRI), ("sphere", "uv_sphere", 32, 16, False, SPH)],
        models=[_m("back", "quad", _WALL, translation=(0, 0.5, 1, 0)),
                _m("floor", "quad", _WALL, (PI_2, 0, 0, 0), (0, -0.5, 0, 0)),
                _m("ceiling", "quad", _WALL, (-PI_2, 0, 0, 0), (0, 1.5, 0, 0)),
                _m("left", "quad", _WALL, (0, PI_2, 0, 0), (-1, 0.5, 0, 0)),
                _m("right", "quad", _WALL, (0, -PI_2, 0, 0), (1, 0.5, 0, 0)),
                _m("sphere_big", "sphere", 0.35, translation=(-0.4, -0.15, 0.2, 0)),
                _m("sphere_small", "sphere", 0.25, translation=(0.45, -0.25, -0.2, 0))]),
    "emissive_mesh": dict(   # an emissive uv_sphere(16, 8) mesh over a diffuse sphere
        meshes=[("light", "uv_sphere", 16, 8, False, TRI), ("sphere", "uv_sphere", 32, 16, False, SPH)],
        models=[_m("lamp", "light", (0.6, 0.3, 0.6, 1.0), (0.0, 0.4, 0.2, 0.0), (0.1, 1.4, 0.0, 0.0)),
                _m("ball", "sphere", 0.6, translation=(0, 0.4, 0, 0))]),
    "shell": dict(           # tests/test_oracle_props.py: the camera inside a huge Oren-Nayar sphere
        meshes=[("sphere", "uv_sphere", 32, 16, False, SPH)],
        models=[_m("shell", "sphere", 50.0)]),
}
PRESETS = ("app_default", "c1_plumbing", "cornell")

# name: (scene, W, H, steps, max_depth); a step is a number of launches or "reset"
FRAMES = {
    "app_default": ("app_default", 96, 54, [4], 5),
    "c1_plumbing": ("c1_plumbing", 64, 64, [1], 2),
    "cornell": ("cornell", 96, 54, [4, 4], 8),
    "emissive_mesh": ("emissive_mesh", 48, 27, [2], 8),
    "shell_d1": ("shell", 16, 8, [2], 1),
    "shell_d2": ("shell", 16, 8, [2], 2),
    "shell_d5": ("shell", 16, 8, [2], 5),
    "reset": ("app_default", 32, 18, [3, "reset", 2], 5),
}


def project_scene(name) -> Scene:
    """The description replayed through the project's scene builder."""
    desc = SCENES[name]
    sc = Scene()
    for mname, gen, a, b, flat, mtype in desc["meshes"]:
        if gen == "tri":
            sc.add_mesh_tri(mname)
        elif gen == "quad":
            sc.add_mesh_quad(mname)
        elif gen == "cube":
            sc.add_mesh_cube(mname)
        elif gen == "reg_polygon":
            sc.add_mesh_reg_polygon(mname, a)
        else:
            sc.add_mesh_uv_sphere(mname, flat, a, b, mtype)
    for mname, mesh, s, r, t in desc["models"]:
        sc.add_model(mname, mesh, scale=s, rotation=r, translation=t)
    return sc


def packet_arrays(pk) -> dict:
    """A PacketDesc (include/iqpt.h) as flat arrays."""
    nt, ns = pk.num_drawcalls[TRI], pk.num_drawcalls[SPH]
    out = {"counts": np.array([nt, ns, pk.num_tri_meshes], np.uint32)}
    for i in range(pk.num_tri_meshes):
        m = pk.tri_meshes[i]
        out[f"mesh{i}.vertices"] = np.ctypeslib.as_array(C.cast(m.vertices, FP), (m.num_vertices, 6)).copy()
        out[f"mesh{i}.indices"] = np.ctypeslib.as_array(C.cast(m.indices, UP), (m.num_indices,)).copy()
    out["tri.transform"] = np.array([list(pk.tri_mesh_dcs[i].transform) for i in range(nt)], F32).reshape(nt, 16)
    out["tri.mesh_id"] = np.array([pk.tri_mesh_dcs[i].mesh_id for i in range(nt)], np.uint32)
    out["sphere.center"] = np.array([list(pk.sphere_dcs[i].center) for i in range(ns)], F32).reshape(ns, 4)
    out["sphere.radius"] = np.array([pk.sphere_dcs[i].radius for i in range(ns)], F32)
    return out


def ref_packet_arrays(ref_scene) -> dict:
    p = ref_scene.packet()
    nt, ns = len(p["tri_dcs"]), len(p["sphere_dcs"])
    out = {"counts": np.array([nt, ns, len(p["meshes"])], np.uint32)}
    for i, (v, idx) in enumerate(p["meshes"]):
        out[f"mesh{i}.vertices"], out[f"mesh{i}.indices"] = v, idx
    out["tri.transform"] = np.array([m for m, _ in p["tri_dcs"]], F32).reshape(nt, 16)
    out["tri.mesh_id"] = np.array([i for _, i in p["tri_dcs"]], np.uint32)
    out["sphere.center"] = np.array([c for c, _ in p["sphere_dcs"]], F32).reshape(ns, 4)
    out["sphere.radius"] = np.array([r for _, r in p["sphere_dcs"]], F32)
    return out


def canonical_packet(d: dict) -> dict:
    """Drawcalls as sorted rows. The reference orders models that share a mesh by the address of their std::map node
    (scene.h's model_comparator: `return a < b`), which the heap decides; the project uses insertion order. The order
    only matters to a ray that hits two primitives at exactly the same t, so packets are compared as sets of
    drawcalls (the mesh id stays part of each row) and frames pin that no such tie occurs in the scenes compared."""
    out = dict(d)
    for rows in (("tri.transform", "tri.mesh_id"), ("sphere.center", "sphere.radius")):
        a, b = (np.asarray(d[k]) for k in rows)
        if len(a) == 0:
            continue
        key = np.concatenate([bits(a).reshape(len(a), -1), bits(b).reshape(len(a), -1)], axis=1).astype(np.uint64)
        order = np.lexsort(key.T[::-1])
        out[rows[0]], out[rows[1]] = a[order], b[order]
    return out


def camera_arrays(cam) -> dict:
    return {k: np.array(list(getattr(cam, k)), F32) for k in ("view", "projection", "inv_view", "inv_proj")}


# ------------------------------------------------------------------------------------------------ comparing
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def first_difference(a: dict, b: dict, inputs: dict | None = None) -> str | None:
    """None when both dicts hold the same keys and the same bits; else the first differing key and case."""
    if sorted(a) != sorted(b):
        return f"keys differ: {sorted(set(a) ^ set(b))}"
    for k in sorted(a):
        x, y = bits(np.asarray(a[k])), bits(np.asarray(b[k]))
        if x.shape != y.shape:
            return f"{k}: shapes {x.shape} != {y.shape}"
        if not np.array_equal(x, y):
            idx = np.argwhere(x != y)[0]
            msg = f"{k}: {int((x != y).sum())} values differ, first at {tuple(int(i) for i in idx)}: " \
                  f"{np.asarray(a[k])[tuple(idx)]!r} != {np.asarray(b[k])[tuple(idx)]!r}"
            if inputs:
                case = int(idx[0])
                msg += " | inputs of that case: " + ", ".join(
                    f"{n}={np.asarray(v)[case].tolist()}" for n, v in inputs.items() if len(v) > case)
            return msg
    return None


def sha(a) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


# ------------------------------------------------------------------------------------------------ unit runners
def _at(a, i):
    return C.cast(a.ctypes.data + i * a.strides[0], FP if a.dtype == np.float32 else UP)


def unit_inputs(n_random) -> dict:
    return {"tri": triangle_inputs(n_random), "sphere": sphere_inputs(n_random), "onb": onb_inputs(n_random),
            "real": real_inputs(n_random), "cosine": cosine_inputs(n_random), "scatter": scatter_inputs(n_random),
            "matrix": matrix_inputs(n_random)}


def recorded_subset(inputs: dict) -> dict:
    """The cases the fixture records: the first N_RECORDED random ones and every edge case after the random block."""
    return {r: {k: np.concatenate([v[:N_RECORDED], v[N_LIVE:]]) for k, v in d.items()} for r, d in inputs.items()}


def oracle_units(inp: dict, flavour: str) -> dict:
    """Every routine of the oracle's unit hooks on the inputs, one case per call."""
    lib = oracle.load(flavour=flavour)
    out = {}
    t = inp["tri"]
    n = len(t["v0"])
    o = {"hit": np.zeros(n, np.int32), "t": np.zeros(n, F32), "p": np.zeros((n, 4), F32), "n": np.zeros((n, 4), F32),
         "front": np.zeros(n, np.int32)}
    tv, fr = C.c_float(), C.c_int()
    for i in range(n):
        o["hit"][i] = lib.iqo_triangle_intersect(*(_at(t[k], i) for k in ("v0", "v1", "v2", "n0", "n1", "n2", "o", "d")),
                                                 t["t_min"][i], t["t_max"][i], C.byref(tv), _at(o["p"], i),
                                                 _at(o["n"], i), C.byref(fr))
        if o["hit"][i]:
            o["t"][i], o["front"][i] = tv.value, fr.value
    out.update({f"tri.{k}": v for k, v in o.items()})

    s = inp["sphere"]
    n = len(s["c"])
    o = {"hit": np.zeros(n, np.int32), "t": np.zeros(n, F32), "p": np.zeros((n, 4), F32), "n": np.zeros((n, 4), F32),
         "front": np.zeros(n, np.int32)}
    for i in range(n):
        o["hit"][i] = lib.iqo_sphere_intersect(_at(s["c"], i), s["r"][i], _at(s["o"], i), _at(s["d"], i), s["t_min"][i],
                                               s["t_max"][i], C.byref(tv), _at(o["p"], i), _at(o["n"], i), C.byref(fr))
        if o["hit"][i]:
            o["t"][i], o["front"][i] = tv.value, fr.value
    out.update({f"sphere.{k}": v for k, v in o.items()})

    nn = inp["onb"]["n"]
    o = {k: np.zeros((len(nn), 4), F32) for k in "uvw"}
    for i in range(len(nn)):
        lib.iqo_onb(_at(nn, i), _at(o["u"], i), _at(o["v"], i), _at(o["w"], i))
    out.update({f"onb.{k}": v for k, v in o.items()})

    r = inp["real"]
    st = r["states"].copy()
    val = np.zeros(len(st), F32)
    for i in range(len(st)):
        val[i] = lib.iqo_real(_at(st, i), r["lo"][i], r["hi"][i])
    out.update({"real.value": val, "real.states": st})

    st = inp["cosine"]["states"].copy()
    dirs = np.zeros((len(st), 4), F32)
    for i in range(len(st)):
        lib.iqo_cosine_weighted(_at(st, i), _at(dirs, i))
    out.update({"cosine.dir": dirs, "cosine.states": st})

    sc = inp["scatter"]
    n = len(sc["p"])
    st = sc["states"].copy()
    o = {"att": np.zeros((n, 4), F32), "pdf": np.zeros(n, F32), "cosw": np.zeros(n, F32), "ro": np.zeros((n, 4), F32),
         "rd": np.zeros((n, 4), F32), "ret": np.zeros(n, np.int32)}
    pdf, cw = C.c_float(), C.c_float()
    for i in range(n):
        o["ret"][i] = lib.iqo_oren_nayar(_at(sc["p"], i), _at(sc["n"], i), _at(sc["d"], i), _at(st, i), _at(o["att"], i),
                                         C.byref(pdf), C.byref(cw), _at(o["ro"], i), _at(o["rd"], i))
        o["pdf"][i], o["cosw"][i] = pdf.value, cw.value
    out.update({f"oren_nayar.{k}": v for k, v in o.items()})
    out["oren_nayar.states"] = st
    # emissive::scatter reads none of its arguments: one record, repeated for every case, and an untouched generator
    att = np.zeros(4, F32)
    ret = lib.iqo_emissive(att.ctypes.data_as(FP), C.byref(pdf), C.byref(cw))
    out.update({"emissive.att": np.tile(att, (n, 1)), "emissive.pdf": np.full(n, pdf.value, F32),
                "emissive.cosw": np.full(n, cw.value, F32), "emissive.ret": np.full(n, ret, np.int32),
                "emissive.states": sc["states"].copy()})

    m, p3 = inp["matrix"]["m"], inp["matrix"]["p3"]
    nm, tp = np.zeros_like(m), np.zeros((len(m), 4), F32)
    for i in range(len(m)):
        lib.iqo_normal_matrix(_at(m, i), _at(nm, i))
        lib.iqo_transform_point(_at(p3, i), _at(m, i), _at(tp, i))
    out.update({"normal_matrix.m": nm, "transform.v": tp})
    return out


def ref_units(inp: dict, ref) -> dict:
    """The same routines of the reference's own source (ref: oracle/ref_oracle.py library)."""
    out = {}
    t, s, sc = inp["tri"], inp["sphere"], inp["scatter"]
    out.update({f"tri.{k}": v for k, v in ref.triangle_intersect(
        *(t[k] for k in ("v0", "v1", "v2", "n0", "n1", "n2", "o", "d", "t_min", "t_max"))).items()})
    out.update({f"sphere.{k}": v for k, v in ref.sphere_intersect(
        *(s[k] for k in ("c", "r", "o", "d", "t_min", "t_max"))).items()})
    out.update({f"onb.{k}": v for k, v in ref.onb(inp["onb"]["n"]).items()})
    out.update({f"real.{k}": v for k, v in ref.real(inp["real"]["states"], inp["real"]["lo"], inp["real"]["hi"]).items()})
    out.update({f"cosine.{k}": v for k, v in ref.cosine_weighted(inp["cosine"]["states"]).items()})
    out.update({f"oren_nayar.{k}": v for k, v in ref.oren_nayar(sc["p"], sc["n"], sc["d"], sc["states"]).items()})
    out.update({f"emissive.{k}": v for k, v in ref.emissive(sc["p"], sc["n"], sc["d"], sc["states"]).items()})
    out["normal_matrix.m"] = ref.normal_matrix(inp["matrix"]["m"])["m"]
    out["transform.v"] = ref.transform_point(inp["matrix"]["p3"], inp["matrix"]["m"])["v"]
    return out


MATRICES = ("view", "projection", "inv_view", "inv_proj")


def recorded_camera_cases(g: dict):
    """camera_cases() with the pixels and states a fixture holds (numpy promises no stream across versions)."""
    for key, kw, w, h, _xs, _ys, _states in camera_cases():
        yield key, kw, w, h, g[f"in.camera.{key}.x"], g[f"in.camera.{key}.y"], g[f"in.camera.{key}.states"]


def project_cameras(flavour: str, matrices: dict | None = None, cases=None) -> dict:
    """make_camera's matrices and the oracle's get_ray for every camera case. With ``matrices`` (a ref_cameras()
    result), the oracle's get_ray runs on those matrices instead of make_camera's."""
    lib = oracle.load(flavour=flavour)
    out = {}
    for key, kw, w, h, xs, ys, states in (cases if cases is not None else camera_cases()):
        cam = make_camera(w, h, **kw)
        if matrices is not None:
            for k in MATRICES:
                getattr(cam, k)[:] = [float(x) for x in matrices[f"{key}.{k}"]]
        out.update({f"{key}.{k}": v for k, v in camera_arrays(cam).items()})
        st = states.copy()
        o, d = np.zeros((len(st), 4), F32), np.zeros((len(st), 4), F32)
        for i in range(len(st)):
            lib.iqo_get_ray(C.byref(cam), int(xs[i]), int(ys[i]), _at(st, i), _at(o, i), _at(d, i))
        out.update({f"{key}.o": o, f"{key}.d": d, f"{key}.states": st})
    return out


def ref_cameras(ref, cases=None) -> dict:
    out = {}
    for key, kw, w, h, xs, ys, states in (cases if cases is not None else camera_cases()):
        cam = ref.camera(w, h, kw.get("fovh", 45.0), position=kw.get("position"), forward=kw.get("forward"))
        out.update({f"{key}.{k}": v for k, v in cam.matrices().items()})
        out.update({f"{key}.{k}": v for k, v in cam.get_ray(xs, ys, states).items()})
    return out


def model_transform_cases():
    seen, cases = set(), []
    for desc in SCENES.values():
        for _n, _mesh, s, r, t in desc["models"]:
            if (tuple(s), tuple(r), tuple(t)) not in seen:
                seen.add((tuple(s), tuple(r), tuple(t)))
                cases.append((s, r, t))
    rng = np.random.default_rng(109)
    for _ in range(64):
        cases.append(([float(F32(x)) for x in rng.uniform(0.1, 3, size=4)],
                      [float(F32(x)) for x in rng.uniform(-4, 4, size=4)],
                      [float(F32(x)) for x in rng.normal(size=4) * 3]))
    return cases


def project_model_transforms(cases=None) -> dict:
    sc = Scene()
    sc.add_mesh_tri("t")
    cases = cases if cases is not None else model_transform_cases()
    for i, (s, r, t) in enumerate(cases):
        sc.add_model(f"m{i:04d}", "t", scale=s, rotation=r, translation=t)
    return {"model.transform": np.array([it["transform"].reshape(16) for it in sc.draw_list()], F32)}


def ref_model_transforms(ref, cases=None) -> dict:
    cases = cases if cases is not None else model_transform_cases()
    return {"model.transform": np.array([ref.model_transform(s, r, t) for s, r, t in cases], F32)}


def project_mesh(spec) -> dict:
    gen, a, b, mtype = spec[:4]
    flat = spec[4] if len(spec) > 4 else False
    sc = Scene()
    if gen == "tri":
        sc.add_mesh_tri("m")
    elif gen == "quad":
        sc.add_mesh_quad("m")
    elif gen == "cube":
        sc.add_mesh_cube("m")
    elif gen == "reg_polygon":
        sc.add_mesh_reg_polygon("m", a)
    else:
        sc.add_mesh_uv_sphere("m", flat, a, b, mtype)
    sc.add_model("model", "m")
    it = sc.draw_list()[0]
    out = {"vertices": it["vertices"], "indices": it["indices"], "mesh_type": np.array([it["mesh_type"]], np.int32)}
    if mtype == TRI:   # and as the packet carries it to the path tracer
        pk = packet_arrays(sc.build_packet())
        out["packet.vertices"], out["packet.indices"] = pk["mesh0.vertices"], pk["mesh0.indices"]
    return out


def ref_mesh(ref, spec) -> dict:
    gen, a, b, mtype = spec[:4]
    flat = spec[4] if len(spec) > 4 else False
    m = ref.mesh(gen, a, b, flat, mtype)
    out = {"vertices": m["vertices"], "indices": m["indices"], "mesh_type": np.array([m["mesh_type"]], np.int32)}
    if mtype == TRI:
        out["packet.vertices"], out["packet.indices"] = m["vertices"], m["indices"]
    return out


# ------------------------------------------------------------------------------------------------ frames
def oracle_frame(name: str, flavour: str) -> dict:
    scene, w, h, steps, depth = FRAMES[name]
    sc = project_scene(scene)
    pk = sc.build_packet()
    cam = make_camera(w, h)
    fr = oracle.OracleFrame(w, h, max_depth=depth, flavour=flavour)
    for s in steps:
        if s == "reset":
            fr.reset()
        else:
            fr.render(pk, cam, s)
    return {"lin": fr.lin, "bgra": fr.bgra, "states": fr.states}


def ref_frame(name: str, ref) -> dict:
    import ref_oracle
    scene, w, h, steps, depth = FRAMES[name]
    rs = ref_oracle.RefScene(ref, SCENES[scene]["meshes"], SCENES[scene]["models"])
    fr = ref_oracle.RefFrame(ref, w, h, depth)
    for s in steps:
        if s == "reset":
            fr.reset()
        else:
            fr.render(rs, s)
    return fr.read()


def frame_inputs(name: str) -> dict:
    """What the project feeds the renderers for a frame case: packet and camera, as flat arrays."""
    scene, w, h, _steps, _depth = FRAMES[name]
    sc = project_scene(scene)
    out = {f"packet.{k}": v for k, v in canonical_packet(packet_arrays(sc.build_packet())).items()}
    out.update({f"camera.{k}": v for k, v in camera_arrays(make_camera(w, h)).items()})
    return out


def ref_frame_inputs(name: str, ref) -> dict:
    import ref_oracle
    scene, w, h, _steps, depth = FRAMES[name]
    rs = ref_oracle.RefScene(ref, SCENES[scene]["meshes"], SCENES[scene]["models"])
    out = {f"packet.{k}": v for k, v in canonical_packet(ref_packet_arrays(rs)).items()}
    out.update({f"camera.{k}": v for k, v in ref_oracle.RefFrame(ref, w, h, depth).camera_matrices().items()})
    return out
