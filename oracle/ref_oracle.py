"""TEST INFRASTRUCTURE ONLY — ctypes wrapper of the reference's own source built as a host library
(oracle/_ref/libref_<flavour>.so, made by oracle/ref/build_ref.py from oracle/ref/ref_driver.cpp).

Flavour "a" is glibc libm (none of this project's arithmetic on the reference side, never recorded: glibc differs
between machines); flavour "b" redirects the reference's six transcendentals to csrc/iq_fp.h and is the bit-exact
target of the oracle and the kernels. The random generator is csrc/iq_xorwow.h on both sides: cuRAND is the one
part the reference does not contain.

Only tests/ and tests/golden/make_ref_golden.py import this module; nothing that runs on a GPU does.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
REF_DIR = _HERE / "_ref"
_cache: dict[str, "RefLib"] = {}

MESH_TRIANGLES, MESH_SPHERES = 0, 1
_P = C.c_void_p


def lib_path(flavour: str) -> Path:
    return REF_DIR / f"libref_{flavour}.so"


def available(flavour: str = "b") -> bool:
    return lib_path(flavour).exists()


def _p(a: np.ndarray):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def f32(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.reshape(shape) if shape is not None else a


class RefLib:
    def __init__(self, flavour: str):
        self.flavour = flavour
        lib = C.CDLL(str(lib_path(flavour)))
        assert lib.ref_flavour_b() == (1 if flavour == "b" else 0)
        i64 = C.c_int64
        lib.ref_triangle_intersect.argtypes = [i64] + [_P] * 15
        lib.ref_sphere_intersect.argtypes = [i64] + [_P] * 11
        lib.ref_onb.argtypes = [i64] + [_P] * 4
        lib.ref_real.argtypes = [i64] + [_P] * 4
        lib.ref_cosine_weighted.argtypes = [i64, _P, _P]
        lib.ref_oren_nayar.argtypes = [i64, _P, C.c_float] + [_P] * 10
        lib.ref_emissive.argtypes = [i64, _P, C.c_float] + [_P] * 8
        lib.ref_normal_matrix.argtypes = [i64, _P, _P]
        lib.ref_transform_point.argtypes = [i64, _P, _P, _P]
        lib.ref_model_transform.argtypes = [_P] * 4
        lib.ref_camera_create.argtypes = [C.c_uint16, C.c_uint16, C.c_float, C.c_float, C.c_float, _P, _P]
        lib.ref_camera_create.restype = _P
        lib.ref_camera_destroy.argtypes = [_P]
        lib.ref_camera_matrices.argtypes = [_P] * 5
        lib.ref_get_ray.argtypes = [_P, i64] + [_P] * 5
        lib.ref_mesh_generate.argtypes = [C.c_char_p, C.c_uint, C.c_uint, C.c_int, C.c_int, _P, C.c_uint32, _P,
                                          C.c_uint32, _P]
        lib.ref_scene_create.restype = _P
        lib.ref_scene_destroy.argtypes = [_P]
        lib.ref_scene_add_mesh.argtypes = [_P, C.c_char_p, C.c_char_p, C.c_uint, C.c_uint, C.c_int, C.c_int]
        lib.ref_scene_add_model.argtypes = [_P, C.c_char_p, C.c_char_p, _P, _P, _P]
        lib.ref_scene_build.argtypes = [_P]
        lib.ref_packet_counts.argtypes = [_P, _P]
        lib.ref_packet_mesh_counts.argtypes = [_P, C.c_uint32, _P]
        lib.ref_packet_mesh.argtypes = [_P, C.c_uint32, _P, _P]
        lib.ref_packet_tri_drawcall.argtypes = [_P, C.c_uint32, _P, _P]
        lib.ref_packet_sphere_drawcall.argtypes = [_P, C.c_uint32, _P, _P]
        lib.ref_frame_create.argtypes = [C.c_uint16, C.c_uint16, C.c_int]
        lib.ref_frame_create.restype = _P
        lib.ref_frame_destroy.argtypes = [_P]
        lib.ref_frame_reset.argtypes = [_P]
        lib.ref_frame_render.argtypes = [_P, _P, C.c_uint32]
        lib.ref_frame_read.argtypes = [_P] * 4
        lib.ref_frame_camera.argtypes = [_P] * 5
        self.lib = lib

    # ---- unit level: dicts of arrays in, dicts of arrays out (the layout of tests/ref_cases.py)
    def triangle_intersect(self, v0, v1, v2, n0, n1, n2, o, d, t_min, t_max):
        n = len(v0)
        out = {"hit": np.zeros(n, np.int32), "t": np.zeros(n, np.float32), "p": np.zeros((n, 4), np.float32),
               "n": np.zeros((n, 4), np.float32), "front": np.zeros(n, np.int32)}
        self.lib.ref_triangle_intersect(n, *map(_p, (v0, v1, v2, n0, n1, n2, o, d, t_min, t_max)),
                                        _p(out["hit"]), _p(out["t"]), _p(out["p"]), _p(out["n"]), _p(out["front"]))
        return out

    def sphere_intersect(self, c, r, o, d, t_min, t_max):
        n = len(c)
        out = {"hit": np.zeros(n, np.int32), "t": np.zeros(n, np.float32), "p": np.zeros((n, 4), np.float32),
               "n": np.zeros((n, 4), np.float32), "front": np.zeros(n, np.int32)}
        self.lib.ref_sphere_intersect(n, *map(_p, (c, r, o, d, t_min, t_max)),
                                      _p(out["hit"]), _p(out["t"]), _p(out["p"]), _p(out["n"]), _p(out["front"]))
        return out

    def onb(self, nrm):
        n = len(nrm)
        out = {k: np.zeros((n, 4), np.float32) for k in "uvw"}
        self.lib.ref_onb(n, _p(nrm), _p(out["u"]), _p(out["v"]), _p(out["w"]))
        return out

    def real(self, states, lo, hi):
        st = states.copy()
        out = np.zeros(len(st), np.float32)
        self.lib.ref_real(len(st), _p(st), _p(lo), _p(hi), _p(out))
        return {"value": out, "states": st}

    def cosine_weighted(self, states):
        st = states.copy()
        out = np.zeros((len(st), 4), np.float32)
        self.lib.ref_cosine_weighted(len(st), _p(st), _p(out))
        return {"dir": out, "states": st}

    def oren_nayar(self, p, nrm, d_in, states, albedo=(0.5, 0.5, 0.5, 0.0), sigma=1.0):
        n = len(p)
        st = states.copy()
        out = {"att": np.zeros((n, 4), np.float32), "pdf": np.zeros(n, np.float32), "cosw": np.zeros(n, np.float32),
               "ro": np.zeros((n, 4), np.float32), "rd": np.zeros((n, 4), np.float32), "ret": np.zeros(n, np.int32)}
        alb = f32(albedo)
        self.lib.ref_oren_nayar(n, _p(alb), sigma, _p(p), _p(nrm), _p(d_in), _p(st), _p(out["att"]),
                                _p(out["pdf"]), _p(out["cosw"]), _p(out["ro"]), _p(out["rd"]), _p(out["ret"]))
        out["states"] = st
        return out

    def emissive(self, p, nrm, d_in, states, albedo=(1.0, 1.0, 1.0, 1.0), strength=10.0):
        n = len(p)
        st = states.copy()
        out = {"att": np.zeros((n, 4), np.float32), "pdf": np.zeros(n, np.float32), "cosw": np.zeros(n, np.float32),
               "ret": np.zeros(n, np.int32)}
        alb = f32(albedo)
        self.lib.ref_emissive(n, _p(alb), strength, _p(p), _p(nrm), _p(d_in), _p(st), _p(out["att"]),
                              _p(out["pdf"]), _p(out["cosw"]), _p(out["ret"]))
        out["states"] = st
        return out

    def normal_matrix(self, m):
        out = np.zeros_like(m)
        self.lib.ref_normal_matrix(len(m), _p(m), _p(out))
        return {"m": out}

    def transform_point(self, p3, m):
        out = np.zeros((len(p3), 4), np.float32)
        self.lib.ref_transform_point(len(p3), _p(p3), _p(m), _p(out))
        return {"v": out}

    def model_transform(self, scale4, rotation4, translation4):
        out = np.zeros(16, np.float32)
        s, r, t = f32(scale4), f32(rotation4), f32(translation4)
        self.lib.ref_model_transform(_p(s), _p(r), _p(t), _p(out))
        return out

    def camera(self, width, height, fovh=45.0, znear=0.01, zfar=100.0, position=None, forward=None):
        return RefCamera(self, width, height, fovh, znear, zfar, position, forward)

    def mesh(self, generator, a=0, b=0, flat=False, mesh_type=MESH_SPHERES):
        counts = np.zeros(3, np.uint32)
        assert self.lib.ref_mesh_generate(generator.encode(), a, b, int(flat), mesh_type, None, 0, None, 0,
                                          _p(counts)) == 0
        v = np.zeros((int(counts[0]), 6), np.float32)
        i = np.zeros(int(counts[1]), np.uint32)
        self.lib.ref_mesh_generate(generator.encode(), a, b, int(flat), mesh_type, _p(v), len(v), _p(i), len(i),
                                   _p(counts))
        return {"vertices": v, "indices": i, "mesh_type": int(counts[2])}


class RefCamera:
    def __init__(self, ref: RefLib, width, height, fovh, znear, zfar, position, forward):
        self.ref = ref
        pos = f32(position) if position is not None else None
        fwd = f32(forward) if forward is not None else None
        self.h = ref.lib.ref_camera_create(width, height, fovh, znear, zfar, _p(pos) if pos is not None else None,
                                           _p(fwd) if fwd is not None else None)

    def matrices(self):
        m = {k: np.zeros(16, np.float32) for k in ("view", "projection", "inv_view", "inv_proj")}
        self.ref.lib.ref_camera_matrices(self.h, *(_p(m[k]) for k in ("view", "projection", "inv_view", "inv_proj")))
        return m

    def get_ray(self, x, y, states):
        st = states.copy()
        n = len(st)
        out = {"o": np.zeros((n, 4), np.float32), "d": np.zeros((n, 4), np.float32)}
        self.ref.lib.ref_get_ray(self.h, n, _p(np.ascontiguousarray(x, np.uint32)),
                                 _p(np.ascontiguousarray(y, np.uint32)), _p(st), _p(out["o"]), _p(out["d"]))
        out["states"] = st
        return out

    def __del__(self):
        if getattr(self, "h", None):
            self.ref.lib.ref_camera_destroy(self.h)
            self.h = None


class RefScene:
    """The reference's scene built from a plain description: ``meshes`` = [(name, generator, a, b, flat, type)],
    ``models`` = [(name, mesh name, scale4, rotation4, translation4)], added in that order."""

    def __init__(self, ref: RefLib, meshes, models):
        self.ref = ref
        self.h = ref.lib.ref_scene_create()
        for name, gen, a, b, flat, mtype in meshes:
            assert ref.lib.ref_scene_add_mesh(self.h, name.encode(), gen.encode(), a, b, int(flat), mtype) == 0
        for name, mesh_name, s, r, t in models:
            s, r, t = f32(s), f32(r), f32(t)
            ref.lib.ref_scene_add_model(self.h, name.encode(), mesh_name.encode(), _p(s), _p(r), _p(t))
        ref.lib.ref_scene_build(self.h)

    def packet(self) -> dict:
        lib = self.ref.lib
        counts = np.zeros(3, np.uint32)
        lib.ref_packet_counts(self.h, _p(counts))
        out = {"meshes": [], "tri_dcs": [], "sphere_dcs": []}
        for i in range(int(counts[2])):
            mc = np.zeros(2, np.uint32)
            lib.ref_packet_mesh_counts(self.h, i, _p(mc))
            v, idx = np.zeros((int(mc[0]), 6), np.float32), np.zeros(int(mc[1]), np.uint32)
            lib.ref_packet_mesh(self.h, i, _p(v), _p(idx))
            out["meshes"].append((v, idx))
        for i in range(int(counts[0])):
            m, mid = np.zeros(16, np.float32), np.zeros(1, np.uint32)
            lib.ref_packet_tri_drawcall(self.h, i, _p(m), _p(mid))
            out["tri_dcs"].append((m, int(mid[0])))
        for i in range(int(counts[1])):
            c, r = np.zeros(4, np.float32), np.zeros(1, np.float32)
            lib.ref_packet_sphere_drawcall(self.h, i, _p(c), _p(r))
            out["sphere_dcs"].append((c, r[0]))
        return out

    def __del__(self):
        if getattr(self, "h", None):
            self.ref.lib.ref_scene_destroy(self.h)
            self.h = None


class RefFrame:
    """The path tracer's buffers for a width x height window with the reference's camera; ``render(scene, n)`` is n
    launches of the reference's render_kernel as a host loop."""

    def __init__(self, ref: RefLib, width: int, height: int, max_depth: int = 5):
        self.ref, self.width, self.height = ref, width, height
        self.h = ref.lib.ref_frame_create(width, height, max_depth)
        if not self.h:
            raise ValueError(f"libref has no kernel for max_depth {max_depth} (build_ref.DEPTHS)")

    def render(self, scene: RefScene, launches: int):
        assert self.ref.lib.ref_frame_render(self.h, scene.h, launches) == 0

    def reset(self):
        self.ref.lib.ref_frame_reset(self.h)

    def read(self) -> dict:
        n = self.width * self.height
        out = {"lin": np.zeros((n, 4), np.float32), "bgra": np.zeros((n, 4), np.uint8),
               "states": np.zeros((n, 6), np.uint32)}
        self.ref.lib.ref_frame_read(self.h, _p(out["lin"]), _p(out["bgra"]), _p(out["states"]))
        return out

    def camera_matrices(self) -> dict:
        m = {k: np.zeros(16, np.float32) for k in ("view", "projection", "inv_view", "inv_proj")}
        self.ref.lib.ref_frame_camera(self.h, *(_p(m[k]) for k in ("view", "projection", "inv_view", "inv_proj")))
        return m

    def __del__(self):
        if getattr(self, "h", None):
            self.ref.lib.ref_frame_destroy(self.h)
            self.h = None


def load(flavour: str = "b") -> RefLib:
    if flavour not in _cache:
        if not available(flavour):
            raise ImportError(f"{lib_path(flavour)} missing: needs the reference directory (oracle/ref/build_ref.py)")
        _cache[flavour] = RefLib(flavour)
    return _cache[flavour]
