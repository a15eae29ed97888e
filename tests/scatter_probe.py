"""Cases, reference and vote prediction shared by tests/test_scatter_probe_cases.py (CPU) and
tests/test_gpu_scatter_probe.py: single Oren-Nayar scatters fed to the device probe (iqpt_debug_scatter,
iqpt_scatter_probe_kernel) and to the oracle's batch export (iqo_oren_nayar_batch), compared bit for bit.

Everything here runs on the CPU. The reference is computed once per case set and shared (functools.lru_cache); the
arrays it returns are never changed."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import oracle
import ref_cases

F32 = np.float32
FP = C.POINTER(C.c_float)
UP = C.POINTER(C.c_uint32)
BP = C.POINTER(C.c_uint8)
M32 = 0xFFFFFFFF
WEYL = 362437

# the probe's forms (csrc/iqpt_internal.hpp launch_scatter_probe)
FORMS = {"fastdiv_lean": 0, "fastdiv_full": 1, "ieee_lean": 2, "ieee_full": 3, "plain": 4}
LEAN_FORMS = ("fastdiv_lean", "ieee_lean")
FULL_FORMS = ("fastdiv_full", "ieee_full")
SPHERE_FORMS = LEAN_FORMS + FULL_FORMS

SENTINEL_WORD = 0xDEADBEEF            # every output word before a launch (as float: a NaN with this payload)
SENTINEL_BYTE = 0xAA

# draws: u = (float)r * 2^-32 is 0 for r = 0, 2^-32 for r = 1, 1 - 2^-24 for r = 0xFFFFFF7F and exactly 1 from
# r = 0xFFFFFF80 on ((float)r rounds to 2^32)
R_ZERO, R_MIN, R_BELOW_ONE, R_ONE, R_MAX = 0, 1, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF
EDGE_DRAWS = (R_ZERO, R_MIN, R_BELOW_ONE, R_ONE, R_MAX)

SIGMAS = ((1.0, 0.5), (0.4, 0.8), (0.0, 0.18))       # (sigma, albedo); the first is the reference's sphere material


# ---------------------------------------------------------------------------------------------- generator states
def _solve_xor_shl(a, s):
    """t with t ^ (t << s) == a (32 bits): bit i of t is a_i ^ t_(i - s)."""
    t = 0
    for i in range(32):
        t |= (((a >> i) ^ ((t >> (i - s)) if i >= s else 0)) & 1) << i
    return t


def _solve_xor_shr(a, s):
    """v with v ^ (v >> s) == a (32 bits): bit i of v is a_i ^ v_(i + s)."""
    v = 0
    for i in reversed(range(32)):
        v |= (((a >> i) ^ ((v >> (i + s)) if i + s < 32 else 0)) & 1) << i
    return v


def crafted_state(x1, x2, free):
    """A six-word XORWOW state (v0..v4, d) whose next two iq_xorwow_next outputs are x1 and x2. The step
    (csrc/iq_xorwow.h) returns v4' + d' with v4' = (v4 ^ (v4 << 4)) ^ (t ^ (t << 1)), t = v0 ^ (v0 >> 2); both maps of
    t are bijections, so with v2, v3, v4 and d free (`free`: four 32-bit words) v0 follows from x1 and v1 from x2."""
    v2, v3, v4, d = (int(q) & M32 for q in free)
    w1 = (x1 - d - WEYL) & M32                 # v4 after the first step
    w2 = (x2 - d - 2 * WEYL) & M32             # v4 after the second
    v0 = _solve_xor_shr(_solve_xor_shl(w1 ^ v4 ^ ((v4 << 4) & M32), 1), 2)
    v1 = _solve_xor_shr(_solve_xor_shl(w2 ^ w1 ^ ((w1 << 4) & M32), 1), 2)
    return np.array([v0, v1, v2, v3, v4, d], dtype=np.uint32)


def draw_unit(r):
    """iq_u32_to_unit: (float)r * 2^-32 in binary32."""
    return F32(F32(r) * F32(2.0 ** -32))


# ---------------------------------------------------------------------------------------------- the case set
def _unit(a):
    return ref_cases._unit(a)


def _rows(rows):
    """[(n3, d3, state6, tag)] -> dict of arrays (p fixed, as the edge cases of ref_cases.scatter_inputs)."""
    n = np.array([r[0] for r in rows], F32).reshape(-1, 3)
    d = np.array([r[1] for r in rows], F32).reshape(-1, 3)
    p = np.tile(np.array([[0.25, 1.0, -0.5]], F32), (len(rows), 1))
    return {"p": ref_cases._v4(p, 1.0), "n": ref_cases._v4(n, 0.0), "d": ref_cases._v4(d, 0.0),
            "states": np.stack([r[2] for r in rows]).astype(np.uint32), "tag": [r[3] for r in rows]}


AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
OBLIQUE = [tuple(_unit([1, 2, 3])), tuple(_unit([-0.95, 0.1, 0.2]))]     # |w.x| below and above the ONB's 0.9


def crafted_draw_cases():
    """Every axis-aligned normal and two oblique ones, crossed with (u1, u2) over the edge draws."""
    rng = np.random.default_rng(2201)
    rows = []
    for a in AXES + OBLIQUE:
        a = np.array(a, F32)
        d_in = _unit(-a + 0.4 * _unit(np.cross(a, [0.3, -0.5, 0.8])))       # from above the surface, oblique
        for r1 in EDGE_DRAWS:
            for r2 in EDGE_DRAWS:
                rows.append((a, d_in, crafted_state(r1, r2, rng.integers(0, 1 << 32, 4, dtype=np.uint64)),
                             f"draw:{r1:#x},{r2:#x}"))
    return _rows(rows)


PDF_MIN = F32(0.00001)                 # oren_nayar::scatter replaces a pdf below this


def pdf_threshold_lengths(axis, d_in, state):
    """Three consecutive binary32 lengths s of a normal s * axis under a state whose second draw is 0: the oracle's
    pdf is replaced at the first, is exactly PDF_MIN (and kept) at the second, and is above it at the third."""
    s = F32(PDF_MIN * F32(np.pi))
    cand = [s]
    for _ in range(8):
        cand.insert(0, np.nextafter(cand[0], F32(0)))
        cand.append(np.nextafter(cand[-1], F32(1)))
    m = len(cand)
    n = ref_cases._v4(np.array([axis * c for c in cand], F32), 0.0)
    ref = oracle_scatter(ref_cases._v4(np.zeros((m, 3), F32), 1.0), n, ref_cases._v4(np.tile(d_in, (m, 1)), 0.0),
                         np.tile(state, (m, 1)), 1.0, 0.5)
    at = np.flatnonzero(ref["pdf"] == PDF_MIN)
    assert len(at) == 1 and 0 < at[0] < m - 1, ref["pdf"]
    k = int(at[0])
    assert ref["pdf"][k - 1] == F32(1.0) / F32(np.pi) and PDF_MIN < ref["pdf"][k + 1] < F32(1.1e-5), ref["pdf"]
    return cand[k - 1], cand[k], cand[k + 1]


def out_of_domain_cases():
    """Operands outside the lean domains that a kernel can meet, each under a seeded state and under the draws that
    matter for it."""
    rng = np.random.default_rng(2202)
    up1 = np.nextafter(F32(1), F32(2))
    rows = []

    def free():
        return rng.integers(0, 1 << 32, 4, dtype=np.uint64)

    def add(n, d, tag, draws=None):
        st = ref_cases._states(rng, 1)[0] if draws is None else crafted_state(draws[0], draws[1], free())
        rows.append((np.array(n, F32), np.array(d, F32), st, tag))

    obl = _unit([0.3, 0.5, 0.8])
    for k in range(3):
        add(obl, _unit([0.0, -0.6, -0.8]), "wox=0")                     # wox = -0 * -1 = +0 exactly
        add(obl, _unit([-0.6, 0.0, -0.8]), "woy=0")
        add((0, 0, 1), (0.0, 0.0, -1.0), "wox=woy=0")
    for a in AXES:                                                      # a normal one ulp longer than unit, head-on
        a = np.array(a, F32)
        add(a * up1, -a, "cto>1")
        add(a * up1, -a, "cto>1,u2=0", draws=(0x40000000, R_ZERO))      # d = w exactly: cti = |n| > 1 as well
        add(a * up1, -a, "cto>1,u2=1", draws=(0x40000000, R_ONE))
    long = F32(1.0 + 2.0 ** -21)                                        # longer than unit, inside 1 +- 2^-20
    for v in ([0.3, 0.5, 0.8], [-0.7, 0.2, 0.6], [0.5, -0.5, 0.7], [0.2, 0.9, -0.3]):
        n = (_unit(v) * long).astype(F32)
        add(n, -_unit(v), "oblique cto>1")                              # head-on: cto = |n| up to rounding
        add(n, _unit(-_unit(v) + 0.8 * _unit(np.cross(v, [0.3, -0.5, 0.8]))), "oblique cti>1",
            draws=(0x40000000, R_ZERO))                                 # u2 = 0: d = w, cti = |n| up to rounding
    for a in AXES:                                                      # u2 = 1: lz = 0, the pdf is replaced, d = n
        add(a, _unit(-np.array(a, F32) + 0.3 * obl), "dx=0|dy=0 by pdf replacement", draws=(0x12345678, R_ONE))
    # the pdf exactly at its threshold. With unit normals it cannot be: n . d is lz = sqrt(1 - u2) up to rounding,
    # which is 0 or >= 2^-12, so the pdf is rounding noise or >= 7e-5. An axis normal of length s with u2 = 0 has
    # d = w and n . d = s exactly, so s / pi decides: the s whose quotient is RN(1e-5), and its neighbours
    for a in AXES:
        a = np.array(a, F32)
        d_in = _unit(-a + 0.3 * obl)
        st = crafted_state(0x9abcdef0, R_ZERO, free())
        for k, s in enumerate(pdf_threshold_lengths(a, d_in, st)):
            rows.append((a * s, d_in, st, f"pdf threshold {k - 1:+d}"))
    nan = F32(np.nan)
    add((nan, 0.0, 1.0), (0.0, 0.6, -0.8), "nan normal x")
    add((0.0, nan, 0.0), _unit([0.3, -0.9, 0.1]), "nan normal y")
    add((nan, nan, nan), _unit([0.3, -0.9, 0.1]), "nan normal")
    add((0.6, 0.0, 0.8), (nan, 0.0, -1.0), "nan direction")
    add((0, 0, 0), _unit([0.3, -0.9, 0.1]), "null normal")
    add((0, 0, 0), (0.0, 0.0, -1.0), "null normal, wox=woy=0")
    add((9e-6, -9e-6, 9e-6), _unit([0.3, -0.9, 0.1]), "normal under is_null's epsilon")
    return _rows(rows)


@functools.lru_cache(maxsize=None)
def main_cases():
    """The cases every form runs: ref_cases.scatter_inputs (the random block and its edge cases, the very cases that
    pin the oracle's scatter to the reference), the crafted draws and the out-of-domain operands.
    has_nan: an input of the case holds a NaN. nonunit: the normal's length is outside 1 +- 2^-20 and the normal is
    neither null (normalize3's test) nor NaN: no hit routine of the kernels produces such a normal."""
    base = ref_cases.scatter_inputs(ref_cases.N_LIVE)
    parts = [dict(base, tag=["random"] * ref_cases.N_LIVE + ["edge"] * (len(base["p"]) - ref_cases.N_LIVE)),
             crafted_draw_cases(), out_of_domain_cases()]
    out = {k: np.ascontiguousarray(np.concatenate([q[k] for q in parts])) for k in ("p", "n", "d", "states")}
    out["tag"] = sum((q["tag"] for q in parts), [])
    n3 = out["n"][:, :3].astype(np.float64)
    out["has_nan"] = np.isnan(out["n"]).any(1) | np.isnan(out["d"]).any(1) | np.isnan(out["p"]).any(1)
    null = (np.abs(out["n"][:, :3]) < F32(0.00001)).all(1)
    length = np.sqrt((n3 ** 2).sum(1))
    with np.errstate(invalid="ignore"):
        out["nonunit"] = ~out["has_nan"] & ~null & (np.abs(length - 1.0) > 2.0 ** -20)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------- the reference
def material_constants(sigma):
    """A and B in binary32 in the order of the material upload (csrc/iqpt_runtime.cpp; material.cu:22-24)."""
    sigma = F32(sigma)
    sigma2 = F32(sigma * sigma)
    A = F32(F32(1.0) - F32(F32(F32(0.5) * sigma2) / F32(sigma2 + F32(0.33))))
    B = F32(F32(F32(0.45) * sigma2) / F32(sigma2 + F32(0.09)))
    return A, B


def oracle_scatter(p, n, d, states, sigma, albedo):
    """iqo_oren_nayar_batch on the cases: att (n, 4), pdf, cosw, ro, rd (n, 4), states after."""
    lib = oracle.load()
    m = len(p)
    st = np.ascontiguousarray(states, np.uint32).copy()
    o = {"att": np.zeros((m, 4), F32), "pdf": np.zeros(m, F32), "cosw": np.zeros(m, F32), "ro": np.zeros((m, 4), F32),
         "rd": np.zeros((m, 4), F32)}
    alb = np.array([albedo, albedo, albedo, 0.0], F32)
    args = [np.ascontiguousarray(a, F32) for a in (p, n, d)]
    lib.iqo_oren_nayar_batch(m, F32(sigma), alb.ctypes.data_as(FP), *(a.ctypes.data_as(FP) for a in args),
                             st.ctypes.data_as(UP), *(o[k].ctypes.data_as(FP) for k in ("att", "pdf", "cosw", "ro", "rd")))
    o["states"] = st
    with np.errstate(all="ignore"):
        o["q"] = (o["cosw"] / o["pdf"]).astype(F32)           # the IEEE quotient in binary32
    return o


@functools.lru_cache(maxsize=None)
def main_reference(sigma, albedo):
    c = main_cases()
    o = oracle_scatter(c["p"], c["n"], c["d"], c["states"], sigma, albedo)
    for v in o.values():
        v.setflags(write=False)
    return o


# ---------------------------------------------------------------------------------------------- the vote
def _dot3(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z in binary32, the kernels' order."""
    with np.errstate(all="ignore"):
        return ((a[:, 0] * b[:, 0]).astype(F32) + (a[:, 1] * b[:, 1]).astype(F32)).astype(F32) + \
            (a[:, 2] * b[:, 2]).astype(F32)


def _fmax0(x):
    """iq_fmaxf(0.0f, x): 0 for a NaN, else 0 > x ? 0 : x (so -0 stays -0)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x) | (F32(0) > x), F32(0), x).astype(F32)


def _atan2_ok(y, x):
    lo, hi = F32(2.0 ** -62), F32(2.0 ** 62)
    with np.errstate(invalid="ignore"):
        ay, ax = np.abs(y), np.abs(x)
        return (ay >= lo) & (ay <= hi) & (ax >= lo) & (ax <= hi)


def _acos_ok(x):
    return np.ascontiguousarray(x, F32).view(np.uint32) <= 0x3F800000


KINDS = ("wo", "d", "cto", "cti")


def objections(n, d_in, rd):
    """Per case, from the oracle's outgoing direction rd and binary32 dot products in the kernel's order: which of
    the four lean-domain tests of iq_scatter_lean_ok (csrc/iq_fp2.h) refuse it, and cto, cti."""
    n3, rd3 = np.ascontiguousarray(n[:, :3], F32), np.ascontiguousarray(rd[:, :3], F32)
    wo = (-np.ascontiguousarray(d_in[:, :3], F32)).astype(F32)
    cto = _fmax0(_dot3(wo, n3))
    cti = _fmax0(_dot3(rd3, n3))
    return {"wo": ~_atan2_ok(wo[:, 1], wo[:, 0]), "d": ~_atan2_ok(rd3[:, 1], rd3[:, 0]), "cto": ~_acos_ok(cto),
            "cti": ~_acos_ok(cti), "cto_value": cto, "cti_value": cti}


def objects(obj):
    return obj["wo"] | obj["d"] | obj["cto"] | obj["cti"]


def predicted_fallback(form, objecting, active):
    """fell_back per case (lane i % 64 of wave i / 64): under a lean form every active lane of a wave reports whether
    any active lane of that wave objects; under a full form every active lane reports the fallback; the plain form
    reports nothing. Inactive lanes keep the sentinel."""
    m = len(active)
    out = np.full(m, SENTINEL_BYTE, np.uint8)
    act = active.astype(bool)
    if form in LEAN_FORMS:
        for w in range(0, m, 64):
            s = slice(w, min(w + 64, m))
            out[s][act[s]] = int(np.any(objecting[s] & act[s]))
    else:
        out[act] = 1 if form in FULL_FORMS else 0
    return out


# ---------------------------------------------------------------------------------------------- placement cases
PLACEMENT_N = 3 * 64 + 5
PLACEMENT_AT = (0, 31, 32, 63, 64, 127, 191, 192, 196)


@functools.lru_cache(maxsize=None)
def placement_cases():
    """Three full waves and a fourth of 5 lanes of in-domain cases (the first of the random block that the CPU
    predicate accepts), and one objecting case per kind of objection (objecting for that reason alone). Reference
    for sigma 1, albedo .5. Returns (base indices, {kind: index}) into main_cases()."""
    c, ref = main_cases(), main_reference(*SIGMAS[0])
    obj = objections(c["n"], c["d"], ref["rd"])
    bad = objects(obj)
    base = np.flatnonzero(~bad[:ref_cases.N_LIVE])[:PLACEMENT_N]
    assert len(base) == PLACEMENT_N
    pick = {}
    for k in KINDS:
        others = np.zeros_like(bad)
        for j in KINDS:
            if j != k:
                others |= obj[j]
        idx = np.flatnonzero(obj[k] & ~others & ~c["has_nan"] & ~c["nonunit"])
        assert len(idx), f"no case objects for {k} alone"
        pick[k] = int(idx[0])
    return base, pick


# ---------------------------------------------------------------------------------------------- sphere mode
SPHERE_RADII = (0.05, 0.5, 10.0, 2.0 ** -20, 2.0 ** 20)
T_MIN, T_MAX = ref_cases.T_MIN, ref_cases.T_MAX


@functools.lru_cache(maxsize=None)
def sphere_cases():
    """Rays that meet a sphere from outside, from inside (the normal is flipped) and grazing, per radius; t, the hit
    point and the normal from iqo_sphere_intersect, the record from the oracle's scatter at that hit (sigma 1, albedo
    .5: the reference's sphere material). Candidates the oracle's sphere test rejects are not cases."""
    lib = oracle.load()
    rng = np.random.default_rng(2203)
    rows = []
    per = 24
    for rad in SPHERE_RADII:
        r = F32(rad)
        c = (rng.normal(size=3) * min(3.0, 4.0 * rad)).astype(F32)
        count = {"outside": 0, "inside": 0, "grazing": 0}
        for kind in count:
            tries = 0
            while count[kind] < per:
                tries += 1
                assert tries < 4000, (rad, kind, count)
                s = _unit(rng.normal(size=3)).astype(np.float64)                 # a point of the surface
                # the origin's distance from the surface: within the radius, and small enough for t < t_max
                h = min(rad, 2.0) * rng.uniform(0.1, 0.95)
                if kind == "outside":
                    o = c + s * (rad + h)
                    d = _unit((c + _unit(rng.normal(size=3)) * rad * rng.uniform(0, 0.9)) - o)
                elif kind == "inside":
                    o = c + s * (rad - h)
                    d = _unit(rng.normal(size=3))
                else:
                    o = c + s * (rad + h)
                    # incidence with cosine ci at the hit: sin(angle to -s) = sin(incidence) r / (r + h)
                    ci = rng.uniform(0.01, 0.15)
                    tdir = _unit(np.cross(s, rng.normal(size=3)))
                    sa = np.sqrt(1.0 - ci * ci) * rad / (rad + h)
                    d = _unit(-s * np.sqrt(1.0 - sa * sa) + tdir * sa)
                o4, d4, c4 = ref_cases._v4(o.astype(F32), 1.0), ref_cases._v4(d.astype(F32), 0.0), ref_cases._v4(c, 0.0)
                t, p4, n4, front = C.c_float(), np.zeros(4, F32), np.zeros(4, F32), C.c_int()
                hit = lib.iqo_sphere_intersect(c4.ctypes.data_as(FP), r, o4.ctypes.data_as(FP), d4.ctypes.data_as(FP),
                                               T_MIN, T_MAX, C.byref(t), p4.ctypes.data_as(FP), n4.ctypes.data_as(FP),
                                               C.byref(front))
                if not hit or front.value != (0 if kind == "inside" else 1):
                    continue
                count[kind] += 1
                rows.append(dict(c=c4, r=r, o=o4, d=d4, t=F32(t.value), p=p4, n=n4, kind=kind))
    m = len(rows)
    out = {k: np.ascontiguousarray(np.stack([q[k] for q in rows])) for k in ("c", "o", "d", "p", "n")}
    out["r"] = np.array([q["r"] for q in rows], F32)
    out["t"] = np.array([q["t"] for q in rows], F32)
    out["kind"] = [q["kind"] for q in rows]
    out["states"] = ref_cases._states(rng, m)
    ref = oracle_scatter(out["p"], out["n"], out["d"], out["states"], *SIGMAS[0])
    with np.errstate(all="ignore"):
        ref["value"] = (ref["att"][:, 0] * ref["q"]).astype(F32)               # att.x * (cosw / pdf)
    for v in list(out.values()) + list(ref.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out, ref


# ---------------------------------------------------------------------------------------------- the device side
def probe_inputs(p, n, d):
    """The probe's 12 floats per case: hit point, hit normal, incoming direction."""
    a = np.zeros((len(p), 12), F32)
    a[:, 0:3], a[:, 3:6], a[:, 6:9] = p[:, :3], n[:, :3], d[:, :3]
    return a


def sphere_probe_inputs(s):
    a = np.zeros((len(s["c"]), 12), F32)
    a[:, 0:3], a[:, 3], a[:, 4:7], a[:, 7:10], a[:, 10] = s["c"][:, :3], s["r"], s["o"][:, :3], s["d"][:, :3], s["t"]
    return a


def gpu_scatter(form, inputs, states, active=None, sigma=1.0, albedo=0.5, sphere=False):
    """One launch of the device probe. Outputs start as the sentinel: ray (m, 6), vals (m, 3) as uint32 views of the
    floats, states (m, 6), fell_back (m,)."""
    from iqpt import _lib
    lib = _lib.load()
    f = lib.iqpt_debug_scatter
    f.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, FP, UP, BP, C.c_uint64, FP, FP, UP, BP]
    f.restype = C.c_int
    m = len(inputs)
    inputs = np.ascontiguousarray(inputs, F32)
    states = np.ascontiguousarray(states, np.uint32)
    active = np.ones(m, np.uint8) if active is None else np.ascontiguousarray(active, np.uint8)
    assert inputs.shape == (m, 12) and states.shape == (m, 6) and active.shape == (m,)
    ray = np.full((m, 6), SENTINEL_WORD, np.uint32)
    vals = np.full((m, 3), SENTINEL_WORD, np.uint32)
    st = np.full((m, 6), SENTINEL_WORD, np.uint32)
    fb = np.full(m, SENTINEL_BYTE, np.uint8)
    A, B = material_constants(sigma)
    rc = f(FORMS[form], int(sphere), A, B, F32(albedo), inputs.ctypes.data_as(FP), states.ctypes.data_as(UP),
           active.ctypes.data_as(BP), m, ray.ctypes.data_as(FP), vals.ctypes.data_as(FP), st.ctypes.data_as(UP),
           fb.ctypes.data_as(BP))
    assert rc == 0, lib.iqpt_last_error()
    return {"ray": ray, "vals": vals, "states": st, "fell_back": fb}
