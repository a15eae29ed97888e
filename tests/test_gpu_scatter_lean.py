"""The lean transcendental paths of the Oren-Nayar scatter (csrc/iq_fp2.h): under kOptScatter2 every
scattering lane checks that its operands lie in the lean forms' domains (iq_scatter_lean_ok) and the wave takes the
lean coefficient only if no lane objects; otherwise it runs the branch-free forms as before.

(a) each lean form equals the existing form on its domain, bit for bit (iqpt_libm_kernel, function ids 20-26 against
    12-18), on >= 100 k seeded operands per function and the domains' edges;
(b) the per-lane predicate itself (ids 27-30) accepts the domains' edges and refuses operands just outside them;
(c) frames equal the oracle in accumulator bits, BGRA8, the six XORWOW words and the ray count, and equal the frames
    of the library built with -DIQPT_SCATTER_LEAN=0 (the scatter before);
(d) the fallback runs: a frame whose first scatters have cos(theta_o) > 1 (checked on the CPU with the oracle's own
    camera, sphere and dot product before the GPU is asked) counts scatter_fallback_iterations > 0 in the instrumented
    library, and an ordinary crop counts fewer fallbacks than scatter iterations, so both paths are covered.

A process binds one library, so the other libraries' renders run this file as a worker process."""
import ctypes as C
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

K_OPT_PIPE = 1 << 21
K_OPT_STATS = 1 << 7
K_OPT_PRIO = 1 << 17
K_OPT_OVERLAP = 1 << 19

W, H = 1920, 1080
# 64 x 64 pixels each over the facing silhouettes of the two spheres (the gap between them is wider than 64 pixels):
# the big sphere's right edge and the small sphere's left edge, sphere pixels and pixels that miss in both
CROP_BIG = (880, 944, 590, 1, 64)
CROP_SMALL = (1000, 1064, 600, 1, 64)
# a band through both spheres, large enough (>= 64 blocks of 256 pixels) for overlapped launches
CROP_BAND = (720, 1200, 600, 1, 40)
# the Cornell box with a third sphere of radius 0.05 around the eye: every camera ray meets it from inside along its
# own normal, so cos(theta_o) = wo . n is 1 up to rounding, and above 1 for part of the pixels
EYE_SCENE = "cornell_eye_sphere"
EYE_POS = (0.0, 0.5, -3.0)
EYE_RADIUS = 0.05

WORKER_TIMEOUT_S = 240
F32 = np.float32
FP = C.POINTER(C.c_float)


def _paths():
    repo = Path(__file__).resolve().parent.parent
    for p in (str(repo / "path-tracer-and-rasterizer-engine_amd"), str(repo / "oracle"), str(repo),
              str(repo / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def scene_of(name):
    from helpers import scene_for
    from iqpt import Scene
    if name != EYE_SCENE:
        return scene_for(name)
    sc = Scene()
    sc.add_preset("cornell")
    sc.add_model("eye", "sphere", EYE_RADIUS, 0.0, EYE_POS)      # the preset's sphere mesh
    return sc, sc.build_packet()


def render(preset, w, h, launches, depth=8, crop=None, overlap=True, stats=False):
    """One context on the bound library: the frame after `launches`, the option set of every launch and, with stats
    (an instrumented library), the 24 header counters and the words after them of every launch."""
    from iqpt import PathTracer, _lib, make_camera
    from iqpt.render import pixel_set
    _sc, pk = scene_of(preset)
    cam = make_camera(w, h)
    pt = PathTracer(w, h, pixels=pixel_set(w, h, *crop) if crop else None, max_depth=depth)
    pt.set_split(_lib.SPLIT_OFF)
    pt.set_overlap(_lib.OVERLAP_AUTO if overlap else _lib.OVERLAP_OFF)
    pt.set_camera(cam)
    pt.upload_packet(pk)
    lb = _lib.load()
    lb.iqpt_debug_last_options.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    if stats:
        lb.iqpt_debug_set_kernel_options.argtypes = [C.c_void_p, C.c_int]
        lb.iqpt_debug_default_options.restype = C.c_int
        lb.iqpt_debug_read_stats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
        lb.iqpt_debug_read_stats_ext.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_uint32,
                                                 C.POINTER(C.c_uint32)]
        opt = lb.iqpt_debug_default_options() | K_OPT_PRIO | K_OPT_STATS | K_OPT_PIPE
        _lib.check(lb.iqpt_debug_set_kernel_options(pt._h, opt), "iqpt_debug_set_kernel_options")
    opts, words, ext = [], [], []
    for s in launches:
        pt.render(s)
        o = C.c_int(0)
        _lib.check(lb.iqpt_debug_last_options(pt._h, C.byref(o)), "iqpt_debug_last_options")
        opts.append(o.value)
        if stats:
            pt.sync()
            e, n = (C.c_ulonglong * 8)(), C.c_uint32(0)
            _lib.check(lb.iqpt_debug_read_stats_ext(pt._h, e, 8, C.byref(n)), "iqpt_debug_read_stats_ext")
            assert n.value >= 1
            buf = (C.c_ulonglong * 24)()
            _lib.check(lb.iqpt_debug_read_stats(pt._h, buf), "iqpt_debug_read_stats")   # reads and clears
            words.append([int(v) for v in buf])
            ext.append([int(v) for v in e])
    pt.sync()
    lin, bgra = pt.read()
    out = (lin, bgra, pt.read_rng(), pt.rays())
    pt.close()
    return out, opts, words, ext


# ---- worker process: the same renders on another library, results to an .npz ----
def worker_main(argv):
    lib, out_path, cases = argv[0], argv[1], json.loads(argv[2])
    _paths()
    from iqpt import _lib
    _lib.LIB_PATH = Path(lib).resolve()
    res = {}
    for i, c in enumerate(cases):
        (lin, bgra, rng, rays), opts, words, ext = render(c["preset"], c["w"], c["h"], c["launches"], depth=c["depth"],
                                                          crop=tuple(c["crop"]) if c["crop"] else None,
                                                          overlap=c["overlap"], stats=c["stats"])
        res[f"lin{i}"], res[f"bgra{i}"], res[f"rng{i}"] = lin, bgra, rng
        res[f"rays{i}"] = np.array([rays], dtype=np.uint64)
        res[f"opts{i}"] = np.array(opts, dtype=np.int64)
        res[f"words{i}"] = np.array(words, dtype=np.uint64).reshape(len(words), 24)
        res[f"ext{i}"] = np.array(ext, dtype=np.uint64).reshape(len(ext), 8)
    np.savez(out_path, **res)


if __name__ == "__main__":
    worker_main(sys.argv[1:])
    sys.exit(0)


pytestmark = pytest.mark.gpu


def case(preset, w, h, launches, depth=8, crop=None, overlap=True, stats=False):
    return {"preset": preset, "w": w, "h": h, "launches": list(launches), "depth": depth,
            "crop": list(crop) if crop else None, "overlap": overlap, "stats": stats}


def run_on(lib, cases, tmp_path):
    """The cases in one worker process bound to `lib`: a list of ((lin, bgra, rng, rays), opts, words, ext)."""
    out = tmp_path / (Path(lib).stem + ".npz")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [__file__, str(lib), str(out), json.dumps(cases)]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=WORKER_TIMEOUT_S)
    assert proc.returncode == 0, f"worker on {lib} ended with {proc.returncode}\n{proc.stdout}\n{proc.stderr}"
    z = np.load(out)
    return [((z[f"lin{i}"], z[f"bgra{i}"], z[f"rng{i}"], int(z[f"rays{i}"][0])), z[f"opts{i}"].tolist(),
             z[f"words{i}"].astype(np.uint64), z[f"ext{i}"].astype(np.uint64)) for i in range(len(cases))]


# ------------------------------------------------------------------ (a), (b): the forms and the predicate
GPU_FN = dict(atan2_x2_lo=12, atan2_x2_hi=13, acos_x2_lo=14, acos_x2_hi=15, sin_x2=16, cos_x2=17, tan_bf=18,
              atan2_lean_lo=20, atan2_lean_hi=21, acos_lean_lo=22, acos_lean_hi=23, sin_lean=24, cos_lean=25,
              tan_lean=26, ok_wo=27, ok_d=28, ok_cos=29, ok_trig=30)
N = 1 << 17                      # 131,072 seeded operands per function


def gpu(fn, a, b=None):
    from iqpt import _lib
    lib = _lib.load()
    f = lib.iqpt_debug_libm
    f.argtypes = [C.c_int, FP, FP, FP, C.c_uint64]
    f.restype = C.c_int
    a = np.ascontiguousarray(a, dtype=F32)
    b = np.ascontiguousarray(b if b is not None else np.zeros_like(a), dtype=F32)
    out = np.empty_like(a)
    assert f(GPU_FN[fn], a.ctypes.data_as(FP), b.ctypes.data_as(FP), out.ctypes.data_as(FP), a.size) == 0, \
        lib.iqpt_last_error()
    return out


def check_bits(got, want, *inputs):
    ok = got.view(np.uint32) == want.view(np.uint32)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{(~ok).sum()} mismatches, first at inputs {[float(v[i]) for v in inputs]}: "
                             f"got {got[i]!r} ({got[i:i+1].view(np.uint32)[0]:08x}) want {want[i]!r} "
                             f"({want[i:i+1].view(np.uint32)[0]:08x})")


def around(v):
    """v and its two neighbours in binary32."""
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


def atan2_domain_operands():
    """(y, x) inside the atan2 pair's lean domain: every sign, magnitudes over all of [2^-62, 2^62] and in [-1, 1],
    the domain's edges with the operands next to them (inside), quotients at and around tan(pi/8) and tan(3 pi/8)."""
    rng = np.random.default_rng(808)
    def mags(n):
        return (np.exp2(rng.uniform(-62.0, 62.0, n)) * rng.choice([-1.0, 1.0], n)).astype(F32)
    lo, hi = F32(2.0 ** -62), F32(2.0 ** 62)
    y = [mags(N // 2), rng.uniform(-1, 1, N // 2).astype(F32)]
    x = [mags(N // 2), rng.uniform(-1, 1, N // 2).astype(F32)]
    edge = np.array([lo, np.nextafter(lo, F32(1)), hi, np.nextafter(hi, F32(1)), F32(1.0), F32(-1.0), -lo, -hi,
                     -np.nextafter(lo, F32(1)), -np.nextafter(hi, F32(1))], dtype=F32)
    ey, ex = np.meshgrid(edge, edge)
    y.append(ey.ravel())
    x.append(ex.ravel())
    # quotients at the arctangent's range thresholds: y = t x for t at and next to tan(pi/8), tan(3 pi/8)
    ts = np.array(around(0.4142135623730950) + around(2.414213562373095), dtype=F32)
    for xv in (1.0, -1.0, 3.0, 0.7, 2.0 ** 40, 2.0 ** -40):
        for s in (1.0, -1.0):
            y.append((ts * F32(xv) * F32(s)).astype(F32))
            x.append(np.full(ts.size, xv, dtype=F32))
    y, x = np.concatenate(y), np.concatenate(x)
    ay, ax = np.abs(y), np.abs(x)
    keep = (ay >= lo) & (ay <= hi) & (ax >= lo) & (ax <= hi)          # the stated domain, nothing else
    assert keep.sum() >= 100_000
    return y[keep], x[keep]


def test_atan2_lean_equals_existing(require_gpu):
    y, x = atan2_domain_operands()
    want_lo, want_hi = gpu("atan2_x2_lo", y, x), gpu("atan2_x2_hi", y, x)
    check_bits(want_lo, want_hi, y, x)
    check_bits(gpu("atan2_lean_lo", y, x), want_lo, y, x)
    check_bits(gpu("atan2_lean_hi", y, x), want_lo, y, x)


def test_acos_lean_equals_existing(require_gpu):
    rng = np.random.default_rng(809)
    a = np.concatenate([rng.uniform(0.0, 1.0, N).astype(F32),
                        np.array(around(0.5) + around(1.0e-4) + [F32(0.0), F32(1.0), np.nextafter(F32(1), F32(0)),
                                                                  F32(1e-45), F32(2.0 ** -126), F32(0.25), F32(0.75)],
                                 dtype=F32)])
    a = a[(a >= 0) & (a <= 1)]
    assert not np.signbit(a).any() and a.size >= 100_000
    want = gpu("acos_x2_lo", a)
    check_bits(gpu("acos_lean_lo", a), want, a)
    check_bits(gpu("acos_lean_hi", a), want, a)


def trig_operands(seed):
    """[0, 8192]: uniform over the whole domain and over [0, 2 pi], every multiple of pi/4 up to 8192 with its
    neighbours, 1e-4 with its neighbours, 0 and 8192."""
    rng = np.random.default_rng(seed)
    k = np.arange(0, int(8192 / (np.pi / 4)) + 1, dtype=np.float64)
    m = (k * (np.pi / 4)).astype(F32)
    a = np.concatenate([rng.uniform(0.0, 8192.0, N // 2).astype(F32), rng.uniform(0.0, 2 * np.pi, N // 2).astype(F32),
                        m, np.nextafter(m, F32(np.inf)), np.nextafter(m, F32(-np.inf)),
                        np.array(around(1.0e-4) + [F32(0.0), F32(8192.0), np.nextafter(F32(8192), F32(0)),
                                                   F32(1e-45), F32(np.pi / 2), F32(np.pi), F32(2 * np.pi)], dtype=F32)])
    a = a[(a >= 0) & (a <= 8192) & ~np.signbit(a)]
    assert a.size >= 100_000
    return a


def test_sin_cos_tan_lean_equal_existing(require_gpu):
    a = trig_operands(810)
    check_bits(gpu("sin_lean", a), gpu("sin_x2", a), a)
    check_bits(gpu("tan_lean", a), gpu("tan_bf", a), a)
    # the cosine slot takes either sign (phi_i - phi_o): |v| <= 8192
    c = np.concatenate([a, -a[a > 0]])
    check_bits(gpu("cos_lean", c), gpu("cos_x2", c), c)


def test_predicate_accepts_the_domains_and_refuses_outside(require_gpu):
    lo, hi = F32(2.0 ** -62), F32(2.0 ** 62)
    up, dn = F32(np.inf), F32(0)
    inside = np.array([lo, hi, -lo, -hi, np.nextafter(lo, up), np.nextafter(hi, dn), F32(1), F32(-1), F32(0.3)],
                      dtype=F32)
    outside = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** 63, -2.0 ** 63, 2.0 ** -63, -2.0 ** -63,
                        np.nextafter(hi, up), -np.nextafter(hi, up), np.nextafter(lo, dn), -np.nextafter(lo, dn),
                        1e-45, -1e-45, 2.0 ** -126, 3.4e38], dtype=F32)
    y, x = atan2_domain_operands()
    y, x = y[:4096], x[:4096]
    for fn in ("ok_wo", "ok_d"):                   # (a, b) = (woy, wox) and (dy, dx)
        assert np.all(gpu(fn, y, x) == 1.0), fn
        ia, ib = (v.ravel() for v in np.meshgrid(inside, inside))
        assert np.all(gpu(fn, ia, ib) == 1.0), fn
        for part in inside:                        # one operand outside, in either slot, refuses the lane
            p = np.full(outside.size, part, dtype=F32)
            assert np.all(gpu(fn, outside, p) == 0.0), (fn, "y", float(part))
            assert np.all(gpu(fn, p, outside) == 0.0), (fn, "x", float(part))
    cos_in = np.array([0.0, 1.0, 0.5, 1e-45, 1e-4, np.nextafter(F32(1), dn)], dtype=F32)
    cos_out = np.array([-0.0, np.nan, np.nextafter(F32(1), up), 2.0, -1e-45, -0.5, -1.0, np.inf, -np.inf], dtype=F32)
    ia, ib = (v.ravel() for v in np.meshgrid(cos_in, cos_in))
    assert np.all(gpu("ok_cos", ia, ib) == 1.0)
    for part in cos_in:
        p = np.full(cos_out.size, part, dtype=F32)
        assert np.all(gpu("ok_cos", cos_out, p) == 0.0), ("cto", float(part))
        assert np.all(gpu("ok_cos", p, cos_out) == 0.0), ("cti", float(part))
    trig_in = np.array([0.0, 8192.0, np.pi, 1e-45, np.nextafter(F32(8192), dn)], dtype=F32)
    trig_out = np.array([-0.0, -1e-3, -np.pi, -1e-45, np.nextafter(F32(8192), up), 1e9, np.nan, np.inf, -np.inf],
                        dtype=F32)
    assert np.all(gpu("ok_trig", trig_in) == 1.0)
    assert np.all(gpu("ok_trig", trig_out) == 0.0)


# ------------------------------------------------------------------ (c): frames
@functools.lru_cache(maxsize=None)
def oracle_frame(preset, w, h, crop, launches, depth):
    """The oracle frame after the launches; computed once per case and shared, never changed."""
    import oracle
    from iqpt import make_camera
    from iqpt.render import pixel_set
    _sc, pk = scene_of(preset)
    fr = oracle.OracleFrame(w, h, pixels=pixel_set(w, h, *crop) if crop else None, max_depth=depth)
    cam = make_camera(w, h)
    for s in launches:
        fr.render(pk, cam, s)
    return fr


def same_as_oracle(out, fr):
    lin, bgra, rng, rays = out
    a, b = lin[:, :3], fr.lin[:, :3]
    both_nan = np.isnan(a) & np.isnan(b)
    assert np.all((a.view(np.uint32) == b.view(np.uint32)) | both_nan)
    assert np.array_equal(bgra, fr.bgra)
    assert np.array_equal(rng, fr.states)
    assert rays == int(fr.rays.sum())


def same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2])
    assert a[3] == b[3]


FRAME_CASES = [case("cornell", W, H, [1, 2, 3, 64], depth=d, crop=cr) for d in (1, 2, 8, 16)
               for cr in (CROP_BIG, CROP_SMALL)] + [
    case("c1_plumbing", 128, 72, [3, 4]),
    case("cornell", W, H, [3, 64], crop=CROP_BAND),          # two overlapped launches
]


def oracle_of(c):
    return oracle_frame(c["preset"], c["w"], c["h"], tuple(c["crop"]) if c["crop"] else None, tuple(c["launches"]),
                        c["depth"])


def first_hits(c):
    """Per pixel of the case's crop, from the oracle's own camera and sphere test: the first sample's camera ray and,
    per sphere of the scene, whether it hits, with t and the normal."""
    import oracle
    from iqpt import make_camera
    from iqpt.render import pixel_set
    lib = oracle.load()
    _sc, pk = scene_of(c["preset"])
    cam = make_camera(c["w"], c["h"])
    crop = tuple(c["crop"]) if c["crop"] else (0, c["w"], 0, 1, c["h"])
    fr = oracle.OracleFrame(c["w"], c["h"], pixels=pixel_set(c["w"], c["h"], *crop), max_depth=c["depth"])
    x0, x1, y0, ystep, nrows = crop
    ns = pk.num_drawcalls[1]
    rows = []
    i = 0
    for r in range(nrows):
        for x in range(x0, x1):
            st = np.array(fr.states[i], dtype=np.uint32).copy()
            o, d = np.zeros(4, F32), np.zeros(4, F32)
            lib.iqo_get_ray(C.byref(cam), x, y0 + r * ystep, st.ctypes.data_as(C.POINTER(C.c_uint32)),
                            o.ctypes.data_as(FP), d.ctypes.data_as(FP))
            best = None
            for k in range(ns):
                cen = np.array(list(pk.sphere_dcs[k].center), dtype=F32)
                t, p4, n4, front = np.zeros(1, F32), np.zeros(4, F32), np.zeros(4, F32), C.c_int(0)
                # t_min and t_max of ray_color (path_tracer.cu:253)
                hit = lib.iqo_sphere_intersect(cen.ctypes.data_as(FP), pk.sphere_dcs[k].radius, o.ctypes.data_as(FP),
                                               d.ctypes.data_as(FP), 0.000001, 999.99, t.ctypes.data_as(FP),
                                               p4.ctypes.data_as(FP), n4.ctypes.data_as(FP), C.byref(front))
                if hit and (best is None or t[0] < best[1]):
                    best = (k, float(t[0]), n4.copy())
            rows.append((d.copy(), best))
            i += 1
    return rows


def test_crops_run_through_both_spheres():
    """From the oracle alone: camera rays of CROP_BIG meet the big sphere (0) or nothing, those of CROP_SMALL the
    small sphere (1) or nothing, some of each."""
    for c, k in ((FRAME_CASES[0], 0), (FRAME_CASES[1], 1)):
        hit = [b[0] if b is not None else -1 for _d, b in first_hits(c)]
        assert set(hit) == {k, -1}, (c["crop"], set(hit))
        assert min(hit.count(k), hit.count(-1)) >= 256, (c["crop"], hit.count(k), hit.count(-1))


@pytest.fixture(scope="module")
def full_form(require_gpu, tmp_path_factory):
    """Every frame case on the -DIQPT_SCATTER_LEAN=0 library, in one worker process."""
    from iqpt import _build
    lib = _build.build_lib(flags=_build.SCATTER_FULL_FLAGS, target=_build.SCATTER_FULL_LIB)
    return run_on(lib, FRAME_CASES, tmp_path_factory.mktemp("scatterfull"))


@pytest.mark.parametrize("i", range(len(FRAME_CASES)),
                         ids=[f"depth{d}_{s}" for d in (1, 2, 8, 16) for s in ("big", "small")] +
                             ["c1_128x72", "overlapped"])
def test_frames_equal_oracle_and_former_scatter(require_gpu, full_form, i):
    c = FRAME_CASES[i]
    out, opts, _, _ = render(c["preset"], c["w"], c["h"], c["launches"], depth=c["depth"],
                             crop=tuple(c["crop"]) if c["crop"] else None, overlap=c["overlap"])
    assert all(o & K_OPT_PIPE for o in opts), [hex(o) for o in opts]
    if c["crop"] == list(CROP_BAND):
        assert any(o & K_OPT_OVERLAP for o in opts), [hex(o) for o in opts]
    same_as_oracle(out, oracle_of(c))
    out_f, opts_f, _, _ = full_form[i]
    assert [o & K_OPT_PIPE for o in opts_f] == [o & K_OPT_PIPE for o in opts]
    same(out, out_f)


# ------------------------------------------------------------------ (d): the fallback runs
EYE_CASE = case(EYE_SCENE, 64, 64, [2], depth=2, overlap=False, stats=True)
ORDINARY_CASE = case("cornell", W, H, [64], depth=8, crop=CROP_BIG, overlap=False, stats=True)


def dot3(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


@functools.lru_cache(maxsize=None)
def eye_scene_out_of_domain():
    """Pixels of the eye-sphere frame whose first scatter has an operand outside the lean domains, from the oracle's
    camera ray and sphere hit: cos(theta_o) = max(0, wo . n) above 1, or wox / woy outside [2^-62, 2^62]."""
    lo, hi = F32(2.0 ** -62), F32(2.0 ** 62)
    n_cos = n_dir = n_hit = 0
    for d, best in first_hits(EYE_CASE):
        if best is None:
            continue
        n_hit += 1
        wo = -d
        cto = max(F32(0.0), dot3(wo, best[2]))
        n_cos += int(not (cto <= F32(1.0)))
        n_dir += int(not (lo <= abs(wo[0]) <= hi and lo <= abs(wo[1]) <= hi))
    return n_hit, n_cos, n_dir


def test_eye_scene_leaves_the_domains_on_the_cpu():
    n_hit, n_cos, n_dir = eye_scene_out_of_domain()
    print(f"eye-sphere 64 x 64, first sample: {n_hit} sphere hits, {n_cos} with cos(theta_o) > 1, {n_dir} with wox / "
          f"woy outside [2^-62, 2^62]")
    assert n_hit == 64 * 64          # the sphere encloses the eye: every camera ray meets a sphere first
    assert n_cos + n_dir >= 1


def test_fallback_runs_and_both_paths_are_covered(require_gpu, tmp_path):
    from iqpt import _build
    n_hit, n_cos, n_dir = eye_scene_out_of_domain()
    assert n_cos + n_dir >= 1
    lib = _build.build_lib(stats=True)
    (eye, o_eye, w_eye, x_eye), (ordi, o_ord, w_ord, x_ord) = run_on(lib, [EYE_CASE, ORDINARY_CASE], tmp_path)
    assert all(o & K_OPT_STATS for o in o_eye + o_ord), [hex(o) for o in o_eye + o_ord]
    same_as_oracle(eye, oracle_of(EYE_CASE))
    same_as_oracle(ordi, oracle_of(ORDINARY_CASE))
    print("scatter iterations / fallback iterations: eye", w_eye[:, 3].tolist(), x_eye[:, 0].tolist(), "ordinary",
          w_ord[:, 3].tolist(), x_ord[:, 0].tolist())
    assert np.all(x_eye[:, 0] > 0)                       # scatter_fallback_iterations > 0
    assert np.all(x_eye[:, 0] <= w_eye[:, 3])
    assert np.all(w_ord[:, 3] > 0)
    assert np.all(x_ord[:, 0] < w_ord[:, 3])             # the lean path ran too
