"""The HIP variance-guided filter against its numpy reference (tests/svgf_ref.py): every float4 is
compared as uint32, every BGRA byte for equality, every count for equality.

csrc/svgf/iq_svgf_kernels.hip ships iqs_moments_kernel and iqs_variance_kernel (every resolve),
iqs_level_kernel<false> and <true> (levels >= 2 and >= 1), and levels == 0 runs iqp_encode_kernel of
csrc/post/iq_post_kernels.hip; all are reached by
every test_synthetic case, and both branches of the variance kernel by both values of min_history together."""
import contextlib

import numpy as np
import pytest

import denoise_ref as dr
import iqpt
import oracle
import svgf_ref as sr
import temporal_ref as tr
from iqpt import Denoiser, PathTracer, Rasterizer, Scene, Svgf, Temporal, align_camera, make_camera

pytestmark = pytest.mark.gpu
NO = sr.NO_PRIM
F = np.float32
BIG = 1 << 24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want, what):
    assert np.array_equal(bits(got), bits(want)), \
        f"{what}: {int(np.sum(np.any(bits(got) != bits(want), axis=-1)))} pixels differ"


def assert_same(got, want, what):
    same(got[0], want[0], what)
    assert np.array_equal(got[1], want[1]), what


def assert_stages(s, ref, what):
    """read_stages, read and stats of a resolved Svgf against the resolved reference."""
    t, c0 = s.read_stages()
    same(t, ref.temporal_out, what + ": temporal stage")
    same(c0, ref.c0, what + ": variance stage")
    assert_same(s.read(), (ref.stages[-1], dr.encode_bgra(ref.stages[-1])), what)
    assert s.stats() == ref.stats(), what


# ------------------------------------------------------------------------------------------------ synthetic
# The four seeded views of tests/test_gpu_temporal.py, restated; the colours carry one more special value, a finite
# one whose squared luminance overflows.
POS_A = np.array([0.0, 0.5, -3.0])
FWD = np.array([0.0, -0.5, 3.0])
FWD_UNIT = FWD / np.linalg.norm(FWD)
WALL = 5.0                       # the distance of the wall from camera A along its forward vector


def camera_at(w, h, pos, fwd=FWD):
    return make_camera(w, h, position=[*pos, 0.0], forward=[*fwd, 0.0])


def wall_depth(cam, w, h):
    p = np.array([[*(POS_A + WALL * FWD_UNIT), 1.0]], np.float32)
    c = tr.rr.dot4(tr.rr.dot4(p, np.array(cam.view, np.float32)), np.array(cam.projection, np.float32))
    return F(c[0, 2] / c[0, 3])


def special_colours(rng, h, w):
    c = rng.random((h, w, 4), dtype=np.float32)
    special = np.array([0.0, -0.0, 1e-40, -3e-42, np.nan, np.inf, -np.inf, 1.5, 37.0, 1e-38, 3e19], np.float32)
    pick = rng.random((h, w, 4)) < 0.06
    c[pick] = rng.choice(special, size=int(pick.sum()))
    return c


def synthetic_views(w, h, seed):
    """Four views of one wall: (camera, normal_z, ids, colour) each.
    0: camera A. 1: camera B, moved back and sideways: the border falls off A's frame on all four sides. 2: B again
    with speckles of another id, another normal, another depth, NaN and +-inf depths and NO_PRIM. 3: at B, looking
    the other way: everything lies behind the previous camera."""
    rng = np.random.default_rng(seed)
    normal = (-FWD_UNIT).astype(np.float32)
    pos_b = POS_A - 1.8 * FWD_UNIT + np.array([0.1, 0.0, 0.0])
    cams = [camera_at(w, h, POS_A), camera_at(w, h, pos_b), camera_at(w, h, pos_b), camera_at(w, h, pos_b, -FWD)]
    views = []
    for k, cam in enumerate(cams):
        nz = np.empty((h, w, 4), np.float32)
        nz[..., :3] = normal
        nz[..., 3] = wall_depth(cam, w, h) if k < 3 else F(0.998)
        ids = np.full((h, w), 2, np.uint32)
        if k == 0:
            ids[:, : w // 3] = 1
        if k in (1, 2):
            ids[:, : max(1, (w // 3 + w // 6) * 3 // 4)] = 1
        if k == 2:
            sp = rng.random((h, w))
            ids[sp < 0.05] = 0
            other = rng.normal(size=(h, w, 3)).astype(np.float32)
            other /= np.linalg.norm(other, axis=2, keepdims=True).astype(np.float32)
            m = (sp >= 0.05) & (sp < 0.12)
            nz[m, :3] = other[m]
            m = (sp >= 0.12) & (sp < 0.2)
            nz[m, 3] = rng.random(int(m.sum()), dtype=np.float32)
            m = (sp >= 0.2) & (sp < 0.24)
            nz[m, 3] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, 1.0], np.float32), size=int(m.sum()))
        ids[rng.random((h, w)) < 0.08] = NO
        views.append((cam, nz, ids, special_colours(rng, h, w)))
    return views


# a frame smaller than the halo, one partial block, a block edge in x, one in y, both with interior blocks
FRAMES = [(1, 1), (5, 3), (17, 13), (33, 9), (65, 33)]
RESOLVES = [(0, 1, BIG, 7), (0, 1, 7, BIG), (BIG, 7, 0, 1), (1, 7, BIG, 0)]
TEMPORAL = (0.9, 0.01, 16)
LEVELS = (0, 1, 3, 5)
SIGMAS = (0.0, 4.0)
FLOORS = (1e-6, 1.0)
Q, S_Z = 5, 1024.0


@pytest.mark.parametrize("min_history", [1, 4])
@pytest.mark.parametrize("w,h", FRAMES)
def test_synthetic(require_gpu, w, h, min_history):
    """Every view and n with every filter setting: the histories and the variance estimate do not depend on the
    filter's parameters and a resolve modifies neither history, so each (view, n) is resolved once per setting and
    the reference's levels run once per (sigma, floor) on its c_0."""
    views = synthetic_views(w, h, seed=100 * w + h)
    ref = sr.Svgf(w, h, *TEMPORAL, min_history, 0, Q, S_Z, 4.0, 1e-6)
    with Svgf(w, h) as s:
        for k, (cam, nz, ids, c) in enumerate(views):
            ref.begin_view(cam, nz, ids)
            s.begin_view(cam, nz, ids)
            assert s.stats() == ref.stats(), f"{w}x{h} view {k}"
            for n in RESOLVES[k]:
                ref.resolve(c, n)
                assert np.all(np.isfinite(ref.c0[..., 3])) and np.all(ref.c0[..., 3] >= 0)
                for sigma in SIGMAS:
                    for floor in FLOORS:
                        chain = [ref.c0]
                        for i in range(max(LEVELS)):
                            chain.append(sr.level(chain[-1], nz, ids, i, Q, S_Z, sigma, floor))
                            assert np.all(np.isfinite(chain[-1][..., 3])) and np.all(chain[-1][..., 3] >= 0)
                        for levels in LEVELS:
                            what = f"{w}x{h} view {k} n={n} L={levels} sigma={sigma} floor={floor}"
                            s.set_params(*TEMPORAL, min_history, levels, Q, S_Z, sigma, floor)
                            s.resolve(c, n)
                            ref.stages = chain[:levels + 1]
                            assert_stages(s, ref, what)
        tm = s.time()
        runs = 16 * len(SIGMAS) * len(FLOORS) * len(LEVELS)
        assert tm["resolves"] == runs and tm["moments_ms"] > 0.0 and tm["variance_ms"] > 0.0 and tm["level_ms"][4] > 0.0
        assert min(tm["view_ms"]) > 0.0 and min(tm["history_resolve_ms"]) > 0.0


def test_both_estimates_run_on_every_size(require_gpu):
    """What test_synthetic's two values of min_history are for, from the reference alone: with 4 some pixel of every
    frame takes the spatial estimate, with 1 some pixel takes the temporal one."""
    for w, h in FRAMES:
        for min_history, want in ((1, False), (4, True)):
            ref = sr.Svgf(w, h, *TEMPORAL, min_history, 0, Q, S_Z, 4.0, 1e-6)
            seen = set()
            for k, (cam, nz, ids, c) in enumerate(synthetic_views(w, h, seed=100 * w + h)):
                ref.begin_view(cam, nz, ids)
                for n in RESOLVES[k]:
                    ref.resolve(c, n)
                    live = (ids != NO) & np.all(np.isfinite(ref.c0[..., :3]), axis=-1)
                    seen |= {bool(x) for x in ref.spatial[live]}
            assert want in seen, (w, h, min_history)


# ------------------------------------------------------------------------------------------------ real scenes
W, H = 96, 54
SCENE_PARAMS = (0.9, 0.01, 256, 2, 3, 5, 1024.0, 4.0, 1e-6)
DENOISE = (2, 5, 1024.0, 1.0)


def view_camera(k):
    return make_camera(W, H, position=[0.05 * k, 0.5, -3.0, 0.0], forward=[-0.02 * k, -0.5, 3.0, 0.0])


def beside(sc, with_svgf):
    """The three-view sequence through a Temporal and a Denoiser, with or without an Svgf resolving the same
    accumulator in between: what the two return at every step."""
    out = []
    with PathTracer(W, H, max_depth=8) as pt, Rasterizer(W, H) as r, Temporal(W, H) as t, Denoiser(W, H) as d, \
            (Svgf(W, H) if with_svgf else contextlib.nullcontext()) as s:
        if with_svgf:
            s.set_params(*SCENE_PARAMS)
        t.set_params(*SCENE_PARAMS[:3])
        d.set_params(*DENOISE)
        pt.upload_packet(sc.build_packet())
        r.upload_scene(sc)
        for k in range(3):
            cam = view_camera(k)
            pt.set_camera(align_camera(cam))              # DESIGN.md §9.7; every other object takes the plain one
            pt.reset()
            r.set_camera(cam)
            t.begin_view_raster(r)
            if with_svgf:
                s.begin_view_raster(r)
            for spp in (1, 2):
                pt.render(1)
                if with_svgf:
                    s.resolve_ctx(pt)
                t.resolve_ctx(pt)
                d.frame(pt, r)
                if with_svgf:
                    s.read()
                out.append((t.read(), d.read()))
    return out


@pytest.mark.parametrize("name", ["cornell_lit", "app_default"])
def test_scenes(require_gpu, name):
    """Three views through Rasterizer.gbuffer() and PathTracer with reset(): begin_view_raster + resolve_ctx, the
    host-plane path and the reference agree at every stage; the path tracer's own state still equals the oracle's
    afterwards; a Temporal and a Denoiser run beside it return what they return without it."""
    depth = 8
    sc = Scene()
    sc.add_preset(name)
    pk = sc.build_packet()
    ref = sr.Svgf(W, H, *SCENE_PARAMS)
    fr = oracle.OracleFrame(W, H, max_depth=depth)
    spatial = []
    with PathTracer(W, H, max_depth=depth) as pt, Rasterizer(W, H) as r, Svgf(W, H) as s, Svgf(W, H) as s_host:
        s.set_params(*SCENE_PARAMS)
        s_host.set_params(*SCENE_PARAMS)
        pt.upload_packet(pk)
        r.upload_scene(sc)
        for k in range(3):
            cam = view_camera(k)
            pt.set_camera(align_camera(cam))              # DESIGN.md §9.7; every other object takes the plain one
            pt.reset()
            r.set_camera(cam)
            s.begin_view_raster(r)
            nz, ids = r.gbuffer()
            s_host.begin_view(cam, nz, ids)
            ref.begin_view(cam, nz, ids)
            assert s.stats() == s_host.stats() == ref.stats()
            # before the first sample of the view: the reprojected history, filtered
            assert pt.frames() == 0
            ref.resolve(np.zeros((H, W, 4), np.float32), 0)
            s.resolve_ctx(pt)
            assert_stages(s, ref, f"{name} view {k} preview")
            for spp in (1, 2):                            # the same view resolved again as the accumulator grows
                pt.render(1)
                acc, _ = pt.read()
                assert pt.frames() == spp
                ref.resolve(acc, spp)
                s.resolve_ctx(pt)
                s_host.resolve(acc, spp)
                assert_stages(s, ref, f"{name} view {k} spp {spp}")
                assert_stages(s_host, ref, f"{name} view {k} spp {spp} (host planes)")
                v = ref.stages[-1][..., 3]
                assert np.all(np.isfinite(v)) and np.all(v >= 0)
                spatial.append(ref.stats())
            fr.reset()
            fr.render(pk, align_camera(cam), 2)
        # the first view is all spatial; later ones take the temporal estimate where the history holds
        guided, valid, took = spatial[0]
        assert valid == 0 and took == guided > W * H // 4
        guided, valid, took = spatial[-1]
        assert valid > guided // 2 and 0 < took < guided // 2
        assert np.any(ref.c0[..., 3] > 0)
        # the path tracer is untouched: accumulator, frame and RNG states still equal the oracle's
        acc, acc_bgra = pt.read()
        assert np.array_equal(bits(acc), bits(fr.lin)) and np.array_equal(acc_bgra, fr.bgra)
        assert np.array_equal(pt.read_rng(), fr.states)
    for step, (a, b) in enumerate(zip(beside(sc, True), beside(sc, False))):
        assert_same(a[0], b[0], f"{name} step {step}: Temporal beside Svgf")
        assert_same(a[1], b[1], f"{name} step {step}: Denoiser beside Svgf")


def test_clear_copies_and_device_forms(require_gpu):
    import torch
    sc = Scene()
    sc.add_preset("cornell_lit")
    ref = sr.Svgf(W, H, *SCENE_PARAMS)
    rng = np.random.default_rng(3)
    with Rasterizer(W, H) as r, Svgf(W, H) as s, PathTracer(W, H, max_depth=8) as pt:
        s.set_params(*SCENE_PARAMS)
        r.upload_scene(sc)
        pt.upload_packet(sc.build_packet())
        for k in range(2):
            cam = view_camera(k)
            r.set_camera(cam)
            nz, ids = r.gbuffer()
            nz_d, id_d = torch.from_numpy(nz.copy()).cuda(), torch.from_numpy(ids.view(np.int32).copy()).cuda()
            s.begin_view_device(cam, nz_d.data_ptr(), id_d.data_ptr())
            ref.begin_view(cam, nz, ids)
            with pytest.raises(iqpt.IqptError) as e:
                s.read()                                  # the result is invalid until the next resolve
            assert e.value.status == 5
            c = rng.random((H, W, 4), dtype=np.float32)
            src = torch.from_numpy(c.copy()).cuda()
            s.resolve_device(src.data_ptr(), 3)           # reads a caller's buffer in place and leaves it alone
            ref.resolve(c, 3)
            assert_stages(s, ref, f"device forms, view {k}")
            assert np.array_equal(bits(src.cpu().numpy()), bits(c))
        assert ref.stats()[1] > 0 and 0 < ref.stats()[2] < ref.stats()[0]
        dst = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        s.copy_frame_device(dst.data_ptr(), W * H * 4)
        assert np.array_equal(dst.cpu().numpy().view(np.uint8).reshape(H, W, 4), dr.encode_bgra(ref.stages[-1]))
        s.sync()

        # clear() forgets everything
        s.clear()
        ref.clear()
        for call in (lambda: s.resolve(c, 1), lambda: s.resolve_ctx(pt), lambda: s.read(), lambda: s.read_stages(),
                     lambda: s.stats(), lambda: s.resolve_device(src.data_ptr(), 1),
                     lambda: s.copy_frame_device(dst.data_ptr(), W * H * 4)):
            with pytest.raises(iqpt.IqptError) as e:
                call()
            assert e.value.status == 5                    # IQPT_ERR_NOT_READY
        s.begin_view(cam, nz, ids)
        ref.begin_view(cam, nz, ids)
        assert s.stats() == ref.stats() == (int(np.sum(ids != NO)), 0, 0)
        s.resolve(c, 1)
        ref.resolve(c, 1)
        assert_stages(s, ref, "after clear")
        assert ref.stats()[2] == int(np.sum(ids != NO))    # no history: the spatial estimate everywhere


def test_argument_checks(require_gpu):
    cam = make_camera(W, H)
    with PathTracer(32, 16) as small, Rasterizer(32, 16) as r_small, Rasterizer(W, H) as r, Svgf(W, H) as s, \
            PathTracer(W, H, pixels=iqpt.pixel_set(W, H, y0=0, ystep=2)) as part:
        planes = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32)
        with pytest.raises(iqpt.IqptError) as e:
            s.begin_view(make_camera(32, 16), *planes)    # a camera of another size
        assert e.value.status == 1
        with pytest.raises(iqpt.IqptError) as e:
            s.begin_view_raster(r_small)                  # a rasterizer of another size
        assert e.value.status == 1
        with pytest.raises(iqpt.IqptError) as e:
            s.begin_view_raster(r)                        # no camera, no scene
        assert e.value.status == 5
        with pytest.raises(iqpt.IqptError) as e:
            s.resolve(planes[0], 1)                       # no view
        assert e.value.status == 5
        s.begin_view(cam, *planes)
        for ctx in (small, part):                         # a context of another size, one that owns every other row
            with pytest.raises(iqpt.IqptError) as e:
                s.resolve_ctx(ctx)
            assert e.value.status == 1
        good = list(SCENE_PARAMS)
        for field, bad in ((1, -1.0), (3, 0), (4, 9), (5, 8), (6, float("inf")), (7, -1.0), (8, 0.0)):
            args = list(good)
            args[field] = bad
            with pytest.raises(iqpt.IqptError) as e:
                s.set_params(*args)
            assert e.value.status == 1 and "must be" in e.value.detail
        with pytest.raises(iqpt.IqptError) as e:
            s.copy_frame_device(1, 4)                     # no result yet
        assert e.value.status == 5
        s.resolve(planes[0], 1)
        with pytest.raises(iqpt.IqptError) as e:
            s.copy_frame_device(1, 4)                     # a wrong size
        assert e.value.status == 1
