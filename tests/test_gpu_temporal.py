"""The HIP temporal reprojection against its numpy reference (tests/temporal_ref.py): every float4
is compared as uint32, every BGRA byte for equality.

csrc/temporal/iq_temporal_kernels.hip ships three kernels: iqt_view_kernel (every begin_view, with and without a
previous result), iqt_resolve_kernel (every resolve) and iqt_stats_kernel (every stats call); all three are reached
by every test_synthetic case."""
import numpy as np
import pytest

import denoise_ref as dr
import iqpt
import oracle
import temporal_ref as tr
from iqpt import Denoiser, PathTracer, Rasterizer, Scene, Temporal, align_camera, make_camera

pytestmark = pytest.mark.gpu
NO = tr.NO_PRIM
F = np.float32
BIG = 1 << 24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what):
    lin, bgra = got
    ref, ref_bgra = want
    assert np.array_equal(bits(lin), bits(ref)), \
        f"{what}: {int(np.sum(np.any(bits(lin) != bits(ref), axis=-1)))} pixels differ"
    assert np.array_equal(bgra, ref_bgra), what


# ------------------------------------------------------------------------------------------------ synthetic
POS_A = np.array([0.0, 0.5, -3.0])
FWD = np.array([0.0, -0.5, 3.0])
FWD_UNIT = FWD / np.linalg.norm(FWD)
WALL = 5.0                       # the distance of the wall from camera A along its forward vector


def camera_at(w, h, pos, fwd=FWD):
    return make_camera(w, h, position=[*pos, 0.0], forward=[*fwd, 0.0])


def wall_depth(cam, w, h):
    """The D32 depth of the world plane through POS_A + WALL * forward, perpendicular to forward, in a camera that
    looks along forward too: constant over the frame."""
    p = np.array([[*(POS_A + WALL * FWD_UNIT), 1.0]], np.float32)
    c = tr.rr.dot4(tr.rr.dot4(p, np.array(cam.view, np.float32)), np.array(cam.projection, np.float32))
    return F(c[0, 2] / c[0, 3])


def special_colours(rng, h, w):
    c = rng.random((h, w, 4), dtype=np.float32)
    special = np.array([0.0, -0.0, 1e-40, -3e-42, np.nan, np.inf, -np.inf, 1.5, 37.0, 1e-38], np.float32)
    pick = rng.random((h, w, 4)) < 0.06
    c[pick] = rng.choice(special, size=int(pick.sum()))
    return c


def synthetic_views(w, h, seed):
    """Four views of one wall: (camera, normal_z, ids, colour) each.
    0: camera A. 1: camera B, moved back and sideways, sees more than A did: the border falls off A's frame on all
    four sides. 2: B again with speckles of another id, another normal, another depth, NaN and +-inf depths and
    NO_PRIM. 3: at B, looking the other way: everything lies behind the previous camera."""
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
            ids[:, : w // 3] = 1                                 # a second model on the wall's left third
        if k in (1, 2):
            # roughly the same split seen from B; the columns where it is off reproject onto the other id
            ids[:, : max(1, (w // 3 + w // 6) * 3 // 4)] = 1
        if k == 2:
            sp = rng.random((h, w))
            ids[sp < 0.05] = 0                                   # id mismatch
            other = rng.normal(size=(h, w, 3)).astype(np.float32)
            other /= np.linalg.norm(other, axis=2, keepdims=True).astype(np.float32)
            m = (sp >= 0.05) & (sp < 0.12)
            nz[m, :3] = other[m]                                 # normal
            m = (sp >= 0.12) & (sp < 0.2)
            nz[m, 3] = rng.random(int(m.sum()), dtype=np.float32)          # plane distance
            m = (sp >= 0.2) & (sp < 0.24)
            nz[m, 3] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, 1.0], np.float32), size=int(m.sum()))
        ids[rng.random((h, w)) < 0.08] = NO
        views.append((cam, nz, ids, special_colours(rng, h, w)))
    return views


FRAMES = [(1, 1), (5, 3), (17, 13), (33, 9), (65, 33)]   # one past the block's width and height, edge blocks, a 65th column
# the samples of every view's resolves, in order; the last one is what the next view inherits
RESOLVES = [(0, 1, BIG, 7), (0, 1, 7, BIG), (BIG, 7, 0, 1), (1, 7, BIG, 0)]
SYNTH_PARAMS = (0.9, 0.01, 16)


@pytest.mark.parametrize("w,h", FRAMES)
def test_synthetic(require_gpu, w, h):
    views = synthetic_views(w, h, seed=100 * w + h)
    ref = tr.Temporal(w, h, *SYNTH_PARAMS)
    reasons = []
    with Temporal(w, h) as t:
        t.set_params(*SYNTH_PARAMS)
        for k, (cam, nz, ids, c) in enumerate(views):
            ref.begin_view(cam, nz, ids)
            t.begin_view(cam, nz, ids)
            reasons.append(ref.reasons)
            assert t.stats() == ref.stats(), f"{w}x{h} view {k}"
            hist = ref.hist.copy()
            for n in RESOLVES[k]:
                want = ref.resolve(c, n)
                t.resolve(c, n)
                assert_same(t.read(), want, f"{w}x{h} view {k} n={n}")
                if n == 0:
                    assert np.array_equal(bits(want[0]), bits(hist))         # the history itself was compared
        vms, nv, rms, nr = t.time()
        assert nv == 4 and nr == 16 and vms > 0.0 and rms > 0.0
    if (w, h) != FRAMES[-1]:
        return
    # the largest frame went through every branch (the smaller ones run the same code at the frame's edges)
    assert not reasons[0]
    r = reasons[1]
    assert np.all(r["cw"] > 0) and np.any(r["valid"])
    assert np.any(r["xs"] < 0) and np.any(r["xs"] >= w) and np.any(r["ys"] < 0) and np.any(r["ys"] >= h)
    assert np.any(r["valid"] & ((r["qy"] != np.arange(h)[:, None]) | (r["qx"] != np.arange(w)[None, :])))
    r = reasons[2]
    sofar = r["guided"] & r["inside"]
    assert np.any(~r["guided"]) and np.any(r["guided"] & ~r["inside"])
    for name in ("same_id", "normal_ok", "plane_ok", "hist_ok"):
        assert np.any(sofar & ~r[name]), name
        sofar = sofar & r[name]
    assert np.array_equal(sofar, r["valid"]) and np.any(sofar)
    assert np.any(~np.isfinite(views[2][1][..., 3]) & r["guided"])
    r = reasons[3]
    assert np.all(r["cw"][r["guided"]] <= 0) and not np.any(r["valid"])


def test_the_cap_and_the_clamp(require_gpu):
    """max_history caps what a view inherits; n above 2^24 is clamped."""
    w, h = 33, 9
    cam = camera_at(w, h, POS_A)
    nz = np.empty((h, w, 4), np.float32)
    nz[..., :3] = (-FWD_UNIT).astype(np.float32)
    nz[..., 3] = wall_depth(cam, w, h)
    ids = np.zeros((h, w), np.uint32)
    rng = np.random.default_rng(9)
    ref = tr.Temporal(w, h, 0.9, 0.01, 5)
    with Temporal(w, h) as t:
        t.set_params(0.9, 0.01, 5)
        for k, n in enumerate((1000, 3, 1 << 40)):
            c = rng.random((h, w, 4), dtype=np.float32)
            ref.begin_view(cam, nz, ids)
            t.begin_view(cam, nz, ids)
            assert t.stats() == ref.stats() == (w * h, w * h if k else 0)
            want = ref.resolve(c, n)
            t.resolve(c, n)
            got = t.read()
            assert_same(got, want, f"view {k}")
            assert np.all(got[0][..., 3] == [1000, 8, F(5) + F(BIG)][k])


# ------------------------------------------------------------------------------------------------ real scenes
W, H = 96, 54
SCENE_PARAMS = (0.9, 0.01, 256)


def view_camera(k):
    return make_camera(W, H, position=[0.05 * k, 0.5, -3.0, 0.0], forward=[-0.02 * k, -0.5, 3.0, 0.0])


@pytest.mark.parametrize("name", ["cornell_lit", "app_default"])
def test_scenes(require_gpu, name):
    """Three views through Rasterizer.gbuffer() and PathTracer with reset(): begin_view_raster + resolve_ctx, the
    host-plane path and the reference agree; the path tracer's own state still equals the oracle's afterwards."""
    depth = 8
    sc = Scene()
    sc.add_preset(name)
    pk = sc.build_packet()
    ref = tr.Temporal(W, H, *SCENE_PARAMS)
    fr = oracle.OracleFrame(W, H, max_depth=depth)
    with PathTracer(W, H, max_depth=depth) as pt, Rasterizer(W, H) as r, Temporal(W, H) as t, Temporal(W, H) as t_host:
        t.set_params(*SCENE_PARAMS)
        t_host.set_params(*SCENE_PARAMS)
        pt.upload_packet(pk)
        r.upload_scene(sc)
        for k in range(3):
            cam = view_camera(k)
            pt.set_camera(align_camera(cam))              # DESIGN.md §9.7; every other object takes the plain one
            pt.reset()
            r.set_camera(cam)
            t.begin_view_raster(r)
            nz, ids = r.gbuffer()
            t_host.begin_view(cam, nz, ids)
            ref.begin_view(cam, nz, ids)
            assert t.stats() == t_host.stats() == ref.stats()
            guided, valid = ref.stats()
            assert guided > W * H // 4 and (valid > 0.5 * guided if k else valid == 0)
            # before the first sample of the view: the reprojected history alone
            assert pt.frames() == 0
            t.resolve_ctx(pt)
            assert_same(t.read(), (ref.hist, dr.encode_bgra(ref.hist)), f"{name} view {k} preview")
            for spp in (1, 2):                            # the same view resolved again as the accumulator grows
                pt.render(1)
                acc, _ = pt.read()
                assert pt.frames() == spp
                want = ref.resolve(acc, spp)
                t.resolve_ctx(pt)
                t_host.resolve(acc, spp)
                assert_same(t.read(), want, f"{name} view {k} spp {spp}")
                assert_same(t_host.read(), want, f"{name} view {k} spp {spp} (host planes)")
            fr.reset()
            fr.render(pk, align_camera(cam), 2)
        assert float(want[0][ids != NO][:, 3].mean()) > 4.0          # 2 + 2 + 2 samples where the history held
        # the path tracer is untouched: accumulator, frame and RNG states still equal the oracle's
        acc, acc_bgra = pt.read()
        assert np.array_equal(bits(acc), bits(fr.lin)) and np.array_equal(acc_bgra, fr.bgra)
        assert np.array_equal(pt.read_rng(), fr.states)


def test_denoise_chain_clear_and_copies(require_gpu):
    import torch
    depth, levels = 8, (2, 5, 1024.0, 1.0)
    sc = Scene()
    sc.add_preset("cornell_lit")
    ref = tr.Temporal(W, H, *SCENE_PARAMS)
    with PathTracer(W, H, max_depth=depth) as pt, Rasterizer(W, H) as r, Temporal(W, H) as t, Denoiser(W, H) as d:
        t.set_params(*SCENE_PARAMS)
        d.set_params(*levels)
        pt.upload_packet(sc.build_packet())
        r.upload_scene(sc)
        out_ptr = t.output_device()
        for k in range(2):
            cam = view_camera(k)
            pt.set_camera(align_camera(cam))              # DESIGN.md §9.7; every other object takes the plain one
            pt.reset()
            pt.render(1)
            r.set_camera(cam)
            t.begin_view_raster(r)
            t.resolve_ctx(pt)
            nz, ids = r.gbuffer()
            ref.begin_view(cam, nz, ids)
            want = ref.resolve(pt.read()[0], 1)
        assert_same(t.read(), want, "second view")
        # the device result, handed to the denoiser in place
        assert t.output_device() == out_ptr and out_ptr
        t.sync()
        d.set_guides(nz, ids)
        d.run_device(out_ptr)
        assert_same(d.read(), dr.denoise(want[0], nz, ids, *levels), "denoise(temporal)")
        assert_same(t.read(), want, "the result after the denoiser read it")
        dst = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        t.copy_frame_device(dst.data_ptr(), W * H * 4)
        assert np.array_equal(dst.cpu().numpy().view(np.uint8).reshape(H, W, 4), want[1])
        # resolve_device reads a caller's buffer in place and leaves it alone
        c = np.random.default_rng(3).random((H, W, 4), dtype=np.float32)
        src = torch.from_numpy(c.copy()).cuda()
        t.resolve_device(src.data_ptr(), 7)
        assert_same(t.read(), ref.resolve(c, 7), "resolve_device")
        assert np.array_equal(bits(src.cpu().numpy()), bits(c))
        # begin_view_device equals begin_view
        nz_d, id_d = torch.from_numpy(nz.copy()).cuda(), torch.from_numpy(ids.view(np.int32).copy()).cuda()
        t.begin_view_device(cam, nz_d.data_ptr(), id_d.data_ptr())
        ref.begin_view(cam, nz, ids)
        assert t.stats() == ref.stats() and ref.stats()[1] > 0
        with pytest.raises(iqpt.IqptError) as e:
            t.read()                                      # the result is invalid until the next resolve
        assert e.value.status == 5
        t.resolve(c, 0)
        assert_same(t.read(), ref.resolve(c, 0), "begin_view_device")

        # clear() forgets everything
        t.clear()
        for call in (lambda: t.resolve(c, 1), lambda: t.resolve_ctx(pt), lambda: t.read(), lambda: t.stats(),
                     lambda: t.copy_frame_device(dst.data_ptr(), W * H * 4)):
            with pytest.raises(iqpt.IqptError) as e:
                call()
            assert e.value.status == 5                    # IQPT_ERR_NOT_READY
        t.begin_view(cam, nz, ids)
        assert t.stats() == (int(np.sum(ids != NO)), 0)
        t.resolve(c, 0)
        lin, bgra = t.read()
        assert not bits(lin).any() and np.array_equal(bgra, dr.encode_bgra(np.zeros((H, W, 4), np.float32)))


def test_argument_checks(require_gpu):
    cam = make_camera(W, H)
    with PathTracer(32, 16) as small, Rasterizer(32, 16) as r_small, Rasterizer(W, H) as r, Temporal(W, H) as t, \
            PathTracer(W, H, pixels=iqpt.pixel_set(W, H, y0=0, ystep=2)) as part:
        planes = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32)
        with pytest.raises(iqpt.IqptError) as e:
            t.begin_view(make_camera(32, 16), *planes)    # a camera of another size
        assert e.value.status == 1
        with pytest.raises(iqpt.IqptError) as e:
            t.begin_view_raster(r_small)                  # a rasterizer of another size
        assert e.value.status == 1
        with pytest.raises(iqpt.IqptError) as e:
            t.begin_view_raster(r)                        # no camera, no scene
        assert e.value.status == 5
        with pytest.raises(iqpt.IqptError) as e:
            t.resolve(planes[0], 1)                       # no view
        assert e.value.status == 5
        t.begin_view(cam, *planes)
        for ctx in (small, part):                         # a context of another size, one that owns every other row
            with pytest.raises(iqpt.IqptError) as e:
                t.resolve_ctx(ctx)
            assert e.value.status == 1
        with pytest.raises(iqpt.IqptError) as e:
            t.set_params(0.9, -1.0, 256)
        assert e.value.status == 1
        with pytest.raises(iqpt.IqptError) as e:
            t.copy_frame_device(1, 4)                     # no result yet
        assert e.value.status == 5
