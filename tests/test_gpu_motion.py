"""The HIP moving-model reprojection (libiqpt_motion.so) against its numpy reference (tests/motion_ref.py, DESIGN.md
§15): every float4 is compared as uint32, every BGRA byte and the four counts for equality.

csrc/motion/iq_motion_kernels.hip ships two kernels: iqm_view_kernel (every begin_view; its per-lane gather and its
table-free path are reached by every synthetic case and by the n = 0 cases; the A/B library's wave-uniform entry
path by the "waves" layout and its gather fallback by "checker" and "foreign") and iqm_stats_kernel (every stats
call). The resolve is libiqpt.so's iqt_resolve_kernel."""
import numpy as np
import pytest

import denoise_ref as dr
import iqpt
import motion_cases as mc
import motion_ref as mr
import oracle
from iqpt import Denoiser, Motion, PathTracer, Rasterizer, Temporal, _build, align_camera, make_camera

pytestmark = pytest.mark.gpu
NO = mr.NO_PRIM
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what):
    lin, bgra = got
    ref, ref_bgra = want
    assert np.array_equal(bits(lin), bits(ref)), \
        f"{what}: {int(np.sum(np.any(bits(lin) != bits(ref), axis=-1)))} pixels differ"
    assert np.array_equal(bgra, ref_bgra), what


# ------------------------------------------------------------------------------------------------ synthetic
FRAMES = [(1, 1), (17, 13), (65, 33), (66, 18)]     # partial blocks and waves, a second block row and column
TABLES = [1, 3, 77]


def run_case(m, ref, views, what):
    """The views through a Motion (or anything with its methods) and the reference; returns the reference's stats
    and reasons per view."""
    seen = []
    for k, (cam, nz, ids, colour, samples, table) in enumerate(views):
        ref.begin_view(cam, nz, ids, table)
        m.begin_view(cam, nz, ids, motion=table)
        want_stats = ref.stats()
        seen.append((want_stats, ref.reasons))
        assert m.stats() == want_stats, f"{what} view {k}"
        for n in (0, samples):          # the history itself, then the blend the next view inherits
            want = ref.resolve(colour, n)
            m.resolve(colour, n)
            assert_same(m.read(), want, f"{what} view {k} n={n}")
    return seen


@pytest.mark.parametrize("layout", mc.LAYOUTS)
@pytest.mark.parametrize("n", TABLES)
@pytest.mark.parametrize("w,h", FRAMES)
def test_synthetic(require_gpu, w, h, n, layout):
    views = mc.synthetic_views(w, h, n, layout, seed=1000 * w + 10 * h + n)
    ref = mr.Motion(w, h, *mc.PARAMS)
    # before comparing: the reference itself has something to compare wherever the case can have it
    probe = mr.Motion(w, h, *mc.PARAMS)
    for k, (cam, nz, ids, colour, samples, table) in enumerate(views):
        probe.begin_view(cam, nz, ids, table)
        probe.resolve(colour, samples)
        if k == 1:
            guided, valid, moved, moved_valid = probe.stats()
            assert guided > 0
            if (w, h) != (1, 1):
                assert valid > 0 and moved > 0 and moved_valid > 0, (valid, moved, moved_valid)
            else:                       # one pixel: its id is 0, which a table of one entry moves (by nothing)
                assert valid == 1 and (moved, moved_valid) == ((1, 1) if n == 1 or layout != "waves" else (0, 0))
    with Motion(w, h) as m:
        m.set_params(*mc.PARAMS)
        seen = run_case(m, ref, views, f"{w}x{h} n={n} {layout}")
        vms, nv, rms, nr = m.time()
        assert nv == 3 and nr == 6 and vms > 0.0 and rms > 0.0
    if (w, h) != (65, 33) or n != 77:
        return
    # the largest case went through every branch of the moved path
    r = seen[2][1]
    mv = r["moved_reasons"]
    sofar = r["moved"] & mv["inside"]
    assert np.any(r["moved"] & ~mv["inside"]) and np.any(r["moved"] & ~(mv["cw"] > 0))
    for name in ("same_id", "normal_ok", "plane_ok", "hist_ok"):
        assert np.any(sofar & ~mv[name]), name
        sofar = sofar & mv[name]
    assert np.any(sofar)
    if layout == "waves":               # the other layouts keep every id inside the table
        assert np.any(~r["in_table"] & r["guided"]) and np.any(~r["guided"])
    assert np.any(r["moved"] & ~np.isfinite(mv["Pm"][..., 0]))              # the NaN entry


@pytest.mark.parametrize("table", ["none", "static"])
def test_a_static_table_is_temporal_on_the_device(require_gpu, table):
    w, h, n = 65, 33, 3
    views = mc.synthetic_views(w, h, n, "waves", seed=77)
    with Motion(w, h) as m, Temporal(w, h) as t:
        m.set_params(*mc.PARAMS)
        t.set_params(*mc.PARAMS)
        valid = 0
        for k, (cam, nz, ids, colour, samples, _) in enumerate(views):
            ids = np.where(ids == NO, NO, ids % n).astype(np.uint32)
            m.begin_view(cam, nz, ids, motion=None if table == "none" else mr.identity_table(n))
            t.begin_view(cam, nz, ids)
            assert m.stats() == t.stats() + (0, 0)
            valid += t.stats()[1]
            for s in (0, samples):
                m.resolve(colour, s)
                t.resolve(colour, s)
                assert_same(m.read(), t.read(), f"view {k} n={s}")
        assert valid > 0


@pytest.mark.parametrize("layout", mc.LAYOUTS)
def test_both_forms_give_the_same_bits(require_gpu, layout):
    """The default library (every lane gathers its entry) and the A/B library (wave-uniform entry loads, the gather
    as the fallback)."""
    w, h, n = 66, 18, 77
    views = mc.synthetic_views(w, h, n, layout, seed=4)
    with Motion(w, h) as a, Motion(w, h, lib=_build.MOTION_UNIFORM_LIB_PATH) as b:
        assert a._lib is not b._lib
        moved_valid = 0
        for k, (cam, nz, ids, colour, samples, table) in enumerate(views):
            for m in (a, b):
                m.set_params(*mc.PARAMS)
                m.begin_view(cam, nz, ids, motion=table)
                m.resolve(colour, samples)
            assert a.stats() == b.stats()
            moved_valid += a.stats()[3]
            assert_same(a.read(), b.read(), f"{layout} view {k}")
        assert moved_valid > 0


# ------------------------------------------------------------------------------------------------ the movers scene
W, H = 96, 54
SCENE_PARAMS = (0.9, 0.01, 256)


def test_movers_end_to_end(require_gpu):
    """Two scenes, two uploads to one Rasterizer and one PathTracer with reset() between: begin_view_raster with
    motion_table's table + resolve_ctx (resolved again as the accumulator grows), the host-plane and the device-plane
    forms and the reference agree; output_device feeds the denoiser; the path tracer's own state still equals the
    oracle's afterwards."""
    import torch
    depth, levels = 8, (2, 5, 1024.0, 1.0)
    cam = mc.movers_camera(W, H)
    ref = mr.Motion(W, H, *SCENE_PARAMS)
    fr = oracle.OracleFrame(W, H, max_depth=depth)
    scenes = [mc.movers(0), mc.movers(1)]
    with PathTracer(W, H, max_depth=depth) as pt, Rasterizer(W, H) as r, Motion(W, H) as m, Motion(W, H) as m_host, \
            Motion(W, H) as m_dev, Denoiser(W, H) as d:
        for o in (m, m_host, m_dev):
            o.set_params(*SCENE_PARAMS)
        d.set_params(*levels)
        pt.set_camera(align_camera(cam))                  # DESIGN.md §9.7; every other object takes the plain one
        r.set_camera(cam)
        out_ptr = m.output_device()
        for k, sc in enumerate(scenes):
            table = iqpt.motion_table(scenes[k - 1], sc) if k else None
            if k:
                assert list(table["moved"]) == [0, 0, 1]
            pk = sc.build_packet()
            pt.upload_packet(pk)
            pt.reset()
            r.upload_scene(sc)
            m.begin_view_raster(r, motion=table)
            nz, ids = r.gbuffer()
            m_host.begin_view(cam, nz, ids, motion=table)
            nz_d, id_d = torch.from_numpy(nz.copy()).cuda(), torch.from_numpy(ids.view(np.int32).copy()).cuda()
            m_dev.begin_view_device(cam, nz_d.data_ptr(), id_d.data_ptr(), motion=table)
            ref.begin_view(cam, nz, ids, table)
            assert m.stats() == m_host.stats() == m_dev.stats() == ref.stats()
            guided, valid, moved, moved_valid = ref.stats()
            if k:
                assert valid > 0.8 * guided and moved > 50 and moved_valid > moved // 2
                assert int(np.sum(ids == mc.MOVER)) == moved
            assert pt.frames() == 0
            for spp in (1, 2):                            # the same view resolved again as the accumulator grows
                pt.render(1)
                acc, _ = pt.read()
                want = ref.resolve(acc, spp)
                m.resolve_ctx(pt)
                m_host.resolve(acc, spp)
                src = torch.from_numpy(acc.copy()).cuda()
                m_dev.resolve_device(src.data_ptr(), spp)
                for o, name in ((m, "raster"), (m_host, "host planes"), (m_dev, "device planes")):
                    assert_same(o.read(), want, f"view {k} spp {spp} ({name})")
            fr.reset()
            fr.render(pk, align_camera(cam), 2)
        assert float(want[0][ids == mc.MOVER][:, 3].mean()) > 3.0       # 2 + 2 samples where the mover's history held
        # the device result, handed to the denoiser in place
        assert m.output_device() == out_ptr and out_ptr
        m.sync()
        d.set_guides(nz, ids)
        d.run_device(out_ptr)
        assert_same(d.read(), dr.denoise(want[0], nz, ids, *levels), "denoise(motion)")
        assert_same(m.read(), want, "the result after the denoiser read it")
        dst = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        m.copy_frame_device(dst.data_ptr(), W * H * 4)
        assert np.array_equal(dst.cpu().numpy().view(np.uint8).reshape(H, W, 4), want[1])
        # the path tracer is untouched: accumulator, frame and RNG states still equal the oracle's
        acc, acc_bgra = pt.read()
        assert np.array_equal(bits(acc), bits(fr.lin)) and np.array_equal(acc_bgra, fr.bgra)
        assert np.array_equal(pt.read_rng(), fr.states)
        # clear() forgets everything
        m.clear()
        for call in (lambda: m.resolve(acc, 1), lambda: m.resolve_ctx(pt), lambda: m.read(), lambda: m.stats(),
                     lambda: m.copy_frame_device(dst.data_ptr(), W * H * 4)):
            with pytest.raises(iqpt.IqptError) as e:
                call()
            assert e.value.status == 5                    # IQPT_ERR_NOT_READY
        m.begin_view(cam, nz, ids, motion=table)
        assert m.stats() == (int(np.sum(ids != NO)), 0, int(np.sum(ids == mc.MOVER)), 0)


def test_the_table_buffer_grows(require_gpu):
    """Tables of 1, 77, 3 and 2^12 entries through one object: the device buffer grows on demand and a shorter table
    after a longer one bounds the ids by its own n."""
    w, h = 17, 13
    ref = mr.Motion(w, h, *mc.PARAMS)
    with Motion(w, h) as m:
        m.set_params(*mc.PARAMS)
        for k, n in enumerate((1, 77, 3, 1 << 12)):
            cam, nz, ids, colour, samples, _ = mc.synthetic_views(w, h, 77, "waves", seed=k)[1]
            table = mc.make_table(n, cam, w)
            ref.begin_view(cam, nz, ids, table)
            m.begin_view(cam, nz, ids, motion=table)
            assert m.stats() == ref.stats()
            want = ref.resolve(colour, samples)
            m.resolve(colour, samples)
            assert_same(m.read(), want, f"n={n}")


def test_argument_checks(require_gpu):
    cam = make_camera(W, H)
    with PathTracer(32, 16) as small, Rasterizer(32, 16) as r_small, Rasterizer(W, H) as r, Motion(W, H) as m, \
            PathTracer(W, H, pixels=iqpt.pixel_set(W, H, y0=0, ystep=2)) as part:
        planes = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32)
        table = mr.identity_table(2)
        with pytest.raises(iqpt.IqptError) as e:
            m.begin_view(make_camera(32, 16), *planes)    # a camera of another size
        assert e.value.status == 1
        with pytest.raises(iqpt.IqptError) as e:
            m.begin_view_raster(r_small)                  # a rasterizer of another size
        assert e.value.status == 1
        with pytest.raises(iqpt.IqptError) as e:
            m.begin_view_raster(r)                        # no camera, no scene
        assert e.value.status == 5
        with pytest.raises(iqpt.IqptError) as e:
            m.resolve(planes[0], 1)                       # no view
        assert e.value.status == 5
        for field, value in (("moved", 2), ("moved", 0x80000000), ("reserved", 7)):
            bad = table.copy()
            bad[field][1] = value
            for call in (lambda: m.begin_view(cam, *planes, motion=bad), lambda: m.begin_view_device(cam, 1, 1, motion=bad),
                         lambda: m.begin_view_raster(r, motion=bad)):
                with pytest.raises(iqpt.IqptError) as e:
                    call()
                assert e.value.status == 1
        lib = iqpt._lib.load_motion()
        import ctypes as C
        nzp = planes[0].ctypes.data_as(C.POINTER(C.c_float))
        idp = planes[1].ctypes.data_as(C.POINTER(C.c_uint32))
        assert lib.iqpt_motion_begin_view(m.handle, C.byref(cam), nzp, idp, None, 2) == 1         # NULL with n > 0
        assert lib.iqpt_motion_begin_view(m.handle, C.byref(cam), nzp, idp, C.c_void_p(table.ctypes.data),
                                          (1 << 20) + 1) == 1
        with pytest.raises(ValueError):
            m.begin_view(cam, *planes, motion=np.zeros(2, np.float32))
        with pytest.raises(iqpt.IqptError) as e:
            m.stats()                                     # none of the refused calls began a view
        assert e.value.status == 5
        m.begin_view(cam, *planes, motion=table)
        for ctx in (small, part):                         # a context of another size, one that owns every other row
            with pytest.raises(iqpt.IqptError) as e:
                m.resolve_ctx(ctx)
            assert e.value.status == 1
        with pytest.raises(iqpt.IqptError) as e:
            m.set_params(0.9, -1.0, 256)
        assert e.value.status == 1
        with pytest.raises(iqpt.IqptError) as e:
            m.read()                                      # no result yet
        assert e.value.status == 5
        with pytest.raises(iqpt.IqptError) as e:
            m.copy_frame_device(1, 4)                     # no result yet
        assert e.value.status == 5
        m.resolve(planes[0], 1)
        with pytest.raises(iqpt.IqptError) as e:
            m.copy_frame_device(1, 4)                     # not a frame's size
        assert e.value.status == 1
