"""The HIP upscaler against its numpy reference (tests/upscale_ref.py): every float4 is compared as
uint32, every BGRA byte and the three class counts for equality.

csrc/upscale/iq_upscale_kernels.hip ships two kernels: iqu_upscale_kernel, with direct global loads (there is no LDS
variant), which every case below reaches, in every case with lanes of all three stages (the 2x2 one under
s_z = 1024); and iqu_stats_kernel, which every stats() call runs."""
import itertools

import numpy as np
import pytest

import denoise_ref as dr
import iqpt
import oracle
import upscale_ref as ur
from iqpt import Denoiser, PathTracer, Rasterizer, Scene, Upscaler, align_camera, make_camera

pytestmark = pytest.mark.gpu
NO = ur.NO_PRIM
FOREIGN_LO, FOREIGN_HI = 5, 7          # ids only the lo guides have, only the hi guides have


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def special_colours(rng, shape):
    """Colours in [0, 1) with +-0, subnormals, NaN, +-inf and values above 1 (test_gpu_denoise.py's values)."""
    c = rng.random(shape, dtype=np.float32)
    special = np.array([0.0, -0.0, 1e-40, -3e-42, np.nan, np.inf, -np.inf, 1.5, 37.0, 1e-38], np.float32)
    pick = rng.random(shape) < 0.06
    c[pick] = rng.choice(special, size=int(pick.sum()))
    return c


def guides(rng, h, w, ids):
    """Unit normals, mostly one of them so that q = 5 leaves weight, a few zero; z in [0, 1), 0.5 on most rows so that
    s_z = 1024 leaves weight, with speckles of NaN and +-inf."""
    yy, xx = np.mgrid[0:h, 0:w]
    n = rng.normal(size=(h, w, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=2, keepdims=True).astype(np.float32)
    n[(xx + yy) % 4 != 0] = np.array([0.36, 0.48, 0.8], np.float32)
    n[rng.random((h, w)) < 0.03] = 0.0
    z = rng.random((h, w), dtype=np.float32)
    z[yy % 3 != 0] = np.float32(0.5)
    bad = rng.random((h, w))
    z[bad < 0.02] = np.nan
    z[(bad >= 0.02) & (bad < 0.03)] = np.inf
    z[(bad >= 0.03) & (bad < 0.04)] = -np.inf
    return np.concatenate([n, z[..., None]], axis=2).astype(np.float32), ids.astype(np.uint32)


def synthetic(w, h, f, seed):
    """(colour_lo, nz_lo, id_lo, nz_hi, id_hi). Surfaces of three ids in patches and the sky, the hi ids those of the
    nearest lo pixel; then, independently at the two sizes, speckles of a foreign id, of NO_PRIM and of non-finite
    depth, and in the lo frame 2x2 blocks of the foreign id, whose hi pixels find their own id only in the widened
    stage."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = ((xx // 6 + yy // 4) % 4).astype(np.uint32)
    base[base == 3] = NO
    id_hi = np.repeat(np.repeat(base, f, axis=0), f, axis=1)
    id_lo = base.copy()
    for by, bx in ((1, 1), (h - 4, w - 5), (h // 2, w // 2), (2, w - 3), (h - 3, 2)):
        if 0 <= by and by + 2 <= h and 0 <= bx and bx + 2 <= w:
            id_lo[by:by + 2, bx:bx + 2] = FOREIGN_LO
    s = rng.random((h, w))
    id_lo[s < 0.04] = FOREIGN_LO
    id_lo[(s >= 0.04) & (s < 0.08)] = NO
    s = rng.random((h * f, w * f))
    id_hi[s < 0.03] = FOREIGN_HI
    id_hi[(s >= 0.03) & (s < 0.06)] = NO
    if w * h == 1:                                   # four hi pixels: three of the lo pixel's surface, one not
        id_lo[0, 0] = 1
        id_hi[:] = [[1, 1], [1, FOREIGN_HI]]
    nz_lo, id_lo = guides(rng, h, w, id_lo)
    nz_hi, id_hi = guides(rng, h * f, w * f, id_hi)
    c = special_colours(rng, (h, w, 4))
    if w * h == 1:
        # The lone lo pixel is every hi pixel's one tap, with g = 0.5625 in stage A and 1 in stage B. Hi (0, 0) is
        # guided. The other two are widened under s_z = 1024, where 1 + t t = 2: (0, 1) at q = 0 with d = 2^-148
        # (stage A: RN(0.5625 d) = 2^-149, halved it ties to even, 0; stage B: d / 2 = 2^-149), and (1, 0) at q = 5
        # with d = RN(2^-4.625), which five squarings take to 2^-148 (at q = 5 the d of (0, 1) squares to 0: class 2).
        c[0, 0] = [0.5, 1e-40, 37.0, -0.0]
        nz_lo[0, 0] = nz_hi[0, 0] = [1.0, 0.0, 0.0, 0.5]
        nz_hi[0, 1] = [2.0 ** -148, 0.0, 0.0, 0.5 + 2.0 ** -10]
        nz_hi[1, 0] = [np.float32(2.0 ** -4.625), 0.0, 0.0, 0.5 + 2.0 ** -10]
    return c, nz_lo, id_lo, nz_hi, id_hi


# (W, H, f): the smallest frame; one block and a bit in x, several in y; f = 3 and f = 4; partial blocks on both axes
# with x0 = -1 and x0 + 1 = w at the borders
FRAMES = [(2, 2, 2), (34, 26, 2), (51, 39, 3), (68, 36, 4), (66, 18, 2)]
PARAMS = list(itertools.product((0, 5), (0.0, 1024.0)))


@pytest.mark.parametrize("W,H,f", FRAMES)
def test_synthetic(require_gpu, W, H, f):
    w, h = W // f, H // f
    c, nz_lo, id_lo, nz_hi, id_hi = synthetic(w, h, f, seed=1000 * W + 10 * H + f)
    before = [a.copy() for a in (c, nz_lo, id_lo, nz_hi, id_hi)]
    with Upscaler(W, H, f) as u:
        assert (u.lo_width, u.lo_height) == (w, h)
        u.set_guides(nz_lo, id_lo, nz_hi, id_hi)
        for q, s_z in PARAMS:
            want, want_bgra, counts = ur.upscale(c, nz_lo, id_lo, nz_hi, id_hi, f, q, s_z)
            what = f"{W}x{H} f={f} q={q} s_z={s_z}"
            # A lone lo pixel cannot be widened where 1 + t t = 1, so under s_z = 0: its stage A weight is then
            # RN(0.5625 d) against d in stage B, and that rounds to zero only if d is zero. There the 2x2 frame has
            # classes 0 and 2 only; under s_z = 1024 it has all three (synthetic), as every other frame has throughout.
            assert counts[0] > 0 and counts[2] > 0 and (counts[1] > 0 or (w * h == 1 and s_z == 0.0)), \
                f"{what}: counts {counts}"
            u.set_params(q, s_z)
            u.run(c)
            lin, bgra = u.read()
            assert np.array_equal(bits(lin), bits(want)), \
                f"{what}: {int(np.sum(np.any(bits(lin) != bits(want), axis=2)))} pixels differ"
            assert np.array_equal(bgra, want_bgra), what
            assert u.stats() == counts, what
    for a, b in zip(before, (c, nz_lo, id_lo, nz_hi, id_hi)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_counts_beyond_one_pass(require_gpu):
    """1024x260 is 266240 pixels, past the 1024 blocks of 256 threads iqu_stats_kernel launches at most: some of its
    threads count two pixels. f = 4 from 256x65, several blocks on both axes."""
    W, H, f = 1024, 260, 4
    c, nz_lo, id_lo, nz_hi, id_hi = synthetic(W // f, H // f, f, seed=3)
    want, want_bgra, counts = ur.upscale(c, nz_lo, id_lo, nz_hi, id_hi, f, 5, 1024.0)
    assert all(n > 0 for n in counts) and sum(counts) == W * H > 1024 * 256
    with Upscaler(W, H, f) as u:
        u.set_guides(nz_lo, id_lo, nz_hi, id_hi)
        u.run(c)
        lin, bgra = u.read()
        assert np.array_equal(bits(lin), bits(want)) and np.array_equal(bgra, want_bgra)
        assert u.stats() == counts
        assert u.stats() == counts                        # counted afresh at every call


def test_run_device_and_copies(require_gpu):
    """run_device reads its input in place and leaves it alone; the device copies of the result are the result."""
    import torch
    W, H, f = 34, 26, 2
    w, h = W // f, H // f
    c, nz_lo, id_lo, nz_hi, id_hi = synthetic(w, h, f, seed=11)
    want, want_bgra, counts = ur.upscale(c, nz_lo, id_lo, nz_hi, id_hi, f, 5, 1024.0)
    dev = [torch.from_numpy(a.view(np.int32).copy()).cuda() for a in (c, nz_lo, id_lo, nz_hi, id_hi)]
    with Upscaler(W, H, f) as u:
        with pytest.raises(iqpt.IqptError) as e:
            u.read()
        assert e.value.status == 5                        # IQPT_ERR_NOT_READY: nothing was run
        with pytest.raises(iqpt.IqptError) as e:
            u.run(c)
        assert e.value.status == 5                        # no guides yet
        with pytest.raises(iqpt.IqptError) as e:
            u.set_params(8, 0.0)
        assert e.value.status == 1
        u.set_guides_device(*(t.data_ptr() for t in dev[1:]))
        u.run_device(dev[0].data_ptr())
        u.sync()
        lin, bgra = u.read()
        assert np.array_equal(bits(lin), bits(want)) and np.array_equal(bgra, want_bgra) and u.stats() == counts
        assert np.array_equal(dev[0].cpu().numpy().view(np.uint32), bits(c))
        frame_copy = torch.empty(W * H, dtype=torch.int32, device="cuda")
        u.copy_frame_device(frame_copy.data_ptr(), W * H * 4)
        assert np.array_equal(frame_copy.cpu().numpy().view(np.uint8).reshape(H, W, 4), bgra)
        with pytest.raises(iqpt.IqptError) as e:
            u.copy_frame_device(frame_copy.data_ptr(), W * H * 4 - 4)
        assert e.value.status == 1
        u.run_device(dev[0].data_ptr())
        ms, runs = u.time()
        assert runs == 2 and ms > 0.0
        assert u.time() == (0.0, 0)


# ------------------------------------------------------------------------------------------------ end to end
W, H, F = 96, 54, 2


def cornell():
    sc = Scene()
    sc.add_preset("cornell_lit")
    return sc


def test_frame_end_to_end(require_gpu):
    spp, depth = 4, 8
    w, h = W // F, H // F
    sc = cornell()
    pk = sc.build_packet()
    cam_hi, cam_lo = make_camera(W, H), make_camera(w, h)
    with PathTracer(w, h, max_depth=depth) as pt, Rasterizer(w, h) as r_lo, Rasterizer(W, H) as r_hi, \
            Upscaler(W, H, F) as u, Denoiser(W, H) as d:
        pt.set_camera(align_camera(cam_lo))               # DESIGN.md §9.7; the two rasterizers take the plain ones
        pt.upload_packet(pk)
        pt.render(spp)
        for r, cam in ((r_lo, cam_lo), (r_hi, cam_hi)):
            r.set_camera(cam)
            r.upload_scene(sc)
        u.frame(pt, r_lo, r_hi)
        lin, bgra = u.read()
        acc, acc_bgra = pt.read()
        nz_lo, id_lo = r_lo.gbuffer()
        nz_hi, id_hi = r_hi.gbuffer()
        p = iqpt.upscale.default_params()
        assert p == {"normal_squarings": 5, "depth_sharpness": 1024.0}
        want, want_bgra, counts = ur.upscale(acc, nz_lo, id_lo, nz_hi, id_hi, F, 5, 1024.0)
        assert np.array_equal(bits(lin), bits(want)) and np.array_equal(bgra, want_bgra)
        assert u.stats() == counts and sum(counts) == W * H and counts[0] > 0.98 * W * H
        # the lo path tracer is untouched: accumulator, frame and RNG states still equal the oracle's
        fr = oracle.OracleFrame(w, h, max_depth=depth)
        fr.render(pk, align_camera(cam_lo), spp)
        assert np.array_equal(bits(acc), bits(fr.lin)) and np.array_equal(acc_bgra, fr.bgra)
        assert np.array_equal(pt.read_rng(), fr.states)
        # the same call again gives the same bits
        u.frame(pt, r_lo, r_hi)
        lin2, bgra2 = u.read()
        assert np.array_equal(bits(lin2), bits(lin)) and np.array_equal(bgra2, bgra)
        # the device result feeds a full-size stage: the denoiser under the hi guides
        params = (3, 5, 1024.0, 2.0)
        d.set_params(*params)
        d.set_guides(nz_hi, id_hi)
        d.run_device(u.output_ptr)
        den, den_bgra = d.read()
        want_den, want_den_bgra = dr.denoise(want, nz_hi, id_hi, *params)
        assert np.array_equal(bits(den), bits(want_den)) and np.array_equal(den_bgra, want_den_bgra)
        assert np.array_equal(bits(u.read()[0]), bits(lin))       # which left the upscaler's result alone


def test_frame_argument_checks(require_gpu):
    w, h = W // F, H // F
    sc = cornell()
    cam_hi, cam_lo = make_camera(W, H), make_camera(w, h)
    moved = make_camera(W, H, position=[0.1, 0.0, -3.0, 0.0])
    with PathTracer(w, h) as pt, PathTracer(W, H) as pt_hi, Rasterizer(w, h) as r_lo, Rasterizer(W, H) as r_hi, \
            PathTracer(W, H, pixels=iqpt.pixel_set(W, H, y0=0, ystep=2)) as part, Upscaler(W, H, F) as u:
        def refused(*args):
            with pytest.raises(iqpt.IqptError) as e:
                u.frame(*args)
            return e.value.status

        assert refused(pt, r_lo, r_hi) == 5               # IQPT_ERR_NOT_READY: the rasterizers have no camera yet
        for r, cam in ((r_lo, cam_lo), (r_hi, cam_hi)):
            r.set_camera(cam)
            r.upload_scene(sc)
        assert refused(pt_hi, r_lo, r_hi) == 1            # a context of the hi size
        assert refused(part, r_lo, r_hi) == 1             # a context that owns half the hi frame's rows
        assert refused(pt, r_hi, r_hi) == 1               # a lo rasterizer of the hi size
        assert refused(pt, r_lo, r_lo) == 1               # a hi rasterizer of the lo size
        assert refused(pt, r_hi, r_lo) == 1               # the two swapped
        r_hi.set_camera(moved)
        assert refused(pt, r_lo, r_hi) == 1               # cameras that differ in the view matrix
        assert b"cameras differ" in u._lib.iqpt_last_error()
        r_hi.set_camera(make_camera(W, H, fovh=60.0))
        assert refused(pt, r_lo, r_hi) == 1               # cameras that differ in the projection
        with pytest.raises(iqpt.IqptError) as e:
            u.read()
        assert e.value.status == 5                        # nothing of this ran
        r_hi.set_camera(cam_hi)
        pt.set_camera(cam_lo)
        pt.upload_packet(sc.build_packet())
        pt.render(1)
        u.frame(pt, r_lo, r_hi)
        assert sum(u.stats()) == W * H
    for bad in ((W, H, 5), (W, H, 1), (W + 1, H, 2), (W, H + 1, 2), (W, H, 4)):
        with pytest.raises(iqpt.IqptError) as e:
            Upscaler(*bad)
        assert e.value.status == 1
