"""The HIP denoiser and the rasterizer's G-buffer against their numpy reference (tests/denoise_ref.py, DESIGN.md
§9.6 and §10): every float4 is compared as uint32, every BGRA byte for equality.

Which case reaches which kernel instantiation (csrc/denoise/iq_denoise_kernels.hip ships the two level kernels,
csrc/post/iq_post_kernels.hip the encoding, all with direct global loads; there is no LDS variant):
  iqd_level_kernel<true>   (the last level, writes the BGRA frame too): every test_synthetic case, L = 1..5
  iqd_level_kernel<false>  (the levels before the last):                every test_synthetic case with L >= 2
  iqp_encode_kernel        (L = 0, encoding only):                      test_zero_levels
and csrc/raster/iq_raster_kernels.hip two for the G-buffer, reached by every test_gbuffer_* case:
  iqr_setup_kernel<true>, iqr_guide_tile_kernel."""
import itertools

import numpy as np
import pytest

import denoise_ref as dr
import iqpt
import oracle
import raster_ref as rr
from iqpt import Denoiser, PathTracer, Rasterizer, Scene, align_camera, make_camera

pytestmark = pytest.mark.gpu
NO = dr.NO_PRIM


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def synthetic(w, h, seed):
    """Guides and colours from a seeded generator: ids of 3 values and NO_PRIM in patches and speckles, unit normals
    with a few zero normals, z in [0, 1], colours in [0, 1] with +-0, subnormals, NaN, +-inf and values above 1."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 3, size=(h, w)).astype(np.uint32)
    yy, xx = np.mgrid[0:h, 0:w]
    ids[(xx // 7 + yy // 5) % 3 == 0] = 1                        # patches, so that taps find their own id
    ids[rng.random((h, w)) < 0.15] = NO
    n = rng.normal(size=(h, w, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=2, keepdims=True).astype(np.float32)
    n[(xx + yy) % 4 != 0] = n[0, 0]                              # mostly one normal, so that q = 5 leaves weight
    n[rng.random((h, w)) < 0.05] = 0.0
    z = rng.random((h, w, 1), dtype=np.float32)
    z[yy % 2 == 0] = np.float32(0.5)                             # equal depths, so that s_z = 1024 leaves weight
    nz = np.concatenate([n, z], axis=2).astype(np.float32)
    c = rng.random((h, w, 4), dtype=np.float32)
    special = np.array([0.0, -0.0, 1e-40, -3e-42, np.nan, np.inf, -np.inf, 1.5, 37.0, 1e-38], np.float32)
    pick = rng.random((h, w, 4)) < 0.06
    c[pick] = rng.choice(special, size=int(pick.sum()))
    return c, nz, ids


FRAMES = [(1, 1), (5, 3), (17, 13), (33, 9), (65, 33)]   # one past the block's width and height, edge blocks, frames
                                                          # smaller than the footprint


@pytest.mark.parametrize("w,h", FRAMES)
def test_synthetic(require_gpu, w, h):
    c, nz, ids = synthetic(w, h, seed=100 * w + h)
    with Denoiser(w, h) as d:
        d.set_guides(nz, ids)
        for levels, q, s_z, s_c in itertools.product(range(1, 6), (0, 5), (0.0, 1024.0), (0.0, 2.0)):
            d.set_params(levels, q, s_z, s_c)
            d.run(c)
            lin, bgra = d.read()
            want, want_bgra = dr.denoise(c, nz, ids, levels, q, s_z, s_c)
            what = f"{w}x{h} L={levels} q={q} s_z={s_z} s_c={s_c}"
            assert np.array_equal(bits(lin), bits(want)), \
                f"{what}: {int(np.sum(np.any(bits(lin) != bits(want), axis=2)))} pixels differ"
            assert np.array_equal(bgra, want_bgra), what
    if w * h > 1:
        keep = (ids == NO) | ~np.all(np.isfinite(c[..., :3]), axis=2)
        assert np.array_equal(bits(lin)[keep], bits(c)[keep]) and (w * h < 100 or not np.array_equal(bits(lin), bits(c)))


def test_zero_levels(require_gpu):
    c, nz, ids = synthetic(33, 9, seed=5)
    with Denoiser(33, 9) as d:
        d.set_guides(nz, ids)
        d.set_params(0, 5, 1024.0, 2.0)
        d.run(c)
        lin, bgra = d.read()
    assert np.array_equal(bits(lin), bits(c)) and np.array_equal(bgra, dr.encode_bgra(c))


# ------------------------------------------------------------------------------------------------ G-buffer
W, H = 96, 54


def preset(name):
    sc = Scene()
    sc.add_preset(name)
    return sc


def inside_cube():
    sc = Scene()
    sc.add_mesh_cube("box")
    sc.add_model("room", "box", scale=4.0)
    return sc, make_camera(W, H, position=[0.0, 0.0, 0.0, 0.0], forward=[0.3, -0.2, 1.0, 0.0])


_refs = {}


def gbuffer_ref(name):
    """The reference G-buffer of a scene at 96x54, computed once and shared."""
    if name not in _refs:
        sc, cam = inside_cube() if name == "inside_cube" else (preset(name), make_camera(W, H))
        out = dr.gbuffer_scene(sc.draw_list(), cam, W, H)
        for a in out:
            a.setflags(write=False)
        _refs[name] = out
    return _refs[name]


def assert_gbuffer(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: {int(np.sum(got[1] != want[1]))} ids differ"
    assert np.array_equal(bits(got[0]), bits(want[0])), \
        f"{what}: {int(np.sum(np.any(bits(got[0]) != bits(want[0]), axis=2)))} normal/depth pixels differ"


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("name", ["cornell", "cornell_lit", "app_default", "inside_cube"])
def test_gbuffer_scenes(require_gpu, name, samples):
    sc, cam = inside_cube() if name == "inside_cube" else (preset(name), make_camera(W, H))
    with Rasterizer(W, H, samples=samples) as r:
        r.set_camera(cam)
        r.upload_scene(sc)
        got = r.gbuffer()
    assert_gbuffer(got, gbuffer_ref(name), f"{name}, samples={samples}")    # so identical for samples 1 and 4
    if name == "inside_cube":
        assert np.all(got[1] == 0)
    else:
        assert 0.25 < np.mean(got[1] != NO) < 1.0 and len(np.unique(got[1])) > 3


def test_gbuffer_against_the_draw(require_gpu):
    """With samples=1 the G-buffer's depth is the draw's wherever both are drawn, and its id the draw of that
    primitive; a draw and its readback do not depend on G-buffer passes around them."""
    sc = preset("app_default")
    items = sc.draw_list()
    draw_of_tri = np.concatenate([np.full(d["indices"].size // 3, k) for k, d in enumerate(items)])
    cam_b = make_camera(W, H, position=[0.8, 1.0, -2.5, 0.0], forward=[-0.3, -0.4, 1.0, 0.0])
    with Rasterizer(W, H, samples=1) as r:
        r.set_camera(make_camera(W, H))
        r.upload_scene(sc)
        r.draw()
        plain = r.read(samples=True)
        nz, ids = r.gbuffer()
        after = r.read(samples=True)                      # the last draw's lists are still the draw's
        r.draw()
        again = r.read(samples=True)
        for got in (after, again):
            for a, b in zip(got, plain):
                assert np.array_equal(a, b)
        depth, prim = plain[1][..., 0], plain[2][..., 0]
        both = (prim != rr.NO_PRIM) & (ids != NO)
        assert np.mean(both) > 0.25
        assert np.array_equal(bits(nz[..., 3])[both], bits(depth)[both])
        assert np.array_equal(ids[both], draw_of_tri[prim[both]].astype(np.uint32))
        assert np.all(ids[prim != rr.NO_PRIM] != NO)      # two-sided guides cover at least what the draw covers
        # kept until the camera changes, then recomputed
        assert_gbuffer(r.gbuffer(), (nz, ids), "second call")
        r.set_camera(cam_b)
        moved = r.gbuffer()
        assert not np.array_equal(moved[1], ids)
        assert_gbuffer(moved, dr.gbuffer_scene(items, cam_b, W, H), "after set_camera")
    with Rasterizer(W, H, samples=1) as r:                # G-buffer first, then the draw
        r.set_camera(make_camera(W, H))
        r.upload_scene(sc)
        r.gbuffer()
        r.draw()
        for a, b in zip(r.read(samples=True), plain):
            assert np.array_equal(a, b)
    with Rasterizer(16, 16) as r:
        with pytest.raises(iqpt.IqptError) as e:
            r.gbuffer()
        assert e.value.status == 5                        # IQPT_ERR_NOT_READY


# ------------------------------------------------------------------------------------------------ end to end
def test_frame_end_to_end(require_gpu):
    import torch
    spp, depth = 4, 8
    sc = preset("cornell_lit")
    pk = sc.build_packet()
    cam = make_camera(W, H)
    params = (3, 5, 1024.0, 2.0)
    with PathTracer(W, H, max_depth=depth) as pt, Rasterizer(W, H) as r, Denoiser(W, H) as d:
        pt.set_camera(align_camera(cam))                  # the path tracer's camera is the aligned one
        pt.upload_packet(pk)
        pt.render(spp)
        r.set_camera(cam)
        r.upload_scene(sc)
        d.set_params(*params)
        d.frame(pt, r)
        lin, bgra = d.read()
        acc, acc_bgra = pt.read()
        nz, ids = r.gbuffer()
        want, want_bgra = dr.denoise(acc, nz, ids, *params)
        assert np.array_equal(bits(lin), bits(want)) and np.array_equal(bgra, want_bgra)
        assert_gbuffer((nz, ids), gbuffer_ref("cornell_lit"), "cornell_lit")
        # the path tracer is untouched: its frame still equals the oracle bit for bit
        fr = oracle.OracleFrame(W, H, max_depth=depth)
        fr.render(pk, align_camera(cam), spp)
        assert np.array_equal(bits(acc), bits(fr.lin)) and np.array_equal(acc_bgra, fr.bgra)
        # the filter did something, and the same call again gives the same bits
        guided = ids != NO
        assert not np.array_equal(bits(lin)[guided], bits(acc.reshape(H, W, 4))[guided])
        d.frame(pt, r)
        lin2, bgra2 = d.read()
        assert np.array_equal(bits(lin2), bits(lin)) and np.array_equal(bgra2, bgra)

        # run_device leaves its input alone and equals run
        src = torch.from_numpy(acc.reshape(H, W, 4).copy()).cuda()
        d.run_device(src.data_ptr())
        d.sync()
        lin3, _ = d.read()
        assert np.array_equal(bits(src.cpu().numpy()), bits(acc.reshape(H, W, 4)))
        assert np.array_equal(bits(lin3), bits(lin))
        dst = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        d.copy_frame_device(dst.data_ptr(), W * H * 4)
        assert np.array_equal(dst.cpu().numpy().view(np.uint8).reshape(H, W, 4), bgra)
        ms, levels, runs = d.time()
        assert runs == 3 and ms > 0.0 and all(v > 0.0 for v in levels[:3]) and not any(levels[3:])

        # other parameters, other guides: other results, each the reference's
        d.set_params(2, 0, 0.0, 0.5)
        d.run(acc)
        other, _ = d.read()
        assert not np.array_equal(bits(other), bits(lin))
        assert np.array_equal(bits(other), bits(dr.denoise(acc, nz, ids, 2, 0, 0.0, 0.5)[0]))
        ids2 = ids.copy()
        ids2[:, W // 2:] = NO
        d.set_guides(nz, ids2)
        d.run(acc)
        half, _ = d.read()
        assert not np.array_equal(bits(half), bits(other))
        assert np.array_equal(bits(half), bits(dr.denoise(acc, nz, ids2, 2, 0, 0.0, 0.5)[0]))


def test_frame_argument_checks(require_gpu):
    with PathTracer(32, 16) as pt, Rasterizer(W, H) as r, Denoiser(W, H) as d:
        with pytest.raises(iqpt.IqptError) as e:
            d.frame(pt, r)                                # a context of another size
        assert e.value.status == 1
        with pytest.raises(iqpt.IqptError) as e:
            d.read()
        assert e.value.status == 5                        # nothing was run
        with pytest.raises(iqpt.IqptError) as e:
            d.run(np.zeros((H, W, 4), np.float32))        # no guides yet
        assert e.value.status == 5
        with pytest.raises(iqpt.IqptError) as e:
            d.set_params(9, 0, 0.0, 0.0)
        assert e.value.status == 1
    with PathTracer(W, H, pixels=iqpt.pixel_set(W, H, y0=0, ystep=2)) as part, Rasterizer(W, H) as r, \
            PathTracer(W, H) as whole, Rasterizer(32, 16) as r_small, Denoiser(W, H) as d:
        with pytest.raises(iqpt.IqptError) as e:
            d.frame(part, r)                              # a context that owns every other row
        assert e.value.status == 1
        with pytest.raises(iqpt.IqptError) as e:
            d.frame(whole, r_small)                       # a rasterizer of another size
        assert e.value.status == 1
