"""Is the geometry true? The path tracer is proved against the oracle, the G-buffer against tests/denoise_ref.py and
the reprojection against tests/temporal_ref.py, each a restatement of the same sections of DESIGN.md; a sign, a
transpose or an offset shared by a kernel and its restatement passes all of those. Here the restatements (and the
oracle's camera) are held against tests/truth.py: float64 ray casting through the float64 view @ projection.

(a) the path tracer's camera rays land in their own pixel of the rasterizer's frame (with the aligned
    camera of iqpt_camera_align; with the plain camera they are half a pixel up and to the left);
(b) the G-buffer reference is what the camera sees at the pixel centre;
(c) §11 step 1 rebuilds the world point that was hit, and step 2 finds its pixel in a second view;
(d) §14's hi-to-lo position is where the hi pixel's ray crosses the lo frame;
and iqpt_camera_align is its normative float32 recipe, bit for bit. No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_ref as dr
import oracle
import temporal_ref as tr
import truth
import upscale_ref as ur
from iqpt import Scene, align_camera, make_camera
from test_cull import M32, state_with_outputs

F = np.float32
FP = C.POINTER(C.c_float)
UP = C.POINTER(C.c_uint32)

CAMERAS = {
    "default": {},
    "side": dict(position=[0.8, 1.0, -2.5, 0], forward=[-0.3, -0.4, 1, 0]),
    "wide": dict(fovh=70, znear=0.1, zfar=30, position=[-1.8, 2, 1.5, 0], forward=[0.6, -0.5, -0.7, 0]),   # (a) only
}
FRAMES = [(17, 13), (48, 27)]
RAY_FRAMES = FRAMES + [(1, 1), (300, 7)]
PRESETS = ["cornell", "app_default"]
OFFSETS = np.array([(0, 0), (-1, -1), (1, -1), (-1, 1), (1, 1)], np.float64) / 128   # twice the snapping step
WIDEN = 2.0 ** -22            # D32 rounding and the three float operations of §9.1 step 7
E_MAX = 1.0 / 16


def camera(name, w, h):
    return make_camera(w, h, **CAMERAS[name])


# ------------------------------------------------------------------------------------------------ align, bit for bit
def align_numpy(cam):
    """DESIGN.md §9.7 in numpy float32, one binary32 operation per product, sum and quotient."""
    P = np.array(cam.projection, np.float32).reshape(4, 4)
    IP = np.array(cam.inv_proj, np.float32).reshape(4, 4)
    sx, sy = F(1) / F(cam.width), F(1) / F(cam.height)
    with np.errstate(all="ignore"):
        ip, p = IP.copy(), P.copy()
        ip[3] = (IP[3] + sx * IP[0]) - sy * IP[1]
        p[:, 0] = P[:, 0] - P[:, 3] * sx
        p[:, 1] = P[:, 1] + P[:, 3] * sy
    return p, ip


@pytest.mark.parametrize("size", RAY_FRAMES + [(1920, 1080), (8192, 3)])
@pytest.mark.parametrize("name", list(CAMERAS))
def test_align_is_its_recipe(name, size):
    cam = camera(name, *size)
    al = align_camera(cam)
    p, ip = align_numpy(cam)
    assert np.array_equal(np.array(al.projection, np.float32).view(np.uint32), p.reshape(-1).view(np.uint32))
    assert np.array_equal(np.array(al.inv_proj, np.float32).view(np.uint32), ip.reshape(-1).view(np.uint32))
    for f in ("width", "height", "fovh"):
        assert getattr(al, f) == getattr(cam, f)
    for f in ("position", "forward", "view", "inv_view"):
        assert bytes(getattr(al, f)) == bytes(getattr(cam, f))
    # what the shift leaves in place (the constant w of cam_constants, the zero pattern of cam_axis_constants)
    assert ip[0, 3] == 0 and ip[1, 3] == 0 and ip[3, 0] != 0 and ip[3, 1] != 0
    assert np.array_equal(ip[:3], np.array(cam.inv_proj, np.float32).reshape(4, 4)[:3])
    # and the two shifted matrices are each other's inverse as far as float32 goes
    assert np.allclose(p.astype(np.float64) @ ip.astype(np.float64), np.eye(4), atol=1e-4)


# ------------------------------------------------------------------------------------------------ (a) camera rays
def jitter_of(r):
    """random::real(-0.5, 0.5) of the generator's output r (oracle rand_real)."""
    return (F(r) / F(4294967295.0)) * (F(0.5) - F(-0.5)) + F(-0.5)


def oracle_rays(cam, seed):
    """iqo_get_ray for every pixel with the four corner jitters, the zero jitter and one jitter drawn by a random
    state. Returns (o [N,3], d [N,3], x [N], y [N], jx [N], jy [N]) in float64."""
    lib = oracle.load()
    rng = np.random.default_rng(seed)
    half = 1 << 31                               # (float)2^31 / (float)(2^32 - 1) = 0.5: the zero jitter
    crafted = [state_with_outputs(a, b, rng) for a, b in ((0, 0), (M32, 0), (0, M32), (M32, M32), (half, half))]
    crafted = [(st, float(jitter_of(a)), float(jitter_of(b)))
               for st, (a, b) in zip(crafted, ((0, 0), (M32, 0), (0, M32), (M32, M32), (half, half)))]
    assert crafted[0][1] == -0.5 and crafted[3][2] == 0.5 and crafted[4][1] == 0.0
    out = []
    o, d = np.zeros(4, np.float32), np.zeros(4, np.float32)
    for y in range(cam.height):
        for x in range(cam.width):
            st = rng.integers(1, 1 << 32, 6, dtype=np.uint64).astype(np.uint32)
            chk = st.copy()
            r1 = lib.iqo_xorwow_next(chk.ctypes.data_as(UP))
            r2 = lib.iqo_xorwow_next(chk.ctypes.data_as(UP))
            for s0, jx, jy in crafted + [(st, float(jitter_of(r1)), float(jitter_of(r2)))]:
                s = s0.copy()
                lib.iqo_get_ray(C.byref(cam), x, y, s.ctypes.data_as(UP), o.ctypes.data_as(FP), d.ctypes.data_as(FP))
                out.append((*o[:3], *d[:3], x, y, jx, jy))
    a = np.array(out, np.float64)
    return a[:, 0:3], a[:, 3:6], a[:, 6], a[:, 7], a[:, 8], a[:, 9]


def ray_error(pt_cam, raster_cam, centre, seed=11):
    """The largest distance, in pixels of raster_cam's frame and in either axis, of the points o + s d (s = 0, 3, 50) of
    pt_cam's oracle rays from (x + centre + jx, y + centre + jy)."""
    o, d, x, y, jx, jy = oracle_rays(pt_cam, seed)
    worst = 0.0
    for s in (0.0, 3.0, 50.0):
        sx, sy, _, w = truth.project(raster_cam, o + s * d)
        assert np.all(w > 0)
        worst = max(worst, float(np.max(np.abs(sx - (x + centre + jx)))), float(np.max(np.abs(sy - (y + centre + jy)))))
    return worst


@functools.lru_cache(maxsize=None)
def float32_ray_error(name, w, h):
    """E of (a): twice the error of the plain camera's float32 ray chain against float64, measured against the
    oracle alone (its sample square is centred on the pixel's corner); twice for the one more rounding in each of the
    shifted matrices' entries."""
    cam = camera(name, w, h)
    return 2.0 * ray_error(cam, cam, 0.0)


@pytest.mark.parametrize("size", RAY_FRAMES)
@pytest.mark.parametrize("name", list(CAMERAS))
def test_camera_rays_land_in_their_own_pixel(name, size):
    cam = camera(name, *size)
    E = float32_ray_error(name, *size)
    got = ray_error(align_camera(cam), cam, 0.5)
    print(f"{name} {size[0]}x{size[1]}: E = {E:.3e} px, aligned camera {got:.3e} px")
    assert E < E_MAX
    assert got <= E


@pytest.mark.parametrize("name", list(CAMERAS))
def test_the_plain_pairing_is_half_a_pixel_off(name):
    """The same measurement with one camera struct for both renderers (every pairing before iqpt_camera_align): the
    path tracer's samples are centred half a pixel up and to the left of the rasterizer's pixel centre."""
    cam = camera(name, 17, 13)
    E = float32_ray_error(name, 17, 13)
    got = ray_error(cam, cam, 0.5)
    assert 0.5 - E <= got <= 0.5 + E and got > E


# ------------------------------------------------------------------------------------------------ (b) the G-buffer
@functools.lru_cache(maxsize=None)
def seen(preset, name, w, h):
    """The reference G-buffer of a case and the float64 casts through every pixel's centre and the four points
    (+-1/128, +-1/128) px around it."""
    sc = Scene()
    sc.add_preset(preset)
    dl = sc.draw_list()
    cam = camera(name, w, h)
    nz, ids = dr.gbuffer_scene(dl, cam, w, h)
    tris = truth.world_triangles(dl)
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    sx = px[..., None] + 0.5 + OFFSETS[:, 0]                  # [h, w, 5]
    sy = py[..., None] + 0.5 + OFFSETS[:, 1]
    o, d = truth.unproject(cam, sx, sy)
    tile = np.broadcast_to(((py // 4) * w + px // 4)[..., None], sx.shape)       # 4 x 4 pixels share a cone
    c = truth.cast(tris, o.reshape(-1, 3), d.reshape(-1, 3), apex=truth.eye(cam), group=tile.reshape(-1))
    if preset == "cornell" and w * h <= 17 * 13:          # the culled cast is the brute-force one
        full = truth.cast(tris, o.reshape(-1, 3), d.reshape(-1, 3))
        assert np.array_equal(full["tri"], c["tri"]) and np.array_equal(full["t"], c["t"])
    draw = c["draw"].reshape(h, w, 5)
    point = c["point"].reshape(h, w, 5, 3)
    normal = c["normal"].reshape(h, w, 5, 3)
    depth = truth.project(cam, point)[2]
    decided = np.all(draw == draw[..., :1], axis=-1)
    return dict(cam=cam, nz=nz, ids=ids, sx=sx, sy=sy, draw=draw, point=point, normal=normal, depth=depth,
                decided=decided, hit=decided & (draw[..., 0] >= 0), ndraws=len(dl))


CASES = [(p, n, w, h) for p in PRESETS for n in ("default", "side") for (w, h) in FRAMES]


@pytest.mark.parametrize("preset,name,w,h", CASES)
def test_gbuffer_reference_is_what_the_camera_sees(preset, name, w, h):
    s = seen(preset, name, w, h)
    undecided = 1.0 - float(np.mean(s["decided"]))
    print(f"{preset} {name} {w}x{h}: undecided {100 * undecided:.2f} %, hit {100 * np.mean(s['hit']):.1f} %")
    assert undecided <= 0.02
    dec, hit = s["decided"], s["hit"]
    want = np.where(s["draw"][..., 0] >= 0, s["draw"][..., 0], dr.NO_PRIM).astype(np.uint32)
    assert np.array_equal(s["ids"][dec], want[dec])
    assert hit.sum() > w * h // 4 and len(np.unique(want[hit])) > 2
    # depth within the five float64 depths, widened
    z = s["nz"][..., 3].astype(np.float64)
    lo, hi = s["depth"].min(axis=-1), s["depth"].max(axis=-1)
    assert np.all(s["depth"][hit] < 1.0) and np.all(s["depth"][hit] > 0.0)
    over = np.maximum(lo[hit] - z[hit], z[hit] - hi[hit])
    print(f"  depth beyond the five: {over.max():.3e}")
    assert np.all(over <= WIDEN)
    assert np.all(z[dec & ~hit] == 1.0)
    # the normal within the spread of the five float64 normals, plus 1e-5, of the nearest of them
    n5 = s["normal"][hit]                                                           # [n, 5, 3]
    spread = np.linalg.norm(n5[:, :, None, :] - n5[:, None, :, :], axis=-1).max(axis=(1, 2))
    dist = np.linalg.norm(n5 - s["nz"][..., :3].astype(np.float64)[hit][:, None, :], axis=-1).min(axis=1)
    print(f"  normal beyond the spread: {(dist - spread).max():.3e}")
    assert np.all(dist <= spread + 1e-5)
    assert np.all(s["nz"][..., :3][dec & ~hit] == 0)


# ------------------------------------------------------------------------------------------------ (c) §11
def position_bound(s):
    """Per pixel [h, w], in float64 alone: how far §11 step 1's point may lie from the centre's hit point. By (b) the
    reference depth lies within the five float64 depths widened by 2^-22, so the float64 unprojection of (centre,
    reference depth) lies on the centre's ray between the points at the extreme depths; the bound is the largest
    distance from the centre's hit point to the points unprojected at each of the five depths +- the widening, at the
    centre and at that depth's own screen offset, plus 2^-20 of the distance from the camera for the two float32
    matrix products."""
    cam = s["cam"]
    centre = s["point"][..., 0, :]
    far = np.zeros(centre.shape[:-1])
    for sign in (-1.0, 1.0):
        dz = s["depth"] + sign * WIDEN                                   # [h, w, 5]
        for sx, sy in ((s["sx"], s["sy"]), (s["sx"][..., :1], s["sy"][..., :1])):
            q = truth.unproject_point(cam, sx, sy, dz)
            far = np.maximum(far, np.linalg.norm(q - centre[..., None, :], axis=-1).max(axis=-1))
    return far + 2.0 ** -20 * np.linalg.norm(centre - truth.eye(cam), axis=-1)


@pytest.mark.parametrize("preset,name,w,h", CASES)
def test_step_1_rebuilds_the_hit_point(preset, name, w, h):
    s = seen(preset, name, w, h)
    cam, hit = s["cam"], s["hit"]
    P = tr.positions(cam.inv_proj, cam.inv_view, s["nz"][..., 3])[..., :3].astype(np.float64)
    err = np.linalg.norm(P - s["point"][..., 0, :], axis=-1)
    bound = position_bound(s)
    rel = err[hit] / np.linalg.norm(s["point"][..., 0, :][hit] - truth.eye(cam), axis=-1)
    print(f"{preset} {name} {w}x{h}: worst error / distance {rel.max():.3e}, worst error / bound "
          f"{(err[hit] / bound[hit]).max():.3f}")
    assert np.all(err[hit] <= bound[hit])


@pytest.mark.parametrize("preset,w,h", [(p, w, h) for p in PRESETS for (w, h) in FRAMES])
@pytest.mark.parametrize("new,old", [("default", "side"), ("side", "default")])
def test_step_2_finds_the_pixel_in_the_other_view(preset, w, h, new, old):
    a, b = seen(preset, new, w, h), seen(preset, old, w, h)
    t = tr.Temporal(w, h, 0.9, 0.01, 64)
    t.begin_view(b["cam"], b["nz"], b["ids"])
    t.resolve(np.ones((h, w, 4), np.float32), 1)
    t.begin_view(a["cam"], a["nz"], a["ids"])
    r = t.reasons
    sx, sy, _, cw = truth.project(b["cam"], a["point"][..., 0, :])
    with np.errstate(all="ignore"):
        clear = (np.abs(sx - np.round(sx)) > 1 / 64) & (np.abs(sy - np.round(sy)) > 1 / 64)
        inside = (cw > 0) & (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    m = a["hit"] & clear
    assert np.array_equal(r["inside"][m], inside[m])
    m &= inside
    print(f"{preset} {new} -> {old} {w}x{h}: {int(m.sum())} of {int(a['hit'].sum())} hit pixels compared")
    assert m.sum() > a["hit"].sum() // 4
    assert np.array_equal(r["qx"][m], np.floor(sx[m]).astype(np.int64))
    assert np.array_equal(r["qy"][m], np.floor(sy[m]).astype(np.int64))


# ------------------------------------------------------------------------------------------------ (d) §14
def zero_jitter_rays(cam):
    lib = oracle.load()
    st0 = state_with_outputs(1 << 31, 1 << 31, np.random.default_rng(5))
    o, d = np.zeros(4, np.float32), np.zeros(4, np.float32)
    out = np.zeros((cam.height, cam.width, 6))
    for y in range(cam.height):
        for x in range(cam.width):
            s = st0.copy()
            lib.iqo_get_ray(C.byref(cam), x, y, s.ctypes.data_as(UP), o.ctypes.data_as(FP), d.ctypes.data_as(FP))
            out[y, x, :3], out[y, x, 3:] = o[:3], d[:3]
    return out[..., :3], out[..., 3:]


@pytest.mark.parametrize("lo", [(8, 5), (16, 9)])
@pytest.mark.parametrize("f", ur.FACTORS)
@pytest.mark.parametrize("name", ["default", "side"])
def test_upsampler_positions(name, f, lo):
    """The ray of hi pixel (X, Y) of the aligned hi camera, at zero jitter, crosses the lo frame at (x0 + fx + 1/2,
    y0 + fy + 1/2): where §14 places it among the lo pixels' centres, which the aligned lo camera's zero-jitter rays
    pass through. Tolerances: E of (a) for each frame, in its own pixels (a lo pixel is f hi pixels)."""
    w, h = lo
    W, H = f * w, f * h
    cam_lo, cam_hi = camera(name, w, h), camera(name, W, H)
    assert bytes(cam_lo.view) == bytes(cam_hi.view) and bytes(cam_lo.projection) == bytes(cam_hi.projection)
    E_lo, E_hi = float32_ray_error(name, w, h), float32_ray_error(name, W, H)
    assert E_lo < E_MAX and E_hi < E_MAX
    x0, fx = ur.position(W, f)
    y0, fy = ur.position(H, f)
    want_x = (x0 + fx.astype(np.float64) + 0.5)[None, :]
    want_y = (y0 + fy.astype(np.float64) + 0.5)[:, None]
    o, d = zero_jitter_rays(align_camera(cam_hi))
    worst = 0.0
    for s in (0.0, 3.0, 50.0):
        sx, sy, _, _ = truth.project(cam_lo, o + s * d)
        worst = max(worst, float(np.abs(sx - want_x).max()), float(np.abs(sy - want_y).max()))
    print(f"{name} f = {f} lo {w}x{h}: hi rays {worst:.3e} lo px (E_hi / f = {E_hi / f:.3e})")
    assert worst <= E_hi / f
    o, d = zero_jitter_rays(align_camera(cam_lo))
    py, px = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    for s in (0.0, 3.0, 50.0):
        sx, sy, _, _ = truth.project(cam_lo, o + s * d)
        assert max(float(np.abs(sx - px).max()), float(np.abs(sy - py).max())) <= E_lo
