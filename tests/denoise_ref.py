"""The denoiser's two definitions in numpy: the rasterizer's G-buffer and the edge-avoiding
à-trous filter. What the GPU must equal bit for bit.

float32 arrays throughout, every product, sum and division below one binary32 operation in the stated order;
the filter visits its 25 taps in a loop (dy outer, dx inner, ascending) and accumulates sequentially. The
G-buffer goes through raster_ref's set-up and edge functions on the doubled index list, by brute force over
every (piece, pixel).
"""
from __future__ import annotations

import numpy as np

import raster_ref as rr

F = np.float32
NO_PRIM = rr.NO_PRIM
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], dtype=np.float32)
MAX_LEVELS = 8
MAX_SQUARINGS = 7


# ------------------------------------------------------------------------------------------------ G-buffer
def doubled(indices):
    """Every triangle k = (i0, i1, i2) twice: (i0, i1, i2) at submission 2k, (i0, i2, i1) at 2k + 1."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 3)
    out = np.empty((2 * idx.shape[0], 3), np.int64)
    out[0::2] = idx
    out[1::2] = idx[:, [0, 2, 1]]
    return out.reshape(-1)


def gbuffer_clip(clip, normals, indices, width, height, draw_of_tri=None, budget=1 << 21):
    """(normal_z [H,W,4] float32, id [H,W] uint32) of clip-space triangles; draw_of_tri: the draw index of every
    triangle of `indices` (all 0 when None, as for draw_clip input)."""
    ntri = np.asarray(indices).size // 3
    draw_of_tri = np.zeros(ntri, np.int64) if draw_of_tri is None else np.asarray(draw_of_tri, np.int64)
    s = rr.setup(clip, normals, doubled(indices), width, height, 1)
    py, px = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    X = (px * 256 + 128).reshape(-1).astype(np.int64)
    Y = (py * 256 + 128).reshape(-1).astype(np.int64)
    N = X.size
    depth = np.full(N, F(1.0), np.float32)
    owner = np.full(N, -1, np.int64)
    P = len(s["tri"])
    step = max(1, budget // N)
    nz = np.zeros((N, 4), np.float32)
    ids = np.full(N, NO_PRIM, np.uint32)
    with np.errstate(all="ignore"):
        for c0 in range(0, P, step):
            sub = {k: v[c0:c0 + step] for k, v in s.items()}
            (e0, e1, e2), (t0, t1, t2) = rr._edges(sub, X, Y)
            cov = (((e0 > 0) | ((e0 == 0) & t0)) & ((e1 > 0) | ((e1 == 0) & t1)) & ((e2 > 0) | ((e2 == 0) & t2)))
            fa = sub["area"].astype(np.float32)[:, None]
            z0 = sub["z"][:, 0:1]
            z = (z0 + (e1.astype(np.float32) / fa) * (sub["z"][:, 1:2] - z0)) + \
                (e2.astype(np.float32) / fa) * (sub["z"][:, 2:3] - z0)
            z = np.where(cov, np.fmin(np.fmax(z, F(0)), F(1)), F(np.inf))
            first = np.argmin(z, axis=0)
            zmin = z[first, np.arange(N)]
            win = zmin < depth
            depth = np.where(win, zmin, depth).astype(np.float32)
            owner = np.where(win, c0 + first, owner)
        hit = np.nonzero(owner >= 0)[0]
        if hit.size:
            sub = {k: v[owner[hit]] for k, v in s.items()}
            x, y = sub["sx"], sub["sy"]
            ec = [(x[:, b] - x[:, a]) * (Y[hit] - y[:, a]) - (y[:, b] - y[:, a]) * (X[hit] - x[:, a])
                  for a, b in ((1, 2), (2, 0), (0, 1))]
            fa = sub["area"].astype(np.float32)
            p = [ec[k].astype(np.float32) / fa * sub["rw"][:, k] for k in range(3)]
            tot = (p[0] + p[1]) + p[2]
            wn = np.stack([((p[0] * sub["n"][:, 0, c] + p[1] * sub["n"][:, 1, c]) + p[2] * sub["n"][:, 2, c]) / tot
                           for c in range(3)], axis=1).astype(np.float32)
            # normalized3 (iq_host_math.hpp): zero below eps in every component, else a * (1 / sqrt(dot3(a, a)))
            small = np.all(np.abs(wn) < F(0.00001), axis=1)
            inv = F(1) / np.sqrt((wn[:, 0] * wn[:, 0] + wn[:, 1] * wn[:, 1]) + wn[:, 2] * wn[:, 2])
            nz[hit, :3] = np.where(small[:, None], F(0), wn * inv[:, None])
            ids[hit] = draw_of_tri[sub["tri"] >> 1].astype(np.uint32)
    nz[:, 3] = depth
    return nz.reshape(height, width, 4), ids.reshape(height, width)


def gbuffer_scene(draw_list, cam, width, height):
    """What Rasterizer.upload_scene + set_camera + gbuffer() must return."""
    view = np.array(cam.view, np.float32).reshape(4, 4)
    proj = np.array(cam.projection, np.float32).reshape(4, 4)
    clip, n, idx, _ = rr.scene_clip(draw_list, view, proj)
    draw_of_tri = [np.full(d["indices"].size // 3, k, np.int64) for k, d in enumerate(draw_list)
                   if d["indices"].size and d["vertices"].shape[0]]
    draw_of_tri = np.concatenate(draw_of_tri) if draw_of_tri else np.zeros(0, np.int64)
    return gbuffer_clip(clip, n, idx, width, height, draw_of_tri)


# ------------------------------------------------------------------------------------------------ filter
def _shift(a, dy, dx, fill):
    """a[y + dy, x + dx] where that lies in the frame, `fill` elsewhere."""
    out = np.full_like(a, fill)
    h, w = a.shape[:2]
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def level(c, normal_z, ids, i, normal_squarings, depth_sharpness, colour_sharpness, skip_tap=None):
    """c_{i+1} from c_i [H,W,4]. skip_tap: a frame position (y, x) treated as outside the frame when it is a
    non-centre tap (what test_denoise_ref.py's removed-tap property compares against)."""
    c = np.ascontiguousarray(c, dtype=np.float32)
    hgt, wid = ids.shape
    step = 1 << i
    s_z, s_c = F(depth_sharpness), F(colour_sharpness)
    k_i = F(s_c * s_c) * F(4.0 ** i)
    finite = np.all(np.isfinite(c[..., :3]), axis=2)
    inside = np.ones((hgt, wid), bool)
    if skip_tap is not None:
        inside[skip_tap] = False
    n_p, z_p = normal_z[..., :3], normal_z[..., 3]
    num = np.zeros((hgt, wid, 3), np.float32)
    den = np.zeros((hgt, wid), np.float32)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                hw = H5[dy + 2] * H5[dx + 2]
                if dy == 0 and dx == 0:
                    w = np.full((hgt, wid), hw, np.float32)
                    use = np.ones((hgt, wid), bool)
                    cq = c
                else:
                    oy, ox = dy * step, dx * step
                    cq = _shift(c, oy, ox, F(0))
                    nzq = _shift(normal_z, oy, ox, F(0))
                    use = _shift(inside, oy, ox, False) & (_shift(ids, oy, ox, NO_PRIM) == ids) & \
                        _shift(finite, oy, ox, False)
                    n_q, z_q = nzq[..., :3], nzq[..., 3]
                    d = np.fmax((n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2], F(0))
                    for _ in range(normal_squarings):
                        d = d * d
                    t = (z_p - z_q) * s_z
                    dl = c[..., :3] - cq[..., :3]
                    d2 = (dl[..., 0] * dl[..., 0] + dl[..., 1] * dl[..., 1]) + dl[..., 2] * dl[..., 2]
                    w = (hw * d) / ((F(1) + t * t) * (F(1) + d2 * k_i))
                    use &= w > 0                                           # a NaN weight fails
                num = np.where(use[..., None], num + w[..., None] * cq[..., :3], num)
                den = np.where(use, den + w, den)
        out = np.zeros_like(c)
        out[..., :3] = num / den[..., None]
    keep = (ids == NO_PRIM) | ~finite
    out.view(np.uint32)[keep] = c.view(np.uint32)[keep]
    return out


def encode_bgra(c):
    """The path tracer's frame encoding (oracle/iqpt_oracle.c to_u8): 255 sqrt(channel), NaN -> 0, saturate,
    truncate; B from z, G from y, R from x, alpha 255."""
    with np.errstate(all="ignore"):
        v = F(255) * np.sqrt(c[..., [2, 1, 0]].astype(np.float32))
    u = np.where(v > 0, np.minimum(v, F(255)), F(0)).astype(np.uint8)
    return np.concatenate([u, np.full(u.shape[:-1] + (1,), 255, np.uint8)], axis=-1)


def check_params(levels, normal_squarings, depth_sharpness, colour_sharpness):
    if not 0 <= levels <= MAX_LEVELS:
        raise ValueError("levels must be 0..8")
    if not 0 <= normal_squarings <= MAX_SQUARINGS:
        raise ValueError("normal_squarings must be 0..7")
    if not depth_sharpness >= 0 or not colour_sharpness >= 0:
        raise ValueError("sharpnesses must be >= 0")


def denoise(colour, normal_z, ids, levels, normal_squarings, depth_sharpness, colour_sharpness):
    """(float4 [H,W,4], bgra [H,W,4] uint8) of colour [H,W,4] (or [H*W,4]) under guides normal_z [H,W,4], ids [H,W]."""
    check_params(levels, normal_squarings, depth_sharpness, colour_sharpness)
    ids = np.asarray(ids, dtype=np.uint32)
    normal_z = np.ascontiguousarray(normal_z, dtype=np.float32).reshape(ids.shape + (4,))
    c = np.array(colour, dtype=np.float32).reshape(ids.shape + (4,))
    for i in range(levels):
        c = level(c, normal_z, ids, i, normal_squarings, depth_sharpness, colour_sharpness)
    return c, encode_bgra(c)
