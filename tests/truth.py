"""Geometric truth in numpy float64, for the tests only: what a camera sees of a Scene.draw_list(), computed without
any of the renderers' own steps. No snapping, no edge functions, no clip space: world-space triangles, a brute-force
two-sided Möller–Trumbore cast, and the camera as the float64 product view @ projection and its float64 inverse (the
camera's own float32 inverses are not used).

Conventions of include/iqpt.h: row vectors (v' = v @ M), screen position in pixels with (0, 0) the frame's top-left
corner, so that pixel (x, y) covers [x, x + 1) x [y, y + 1); x_ndc = 2 sx / W - 1, y_ndc = 1 - 2 sy / H; D3D depth z / w.
"""
from __future__ import annotations

import numpy as np


def _mat(m):
    return np.array(m, dtype=np.float64).reshape(4, 4)


def view_proj(cam):
    return _mat(cam.view) @ _mat(cam.projection)


def _normalised(v):
    with np.errstate(all="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------ triangles
def world_triangles(draw_list):
    """(pos [T,3,3], normal [T,3,3], draw [T]) of every triangle of a Scene.draw_list(): position @ transform, normal @
    inverse(transpose(3x3)) normalised (NaN under a singular transform), and the triangle's index in the draw list."""
    pos, nrm, draw = [np.zeros((0, 3, 3))], [np.zeros((0, 3, 3))], [np.zeros(0, np.int64)]
    for k, d in enumerate(draw_list):
        idx = np.asarray(d["indices"], np.int64).reshape(-1, 3)
        v = np.asarray(d["vertices"], np.float64).reshape(-1, 6)
        if idx.shape[0] == 0 or v.shape[0] == 0:
            continue
        M = np.asarray(d["transform"], np.float64).reshape(4, 4)
        p = (np.concatenate([v[:, :3], np.ones((v.shape[0], 1))], axis=1) @ M)[:, :3]
        try:
            n = _normalised(v[:, 3:6] @ np.linalg.inv(M[:3, :3].T))
        except np.linalg.LinAlgError:
            n = np.full((v.shape[0], 3), np.nan)
        pos.append(p[idx])
        nrm.append(n[idx])
        draw.append(np.full(idx.shape[0], k, np.int64))
    return np.concatenate(pos), np.concatenate(nrm), np.concatenate(draw)


def _nearest(pos, o, d, chunk):
    """(triangle [R] or -1, t [R] or inf, u [R], v [R]) of the nearest two-sided hit of every ray, by brute force."""
    R, T = o.shape[0], pos.shape[0]
    best_t = np.full(R, np.inf)
    best = np.full(R, -1, np.int64)
    best_u, best_v = np.zeros(R), np.zeros(R)
    if T == 0 or R == 0:
        return best, best_t, best_u, best_v
    v0, e1, e2 = pos[:, 0], pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    step = max(1, chunk // T)
    for r0 in range(0, R, step):
        oo, dd = o[r0:r0 + step, None, :], d[r0:r0 + step, None, :]
        with np.errstate(all="ignore"):
            pv = np.cross(dd, e2[None])
            det = np.sum(e1[None] * pv, axis=-1)
            tv = oo - v0[None]
            u = np.sum(tv * pv, axis=-1) / det
            qv = np.cross(tv, e1[None])
            v = np.sum(dd * qv, axis=-1) / det
            t = np.sum(e2[None] * qv, axis=-1) / det
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
        t = np.where(ok, t, np.inf)
        j = np.argmin(t, axis=1)
        rows = np.arange(t.shape[0])
        best_t[r0:r0 + step] = t[rows, j]
        best[r0:r0 + step] = np.where(np.isfinite(t[rows, j]), j, -1)
        best_u[r0:r0 + step] = u[rows, j]
        best_v[r0:r0 + step] = v[rows, j]
    return best, best_t, best_u, best_v


def cast(tris, o, d, apex=None, group=None, chunk=1 << 18):
    """The nearest two-sided hit of every ray (o [R,3], d [R,3], t > 0) with tris = world_triangles(...). Returns a
    dict: draw [R] (-1 on a miss), tri [R], t [R] (inf on a miss), bary [R,3] (weights of the three vertices), point
    [R,3], normal [R,3] (the interpolated vertex normals, normalised); NaN where the ray misses.

    Every (ray, triangle) pair is tested unless the rays are a camera's: with apex (the point every ray's line passes
    through, d pointing away from it) and group (an integer per ray, e.g. its screen tile), a group's rays are tested
    against the triangles whose bounding sphere reaches the group's cone of directions only. A point p of a sphere
    (c, r) is seen from the apex within asin(r / |c - apex|) of c, so the others cannot be hit."""
    pos, nrm, draw = tris
    o = np.asarray(o, np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    R, T = o.shape[0], pos.shape[0]
    if apex is None or group is None or T == 0:
        best, best_t, best_u, best_v = _nearest(pos, o, d, chunk)
    else:
        best, best_t = np.full(R, -1, np.int64), np.full(R, np.inf)
        best_u, best_v = np.zeros(R), np.zeros(R)
        apex = np.asarray(apex, np.float64)
        c = pos.mean(axis=1)
        r = np.linalg.norm(pos - c[:, None, :], axis=-1).max(axis=1)
        rel = c - apex
        dist = np.linalg.norm(rel, axis=-1)
        with np.errstate(all="ignore"):
            reach = np.where(dist > r, np.arcsin(np.minimum(r / dist, 1.0)), np.pi)
        group = np.asarray(group).reshape(-1)
        for g in np.unique(group):
            rays = np.flatnonzero(group == g)
            axis = _normalised(d[rays].sum(axis=0))
            width = np.arccos(np.clip(d[rays] @ axis, -1.0, 1.0)).max()
            with np.errstate(all="ignore"):
                off = np.arccos(np.clip(rel @ axis / dist, -1.0, 1.0))
            keep = np.flatnonzero(~(off > width + reach + 1e-9))              # (a NaN angle keeps the triangle)
            b, bt, bu, bv = _nearest(pos[keep], o[rays], d[rays], chunk)
            best[rays] = np.where(b >= 0, keep[np.maximum(b, 0)] if keep.size else -1, -1)
            best_t[rays], best_u[rays], best_v[rays] = bt, bu, bv
    hit = best >= 0
    bary = np.full((R, 3), np.nan)
    bary[hit] = np.stack([1 - best_u[hit] - best_v[hit], best_u[hit], best_v[hit]], axis=-1)
    point = np.full((R, 3), np.nan)
    normal = np.full((R, 3), np.nan)
    point[hit] = o[hit] + best_t[hit, None] * d[hit]
    normal[hit] = _normalised(np.sum(bary[hit][:, :, None] * nrm[best[hit]], axis=1))
    hit_draw = draw[np.maximum(best, 0)] if T else np.full(R, -1, np.int64)
    return {"draw": np.where(hit, hit_draw, -1), "tri": best, "t": best_t, "bary": bary, "point": point,
            "normal": normal}


# ------------------------------------------------------------------------------------------------ camera
def unproject_point(cam, sx, sy, depth):
    """The world point [..., 3] at screen position (sx, sy) in pixels and D3D depth `depth`, through the float64
    inverse of view @ projection."""
    sx, sy, depth = np.broadcast_arrays(np.asarray(sx, np.float64), np.asarray(sy, np.float64),
                                        np.asarray(depth, np.float64))
    ndc = np.stack([2 * sx / cam.width - 1, 1 - 2 * sy / cam.height, depth, np.ones_like(sx)], axis=-1)
    p = ndc @ np.linalg.inv(view_proj(cam))
    return p[..., :3] / p[..., 3:4]


def eye(cam):
    """The centre of projection: the world point every ray of unproject passes through (float64 inverse of view)."""
    return np.linalg.inv(_mat(cam.view))[3, :3]


def unproject(cam, sx, sy):
    """The ray (o [..., 3], d [..., 3] normalised) through screen position (sx, sy) in pixels: from the point at depth 0
    (the near plane) towards the point at depth 1."""
    near = unproject_point(cam, sx, sy, 0.0)
    far = unproject_point(cam, sx, sy, 1.0)
    return near, _normalised(far - near)


def project(cam, world):
    """(sx, sy, depth, w) of world points [..., 3]: screen position in pixels, D3D depth z / w and the clip-space w,
    through the float64 product view @ projection."""
    world = np.asarray(world, np.float64)
    p = np.concatenate([world[..., :3], np.ones(world.shape[:-1] + (1,))], axis=-1) @ view_proj(cam)
    with np.errstate(all="ignore"):
        w = p[..., 3]
        return (p[..., 0] / w + 1) * cam.width / 2, (1 - p[..., 1] / w) * cam.height / 2, p[..., 2] / w, w
