"""The rasterizer's pipeline in numpy: the reference the GPU frame must equal bit for bit.

float32 arrays with the stated operation order (every product and sum below is one binary32 operation, dot
products left to right), int64 edge functions evaluated by brute force over every (triangle, sample): no
tiles, no bins, no incremental edge stepping. Triangles are visited in submission order; the only shortcut is
the specified drop of triangles whose snapped bounding box holds no sample coordinate (``prefilter``), which
tests/test_raster_ref.py shows to change nothing.
"""
from __future__ import annotations

import numpy as np

F = np.float32
NO_PRIM = 0xFFFFFFFF
CLEAR_BGRA = np.array([255, 214, 158, 255], dtype=np.uint8)       # (0.62, 0.84, 1.0, 1) as B, G, R, A
MAX_CLIP_VERTS = 9
MAX_SCREEN = F(32768.0)
# offsets from the pixel centre in 1/256 pixel: D3D11's standard 4x pattern (-2,-6), (6,-2), (-6,2), (2,6) / 16
OFFSETS = {1: (np.array([0]), np.array([0])),
           4: (np.array([-32, 96, -96, 32]), np.array([-96, -32, 32, 96]))}


def _f(a):
    return np.asarray(a, dtype=np.float32)


def dot4(v, m):
    """Row vectors [..., 4] times a row-major 4x4: each component a left-to-right dot product over the column."""
    m = _f(m).reshape(4, 4)
    return ((v[..., 0:1] * m[0] + v[..., 1:2] * m[1]) + v[..., 2:3] * m[2]) + v[..., 3:4] * m[3]


def normal_matrix(model):
    """inversed(transposed(store3x3(model))) in iq_host_math.hpp's operation order; rows 0..2, columns 0..2."""
    a = _f(model).reshape(4, 4)[:3, :3]
    m = a.T.copy()
    with np.errstate(all="ignore"):
        det = (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
               + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))
        if np.abs(det) < F(0.00001):
            return np.diag([F(np.inf)] * 3).astype(np.float32)
        inv = np.zeros((3, 3), np.float32)
        inv[0, 0] = (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) / det
        inv[0, 1] = -(m[0, 1] * m[2, 2] - m[0, 2] * m[2, 1]) / det
        inv[0, 2] = (m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]) / det
        inv[1, 0] = -(m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) / det
        inv[1, 1] = (m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]) / det
        inv[1, 2] = -(m[0, 0] * m[1, 2] - m[0, 2] * m[1, 0]) / det
        inv[2, 0] = (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]) / det
        inv[2, 1] = -(m[0, 0] * m[2, 1] - m[0, 1] * m[2, 0]) / det
        inv[2, 2] = (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]) / det
    return inv


def vertex_stage(vertices, model, view, proj):
    """vertex_shader.hlsl: (clip [n,4], world normal [n,3]) of vertices [n,6] (pos, normal)."""
    v = _f(vertices).reshape(-1, 6)
    with np.errstate(all="ignore"):
        p = np.concatenate([v[:, :3], np.ones((v.shape[0], 1), np.float32)], axis=1)
        clip = dot4(dot4(dot4(p, model), view), proj)
        nm = normal_matrix(model)
        n = v[:, 3:6]
        t = ((n[:, 0:1] * nm[0] + n[:, 1:2] * nm[1]) + n[:, 2:3] * nm[2]) + F(0)
        eps = F(0.00001)
        small = np.all(np.abs(t) < eps, axis=1)
        inv = F(1) / np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
        wn = np.where(small[:, None], F(0), t * inv[:, None]).astype(np.float32)
    return clip.astype(np.float32), wn


def plane_dist(v):
    """[..., 6] distances to z >= 0, z <= w, x >= -4w, x <= 4w, y >= -4w, y <= 4w; inside is d >= 0."""
    x, y, z, w = v[..., 0], v[..., 1], v[..., 2], v[..., 3]
    w4 = F(4) * w
    return np.stack([z, w - z, x + w4, w4 - x, y + w4, w4 - y], axis=-1)


def clip_polygon(poly):
    """Sutherland-Hodgman over the six planes in order; poly [n,7] (clip xyzw, normal). New vertices are
    in + t (out - in) with t = d_in / (d_in - d_out), for the position and the normal alike."""
    poly = [p for p in _f(poly)]
    with np.errstate(all="ignore"):
        for plane in range(6):
            if not poly:
                break
            out = []
            n = len(poly)
            dist = plane_dist(np.array(poly, dtype=np.float32))[:, plane]
            for i in range(n):
                a, b = poly[i], poly[(i + 1) % n]
                da, db = dist[i], dist[(i + 1) % n]
                ia, ib = bool(da >= 0), bool(db >= 0)
                if ia:
                    if len(out) < MAX_CLIP_VERTS:
                        out.append(a)
                    if not ib and len(out) < MAX_CLIP_VERTS:
                        out.append(a + (da / (da - db)) * (b - a))
                elif ib:
                    if len(out) < MAX_CLIP_VERTS:
                        out.append(b + (db / (db - da)) * (a - b))
            poly = out
    return np.array(poly, dtype=np.float32).reshape(-1, 7)


def project(v, width, height):
    """Viewport and 16.8 snapping of vertices [..., 7]: (sx, sy int64, z_s, 1/w, ok)."""
    with np.errstate(all="ignore"):
        x, y, z, w = v[..., 0], v[..., 1], v[..., 2], v[..., 3]
        xs = ((x / w + F(1)) * F(width)) * F(0.5)
        ys = ((F(1) - y / w) * F(height)) * F(0.5)
        ok = (w > 0) & (np.abs(xs) <= MAX_SCREEN) & (np.abs(ys) <= MAX_SCREEN)
        sx = np.where(ok, np.rint(xs * F(256)), 0).astype(np.int64)
        sy = np.where(ok, np.rint(ys * F(256)), 0).astype(np.int64)
        zs = np.fmin(np.fmax(z / w, F(0)), F(1)).astype(np.float32)
        rw = (F(1) / w).astype(np.float32)
    return sx, sy, zs, rw, ok


def setup(clip, normals, indices, width, height, samples, prefilter=True, force_clip=False):
    """Clipping, snapping and culling: the surviving pieces in (submission index, piece) order, as a dict of
    arrays: sx, sy [P,3] int64, z, rw [P,3], n [P,3,3], tri [P], piece [P], area [P] int64."""
    clip = _f(clip).reshape(-1, 4)
    normals = _f(normals).reshape(-1, 3)
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 3)
    verts = np.concatenate([clip, normals], axis=1)[idx]                 # [T,3,7]
    with np.errstate(all="ignore"):
        need = ~np.all(plane_dist(verts) >= 0, axis=(1, 2)) if len(idx) else np.zeros(0, bool)
        # entirely outside one plane: dropped (the clipper would return nothing for it)
        gone = np.any(np.all(~(plane_dist(verts) >= 0), axis=1), axis=1) if len(idx) else np.zeros(0, bool)
    if force_clip:
        need = np.ones(len(idx), bool)
    need &= ~gone
    # triangles inside every plane: one piece
    plain = np.nonzero(~need & ~gone)[0]
    sx, sy, zs, rw, ok = project(verts[plain], width, height)
    keep = np.all(ok, axis=1)
    tri = [plain[keep]]
    piece = [np.zeros(int(keep.sum()), np.int64)]
    SX, SY, ZS, RW, NN = [sx[keep]], [sy[keep]], [zs[keep]], [rw[keep]], [verts[plain][keep][:, :, 4:7]]
    # the others through the clipper, fanned from the polygon's first vertex
    for t in np.nonzero(need)[0]:
        poly = clip_polygon(verts[t])
        if poly.shape[0] < 3:
            continue
        sx, sy, zs, rw, ok = project(poly, width, height)
        if not np.all(ok):
            continue
        for k in range(poly.shape[0] - 2):
            sel = [0, k + 1, k + 2]
            tri.append(np.array([t]))
            piece.append(np.array([k]))
            SX.append(sx[sel][None]); SY.append(sy[sel][None]); ZS.append(zs[sel][None]); RW.append(rw[sel][None])
            NN.append(poly[sel][None, :, 4:7])
    tri = np.concatenate(tri); piece = np.concatenate(piece)
    SX = np.concatenate(SX).reshape(-1, 3); SY = np.concatenate(SY).reshape(-1, 3)
    ZS = np.concatenate(ZS).reshape(-1, 3); RW = np.concatenate(RW).reshape(-1, 3)
    NN = np.concatenate(NN).reshape(-1, 3, 3)
    area = (SX[:, 1] - SX[:, 0]) * (SY[:, 2] - SY[:, 0]) - (SX[:, 2] - SX[:, 0]) * (SY[:, 1] - SY[:, 0])
    keep = area > 0                                                       # CULL_BACK, clockwise front, y down
    if prefilter:
        # a snapped bounding box with no sample coordinate inside: the sample coordinates are the lattice
        # 256 k + 128 (one sample) or 64 k + 32 (four), per axis, over the frame's pixels
        pitch, first = (256, 128) if samples == 1 else (64, 32)
        for c, size in ((SX, width), (SY, height)):
            lo = np.maximum(-((-(c.min(axis=1) - first)) // pitch), 0)           # ceil
            hi = np.minimum((c.max(axis=1) - first) // pitch, size * (256 // pitch) - 1)
            keep &= lo <= hi
    order = np.lexsort((piece[keep], tri[keep]))
    sel = np.nonzero(keep)[0][order]
    return {"sx": SX[sel], "sy": SY[sel], "z": ZS[sel], "rw": RW[sel], "n": NN[sel], "tri": tri[sel],
            "piece": piece[sel], "area": area[sel]}


def _edges(s, X, Y):
    """int64 edge functions [P,N] of pieces s at sample positions X, Y [N]; edge k is opposite vertex k."""
    x, y = s["sx"], s["sy"]
    out, tl = [], []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        dx = (x[:, b] - x[:, a])[:, None]
        dy = (y[:, b] - y[:, a])[:, None]
        out.append(dx * (Y[None, :] - y[:, a][:, None]) - dy * (X[None, :] - x[:, a][:, None]))
        tl.append((dy < 0) | ((dy == 0) & (dx > 0)))                    # left edge, or top edge
    return out, tl


def _unorm8(c):
    return (np.fmin(np.fmax(c, F(0)), F(1)) * F(255) + F(0.5)).astype(np.uint32)


def rasterize(s, width, height, samples, albedo=None, budget=1 << 21):
    """Coverage, depth, shading and resolve of set-up pieces: (bgra [H,W,4] uint8, depth [H,W,S] float32,
    prim [H,W,S] uint32)."""
    ox, oy = OFFSETS[samples]
    py, px, sm = np.meshgrid(np.arange(height), np.arange(width), np.arange(samples), indexing="ij")
    X = (px * 256 + 128 + ox[sm]).reshape(-1).astype(np.int64)
    Y = (py * 256 + 128 + oy[sm]).reshape(-1).astype(np.int64)
    CX = (px * 256 + 128).reshape(-1).astype(np.int64)
    CY = (py * 256 + 128).reshape(-1).astype(np.int64)
    N = X.size
    depth = np.full(N, F(1.0), np.float32)
    owner = np.full(N, -1, np.int64)
    P = len(s["tri"])
    step = max(1, budget // N)
    with np.errstate(all="ignore"):
        for c0 in range(0, P, step):
            sub = {k: v[c0:c0 + step] for k, v in s.items()}
            (e0, e1, e2), (t0, t1, t2) = _edges(sub, X, Y)
            cov = (((e0 > 0) | ((e0 == 0) & t0)) & ((e1 > 0) | ((e1 == 0) & t1)) & ((e2 > 0) | ((e2 == 0) & t2)))
            fa = sub["area"].astype(np.float32)[:, None]
            z0 = sub["z"][:, 0:1]
            dz1 = sub["z"][:, 1:2] - z0
            dz2 = sub["z"][:, 2:3] - z0
            z = (z0 + (e1.astype(np.float32) / fa) * dz1) + (e2.astype(np.float32) / fa) * dz2
            z = np.fmin(np.fmax(z, F(0)), F(1))
            z = np.where(cov, z, F(np.inf))
            first = np.argmin(z, axis=0)                                 # the earliest piece among equal depths
            zmin = z[first, np.arange(N)]
            win = zmin < depth                                            # LESS
            depth = np.where(win, zmin, depth).astype(np.float32)
            owner = np.where(win, c0 + first, owner)

        colour = np.tile(CLEAR_BGRA.astype(np.uint32), (N, 1))
        hit = np.nonzero(owner >= 0)[0]
        if hit.size:
            o = owner[hit]
            sub = {k: v[o] for k, v in s.items()}
            x, y = sub["sx"], sub["sy"]
            cx, cy = CX[hit], CY[hit]
            ec = []
            for a, b in ((1, 2), (2, 0), (0, 1)):
                ec.append((x[:, b] - x[:, a]) * (cy - y[:, a]) - (y[:, b] - y[:, a]) * (cx - x[:, a]))
            fa = sub["area"].astype(np.float32)
            p = [ec[k].astype(np.float32) / fa * sub["rw"][:, k] for k in range(3)]
            tot = (p[0] + p[1]) + p[2]
            wn = [((p[0] * sub["n"][:, 0, c] + p[1] * sub["n"][:, 1, c]) + p[2] * sub["n"][:, 2, c]) / tot
                  for c in range(3)]
            diffuse = np.fmax(((-wn[0]) * F(0) + (-wn[1]) * F(-1)) + (-wn[2]) * F(0), F(0))
            alb = (np.tile(_f([1, 0, 0]), (hit.size, 1)) if albedo is None else _f(albedo)[sub["tri"]])
            amb = [F(0.2) * F(0.62), F(0.2) * F(0.84), F(0.2) * F(1.0)]
            rgb = [(amb[c] + diffuse) * alb[:, c] for c in range(3)]
            colour[hit, 0] = _unorm8(rgb[2])
            colour[hit, 1] = _unorm8(rgb[1])
            colour[hit, 2] = _unorm8(rgb[0])
            colour[hit, 3] = 255
    colour = colour.reshape(height, width, samples, 4)
    if samples == 1:
        bgra = colour[:, :, 0, :]
    else:
        bgra = (colour.sum(axis=2) + 2) >> 2
    prim = np.where(owner >= 0, s["tri"][np.maximum(owner, 0)] if P else 0, NO_PRIM).astype(np.uint32)
    return (bgra.astype(np.uint8), depth.reshape(height, width, samples), prim.reshape(height, width, samples))


def render_clip(clip, normals, indices, width, height, samples, albedo=None, prefilter=True, force_clip=False):
    """The frame of clip-space triangles: what Rasterizer.draw_clip + read(samples=True) must return."""
    s = setup(clip, normals, indices, width, height, samples, prefilter=prefilter, force_clip=force_clip)
    return rasterize(s, width, height, samples, albedo=albedo)


def scene_clip(draw_list, view, proj):
    """The vertex stage over a Scene.draw_list(): (clip, normals, indices, per-triangle albedo)."""
    clips, norms, idxs, albs = [np.zeros((0, 4), np.float32)], [np.zeros((0, 3), np.float32)], [], []
    base = 0
    for d in draw_list:
        if d["indices"].size == 0 or d["vertices"].shape[0] == 0:
            continue
        c, n = vertex_stage(d["vertices"], d["transform"], view, proj)
        clips.append(c); norms.append(n)
        idxs.append(d["indices"].astype(np.int64) + base)
        albs.append(np.tile(_f(d["albedo"]), (d["indices"].size // 3, 1)))
        base += c.shape[0]
    idx = np.concatenate(idxs) if idxs else np.zeros(0, np.int64)
    alb = np.concatenate(albs) if albs else np.zeros((0, 3), np.float32)
    return np.concatenate(clips), np.concatenate(norms), idx, alb


def render_scene(draw_list, cam, width, height, samples):
    """What Rasterizer.upload_scene + set_camera + draw + read(samples=True) must return."""
    view = np.array(cam.view, np.float32).reshape(4, 4)
    proj = np.array(cam.projection, np.float32).reshape(4, 4)
    clip, n, idx, alb = scene_clip(draw_list, view, proj)
    return render_clip(clip, n, idx, width, height, samples, albedo=alb)
