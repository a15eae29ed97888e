"""Temporal reprojection in numpy: the history buffer that follows the camera. What the GPU must
equal bit for bit.

float32 arrays throughout, every product, sum and division below one binary32 operation in the stated order;
dot4 is raster_ref's row-vector product. A Temporal object holds the state of §11: the current view (camera,
guide planes, world positions, history) and the last resolved result.
"""
from __future__ import annotations

import numpy as np

import raster_ref as rr
from denoise_ref import encode_bgra

F = np.float32
NO_PRIM = rr.NO_PRIM
MAX_SAMPLES = 1 << 24          # n and max_history are clamped / limited to what a float counts exactly


def check_params(normal_min, plane_tolerance, max_history):
    if not np.isfinite(normal_min):
        raise ValueError("normal_min must be finite")
    if not plane_tolerance >= 0:
        raise ValueError("plane_tolerance must be >= 0")
    if not 1 <= max_history <= MAX_SAMPLES:
        raise ValueError("max_history must be 1..2^24")


def _mat(m):
    return np.array(m, dtype=np.float32).reshape(4, 4)


def _one(a):
    """[..., 3] -> [..., 4] with w = 1."""
    return np.concatenate([a, np.ones(a.shape[:-1] + (1,), np.float32)], axis=-1)


def positions(inv_proj, inv_view, depth):
    """Step 1: the world position [H,W,4] of every pixel centre at its D32 depth [H,W]."""
    h, w = depth.shape
    py, px = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    with np.errstate(all="ignore"):
        x = ((px + F(0.5)) * F(2)) / F(w) - F(1)
        y = F(1) - ((py + F(0.5)) * F(2)) / F(h)
        v = rr.dot4(np.stack([x, y, depth.astype(np.float32), np.ones_like(x)], axis=-1), _mat(inv_proj))
        rw = F(1) / v[..., 3:4]
        return rr.dot4(_one(v[..., :3] * rw), _mat(inv_view)).astype(np.float32)


def reproject(P, normal_z, ids, prev, normal_min, plane_tolerance, max_history, reasons=None):
    """Step 2: hist [H,W,4] of the new view's P, normal_z, ids from prev = (view, projection, P, normal_z, ids,
    out). reasons (a dict) receives the boolean plane of every condition, for the tests."""
    view, proj, P_prev, nz_prev, ids_prev, out = prev
    h, w = ids.shape
    with np.errstate(all="ignore"):
        c = rr.dot4(rr.dot4(_one(P[..., :3]), _mat(view)), _mat(proj))
        cw = c[..., 3]
        xs = ((c[..., 0] / cw + F(1)) * F(w)) * F(0.5)
        ys = ((F(1) - c[..., 1] / cw) * F(h)) * F(0.5)
        guided = ids != NO_PRIM
        inside = (cw > 0) & (xs >= 0) & (xs < F(w)) & (ys >= 0) & (ys < F(h))
        qx = np.where(inside, np.floor(xs), 0).astype(np.int64)
        qy = np.where(inside, np.floor(ys), 0).astype(np.int64)
        same_id = ids_prev[qy, qx] == ids
        n_p, n_q = normal_z[..., :3], nz_prev[qy, qx, :3]
        normal_ok = ((n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2]) >= F(normal_min)
        D = P_prev[qy, qx, :3] - P[..., :3]
        plane_ok = np.abs((n_p[..., 0] * D[..., 0] + n_p[..., 1] * D[..., 1]) + n_p[..., 2] * D[..., 2]) <= \
            F(plane_tolerance) * cw
        oq = out[qy, qx]
        hist_ok = (oq[..., 3] > 0) & np.all(np.isfinite(oq[..., :3]), axis=-1)
    valid = guided & inside & same_id & normal_ok & plane_ok & hist_ok
    if reasons is not None:
        reasons.update(guided=guided, inside=inside, same_id=same_id, normal_ok=normal_ok, plane_ok=plane_ok,
                       hist_ok=hist_ok, valid=valid, qx=qx, qy=qy, cw=cw, xs=xs, ys=ys)
    hist = np.zeros((h, w, 4), np.float32)
    hist[valid, :3] = oq[valid, :3]
    hist[valid, 3] = np.fmin(oq[valid, 3], F(max_history))
    return hist


def resolve(hist, colour, n):
    """out [H,W,4] of the history and a colour plane [H,W,4] of n samples (the table of §11)."""
    colour = np.ascontiguousarray(colour, dtype=np.float32).reshape(hist.shape)
    n = min(int(n), MAX_SAMPLES)
    nf = F(n)
    m = hist[..., 3]
    cf = np.all(np.isfinite(colour[..., :3]), axis=-1)
    out = np.zeros_like(hist)
    with np.errstate(all="ignore"):
        a = (m > 0) & cf & (n > 0)
        tot = m + nf
        blend = ((hist[..., :3] * m[..., None]) + (colour[..., :3] * nf)) / tot[..., None]
        out[a, :3] = blend[a]
        out[a, 3] = tot[a]
    b = (m > 0) & ~a
    out.view(np.uint32)[b] = hist.view(np.uint32)[b]
    if n > 0:
        cc = ~(m > 0)
        out.view(np.uint32)[cc, :3] = colour.view(np.uint32)[cc, :3]
        out[cc, 3] = np.where(cf[cc], nf, F(0))
    return out


class Temporal:
    """The temporal object of §11 for a W x H frame."""

    def __init__(self, width, height, normal_min, plane_tolerance, max_history):
        check_params(normal_min, plane_tolerance, max_history)
        self.width, self.height = width, height
        self.params = (float(normal_min), float(plane_tolerance), int(max_history))
        self.clear()

    def clear(self):
        self.view = None           # (view, projection, P, normal_z, ids)
        self.hist = None
        self.out = None
        self.reasons = {}

    def begin_view(self, cam, normal_z, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(self.height, self.width)
        normal_z = np.ascontiguousarray(normal_z, dtype=np.float32).reshape(self.height, self.width, 4)
        P = positions(cam.inv_proj, cam.inv_view, normal_z[..., 3])
        self.reasons = {}
        if self.view is None or self.out is None:
            self.hist = np.zeros((self.height, self.width, 4), np.float32)
        else:
            self.hist = reproject(P, normal_z, ids, self.view + (self.out,), *self.params, reasons=self.reasons)
        self.view = (_mat(cam.view), _mat(cam.projection), P, normal_z.copy(), ids.copy())
        self.out = None
        return self.hist

    def resolve(self, colour, n):
        if self.view is None:
            raise RuntimeError("resolve without a view")
        self.out = resolve(self.hist, colour, n)
        return self.out, encode_bgra(self.out)

    def stats(self):
        """(guided pixels, pixels with a valid history) of the last begin_view."""
        return int(np.sum(self.view[4] != NO_PRIM)), int(np.sum(self.hist[..., 3] > 0))
