"""Variance-guided filtering in numpy: two temporal histories (colour and luminance moments), the
per-pixel variance estimate and the à-trous filter whose colour weight that variance normalises. What the GPU must
equal bit for bit.

float32 arrays throughout, every product, sum and division below one binary32 operation in the stated order; the
windows are visited in a loop (dy outer, dx inner, ascending) and accumulate sequentially. The two histories are
temporal_ref.Temporal objects, composed, not restated.
"""
from __future__ import annotations

import numpy as np

import denoise_ref as dr
import temporal_ref as tr
from denoise_ref import H5, _shift, encode_bgra

F = np.float32
NO_PRIM = tr.NO_PRIM
MAX_SAMPLES = tr.MAX_SAMPLES
MAX_LEVELS = dr.MAX_LEVELS
MAX_SQUARINGS = dr.MAX_SQUARINGS
LUMA = np.array([0.2126, 0.7152, 0.0722], dtype=np.float32)
G3 = np.array([1 / 4, 1 / 2, 1 / 4], dtype=np.float32)
RADIUS = 3                      # the spatial estimate's window is 7 x 7


def check_params(normal_min, plane_tolerance, max_history, min_history, levels, normal_squarings, depth_sharpness,
                 colour_sigma, variance_floor):
    tr.check_params(normal_min, plane_tolerance, max_history)
    if not 1 <= min_history <= MAX_SAMPLES:
        raise ValueError("min_history must be 1..2^24")
    if not 0 <= levels <= MAX_LEVELS:
        raise ValueError("levels must be 0..8")
    if not 0 <= normal_squarings <= MAX_SQUARINGS:
        raise ValueError("normal_squarings must be 0..7")
    if not (np.isfinite(depth_sharpness) and depth_sharpness >= 0):
        raise ValueError("depth_sharpness must be finite and >= 0")
    if not (np.isfinite(colour_sigma) and colour_sigma >= 0):
        raise ValueError("colour_sigma must be finite and >= 0")
    if not (np.isfinite(variance_floor) and variance_floor > 0):
        raise ValueError("variance_floor must be finite and > 0")


def luminance(c):
    with np.errstate(all="ignore"):
        return ((LUMA[0] * c[..., 0] + LUMA[1] * c[..., 1]) + LUMA[2] * c[..., 2]).astype(np.float32)


def moments(colour):
    """M = (L, L L, +0, +0) of a colour plane [H,W,4]."""
    m = np.zeros(colour.shape, np.float32)
    lum = luminance(colour)
    with np.errstate(all="ignore"):
        m[..., 0] = lum
        m[..., 1] = lum * lum
    return m


def _pos(a):
    """a where a > 0, else +0 (a NaN, a negative value and -0 all give +0)."""
    return np.where(a > 0, a, F(0)).astype(np.float32)


def _pos_finite(a):
    """_pos, and +inf gives +0 as well."""
    return np.where((a > 0) & (a < F(np.inf)), a, F(0)).astype(np.float32)


def variance(o, mu, ids, n, min_history, skip_tap=None):
    """(c0 [H,W,4], spatial [H,W] bool) of the two resolved planes: c0 = (o.xyz, v)."""
    hgt, wid = ids.shape
    ne = np.fmax(F(min(int(n), MAX_SAMPLES)), F(1))
    finite = np.all(np.isfinite(o[..., :3]), axis=2)
    live = (ids != NO_PRIM) & finite
    inside = np.ones((hgt, wid), bool)
    if skip_tap is not None:
        inside[skip_tap] = False
    lum = luminance(o)
    with np.errstate(all="ignore"):
        temporal = live & (mu[..., 3] >= F(min_history) * ne) & np.isfinite(mu[..., 0]) & np.isfinite(mu[..., 1])
        vt = _pos(mu[..., 1] - mu[..., 0] * mu[..., 0]) * (ne / o[..., 3])
        s1 = np.zeros((hgt, wid), np.float32)
        s2 = np.zeros((hgt, wid), np.float32)
        k = np.zeros((hgt, wid), np.int64)
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                if dy == 0 and dx == 0:
                    use = np.ones((hgt, wid), bool)
                    lq = lum
                else:
                    use = _shift(inside, dy, dx, False) & (_shift(ids, dy, dx, NO_PRIM) == ids) & \
                        _shift(finite, dy, dx, False)
                    lq = _shift(lum, dy, dx, F(0))
                s1 = np.where(use, s1 + lq, s1)
                s2 = np.where(use, s2 + lq * lq, s2)
                k += use
        kf = k.astype(np.float32)
        m1 = s1 / kf
        vs = s2 / kf - m1 * m1
        v = _pos_finite(np.where(temporal, vt, vs))
    c0 = np.array(o, dtype=np.float32)
    c0[..., 3] = np.where(live, v, F(0))
    return c0, live & ~temporal


def level(c, normal_z, ids, i, normal_squarings, depth_sharpness, colour_sigma, variance_floor, skip_tap=None):
    """c_{i+1} from c_i [H,W,4] (w: the variance). skip_tap: a frame position (y, x) treated as outside the frame
    when it is a non-centre tap."""
    c = np.ascontiguousarray(c, dtype=np.float32)
    hgt, wid = ids.shape
    step = 1 << i
    s_z, sigma, eps = F(depth_sharpness), F(colour_sigma), F(variance_floor)
    finite = np.all(np.isfinite(c[..., :3]), axis=2)
    inside = np.ones((hgt, wid), bool)
    if skip_tap is not None:
        inside[skip_tap] = False
    n_p, z_p = normal_z[..., :3], normal_z[..., 3]
    var = c[..., 3]
    with np.errstate(all="ignore"):
        vsum = np.zeros((hgt, wid), np.float32)
        gsum = np.zeros((hgt, wid), np.float32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                gw = G3[dy + 1] * G3[dx + 1]
                if dy == 0 and dx == 0:
                    use = np.ones((hgt, wid), bool)
                    vq = var
                else:
                    use = _shift(inside, dy, dx, False) & (_shift(ids, dy, dx, NO_PRIM) == ids) & \
                        _shift(finite, dy, dx, False)
                    vq = _shift(var, dy, dx, F(0))
                vsum = np.where(use, vsum + gw * vq, vsum)
                gsum = np.where(use, gsum + gw, gsum)
        vb = vsum / gsum
        r = F(1) / (F(sigma * sigma) * vb + eps)
        num = np.zeros((hgt, wid, 3), np.float32)
        den = np.zeros((hgt, wid), np.float32)
        vnum = np.zeros((hgt, wid), np.float32)
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
                    w = (hw * d) / ((F(1) + t * t) * (F(1) + d2 * r))
                    use &= w > 0                                           # a NaN weight fails
                num = np.where(use[..., None], num + w[..., None] * cq[..., :3], num)
                den = np.where(use, den + w, den)
                vnum = np.where(use, vnum + (w * w) * cq[..., 3], vnum)
        out = np.zeros_like(c)
        out[..., :3] = num / den[..., None]
        out[..., 3] = _pos_finite(vnum / (den * den))
    keep = (ids == NO_PRIM) | ~finite
    out.view(np.uint32)[keep] = c.view(np.uint32)[keep]
    return out


class Svgf:
    """The object of §12 for a W x H frame. After resolve(): temporal_out (the colour history's result), c0,
    stages (c_0 ... c_L) and spatial (the pixels that took the spatial estimate)."""

    def __init__(self, width, height, normal_min, plane_tolerance, max_history, min_history, levels, normal_squarings,
                 depth_sharpness, colour_sigma, variance_floor):
        check_params(normal_min, plane_tolerance, max_history, min_history, levels, normal_squarings, depth_sharpness,
                     colour_sigma, variance_floor)
        self.width, self.height = width, height
        self.colour = tr.Temporal(width, height, normal_min, plane_tolerance, max_history)
        self.moments = tr.Temporal(width, height, normal_min, plane_tolerance, max_history)
        self.min_history = int(min_history)
        self.filter = (int(levels), int(normal_squarings), float(depth_sharpness), float(colour_sigma),
                       float(variance_floor))
        self.clear()

    def clear(self):
        self.colour.clear()
        self.moments.clear()
        self.guides = None
        self.temporal_out = self.mu = self.c0 = self.spatial = None
        self.stages = []

    def begin_view(self, cam, normal_z, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(self.height, self.width)
        normal_z = np.ascontiguousarray(normal_z, dtype=np.float32).reshape(self.height, self.width, 4)
        self.colour.begin_view(cam, normal_z, ids)
        self.moments.begin_view(cam, normal_z, ids)
        self.guides = (normal_z.copy(), ids.copy())
        self.temporal_out = self.mu = self.c0 = self.spatial = None
        self.stages = []

    def resolve(self, colour, n, skip_tap=None):
        """(float4 [H,W,4] with w = the filtered variance, bgra [H,W,4] uint8)."""
        if self.guides is None:
            raise RuntimeError("resolve without a view")
        colour = np.ascontiguousarray(colour, dtype=np.float32).reshape(self.height, self.width, 4)
        normal_z, ids = self.guides
        self.temporal_out, _ = self.colour.resolve(colour, n)
        self.mu, _ = self.moments.resolve(moments(colour), n)
        self.c0, self.spatial = variance(self.temporal_out, self.mu, ids, n, self.min_history, skip_tap)
        levels, q, s_z, sigma, eps = self.filter
        c = self.c0
        self.stages = [c]
        for i in range(levels):
            c = level(c, normal_z, ids, i, q, s_z, sigma, eps, skip_tap)
            self.stages.append(c)
        return c, encode_bgra(c)

    def stats(self):
        """(guided pixels, pixels with a valid history, pixels that took the spatial estimate at the last resolve)."""
        guided, valid = self.colour.stats()
        return guided, valid, 0 if self.spatial is None else int(self.spatial.sum())
