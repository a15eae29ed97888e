"""Guided upsampling in numpy: what the GPU must equal bit for bit.

float32 arrays throughout, every product, sum and division below one binary32 operation in the stated order; each
stage visits its taps in a loop (b outer, a inner, ascending) and accumulates sequentially from +0.
"""
from __future__ import annotations

import numpy as np

from denoise_ref import NO_PRIM, encode_bgra

F = np.float32
FACTORS = (2, 3, 4)
MAX_DIM = 8192
MAX_SQUARINGS = 7


def check_args(width, height, factor, normal_squarings=0, depth_sharpness=0.0):
    if factor not in FACTORS:
        raise ValueError("factor must be 2, 3 or 4")
    if not (1 <= width <= MAX_DIM and 1 <= height <= MAX_DIM):
        raise ValueError("frame size must be 1..8192 in each dimension")
    if width % factor or height % factor:
        raise ValueError("width and height must be multiples of factor")
    if not 0 <= normal_squarings <= MAX_SQUARINGS:
        raise ValueError("normal_squarings must be 0..7")
    if not depth_sharpness >= 0:
        raise ValueError("depth_sharpness must be >= 0")


def position(n_hi, f):
    """(x0 [n_hi] int64, fx [n_hi] float32) of the hi coordinates 0 .. n_hi - 1: u = 2 X + 1 - f, x0 = floor(u / 2f),
    fx = (u - 2f x0) / 2f."""
    u = 2 * np.arange(n_hi, dtype=np.int64) + 1 - f
    x0 = u // (2 * f)                                    # floor division: -1 where u < 0
    fx = (u - 2 * f * x0).astype(np.float32) / F(2 * f)
    return x0, fx


def _stage(c, nz_lo, id_lo, finite, nz_hi, id_hi, X0, Y0, taps, q, s_z):
    """(num [H,W,3], den [H,W]) of the taps (a, b, g [H,W]) in their order."""
    h, w = id_lo.shape
    H, W = id_hi.shape
    sky = id_hi == NO_PRIM
    n_p, z_p = nz_hi[..., :3], nz_hi[..., 3]
    num = np.zeros((H, W, 3), np.float32)
    den = np.zeros((H, W), np.float32)
    for a, b, g in taps:
        qx, qy = X0 + a, Y0 + b
        inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
        cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
        cq, nzq = c[cy, cx], nz_lo[cy, cx]
        use = inside & (id_lo[cy, cx] == id_hi) & finite[cy, cx]
        n_q, z_q = nzq[..., :3], nzq[..., 3]
        d = np.fmax((n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2], F(0))
        for _ in range(q):
            d = d * d
        t = (z_p - z_q) * s_z
        wgt = np.where(sky, g, (g * d) / (F(1) + t * t)).astype(np.float32)
        use &= wgt > 0                                   # a NaN weight fails
        num = np.where(use[..., None], num + wgt[..., None] * cq[..., :3], num)
        den = np.where(use, den + wgt, den)
    return num, den


def upscale(colour_lo, nz_lo, id_lo, nz_hi, id_hi, factor, normal_squarings, depth_sharpness):
    """(float4 [H,W,4] with w = the class, bgra [H,W,4] uint8, (guided, widened, unguided)) of colour_lo [h,w,4] (or
    [h*w,4]) under the guides nz_lo [h,w,4], id_lo [h,w], nz_hi [H,W,4], id_hi [H,W]."""
    id_lo = np.asarray(id_lo, dtype=np.uint32)
    id_hi = np.asarray(id_hi, dtype=np.uint32)
    h, w = id_lo.shape
    H, W = id_hi.shape
    f = int(factor)
    check_args(W, H, f, normal_squarings, depth_sharpness)
    if W != f * w or H != f * h:
        raise ValueError("the hi frame must be factor times the lo frame")
    nz_lo = np.ascontiguousarray(nz_lo, dtype=np.float32).reshape(h, w, 4)
    nz_hi = np.ascontiguousarray(nz_hi, dtype=np.float32).reshape(H, W, 4)
    c = np.ascontiguousarray(colour_lo, dtype=np.float32).reshape(h, w, 4)
    s_z = F(depth_sharpness)
    finite = np.all(np.isfinite(c[..., :3]), axis=2)
    x0, fx = position(W, f)
    y0, fy = position(H, f)
    X0, Y0 = np.broadcast_to(x0[None, :], (H, W)), np.broadcast_to(y0[:, None], (H, W))
    FX, FY = np.broadcast_to(fx[None, :], (H, W)), np.broadcast_to(fy[:, None], (H, W))
    one = np.ones((H, W), np.float32)
    with np.errstate(all="ignore"):
        taps_a = [(a, b, (FY if b else F(1) - FY) * (FX if a else F(1) - FX)) for b in (0, 1) for a in (0, 1)]
        num_a, den_a = _stage(c, nz_lo, id_lo, finite, nz_hi, id_hi, X0, Y0, taps_a, normal_squarings, s_z)
        taps_b = [(a, b, one) for b in (-1, 0, 1, 2) for a in (-1, 0, 1, 2)]
        num_b, den_b = _stage(c, nz_lo, id_lo, finite, nz_hi, id_hi, X0, Y0, taps_b, normal_squarings, s_z)
        is_a = den_a > 0
        is_b = ~is_a & (den_b > 0)
        cls = np.where(is_a, 0, np.where(is_b, 1, 2))
        out = np.zeros((H, W, 4), np.float32)
        out[..., :3] = np.where(is_a[..., None], num_a / den_a[..., None], num_b / den_b[..., None])
    nearest = c[np.arange(H)[:, None] // f, np.arange(W)[None, :] // f]
    unguided = cls == 2
    out.view(np.uint32)[unguided, :3] = nearest.view(np.uint32)[unguided, :3]
    out[..., 3] = cls.astype(np.float32)
    counts = tuple(int(np.sum(cls == k)) for k in range(3))
    return out, encode_bgra(out), counts
