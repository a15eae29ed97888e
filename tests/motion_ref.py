"""Moving-model reprojection in numpy: temporal reprojection whose history also follows the models.
What the GPU must equal bit for bit.

Everything that §15.1 takes from §11 is temporal_ref's and raster_ref's own code (positions, the static history
step, resolve, dot4, normal_matrix, encode_bgra); only the moved case of step 2 and the table's checks are written
here. float32 arrays throughout, every product, sum and division one binary32 operation in the stated order. The
motion table is data: a structured array of ENTRY_DTYPE, or None for n = 0.
"""
from __future__ import annotations

import numpy as np

import raster_ref as rr
import temporal_ref as tr
from temporal_ref import encode_bgra  # noqa: F401  (re-exported for the tests)

F = np.float32
NO_PRIM = tr.NO_PRIM
MAX_ENTRIES = 1 << 20
ENTRY_DTYPE = np.dtype([("back", np.float32, (16,)), ("nback", np.float32, (12,)), ("moved", np.uint32),
                        ("reserved", np.uint32, (3,))])
EPS = F(0.00001)


def check_table(table):
    """(table as a flat ENTRY_DTYPE array, n); ValueError where iqpt_motion_begin_view returns INVALID_ARG."""
    if table is None:
        return np.zeros(0, ENTRY_DTYPE), 0
    t = np.ascontiguousarray(table).reshape(-1)
    if t.dtype != ENTRY_DTYPE:
        raise ValueError("the table must be an array of ENTRY_DTYPE")
    if t.size > MAX_ENTRIES:
        raise ValueError("a motion table has at most 2^20 entries")
    if np.any(t["moved"] > 1):
        raise ValueError("a motion entry's moved must be 0 or 1")
    if np.any(t["reserved"] != 0):
        raise ValueError("a motion entry's reserved words must be 0")
    return t, int(t.size)


def identity_table(n):
    t = np.zeros(n, ENTRY_DTYPE)
    t["back"][:, [0, 5, 10, 15]] = 1.0
    t["nback"][:, [0, 5, 10]] = 1.0
    return t


def entry(back, moved=1):
    """One entry from a 4x4 back matrix: nback = the first three rows of normal_matrix(back)."""
    e = identity_table(1)
    b = np.asarray(back, np.float32).reshape(4, 4)
    e["back"][0] = b.reshape(16)
    nb = np.zeros((3, 4), np.float32)
    nb[:, :3] = rr.normal_matrix(b)
    e["nback"][0] = nb.reshape(12)
    e["moved"][0] = moved
    return e[0]


def normalized3(m):
    """§9.6's rule on [..., 3]: zero where every component is below 1e-5 in magnitude, else m * (1 / sqrt(m.m))."""
    with np.errstate(all="ignore"):
        small = np.all(np.abs(m) < EPS, axis=-1)
        inv = F(1) / np.sqrt((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
        return np.where(small[..., None], F(0), m * inv[..., None]).astype(np.float32)


def moved_inputs(P, normal_z, ids, table):
    """Pm [H,W,4] and nm [H,W,3] of §15.1 for every pixel, through table[ids] (ids clipped: the caller masks)."""
    d = np.minimum(ids, len(table) - 1).astype(np.int64)
    B = table["back"][d].reshape(ids.shape + (4, 4))
    N = table["nback"][d].reshape(ids.shape + (3, 4))
    with np.errstate(all="ignore"):
        Pm = ((P[..., 0:1] * B[..., 0, :] + P[..., 1:2] * B[..., 1, :]) + P[..., 2:3] * B[..., 2, :]) + F(1) * B[..., 3, :]
        n = normal_z[..., :3]
        m = (n[..., 0:1] * N[..., 0, :3] + n[..., 1:2] * N[..., 1, :3]) + n[..., 2:3] * N[..., 2, :3]
    return Pm.astype(np.float32), normalized3(m.astype(np.float32))


def reproject(P, normal_z, ids, prev, table, normal_min, plane_tolerance, max_history, reasons=None):
    """Step 2 of §15.1: hist [H,W,4]. table: a checked ENTRY_DTYPE array (n = its length)."""
    n = len(table)
    static_r, moved_r = {}, {}
    hist = tr.reproject(P, normal_z, ids, prev, normal_min, plane_tolerance, max_history, reasons=static_r)
    guided = ids != NO_PRIM
    if n == 0:
        if reasons is not None:
            reasons.update(static_r, moved=np.zeros(ids.shape, bool), in_table=guided)
        return hist
    in_table = guided & (ids < n)
    moved = in_table & (table["moved"][np.minimum(ids, n - 1).astype(np.int64)] == 1)
    hist[~in_table] = 0
    if np.any(moved):
        Pm, nm = moved_inputs(P, normal_z, ids, table)
        # §11's step 2 with Pm for the point and nm for the normal is the moved case's arithmetic word for word
        nz_m = np.concatenate([nm, normal_z[..., 3:4]], axis=-1)
        hist_m = tr.reproject(Pm, nz_m, ids, prev, normal_min, plane_tolerance, max_history, reasons=moved_r)
        hist[moved] = hist_m[moved]
        moved_r.update(Pm=Pm, nm=nm)
    if reasons is not None:
        reasons.update(static_r, moved=moved, in_table=in_table, moved_reasons=moved_r)
    return hist


class Motion:
    """The motion object of §15.1 for a W x H frame."""

    def __init__(self, width, height, normal_min, plane_tolerance, max_history):
        tr.check_params(normal_min, plane_tolerance, max_history)
        self.width, self.height = width, height
        self.params = (float(normal_min), float(plane_tolerance), int(max_history))
        self.clear()

    def clear(self):
        self.view = None           # (view, projection, P, normal_z, ids)
        self.hist = None
        self.out = None
        self.moved = None
        self.reasons = {}

    def begin_view(self, cam, normal_z, ids, table=None):
        table, n = check_table(table)
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(self.height, self.width)
        normal_z = np.ascontiguousarray(normal_z, dtype=np.float32).reshape(self.height, self.width, 4)
        P = tr.positions(cam.inv_proj, cam.inv_view, normal_z[..., 3])
        self.reasons = {}
        guided = ids != NO_PRIM
        self.moved = guided & (ids < n) & (table["moved"][np.minimum(ids, max(n, 1) - 1).astype(np.int64)] == 1) \
            if n else np.zeros(ids.shape, bool)
        if self.view is None or self.out is None:
            self.hist = np.zeros((self.height, self.width, 4), np.float32)
        else:
            self.hist = reproject(P, normal_z, ids, self.view + (self.out,), table, *self.params, reasons=self.reasons)
        self.view = (tr._mat(cam.view), tr._mat(cam.projection), P, normal_z.copy(), ids.copy())
        self.out = None
        return self.hist

    def resolve(self, colour, n):
        if self.view is None:
            raise RuntimeError("resolve without a view")
        self.out = tr.resolve(self.hist, colour, n)
        return self.out, encode_bgra(self.out)

    def stats(self):
        """(guided, valid, moved, moved_valid) of the last begin_view."""
        valid = self.hist[..., 3] > 0
        return (int(np.sum(self.view[4] != NO_PRIM)), int(np.sum(valid)), int(np.sum(self.moved)),
                int(np.sum(self.moved & valid)))
