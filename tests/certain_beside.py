"""Shared by tests/test_certain_beside_sphere.py and tests/test_gpu_certain_beside_sphere.py: the beside-a-sphere
certain-hit rule restated from the host build of csrc/iq_interval.h, per pixel, with
iqpt_debug_cull_tile and iqpt_debug_certain_tile alone (as tests/proof_masks.py restates the tile rule), and the
world-space primitives of a preset's packet without a device."""
import numpy as np

from iqpt import _lib
from proof_masks import CERTAIN_MAX_PAIRS, TILE, _pairs
from test_certain import certain_tile
from test_cull import cull_tile

# iqpt_certain_kernel folds a tile's marked pixels (its fourth plane, kparams::certain) when the tile has at least this
# many, or all of a smaller ragged tile (kCertainBesideMin: DESIGN.md §3.3 has the measurement behind it)
BESIDE_MIN = 32


def folds(mask, npt):
    """Whether a tile of npt pixels with this beside-a-sphere mask folds its marked pixels."""
    return bin(int(mask)).count("1") >= min(BESIDE_MIN, npt)


# a pixel of a tile with a sphere candidate is one of
MARKED, SPHERE, SEAM, MISS = 1, 2, 3, 4
# MARKED  the rule's certain hit: every candidate sphere culled for its own bundle, some candidate triangle certain
# SPHERE  its own bundle is unbounded or does not cull every candidate sphere (it may reach one)
# SEAM    every candidate sphere culled, no candidate triangle certain, some candidate triangle not culled
# MISS    every candidate culled (the sky kernel's)


def tile_grid(ps):
    ncols = ps.x1 - ps.x0
    return ncols, (ncols + TILE - 1) // TILE, (ps.nrows + TILE - 1) // TILE


def tile_box(ps, t):
    """Tile t of the owned set: first and last column and row (of the set), its width and height."""
    ncols, ntx, _ = tile_grid(ps)
    tx, ty = t % ntx, t // ntx
    c0, c1 = tx * TILE, min(tx * TILE + TILE, ncols) - 1
    k0, k1 = ty * TILE, min(ty * TILE + TILE, ps.nrows) - 1
    return c0, c1, k0, k1, c1 - c0 + 1, k1 - k0 + 1


def tile_candidates(cam, ps, t, tris9, sph4):
    """The tile's candidate triangle and sphere pairs (iqpt_bin_kernel's masks, as proof_masks.host_masks)."""
    c0, c1, k0, k1, _, _ = tile_box(ps, t)
    ok, tc, sc = cull_tile(cam, ps.x0 + c0, ps.x0 + c1, ps.y0 + k0 * ps.ystep, ps.y0 + k1 * ps.ystep, tris9, sph4)
    return np.flatnonzero(~(_pairs(tc, len(tris9)) & ok)), np.flatnonzero(~(_pairs(sc, len(sph4)) & ok))


def beside_tile(cam, ps, t, tris9, sph4):
    """The rule for tile t. Returns None for a tile without a sphere candidate (the tile rule's), else
    (mask, kinds): the 64-bit mask of its marked pixels (bit = lane, row-major inside the tile) and each lane's kind
    (0 outside a ragged tile). A tile of more than CERTAIN_MAX_PAIRS candidate pairs marks nothing."""
    jt, js = tile_candidates(cam, ps, t, tris9, sph4)
    if len(js) == 0:
        return None
    ntri, nsph = len(tris9), len(sph4)
    ti = np.array([k for j in jt for k in (2 * j, 2 * j + 1) if k < ntri], np.int64)
    si = np.array([k for j in js for k in (2 * j, 2 * j + 1) if k < nsph], np.int64)
    small = len(jt) + len(js) <= CERTAIN_MAX_PAIRS
    c0, _, k0, _, tw, th = tile_box(ps, t)
    mask, kinds = 0, np.zeros(64, np.uint8)
    for lane in range(tw * th):
        x, y = ps.x0 + c0 + lane % tw, ps.y0 + (k0 + lane // tw) * ps.ystep
        pok, ptc, psc = cull_tile(cam, x, x, y, y, tris9, sph4)
        if not (pok and bool(psc[si].all())):
            kinds[lane] = SPHERE
            continue
        _, pcert = certain_tile(cam, x, x, y, y, tris9)
        if bool(pcert[ti].any()):
            kinds[lane] = MARKED
            mask |= int(small) << lane
        else:
            kinds[lane] = MISS if bool(ptc[ti].all()) else SEAM
    return mask, kinds


def beside_masks(cam, ps, tris9, sph4):
    """Per tile of the owned set: the plane iqpt_certain_kernel must write (uint64 per tile, 0 for a tile without a
    sphere candidate), and {tile: kinds} for the tiles with one."""
    _, ntx, nty = tile_grid(ps)
    plane = np.zeros(ntx * nty, np.uint64)
    kinds = {}
    for t in range(ntx * nty):
        r = beside_tile(cam, ps, t, tris9, sph4)
        if r is not None:
            plane[t] = np.uint64(r[0])
            kinds[t] = r[1]
    return plane, kinds


def lane_pixels(ps, t, mask):
    """(x, y) frame coordinates of the lanes set in a tile's mask."""
    c0, _, k0, _, tw, th = tile_box(ps, t)
    return [(ps.x0 + c0 + lane % tw, ps.y0 + (k0 + lane // tw) * ps.ystep)
            for lane in range(tw * th) if (int(mask) >> lane) & 1]


def packet_primitives(pk):
    """World-space (v0, e1, e2) triangles and (centre, radius) spheres of a packet of identity-scaled sphere draw
    calls, as the runtime builds them: the row-vector transform with the reference's association (vector.h:371-383),
    as tests/test_cull.py's Cornell test."""
    tris = []
    for i in range(pk.num_drawcalls[_lib.MESH_TRIANGLES]):
        dc = pk.tri_mesh_dcs[i]
        m = pk.tri_meshes[dc.mesh_id]
        M = np.array(dc.transform, dtype=np.float32).reshape(4, 4)
        for j in range(0, m.num_indices, 3):
            vs = []
            for q in range(3):
                v = m.vertices[m.indices[j + q]]
                p = np.array([v.pos[0], v.pos[1], v.pos[2], 1.0], np.float32)
                vs.append(np.array([np.float32(((p[0] * M[0, c] + p[1] * M[1, c]) + p[2] * M[2, c]) + p[3] * M[3, c])
                                    for c in range(3)], np.float32))
            tris.append(np.concatenate([vs[0], vs[1] - vs[0], vs[2] - vs[0]]).astype(np.float32))
    ns = int(pk.num_drawcalls[_lib.MESH_SPHERES])
    sph = np.array([list(pk.sphere_dcs[i].center)[:3] + [pk.sphere_dcs[i].radius] for i in range(ns)], np.float32)
    return np.stack(tris), sph.reshape(-1, 4)
