"""The variant census's recipes: for every row of libiqpt.so's kernel variant tables, the settings
that make the runtime launch that row, derived from the row's bits.

`tables()` reads the six tables from the library (iqpt_debug_variant_table: host code, no device). `recipe(table, maxd,
streamed, opt)` is a pure function of a row: it raises `RowError` for a bit it does not know and for a pair of bits no
launch combines, so a row added to a table either gets a case of tests/test_gpu_variant_census.py by itself or fails
tests/test_variant_cases.py on a machine without a GPU. No list of rows is kept here.

How a bit or field becomes a setting:

    maxd 8 / 16                 max_depth 8 / 9 (9 is the smallest depth that takes MAXD 16)
    streamed, no kOptAnyHit     a 900-triangle mesh (pair records above the 32 KiB resident limit) and spheres
    streamed, kOptAnyHit        the triangle mesh alone, the reference's materials
    not streamed                the Cornell box (10 triangles, 2 spheres)
    kOptFastDiv absent          one primitive outside the short divisions' range, added to the scene: a sphere of radius
                                1e-40, or (any-hit scenes: no sphere) two quads with edges of 2^61
    kOptMaterials               a material table, both material classes on triangles and on spheres
    kOptCamAxis / absent        the default pitch-only camera / a yawed one (the runtime then drops the bit)
    kOptPipe / absent           iqpt_debug_set_two_ray 1 / 0
    kOptSplit                   iqpt_set_split(SPLIT_ON)
    a spec row                  iqpt_set_split(SPLIT_SPEC)
    kOptOverlap                 iqpt_set_overlap(OVERLAP_AUTO), 161 x 103 = 16,583 owned pixels (at least 64 blocks of
                                256), three launches (both frame buffers of the overlapped pair)
    a streamed render row       iqpt_debug_set_kernel_options with the row's own kOptLB5 and kOptBvhPrimary (production
                                picks kOptBvhPrimary by timing and kOptLB5 by the launch's samples: a test must not
                                depend on which was faster that day); the runtime takes kOptFastDiv out and adds
                                kOptMaterials and kOptAnyHit from the packet
    kOptPrio                    left to the runtime (every resident row carries it)

NEVER force kOptOverlap, kOptSplit, kOptPipe or kOptStats through iqpt_debug_set_kernel_options. Those kernels read
queue words, per-tile completion counts, tile lists and split sets that only the runtime's own path fills in; a forced
launch without them would spin or read a null pointer, on a machine that others share. They are reached through the
public modes above only, and `recipe` refuses to put one of them into `force_opt`.

Fan, sky, any-hit and split-stitch rows get the launch that runs them beside another kernel: a spec launch (fan), a
plain resident launch without a material table (sky), an any-hit scene left to the runtime (iqpt_anyhit_kernel), a
split launch (stitch).

Frames: 37 x 19 (ragged both ways: 5 x 3 tiles of 8 x 8) for every case but the overlapped ones; spec, split, fan and
stitch cases render the Cornell box at 161 x 91 for its sphere pixels. Launches are 1 then 3 samples (an odd count ends
iqpt_sky_kernel's loop with its one-sample trip), and 2 more for the overlapped rows.

Scenes, cameras and the oracle's frames are cached per (scene, camera, depth, frame, launches): many rows share one
oracle render.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np

TABLES = ("render", "fan", "sky", "anyhit", "spec", "stitch")       # iqpt_debug_variant_table's numbers
# the row counts DESIGN.md §3.16 documents (tests/test_variant_cases.py compares the export with them)
DOCUMENTED_ROWS = {"render": 57, "fan": 3, "sky": 3, "anyhit": 2, "spec": 6, "stitch": 2}

# csrc/iqpt_internal.hpp kOpt*
BITS = {"CamConst": 1 << 0, "AccTable": 1 << 1, "Pair": 1 << 2, "LB5": 1 << 3, "LB6": 1 << 4, "SinCos": 1 << 5,
        "Branchless": 1 << 6, "Stats": 1 << 7, "FastDiv": 1 << 8, "Cull": 1 << 9, "Mat": 1 << 10, "Bvh": 1 << 11,
        "BvhPrimary": 1 << 12, "CamAxis": 1 << 14, "Split": 1 << 16, "Prio": 1 << 17, "Scatter2": 1 << 18,
        "Overlap": 1 << 19, "AnyHit": 1 << 20, "Pipe": 1 << 21}
B = type("B", (), BITS)
# every production row carries these; a row without one of them has no recipe
COMMON = B.CamConst | B.AccTable | B.Pair | B.SinCos | B.Cull | B.Bvh | B.Scatter2
# the bits a recipe turns into settings
VARYING = (B.LB5 | B.FastDiv | B.Mat | B.BvhPrimary | B.CamAxis | B.Split | B.Prio | B.Overlap | B.AnyHit | B.Pipe)
# never in a forced option set (module docstring)
NEVER_FORCED = B.Overlap | B.Split | B.Pipe | B.Stats

SPLIT_OFF, SPLIT_ON, SPLIT_SPEC = 0, 1, 4
SMALL, CORNELL, BIG = (37, 19), (161, 91), (161, 103)
OVERLAP_MIN_PIXELS = 64 * 256


class RowError(ValueError):
    """A table row `recipe` cannot turn into settings."""


def tables() -> dict[str, list[tuple[int, int, int]]]:
    """{table name: [(maxd, streamed, opt), ..]} as the library exports them (-1: the table has no such field)."""
    from iqpt import _lib
    lb = _lib.load()
    out = {}
    for t, name in enumerate(TABLES):
        n = C.c_uint32(0)
        _lib.check(lb.iqpt_debug_variant_table(t, None, 0, C.byref(n)), "iqpt_debug_variant_table")
        rows = np.zeros((max(n.value, 1), 3), np.int32)
        _lib.check(lb.iqpt_debug_variant_table(t, rows.ctypes.data_as(C.POINTER(C.c_int32)), n.value, C.byref(n)),
                   "iqpt_debug_variant_table")
        out[name] = [tuple(int(v) for v in r) for r in rows[:n.value]]
    return out


def default_options() -> int:
    from iqpt import _lib
    return int(_lib.load().iqpt_debug_default_options())


def opt_name(opt: int) -> str:
    """kOptDefault's bits as D, a missing one as ~Name, then the others: D~FastDiv|Mat|Prio."""
    d = default_options()
    s = "D" + "".join(f"~{k}" for k, v in BITS.items() if d & v and not opt & v)
    return "|".join([s] + [k for k, v in BITS.items() if opt & v and not d & v] +
                    [f"0x{opt & ~sum(BITS.values()):x}"] * bool(opt & ~sum(BITS.values())))


def bit_names(bits: int) -> str:
    return "|".join(f"kOpt{k}" for k, v in BITS.items() if bits & v)


def row_id(table: str, row: tuple[int, int, int]) -> str:
    maxd, streamed, opt = row
    parts = [table] + ([str(maxd)] if maxd >= 0 else []) + ([("str" if streamed else "res")] if streamed >= 0 else [])
    return "-".join(parts + [opt_name(opt)])


@dataclass(frozen=True)
class Recipe:
    table: str
    row: tuple                  # (maxd, streamed, opt)
    depth: int
    scene: tuple                # (kind, out_of_range, materials): kind "cornell", "streamed" or "anyhit"
    camera: str                 # "pitch" or "yawed"
    frame: tuple                # (width, height)
    launches: tuple
    two_ray: object             # 1, 0 or None (left at the default)
    split: int                  # SPLIT_*
    overlap: bool
    force_opt: object           # iqpt_debug_set_kernel_options' argument, or None

    @property
    def oracle_key(self):
        return (self.scene, self.camera, self.depth, self.frame, self.launches)

    @property
    def settings(self):
        """Everything the recipe sets (two rows of one table must differ in it)."""
        return (self.depth, self.scene, self.camera, self.frame, self.launches, self.two_ray, self.split, self.overlap,
                self.force_opt)


def _check_bits(table, opt):
    unknown = opt & ~sum(BITS.values())
    if unknown:
        raise RowError(f"{table}: unknown option bits 0x{unknown:x}")
    if opt & ~(COMMON | VARYING):
        raise RowError(f"{table}: no recipe for {bit_names(opt & ~(COMMON | VARYING))} (measurement builds only)")
    if (opt & COMMON) != COMMON:
        raise RowError(f"{table}: a production row lacks {bit_names(COMMON & ~opt)}")


def _refuse(table, opt, bits, why):
    if opt & bits:
        raise RowError(f"{table} {opt_name(opt)}: {bit_names(opt & bits)} {why}")


def recipe(table: str, maxd: int, streamed: int, opt: int) -> Recipe:
    """The settings that make the runtime launch row (maxd, streamed, opt) of `table`. Pure: the same row gives the
    same recipe, and it reads no table. RowError for a row it cannot reach."""
    if table not in TABLES:
        raise RowError(f"unknown table {table!r}")
    _check_bits(table, opt)
    row = (maxd, streamed, opt)
    fast = bool(opt & B.FastDiv)
    mats = bool(opt & B.Mat)
    camera = "pitch" if opt & B.CamAxis else "yawed"
    if table in ("render", "spec"):
        if maxd not in (8, 16):
            raise RowError(f"{table}: maxd {maxd} is neither 8 nor 16")
    elif maxd != -1 or streamed != -1:
        raise RowError(f"{table}: rows carry no maxd and no streamed field")
    depth = 9 if maxd == 16 else 8
    if not fast:
        _refuse(table, opt, B.CamAxis, "with the generic divisions: the runtime builds no such resident row, so it "
                "never adds kOptCamAxis there")
    if table == "render" and streamed == 1:
        _refuse(table, opt, B.CamAxis | B.Pipe | B.Split | B.Overlap | B.Prio, "in a streamed row: resident launches only")
        if opt & B.AnyHit:
            _refuse(table, opt, B.Mat, "with kOptAnyHit: any-hit scenes carry the reference's materials")
        # the row's own kOptLB5 and kOptBvhPrimary; the runtime clears kOptFastDiv and adds the packet's bits
        force = (opt | B.FastDiv) & ~(B.Mat | B.AnyHit)
        assert not force & NEVER_FORCED
        return Recipe(table, row, depth, ("anyhit" if opt & B.AnyHit else "streamed", not fast, mats), "pitch", SMALL,
                      (1, 3), None, SPLIT_OFF, False, force)
    if table == "render":
        if streamed != 0:
            raise RowError(f"render: streamed is {streamed}")
        _refuse(table, opt, B.AnyHit | B.BvhPrimary, "in a resident row: streamed launches only")
        if not opt & B.Prio:
            raise RowError(f"render {opt_name(opt)}: a resident row without kOptPrio (the runtime adds the bit)")
        if not opt & B.LB5:
            raise RowError(f"render {opt_name(opt)}: a resident row without kOptLB5 (the runtime keeps the bit)")
        if opt & B.Split:
            _refuse(table, opt, B.Pipe | B.Overlap | B.CamAxis, "with kOptSplit: split launches take none of them")
            return Recipe(table, row, depth, ("cornell", not fast, mats), "pitch", CORNELL, (1, 3), None, SPLIT_ON,
                          False, None)
        if mats:
            _refuse(table, opt, B.Pipe, "with kOptMaterials: the two-ray kernel is for the reference's materials")
        ovl = bool(opt & B.Overlap)
        return Recipe(table, row, depth, ("cornell", not fast, mats), camera, BIG if ovl else SMALL,
                      (1, 3, 2) if ovl else (1, 3), 1 if opt & B.Pipe else 0, SPLIT_OFF, ovl, None)
    # the other tables: reference materials, resident scenes but for iqpt_anyhit_kernel
    _refuse(table, opt, B.Mat | B.Pipe | B.AnyHit | B.BvhPrimary | B.Split | B.Overlap, f"in a row of the {table} table")
    if table == "spec":
        if streamed != 0:
            raise RowError("spec: rows are resident")
        if not opt & B.Prio:
            raise RowError(f"spec {opt_name(opt)}: the lookup adds kOptPrio, a row without it is never found")
        return Recipe(table, row, depth, ("cornell", not fast, False), camera, CORNELL, (1, 3), None, SPLIT_SPEC, False,
                      None)
    _refuse(table, opt, B.Prio, f"in a row of the {table} table")
    if table == "fan":                     # beside the spec kernel
        return Recipe(table, row, 8, ("cornell", not fast, False), camera, CORNELL, (1, 3), None, SPLIT_SPEC, False, None)
    if table == "sky":                     # ahead of the plain kernel
        return Recipe(table, row, 8, ("cornell", not fast, False), camera, SMALL, (1, 3), None, SPLIT_OFF, False, None)
    if table == "stitch":                  # between a split launch's two rounds
        _refuse(table, opt, B.CamAxis, "in a row of the stitch table")
        return Recipe(table, row, 8, ("cornell", not fast, False), "pitch", CORNELL, (1, 3), None, SPLIT_ON, False, None)
    # iqpt_anyhit_kernel: an any-hit scene left to the runtime
    _refuse(table, opt, B.CamAxis, "in a row of the anyhit table: the runtime adds kOptCamAxis to resident launches only")
    return Recipe(table, row, 8, ("anyhit", not fast, False), "pitch", SMALL, (1, 3), None, SPLIT_OFF, False, None)


# ---- scenes, cameras, the oracle's frames (shared, never changed) ----
def _cornell(sc, out_of_range, materials):
    from iqpt import MAT_EMISSIVE
    sc.add_preset("cornell_lit" if materials else "cornell")
    if materials:
        # cornell_lit: Oren-Nayar walls and spheres, an emissive panel; an emissive sphere makes it both classes on both
        lamp = sc.add_material(MAT_EMISSIVE, (0.9, 0.8, 1.0, 1.0), 4.0)
        sc.add_model("lamp", "sphere", 0.12, 0.0, (0.1, 0.9, 0.3))
        sc.set_model_material("lamp", lamp)
    if out_of_range:
        sc.add_model("dust", "sphere", 1e-40, 0.0, (0.0, 0.5, 0.5))


def _ball(sc):
    """900 triangles: 450 pair records of 128 bytes, above the 32 KiB resident limit."""
    sc.add_mesh_uv_sphere("ball", False, 30, 16, 0)
    sc.add_model("ball", "ball", 0.45, (0.2, 0.1, 0.0), (0.3, 0.35, 0.6))


def _streamed(sc, out_of_range, materials):
    from iqpt import MAT_EMISSIVE, MAT_OREN_NAYAR
    _ball(sc)
    sc.add_mesh_uv_sphere("sphere")
    names = []
    for i in range(21):
        names.append(f"s{i:02d}")
        sc.add_model(names[-1], "sphere", 0.09, 0.0, (-0.9 + 0.3 * (i % 7), 0.1, -0.4 + 0.4 * (i // 7)))
    sc.add_model("ground", "sphere", 10.0, 0.0, (0.0, -10.0, 0.0))
    if materials:
        glow = sc.add_material(MAT_EMISSIVE, (1.0, 0.4, 0.2, 1.0), 2.0)
        rough = sc.add_material(MAT_OREN_NAYAR, (0.6, 0.6, 0.7, 0.0), 0.8)
        sc.add_mesh_quad("quad")
        sc.add_model("panel", "quad", (0.8, 0.8, 1.0), (-1.2, 0.0, 0.0), (-0.5, 1.4, 0.5))
        sc.set_model_material("panel", glow)
        sc.set_model_material("ball", rough)
        sc.set_model_material("ground", rough)
        for k, n in enumerate(names):
            sc.set_model_material(n, glow if k % 3 == 0 else rough)
    if out_of_range:
        sc.add_model("dust", "sphere", 1e-40, 0.0, (0.0, 0.5, 0.5))


def _anyhit(sc, out_of_range, materials):
    from iqpt import MAT_EMISSIVE, MAT_OREN_NAYAR
    _ball(sc)
    if out_of_range:
        s = 2.0 ** 61
        sc.add_mesh_quad("b_quad")
        sc.add_model("giant", "b_quad", (s, s, 1.0), 0.0, (0.0, 0.0, 2.0 ** 62))
        sc.add_model("near", "b_quad", (s, s, 1.0), (0.3, 0.2, 0.0), (0.0, 0.5, 3.0))
    if materials:                           # (a hole of the tables: no any-hit row has kOptMaterials)
        sc.add_material(MAT_EMISSIVE, (1.0, 0.9, 0.7, 1.0), 1.5)
        rough = sc.add_material(MAT_OREN_NAYAR, (0.7, 0.6, 0.5, 0.0), 0.6)
        sc.set_model_material("ball", rough)


@functools.lru_cache(maxsize=None)
def scene_of(key):
    """(scene, packet) of a scene key (kind, out_of_range, materials); the scene is kept while its packet is used."""
    from iqpt import Scene
    kind, out_of_range, materials = key
    sc = Scene()
    {"cornell": _cornell, "streamed": _streamed, "anyhit": _anyhit}[kind](sc, out_of_range, materials)
    return sc, sc.build_packet()


def camera_of(name, frame):
    from iqpt import make_camera
    if name == "pitch":
        return make_camera(*frame)
    return make_camera(*frame, position=(0.6, 0.5, -3.0, 0.0), forward=(-0.6, -0.5, 3.0, 0.0))


@functools.lru_cache(maxsize=None)
def oracle_frame(scene, camera, depth, frame, launches):
    """The oracle's frame after `launches`, read-only and shared by every case with this key."""
    import oracle
    _sc, pk = scene_of(scene)
    fr = oracle.OracleFrame(*frame, max_depth=depth)
    cam = camera_of(camera, frame)
    for s in launches:
        fr.render(pk, cam, s)
    for a in (fr.lin, fr.bgra, fr.states, fr.rays):
        a.setflags(write=False)
    return fr


def last_launch(pt) -> dict:
    """iqpt_debug_last_launch as a dict: maxd, streamed, opt and the rows (-1: not launched) of sky, fan, spec, anyhit,
    stitch."""
    from iqpt import _lib
    out = (C.c_int32 * 8)()
    _lib.check(_lib.load().iqpt_debug_last_launch(pt._h, out), "iqpt_debug_last_launch")
    return dict(zip(("maxd", "streamed", "opt", "sky", "fan", "spec", "anyhit", "stitch"), (int(v) for v in out)))


def last_options(pt) -> int:
    from iqpt import _lib
    lb = _lib.load()
    lb.iqpt_debug_last_options.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    o = C.c_int(0)
    _lib.check(lb.iqpt_debug_last_options(pt._h, C.byref(o)), "iqpt_debug_last_options")
    return o.value


def render(r: Recipe, depth=None, split=None):
    """Apply a recipe and render its launches: ((lin, bgra, rng, rays), [last_launch after each launch], [the
    iqpt_debug_last_options word after each], sky tiles of the masks). `depth` and `split` override the recipe's
    (the holes of tests/test_gpu_variant_census.py)."""
    from iqpt import PathTracer, _lib
    lb = _lib.load()
    _sc, pk = scene_of(r.scene)
    pt = PathTracer(*r.frame, max_depth=r.depth if depth is None else depth)
    try:
        if r.force_opt is not None:
            assert not r.force_opt & NEVER_FORCED, opt_name(r.force_opt)
            lb.iqpt_debug_set_kernel_options.argtypes = [C.c_void_p, C.c_int]
            _lib.check(lb.iqpt_debug_set_kernel_options(pt._h, r.force_opt), "iqpt_debug_set_kernel_options")
        if r.two_ray is not None:
            lb.iqpt_debug_set_two_ray.argtypes = [C.c_void_p, C.c_int]
            _lib.check(lb.iqpt_debug_set_two_ray(pt._h, r.two_ray), "iqpt_debug_set_two_ray")
        pt.set_split(r.split if split is None else split)
        pt.set_overlap(_lib.OVERLAP_AUTO if r.overlap else _lib.OVERLAP_OFF)
        pt.set_camera(camera_of(r.camera, r.frame))
        pt.upload_packet(pk)
        seen, words = [], []
        for s in r.launches:
            pt.render(s)
            seen.append(last_launch(pt))
            words.append(last_options(pt))
        pt.sync()
        lin, bgra = pt.read()
        out = (lin, bgra, pt.read_rng(), pt.rays())
        lb.iqpt_debug_sky_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        px, tl = C.c_uint32(0), C.c_uint32(0)
        _lib.check(lb.iqpt_debug_sky_info(pt._h, C.byref(px), C.byref(tl)), "iqpt_debug_sky_info")
        return out, seen, words, tl.value
    finally:
        pt.close()
