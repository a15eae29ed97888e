"""The variant census's recipes on the host (tests/variant_cases.py): every row the library exports
(iqpt_debug_variant_table: no device) yields a recipe, rows of one table yield different settings, the tables have the
documented sizes and no duplicate row, and a recipe never forces a bit whose kernels need the runtime's own buffers. A
row added to a table with a bit or a pair of bits the recipe function does not understand fails here, on a machine
without a GPU."""
import ctypes as C

import pytest

import variant_cases as vc
from iqpt import _lib

TABLES = vc.tables()


def test_documented_row_counts():
    assert {t: len(rows) for t, rows in TABLES.items()} == vc.DOCUMENTED_ROWS


def test_export_arguments():
    lb = _lib.load()
    n = C.c_uint32(77)
    assert lb.iqpt_debug_variant_table(6, None, 0, C.byref(n)) != 0 and n.value == 0
    assert lb.iqpt_debug_variant_table(-1, None, 0, C.byref(n)) != 0
    assert lb.iqpt_debug_variant_table(0, None, 0, None) != 0
    assert lb.iqpt_debug_variant_table(0, None, 3, C.byref(n)) != 0            # rows wanted, nowhere to put them
    # a short buffer: the first rows, the whole count
    two = (C.c_int32 * 9)(*([-7] * 9))
    assert lb.iqpt_debug_variant_table(0, two, 2, C.byref(n)) == 0 and n.value == len(TABLES["render"])
    assert [tuple(two[3 * i:3 * i + 3]) for i in range(2)] == TABLES["render"][:2] and list(two[6:]) == [-7] * 3
    out = (C.c_int32 * 8)()
    assert lb.iqpt_debug_last_launch(None, out) != 0


def test_fields_a_table_does_not_have_are_minus_one():
    for t in ("fan", "sky", "anyhit", "stitch"):
        assert all(m == -1 and s == -1 for m, s, _ in TABLES[t]), t
    assert all(m in (8, 16) and s in (0, 1) for m, s, _ in TABLES["render"])
    assert all(m in (8, 16) and s == 0 for m, s, _ in TABLES["spec"])
    # fan, sky and any-hit rows give the instantiated set (kOptDefault's bits), not the two key bits
    common = vc.COMMON
    for t in ("fan", "sky", "anyhit", "stitch"):
        assert all(o & common == common for _, _, o in TABLES[t]), t


@pytest.mark.parametrize("table", vc.TABLES)
def test_rows_are_unique(table):
    rows = TABLES[table]
    assert len(set(rows)) == len(rows), [r for r in rows if rows.count(r) > 1]


@pytest.mark.parametrize("table", vc.TABLES)
def test_every_row_yields_a_recipe(table):
    for row in TABLES[table]:
        r = vc.recipe(table, *row)                       # RowError: an unknown bit or a contradictory pair
        assert r.row == row and r.table == table
        assert r == vc.recipe(table, *row)               # pure
        assert r.depth == (9 if row[0] == 16 else 8)
        if r.force_opt is not None:
            assert not r.force_opt & vc.NEVER_FORCED, vc.row_id(table, row)
            assert table == "render" and row[1] == 1     # only streamed render rows fix the option set
        if r.overlap:
            assert r.frame[0] * r.frame[1] >= vc.OVERLAP_MIN_PIXELS and len(r.launches) == 3
        assert any(s % 2 for s in r.launches)


@pytest.mark.parametrize("table", vc.TABLES)
def test_recipes_are_distinct_where_rows_are(table):
    seen = {}
    for row in TABLES[table]:
        s = vc.recipe(table, *row).settings
        assert s not in seen, (vc.row_id(table, row), vc.row_id(table, seen[s]))
        seen[s] = row


def test_row_ids_are_distinct_and_spell_the_row():
    ids = [vc.row_id(t, r) for t, rows in TABLES.items() for r in rows]
    assert len(set(ids)) == len(ids)
    d = vc.default_options()
    assert vc.row_id("render", (8, 0, (d & ~vc.B.FastDiv) | vc.B.Mat | vc.B.Prio)) == "render-8-res-D~FastDiv|Mat|Prio"
    assert vc.row_id("sky", (-1, -1, d)) == "sky-D"


def test_lookups_agree_with_the_export():
    """The export's row counts are the documented ones (test_documented_row_counts); here the option sets the runtime's
    lookups must not find are in no exported row either, with or without kOptPrio, and iqpt_debug_set_kernel_options
    refuses a NULL context before any lookup (on the device, tests/test_gpu_variant_census.py compares the row each
    launch reports with the row the recipe asked for)."""
    lb = _lib.load()
    lb.iqpt_debug_set_kernel_options.argtypes = [C.c_void_p, C.c_int]
    lb.iqpt_debug_set_kernel_options.restype = C.c_int
    assert lb.iqpt_debug_set_kernel_options(None, vc.default_options()) == 1          # IQPT_ERR_INVALID_ARG
    rows8 = {o for m, _, o in TABLES["render"] if m == 8}
    d = vc.default_options()
    absent = [d | vc.B.LB6, d | vc.B.Stats, d | vc.B.Branchless, (d | vc.B.CamAxis) & ~vc.B.FastDiv,
              d | vc.B.Mat | vc.B.Pipe, d | vc.B.AnyHit | vc.B.Mat, d | vc.B.Split | vc.B.Overlap, 0]
    for opt in absent:
        assert opt not in rows8 and opt | vc.B.Prio not in rows8, vc.opt_name(opt)


def test_refused_rows():
    d = vc.default_options()
    for table, row in [("render", (8, 0, d | vc.B.Prio | (1 << 25))),                  # an unknown bit
                       ("render", (8, 0, d | vc.B.Prio | vc.B.Stats)),                 # a measurement build's bit
                       ("render", (8, 0, d)),                                          # resident without kOptPrio
                       ("render", (12, 0, d | vc.B.Prio)),                             # no such MAXD
                       ("render", (8, 1, (d | vc.B.CamAxis) & ~vc.B.LB5)),             # streamed with a resident bit
                       ("render", (8, 0, d | vc.B.Prio | vc.B.Split | vc.B.Pipe)),     # split launches take no kOptPipe
                       ("render", (8, 0, d | vc.B.Prio | vc.B.Mat | vc.B.Pipe)),
                       ("render", (8, 0, (d | vc.B.Prio | vc.B.CamAxis) & ~vc.B.FastDiv)),
                       ("render", (8, 1, (d | vc.B.AnyHit | vc.B.Mat) & ~vc.B.LB5)),
                       ("render", (8, 0, d & ~vc.B.Cull | vc.B.Prio)),                 # not a production set
                       ("anyhit", (-1, -1, d | vc.B.CamAxis)),                         # the row this census found dead
                       ("spec", (8, 0, d)), ("spec", (8, 0, d | vc.B.Prio | vc.B.Mat)),
                       ("sky", (8, 0, d)), ("stitch", (-1, -1, d | vc.B.CamAxis)), ("chain", (-1, -1, d))]:
        with pytest.raises(vc.RowError):
            vc.recipe(table, *row)


def test_cameras():
    """The recipe's two cameras: the default one qualifies for kOptCamAxis, the yawed one does not (host code)."""
    lb = _lib.load()
    lb.iqpt_debug_cam_axis.argtypes = [C.POINTER(_lib.Camera), C.POINTER(C.c_float)]
    k16 = (C.c_float * 16)()
    for frame in (vc.SMALL, vc.CORNELL, vc.BIG):
        assert lb.iqpt_debug_cam_axis(C.byref(vc.camera_of("pitch", frame)), k16) == 1
        assert lb.iqpt_debug_cam_axis(C.byref(vc.camera_of("yawed", frame)), k16) == 0


def test_scenes():
    """Resident and streamed as the recipe says (pair records of 128 bytes against 32 KiB), spheres where any-hit
    scenes must have none."""
    from iqpt.scene import packet_stats
    for kind in ("cornell", "streamed", "anyhit"):
        for oor in (False, True):
            for mats in (False, True):
                st = packet_stats(vc.scene_of((kind, oor, mats))[1])
                if kind == "cornell":
                    assert st["triangles"] <= 12 and 2 <= st["spheres"] <= 4
                else:
                    assert (st["triangles"] + 1) // 2 * 128 > 32 * 1024
                    assert (st["spheres"] == 0) == (kind == "anyhit")
