"""The variant census: every row of libiqpt.so's six kernel variant tables is launched once and
compared with the oracle, bit for bit.

The cases are the rows the library exports (iqpt_debug_variant_table, read at collection time); each row's settings
come from its bits (tests/variant_cases.py). A case renders its launches, asserts from iqpt_debug_last_launch that every
one of them ran this row (and the auxiliary kernels that belong to such a launch), and compares the accumulators'
bits, the BGRA8 frame, the six XORWOW words of every pixel and the ray count with the oracle: no pixel set aside, no
tolerance. Overlapped rows also assert bit 30 of iqpt_debug_last_options (tiles dealt to per-XCD lists): a device that
does not expose 8 XCDs fails them.

test_every_exported_row_was_launched closes the census: the rows the launches reported are the rows exported, for all
six tables, none missing. test_holes covers configurations no row matches exactly, where the runtime's cascade has to
drop a bit and land on a row that exists."""
import numpy as np
import pytest

import variant_cases as vc
from helpers import compare

pytestmark = pytest.mark.gpu

TABLES = vc.tables()
ROWS = [(t, r) for t in vc.TABLES for r in TABLES[t]]
KEY = vc.B.FastDiv | vc.B.CamAxis                 # what the fan, sky, any-hit and stitch lookups read of a launch's set
HIT = {t: set() for t in vc.TABLES}               # rows the launches of this module reported


def aux_row(table, opt):
    """The row of an auxiliary table a launch with `opt` takes (the launchers key on kOptFastDiv and kOptCamAxis), or
    None."""
    bits = vc.B.FastDiv if table == "stitch" else KEY
    found = [i for i, (_, _, o) in enumerate(TABLES[table]) if o & bits == opt & bits]
    return found[0] if found else None


def note(seen):
    """Record what one launch reported; the rows must exist."""
    for s in seen:
        if s["spec"] >= 0:
            assert TABLES["spec"][s["spec"]] == (s["maxd"], 0, s["opt"]), s
            HIT["spec"].add(TABLES["spec"][s["spec"]])
        elif s["opt"] >= 0:
            row = (s["maxd"], s["streamed"], s["opt"])
            assert row in TABLES["render"], (s, vc.opt_name(s["opt"]))
            HIT["render"].add(row)
        else:
            assert s["anyhit"] >= 0, s                                     # some kernel rendered the launch
        for t in ("sky", "fan", "anyhit", "stitch"):
            if s[t] >= 0:
                assert s[t] < len(TABLES[t]), s
                HIT[t].add(TABLES[t][s[t]])


def same_as_oracle(out, fr):
    lin, bgra, rng, rays = out
    c = compare(lin, fr.lin)
    assert c["bitexact"] == c["npix"], c
    assert np.array_equal(bgra, fr.bgra)
    assert np.array_equal(rng, fr.states)
    assert rays == int(fr.rays.sum())


def check_launches(r, seen, words, sky_tiles):
    """Every launch ran the recipe's row and the auxiliary kernels of such a launch, no other."""
    table, (maxd, streamed, opt) = r.table, r.row
    index = TABLES[table].index(r.row)
    for s, word in zip(seen, words):
        sid = (vc.row_id(table, r.row), s, vc.opt_name(s["opt"]) if s["opt"] >= 0 else None)
        if table == "render":
            assert (s["maxd"], s["streamed"], s["opt"]) == (maxd, streamed, opt), sid
            assert s["spec"] == -1 and s["anyhit"] == -1, sid
            if opt & vc.B.Split:
                assert s["stitch"] == aux_row("stitch", opt) and s["sky"] == -1, sid
                assert s["fan"] == (-1 if opt & vc.B.Mat else aux_row("fan", opt)), sid
            else:
                assert s["stitch"] == -1 and s["fan"] == -1, sid
                sky = not streamed and not opt & vc.B.Mat and sky_tiles > 0
                assert s["sky"] == (aux_row("sky", opt) if sky else -1), sid
            if opt & vc.B.Overlap:
                assert word & (1 << 30), sid                   # tiles really dealt to per-XCD lists
            assert word & ~(3 << 29) == opt, sid               # iqpt_debug_last_options keeps its meaning
        elif table == "spec":
            assert (s["maxd"], s["streamed"], s["opt"], s["spec"]) == (maxd, 0, opt, index), sid
            assert s["fan"] == aux_row("fan", opt) and s["stitch"] == -1 and s["anyhit"] == -1, sid
            assert s["sky"] == (aux_row("sky", opt) if sky_tiles > 0 else -1), sid
        elif table == "fan":
            assert s["fan"] == index and s["spec"] >= 0, sid
        elif table == "sky":
            assert sky_tiles > 0 and s["sky"] == index and s["opt"] >= 0 and s["spec"] == -1, sid
        elif table == "anyhit":
            assert s["anyhit"] == index and s["opt"] == -1 and s["streamed"] == 1 and word & (1 << 29), sid
            assert s["sky"] == s["fan"] == s["spec"] == s["stitch"] == -1, sid
        else:
            assert s["stitch"] == index and s["opt"] >= 0 and s["opt"] & vc.B.Split, sid


@pytest.mark.parametrize("table,row", ROWS, ids=[vc.row_id(t, r) for t, r in ROWS])
def test_row(require_gpu, table, row):
    r = vc.recipe(table, *row)
    out, seen, words, sky_tiles = vc.render(r)
    note(seen)
    print(vc.row_id(table, row), seen[-1], "sky tiles", sky_tiles)
    check_launches(r, seen, words, sky_tiles)
    same_as_oracle(out, vc.oracle_frame(*r.oracle_key))


# ---- configurations without a row of their own: the cascade must land on one ----
def _hole(scene, camera="pitch", frame=vc.SMALL, launches=(1, 3), two_ray=None, split=vc.SPLIT_OFF, overlap=False,
          depth=9):
    return vc.Recipe("render", None, depth, scene, camera, frame, launches, two_ray, split, overlap, None)


HOLES = {
    # kOptMaterials | kOptCamAxis is built at MAXD 8 only
    "d9-materials-pitch-overlap": _hole(("cornell", False, True), frame=vc.BIG, launches=(1, 3, 2), overlap=True),
    # the generic divisions with kOptPipe are built at MAXD 8 only
    "d9-out_of_range-two_ray": _hole(("cornell", True, False), camera="yawed", two_ray=1),
    "d9-out_of_range-split_on": _hole(("cornell", True, False), frame=vc.CORNELL, split=vc.SPLIT_ON),
    "d9-materials-split_on": _hole(("cornell", False, True), frame=vc.CORNELL, split=vc.SPLIT_ON),
    # a material table over any-hit geometry (no sphere): kparams::anyhit must be off, no row has both bits
    "streamed-materials-anyhit_geometry": _hole(("anyhit", False, True), depth=8),
    # the generic divisions with kOptAnyHit are built at MAXD 8 only
    "d9-streamed-out_of_range-anyhit_geometry": _hole(("anyhit", True, False)),
    # spec launches take the reference's materials only: the plain path
    "split_spec-materials": _hole(("cornell", False, True), frame=vc.CORNELL, split=vc.SPLIT_SPEC, depth=8),
    "split_spec-yawed-out_of_range": _hole(("cornell", True, False), camera="yawed", frame=vc.CORNELL,
                                           split=vc.SPLIT_SPEC, depth=8),
}


@pytest.mark.parametrize("name", list(HOLES))
def test_holes(require_gpu, name):
    """iqpt_render returns IQPT_OK (vc.render raises otherwise: "render kernel launch: invalid device function" is the
    failure this guards against), every launch reports rows of the exported tables, the frame is the oracle's."""
    r = HOLES[name]
    out, seen, words, sky_tiles = vc.render(r)
    print(name, [(s, vc.opt_name(s["opt"]) if s["opt"] >= 0 else None) for s in seen])
    note(seen)                                     # asserts that the rows exist
    for s in seen:
        assert s["maxd"] == (16 if r.depth > 8 else 8), s
        assert s["streamed"] == (0 if r.scene[0] == "cornell" else 1), s
        if r.scene[2]:                             # a material table: the plain kernel with kOptMaterials, alone
            assert s["opt"] & vc.B.Mat and s["spec"] == s["sky"] == s["fan"] == s["anyhit"] == -1, s
        if r.scene[1] and s["opt"] >= 0:
            assert not s["opt"] & vc.B.FastDiv, s
    if name == "split_spec-materials":
        assert all(s["spec"] == -1 and s["stitch"] == -1 for s in seen), seen
    same_as_oracle(out, vc.oracle_frame(*r.oracle_key))


def test_every_exported_row_was_launched(require_gpu):
    """The rows hit are the rows exported, all six tables, none left out. (Run alone, or with cases deselected, it
    launches the missing rows' recipes itself first, without the comparison.)"""
    for table, row in ROWS:
        if row not in HIT[table]:
            note(vc.render(vc.recipe(table, *row))[1])
    missing = {t: sorted(vc.row_id(t, r) for r in set(TABLES[t]) - HIT[t]) for t in vc.TABLES}
    assert not any(missing.values()), missing
    assert all(HIT[t] == set(TABLES[t]) for t in vc.TABLES)
