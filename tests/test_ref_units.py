"""Every routine the oracle restates, against the reference's own source compiled as a host library (oracle/ref/).

Live: the reference's routines (flavour A: glibc libm, none of this project's arithmetic on the reference side;
flavour B: its transcendentals redirected to csrc/iq_fp.h) against the oracle's hooks of the same flavour on N_LIVE
seeded random cases per routine plus the edge cases of tests/ref_cases.py; cameras, model transforms and mesh
generators against the project's scene builder. Every float is compared as uint32, every flag, integer and generator
state for equality, and no case is left out. Skipped where oracle/_ref/ is absent (no reference directory).

Recorded: tests/golden/ref_units.npz holds the reference's flavour-B outputs (tests/golden/make_ref_golden.py); the
oracle and the scene builder reproduce them bit for bit everywhere, and where oracle/_ref/ exists the live flavour-B
output is compared with the fixture too, so a stale fixture fails.

The generator behind curandState is csrc/iq_xorwow.h on both sides: cuRAND is the one part the reference does not
contain, so equal states prove equal consumption of the generator, not the generator itself.
"""
import functools
from pathlib import Path

import numpy as np
import pytest

import ref_cases as rc
import ref_oracle

GOLDEN = Path(__file__).resolve().parent / "golden"
FLAVOURS = {"a": "glibc", "b": "b"}          # reference flavour -> the oracle flavour it is compared with
ROUTINES = {"tri": "tri", "sphere": "sphere", "onb": "onb", "real": "real", "cosine": "cosine",
            "oren_nayar": "scatter", "emissive": "scatter", "normal_matrix": "matrix", "transform": "matrix"}


def live(flavour):
    if not ref_oracle.available(flavour):
        pytest.skip(f"oracle/_ref/libref_{flavour}.so absent: no reference directory to build it from")
    return ref_oracle.load(flavour)


@functools.lru_cache(maxsize=None)
def inputs():
    return rc.unit_inputs(rc.N_LIVE)


@functools.lru_cache(maxsize=None)
def oracle_out(flavour):
    return rc.oracle_units(inputs(), FLAVOURS[flavour])


@functools.lru_cache(maxsize=None)
def ref_out(flavour):
    return rc.ref_units(inputs(), ref_oracle.load(flavour))


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN / "ref_units.npz", allow_pickle=False) as g:
        return {k: g[k] for k in g.files}


def part(d, routine):
    return {k: v for k, v in d.items() if k.startswith(routine + ".")}


# ------------------------------------------------------------------------------------------------ live
@pytest.mark.parametrize("routine", list(ROUTINES))
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_live_routine_matches_the_reference(flavour, routine):
    live(flavour)
    diff = rc.first_difference(part(ref_out(flavour), routine), part(oracle_out(flavour), routine),
                               inputs()[ROUTINES[routine]])
    assert diff is None, f"{routine} (flavour {flavour}): reference != oracle: {diff}"
    n = len(next(iter(part(ref_out(flavour), routine).values())))
    assert n > rc.N_LIVE          # the random block and the edge cases, none left out


def test_live_cameras_match_the_reference():
    """camera's view / projection matrices and their inverses against make_camera, and get_ray against the oracle's,
    on the four corner pixels, the centre and random pixels of 1x1 ... 3840x2160 frames, for four cameras."""
    ref = live("b")
    diff = rc.first_difference(rc.ref_cameras(ref), rc.project_cameras("b"))
    assert diff is None, f"camera: reference != project: {diff}"


def test_live_get_ray_matches_the_reference_on_its_own_matrices():
    """Flavour A: the reference's camera matrices come from glibc's tanf, the project's (csrc/iq_scene.cpp) always from
    csrc/iq_fp.h, so the matrices have no flavour-A counterpart to be compared with; get_ray has, and is compared on
    the reference's own matrices (no arithmetic of this project on the reference side)."""
    ref = live("a")
    want = rc.ref_cameras(ref)
    diff = rc.first_difference(want, rc.project_cameras("glibc", matrices=want))
    assert diff is None, f"get_ray (flavour a): reference != oracle: {diff}"


def test_live_model_transforms_match_the_reference():
    """model::set_transforms against Scene.add_model's matrix, for every transform of the scenes and random ones
    (flavour B: the host matrices of csrc/iq_scene.cpp have no glibc flavour)."""
    ref = live("b")
    diff = rc.first_difference(rc.ref_model_transforms(ref), rc.project_model_transforms())
    assert diff is None, f"model transform: reference != project: {diff}"


@pytest.mark.parametrize("spec", rc.MESHES, ids=rc.mesh_key)
def test_live_mesh_generators_match_the_reference(spec):
    """Vertex positions, normals, indices, counts and mesh type, through draw_list() and, for triangle meshes,
    build_packet() (flavour B, as above)."""
    ref = live("b")
    diff = rc.first_difference(rc.ref_mesh(ref, spec), rc.project_mesh(spec))
    assert diff is None, f"mesh {rc.mesh_key(spec)}: reference != project: {diff}"


# ------------------------------------------------------------------------------------------------ recorded
def recorded_inputs():
    g = golden()
    out = {}
    for k, v in g.items():
        if k.startswith("in.") and not k.startswith(("in.camera.", "in.model.")):
            _, routine, name = k.split(".", 2)
            out.setdefault(routine, {})[name] = v
    return out


def recorded_outputs():
    return {k[4:]: v for k, v in golden().items() if k.startswith("out.")}


@functools.lru_cache(maxsize=None)
def oracle_on_recorded():
    return rc.oracle_units(recorded_inputs(), "b")


def test_recorded_inputs_are_the_seeded_cases():
    """The fixture's inputs are N_RECORDED random cases and every edge case of ref_cases.py: same shapes, and the
    hand-made edge cases bit for bit (the random block and the two random columns of the edge rows are not compared
    with a fresh draw: numpy does not promise the same stream in every version, and the recorded tests run on the
    fixture's own inputs)."""
    want = rc.recorded_subset(inputs())
    got = recorded_inputs()
    assert sorted(want) == sorted(got)
    drawn = {("scatter", "states"), ("matrix", "p3")}
    for routine in want:
        assert sorted(want[routine]) == sorted(got[routine]), routine
        for k, v in want[routine].items():
            assert got[routine][k].shape == v.shape and got[routine][k].dtype == v.dtype, (routine, k)
            assert len(v) > rc.N_RECORDED, (routine, k)
            if (routine, k) not in drawn:
                assert np.array_equal(rc.bits(got[routine][k][rc.N_RECORDED:]), rc.bits(v[rc.N_RECORDED:])), (routine, k)
    g = golden()
    for key, _kw, w, h, xs, ys, states in rc.camera_cases():
        assert np.array_equal(g[f"in.camera.{key}.x"][:5], xs[:5]) and np.array_equal(g[f"in.camera.{key}.y"][:5], ys[:5])
        assert g[f"in.camera.{key}.states"].shape == states.shape


@pytest.mark.parametrize("routine", list(ROUTINES))
def test_oracle_reproduces_the_recorded_reference(routine):
    diff = rc.first_difference(part(recorded_outputs(), routine), part(oracle_on_recorded(), routine),
                               recorded_inputs()[ROUTINES[routine]])
    assert diff is None, f"{routine}: recorded reference != oracle: {diff}"


def test_project_reproduces_the_recorded_cameras_and_transforms():
    g = golden()
    cams = {k[len("camera."):]: v for k, v in g.items() if k.startswith("camera.")}
    diff = rc.first_difference(cams, rc.project_cameras("b", cases=rc.recorded_camera_cases(g)))
    assert diff is None, f"camera: recorded reference != project: {diff}"
    diff = rc.first_difference({"model.transform": g["model.transform"]},
                               rc.project_model_transforms([tuple(map(list, c)) for c in g["in.model.srt"].tolist()]))
    assert diff is None, f"model transform: recorded reference != project: {diff}"


@pytest.mark.parametrize("spec", rc.MESHES, ids=rc.mesh_key)
def test_project_reproduces_the_recorded_meshes(spec):
    g, key = golden(), rc.mesh_key(spec)
    m = rc.project_mesh(spec)
    assert [len(m["vertices"]), len(m["indices"]), int(m["mesh_type"][0])] == g[f"mesh.{key}.counts"].tolist()
    for what in ("vertices", "indices"):
        assert np.array_equal(rc.sha(m[what]), g[f"mesh.{key}.{what}_sha256"]), what
        if f"mesh.{key}.{what}" in g:
            assert np.array_equal(rc.bits(m[what]), rc.bits(g[f"mesh.{key}.{what}"])), what
        if "packet." + what in m:
            assert np.array_equal(rc.bits(m["packet." + what]), rc.bits(m[what])), what


def test_live_reference_matches_its_recording():
    """A stale fixture fails: the live flavour-B library on the recorded inputs gives the recorded outputs."""
    ref = live("b")
    g = golden()
    diff = rc.first_difference(recorded_outputs(), rc.ref_units(recorded_inputs(), ref))
    assert diff is None, f"ref_units.npz is stale: {diff}"
    cams = {k[len("camera."):]: v for k, v in g.items() if k.startswith("camera.")}
    assert rc.first_difference(cams, rc.ref_cameras(ref, cases=rc.recorded_camera_cases(g))) is None
    srt = [tuple(map(list, c)) for c in g["in.model.srt"].tolist()]
    assert rc.first_difference({"model.transform": g["model.transform"]}, rc.ref_model_transforms(ref, srt)) is None
    for spec in rc.MESHES:
        m, key = rc.ref_mesh(ref, spec), rc.mesh_key(spec)
        assert np.array_equal(rc.sha(m["vertices"]), g[f"mesh.{key}.vertices_sha256"]), key
        assert np.array_equal(rc.sha(m["indices"]), g[f"mesh.{key}.indices_sha256"]), key
