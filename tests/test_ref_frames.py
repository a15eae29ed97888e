"""Whole frames: the reference's render_kernel run as a host loop (oracle/ref/) against the oracle.

Each scene is built by the reference's own scene / mesh / model / camera classes from the plain description of
tests/ref_cases.py (SCENES); lin_fb bits, BGRA bytes and the final generator state of every pixel are compared. Equal
states prove equal consumption of the generator (csrc/iq_xorwow.h on both sides; cuRAND itself is the one part the
reference does not contain). The reference counts no rays, so ray counts are not compared. Scenes with the project's
material table (cornell_lit) have no counterpart in the reference and stay out.

Live (skipped where oracle/_ref/ is absent): reference flavour A against OracleFrame(flavour="glibc"), flavour B against
flavour="b", both on this host. Recorded (always): the oracle reproduces tests/golden/ref_<frame>.npz, the reference's
flavour-B frames, and the project's scene builder and camera reproduce the packet and matrices stored with them.
"""
from pathlib import Path

import numpy as np
import pytest

import ref_cases as rc
import ref_oracle
from iqpt import Scene

GOLDEN = Path(__file__).resolve().parent / "golden"
FLAVOURS = {"a": "glibc", "b": "b"}


def live(flavour):
    if not ref_oracle.available(flavour):
        pytest.skip(f"oracle/_ref/libref_{flavour}.so absent: no reference directory to build it from")
    return ref_oracle.load(flavour)


def golden(name):
    with np.load(GOLDEN / f"ref_{name}.npz", allow_pickle=False) as g:
        return {k: g[k] for k in g.files}


@pytest.mark.parametrize("preset", rc.PRESETS)
def test_descriptions_are_the_presets(preset):
    """The description the reference's scene code replays is the project's preset: same packet, bit for bit."""
    sc = Scene()
    sc.add_preset(preset)
    replayed = rc.project_scene(preset)          # a scene owns the arrays its packet points into
    diff = rc.first_difference(rc.packet_arrays(sc.build_packet()), rc.packet_arrays(replayed.build_packet()))
    assert diff is None, diff


@pytest.mark.parametrize("name", list(rc.FRAMES))
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_live_frame_matches_the_reference(flavour, name):
    ref = live(flavour)
    if flavour == "b":   # the project's host matrices use csrc/iq_fp.h, as the reference's do in this flavour only
        diff = rc.first_difference(rc.ref_frame_inputs(name, ref), rc.frame_inputs(name))
        assert diff is None, f"{name}: the reference's packet / camera != the project's: {diff}"
    diff = rc.first_difference(rc.ref_frame(name, ref), rc.oracle_frame(name, FLAVOURS[flavour]))
    assert diff is None, f"{name} (flavour {flavour}): reference frame != oracle frame: {diff}"


@pytest.mark.parametrize("name", list(rc.FRAMES))
def test_oracle_reproduces_the_recorded_frame(name):
    g = golden(name)
    frame = {k: v for k, v in g.items() if not k.startswith("in.")}
    diff = rc.first_difference(frame, rc.oracle_frame(name, "b"))
    assert diff is None, f"{name}: recorded reference frame != oracle frame: {diff}"
    diff = rc.first_difference({k[3:]: v for k, v in g.items() if k.startswith("in.")}, rc.frame_inputs(name))
    assert diff is None, f"{name}: recorded reference packet / camera != the project's: {diff}"


def test_build_without_the_reference_or_the_recipe_is_quiet(monkeypatch, tmp_path):
    """build_all()'s build_ref step returns None, and writes nothing, where the reference directory is not there and
    where the package is used with an oracle/ directory that has no ref/ recipe."""
    from iqpt import _build
    monkeypatch.setenv("IQPT_REFERENCE", str(tmp_path / "no_reference"))
    assert _build.build_ref() is None
    monkeypatch.delenv("IQPT_REFERENCE")
    monkeypatch.setattr(_build, "ORACLE_DIR", tmp_path)
    assert _build.build_ref() is None
    assert list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("name", list(rc.FRAMES))
def test_live_reference_matches_its_recording(name):
    """A stale fixture fails."""
    ref = live("b")
    g = golden(name)
    got = dict(rc.ref_frame(name, ref))
    got.update({f"in.{k}": v for k, v in rc.ref_frame_inputs(name, ref).items()})
    diff = rc.first_difference(g, got)
    assert diff is None, f"ref_{name}.npz is stale: {diff}"
