"""The HIP path tracer against the reference's own frames (tests/golden/ref_<frame>.npz: render_kernel of the
reference's source run as a host loop, flavour B, recorded by tests/golden/make_ref_golden.py): lin_fb, BGRA bytes and
read_rng() of every pixel, bit for bit. Reads only the fixtures; neither the reference nor the oracle runs here."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ref_cases as rc
from iqpt import PathTracer, _lib, make_camera

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"


def render(name, plain=False):
    scene, w, h, steps, depth = rc.FRAMES[name]
    sc = rc.project_scene(scene)
    pk = sc.build_packet()
    pt = PathTracer(w, h, max_depth=depth)
    if plain:   # the plain kernel: certain-pixel path and split off, as tests/test_gpu_certain.py switches them
        pt.set_split(_lib.SPLIT_OFF)
        lib = _lib.load()
        lib.iqpt_debug_set_certain.argtypes = [C.c_void_p, C.c_int]
        _lib.check(lib.iqpt_debug_set_certain(pt._h, 0), "iqpt_debug_set_certain")
    pt.set_camera(make_camera(w, h))
    pt.upload_packet(pk)
    for s in steps:
        if s == "reset":
            pt.reset()
        else:
            pt.render(s)
    lin, bgra = pt.read()
    out = {"lin": lin, "bgra": bgra, "states": pt.read_rng()}
    pt.close()
    return out


def check(name, got):
    with np.load(GOLDEN / f"ref_{name}.npz", allow_pickle=False) as g:
        want = {k: g[k] for k in ("lin", "bgra", "states")}
    diff = rc.first_difference(want, got)
    assert diff is None, f"{name}: reference frame != HIP frame: {diff}"


@pytest.mark.parametrize("name", list(rc.FRAMES))
def test_gpu_matches_the_reference_frame(require_gpu, name):
    """Through whatever path the runtime picks."""
    check(name, render(name))


def test_gpu_plain_kernel_matches_the_reference_cornell(require_gpu):
    check("cornell", render("cornell", plain=True))
