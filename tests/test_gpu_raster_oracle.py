"""Both engines see the same geometry through the same camera: the rasterizer's silhouette of a rotated cube
against the path tracer's CPU oracle (oracle/iqpt_oracle.c), the one check that does not rest on
tests/raster_ref.py."""
import numpy as np
import pytest

import iqpt
import oracle
import raster_ref as rr
from iqpt import Rasterizer, Scene, make_camera

pytestmark = pytest.mark.gpu

W, H, SPP = 96, 54, 8
COLOUR = [0.25, 0.5, 0.75]


def cube_scene(with_cube=True):
    sc = Scene()
    sc.add_mesh_cube("cube")
    if with_cube:
        sc.add_model("box", "cube", scale=1.1, rotation=[0.5, 0.7, 0.2, 0.0], translation=[0.1, 0.45, 0.0, 0.0])
        sc.set_model_material("box", sc.add_material(iqpt.MAT_EMISSIVE, COLOUR, 1.0))
    return sc


def oracle_classes():
    """(inside, outside, mixed) masks [H,W] from the oracle's accumulator at depth 1, 8 spp."""
    cam = make_camera(W, H)
    frames = []
    for with_cube in (True, False):
        sc = cube_scene(with_cube)
        fr = oracle.OracleFrame(W, H, max_depth=1)
        fr.render(sc.build_packet(), cam, SPP)
        frames.append(fr.lin[:, :3].reshape(H, W, 3).copy())
    lit, empty = frames
    inside = np.all(lit == np.array(COLOUR, np.float32), axis=2)
    outside = np.all(lit.view(np.uint32) == empty.view(np.uint32), axis=2) & ~inside
    return inside, outside, ~(inside | outside)


def dilate(mask):
    """Chebyshev distance <= 1."""
    p = np.pad(mask, 1)
    out = np.zeros_like(mask)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + mask.shape[0], dx:dx + mask.shape[1]]
    return out


def test_silhouette_matches_the_path_tracers_oracle(require_gpu):
    inside, outside, mixed = oracle_classes()
    left_out = dilate(mixed)
    share = float(np.mean(left_out))
    print(f"inside {int(inside.sum())}, outside {int(outside.sum())}, mixed {int(mixed.sum())}, left out {share:.3f}")
    assert share <= 0.25, "the oracle's own frame: too much of it is silhouette"
    assert inside.sum() > 300 and outside.sum() > 1000

    sc = cube_scene()
    with Rasterizer(W, H, samples=4) as r:
        r.set_camera(make_camera(W, H))
        r.upload_scene(sc)
        r.draw()
        bgra = r.read()
    clear = np.all(bgra == rr.CLEAR_BGRA, axis=2)
    check = ~left_out
    assert not np.any(clear & inside & check), f"{int(np.sum(clear & inside & check))} inside pixels are clear"
    assert not np.any(~clear & outside & check), f"{int(np.sum(~clear & outside & check))} outside pixels are drawn"
