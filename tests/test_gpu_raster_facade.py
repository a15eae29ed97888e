"""The two-engine C++ facade (csrc/raster/rasterizer.hpp: iqpt::rasterizer, iqpt::renderer) and the CLI's
--engine raster, on the GPU."""
import json
import subprocess

import numpy as np
import pytest

from iqpt import Rasterizer, Scene, _build, make_camera

pytestmark = pytest.mark.gpu


def raster_frame(preset, w, h, samples):
    sc = Scene()
    sc.add_preset(preset)
    with Rasterizer(w, h, samples=samples) as r:
        r.set_camera(make_camera(w, h))
        r.upload_scene(sc)
        r.draw()
        return r.read()


def ppm_pixels(path, w, h):
    data = path.read_bytes()
    head = f"P6\n{w} {h}\n255\n".encode()
    assert data.startswith(head) and len(data) == len(head) + w * h * 3
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 3)


def fnv1a(raw: bytes) -> int:
    h = 1469598103934665603
    for c in raw:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_renderer_toggles_engines_and_leaves_the_accumulation_alone(require_gpu, tmp_path):
    exe = _build.RASTER_FACADE_TEST_PATH
    assert exe.exists()
    ppm = tmp_path / "raster_facade.ppm"
    res = subprocess.run([str(exe), str(ppm)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["ok"] is True and out["accumulator_equal"] is True
    # the frame the facade's rasterizer showed is the C ABI's frame of the same scene and camera
    bgra = raster_frame("cornell", 96, 64, 4)
    assert out["raster_fnv1a"] == f"{fnv1a(bgra.tobytes()):016x}"
    assert out["raster_nonclear"] == int(np.sum(np.any(bgra != np.array([255, 214, 158, 255], np.uint8), axis=2)))
    assert np.array_equal(ppm_pixels(ppm, 96, 64), bgra[:, :, 2::-1])


@pytest.mark.parametrize("samples", [1, 4])
def test_cli_raster_preview(require_gpu, tmp_path, samples):
    out = tmp_path / "preview.ppm"
    res = subprocess.run([str(_build.CLI_PATH), "--engine", "raster", "--preset", "app_default", "--width", "64",
                          "--height", "36", "--samples", str(samples), "--out", str(out)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert info["engine"] == "raster" and info["draws"] == 1 and info["triangles"] == 12 + 2 * 16128
    assert np.array_equal(ppm_pixels(out, 64, 36), raster_frame("app_default", 64, 36, samples)[:, :, 2::-1])
