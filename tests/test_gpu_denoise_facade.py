"""The renderer facade's denoise block (csrc/raster/rasterizer.hpp: renderer_options::denoise, iqpt::denoiser in
csrc/denoise/denoiser.hpp) and the CLI's --denoise, on the GPU."""
import json
import subprocess

import numpy as np
import pytest

from iqpt import Denoiser, PathTracer, Rasterizer, Scene, _build, align_camera, make_camera

pytestmark = pytest.mark.gpu


def ppm_pixels(path, w, h):
    data = path.read_bytes()
    head = f"P6\n{w} {h}\n255\n".encode()
    assert data.startswith(head) and len(data) == len(head) + w * h * 3
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 3)


def both_frames(preset, w, h, launches, spp, depth, params=None):
    """(the path tracer's bgra, the Denoiser's bgra) [H,W,4] after `launches` launches of `spp` samples."""
    sc = Scene()
    sc.add_preset(preset)
    cam = make_camera(w, h)
    with PathTracer(w, h, max_depth=depth) as pt, Rasterizer(w, h) as r, Denoiser(w, h) as d:
        pt.set_camera(align_camera(cam))                  # what the renderer and the CLI give it
        pt.upload_packet(sc.build_packet())
        for _ in range(launches):
            pt.render(spp)
        r.set_camera(cam)
        r.upload_scene(sc)
        if params is not None:
            d.set_params(*params)
        d.frame(pt, r)
        return pt.read()[1].reshape(h, w, 4), d.read()[1]


def test_renderer_denoise_block(require_gpu, tmp_path):
    exe = _build.DENOISE_FACADE_TEST_PATH
    assert exe.exists()
    plain, den = tmp_path / "plain.ppm", tmp_path / "denoised.ppm"
    res = subprocess.run([str(exe), str(plain), str(den)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["ok"] is True and out["plain_ppm_equal"] is True and out["accumulator_equal"] is True
    # the denoised PPM is Denoiser's BGRA of the same accumulation and G-buffer
    _, want = both_frames("cornell_lit", 96, 54, out["launches"], 1, 8, params=(3, 5, 1024.0, 2.0))
    assert np.array_equal(ppm_pixels(den, 96, 54), want[:, :, 2::-1])
    assert out["pixels_changed"] > 96 * 54 // 4


def test_cli_writes_both_frames(require_gpu, tmp_path):
    noisy, clean = tmp_path / "noisy.ppm", tmp_path / "clean.ppm"
    res = subprocess.run([str(_build.CLI_PATH), "--preset", "cornell_lit", "--width", "64", "--height", "36", "--spp", "2",
                          "--launches", "2", "--max-depth", "8", "--denoise", "--denoise-levels", "2", "--out", str(noisy),
                          "--out-denoised", str(clean)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert info["frames"] == 4 and info["denoise_levels"] == 2 and info["denoise_runs"] == 3
    from iqpt.denoise import default_params
    p = default_params()
    raw, want = both_frames("cornell_lit", 64, 36, 2, 2, 8,
                            params=(2, p["normal_squarings"], p["depth_sharpness"], p["colour_sharpness"]))
    assert np.array_equal(ppm_pixels(noisy, 64, 36), raw[:, :, 2::-1])
    assert np.array_equal(ppm_pixels(clean, 64, 36), want[:, :, 2::-1])
    assert not np.array_equal(ppm_pixels(noisy, 64, 36), ppm_pixels(clean, 64, 36))
    # --denoise needs its output path
    res = subprocess.run([str(_build.CLI_PATH), "--denoise", "--out", str(noisy)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2
