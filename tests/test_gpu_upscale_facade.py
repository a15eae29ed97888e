"""The C++ facade of guided upsampling (iqpt::upscaler in csrc/upscale/upscaler.hpp) and the CLI's --upscale, on the
GPU, against the numpy reference (tests/upscale_ref.py)."""
import json
import subprocess

import numpy as np
import pytest

import upscale_ref as ur
from iqpt import PathTracer, Rasterizer, Scene, _build, align_camera, make_camera

pytestmark = pytest.mark.gpu


def ppm_pixels(path, w, h):
    data = path.read_bytes()
    head = f"P6\n{w} {h}\n255\n".encode()
    assert data.startswith(head) and len(data) == len(head) + w * h * 3
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 3)


def reference_frames(preset, W, H, f, launches, spp, depth):
    """(the lo path tracer's bgra [h,w,4], the reference's upsampled bgra [H,W,4], its class counts) after `launches`
    launches of `spp` samples, under the default parameters."""
    w, h = W // f, H // f
    sc = Scene()
    sc.add_preset(preset)
    with PathTracer(w, h, max_depth=depth) as pt, Rasterizer(w, h) as r_lo, Rasterizer(W, H) as r_hi:
        pt.set_camera(align_camera(make_camera(w, h)))    # what the facade test and the CLI give it
        pt.upload_packet(sc.build_packet())
        for _ in range(launches):
            pt.render(spp)
        acc, lo_bgra = pt.read()
        guides = []
        for r, cam in ((r_lo, make_camera(w, h)), (r_hi, make_camera(W, H))):
            r.set_camera(cam)
            r.upload_scene(sc)
            guides += list(r.gbuffer())
    _, want_bgra, counts = ur.upscale(acc, *guides, f, 5, 1024.0)
    return lo_bgra.reshape(h, w, 4), want_bgra, counts


def test_upscaler_facade(require_gpu, tmp_path):
    exe = _build.UPSCALE_FACADE_TEST_PATH
    assert exe.exists()
    lo, up = tmp_path / "lo.ppm", tmp_path / "up.ppm"
    res = subprocess.run([str(exe), str(lo), str(up)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["ok"] is True and out["accumulator_equal"] is True
    W, H, f = out["width"], out["height"], out["factor"]
    assert (W, H, f) == (96, 54, 2)
    lo_bgra, want, counts = reference_frames("cornell_lit", W, H, f, 1, out["spp"], 8)
    assert np.array_equal(ppm_pixels(lo, W // f, H // f), lo_bgra[:, :, 2::-1])
    assert np.array_equal(ppm_pixels(up, W, H), want[:, :, 2::-1])
    assert (out["guided"], out["widened"], out["unguided"]) == counts


def test_cli_upscale(require_gpu, tmp_path):
    lo, up = tmp_path / "lo.ppm", tmp_path / "up.ppm"
    base = [str(_build.CLI_PATH), "--preset", "cornell_lit", "--width", "63", "--height", "36", "--spp", "2", "--launches", "2",
            "--max-depth", "8", "--out", str(lo)]
    res = subprocess.run(base + ["--upscale", "3", "--out-upscaled", str(up)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert info["upscale"] == 3 and (info["lo_width"], info["lo_height"]) == (21, 12) and info["frames"] == 4
    assert info["upscale_ms"] > 0.0
    lo_bgra, want, counts = reference_frames("cornell_lit", 63, 36, 3, 2, 2, 8)
    assert np.array_equal(ppm_pixels(lo, 21, 12), lo_bgra[:, :, 2::-1])
    assert np.array_equal(ppm_pixels(up, 63, 36), want[:, :, 2::-1])
    assert (info["guided"], info["widened"], info["unguided"]) == counts and sum(counts) == 63 * 36

    def status(*extra):
        return subprocess.run(base + list(extra), capture_output=True, text=True, timeout=60).returncode

    # refused before anything is created
    assert status("--upscale", "3") == 2                                                # no --out-upscaled
    assert status("--out-upscaled", str(up)) == 2                                       # no --upscale
    assert status("--upscale", "2", "--out-upscaled", str(up)) == 2                     # 63 is not divisible by 2
    assert status("--upscale", "4", "--out-upscaled", str(up)) == 2                     # nor by 4
    assert status("--upscale", "5", "--out-upscaled", str(up)) == 2                     # no such factor
    assert status("--upscale", "1", "--out-upscaled", str(up)) == 2
    assert status("--upscale", "3", "--out-upscaled", str(up), "--engine", "raster") == 2
    assert status("--upscale", "3", "--out-upscaled", str(up), "--denoise", "--out-denoised", str(tmp_path / "d.ppm")) == 2
    assert status("--upscale", "3", "--out-upscaled", str(up), "--temporal", "--out-temporal", str(tmp_path / "t.ppm")) == 2
    assert status("--upscale", "3", "--out-upscaled", str(up), "--svgf", "--out-svgf", str(tmp_path / "s.ppm")) == 2
