"""The renderer facade's svgf block (csrc/raster/rasterizer.hpp: renderer_options::svgf, iqpt::svgf in
csrc/svgf/svgf.hpp) and the CLI's --svgf, on the GPU."""
import json
import subprocess

import numpy as np
import pytest

from iqpt import PathTracer, Rasterizer, Scene, Svgf, _build, align_camera, make_camera

pytestmark = pytest.mark.gpu


def ppm_pixels(path, w, h):
    data = path.read_bytes()
    head = f"P6\n{w} {h}\n255\n".encode()
    assert data.startswith(head) and len(data) == len(head) + w * h * 3
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 3)


def sequence(preset, w, h, depth, views, params):
    """The frames of a sequence of views, each (camera, launches, spp): the path tracer is reset and the svgf view
    begun from the rasterizer's G-buffer at every view. Returns per view (path tracer bgra, svgf bgra, stats), the
    frames [H,W,4]."""
    sc = Scene()
    sc.add_preset(preset)
    out = []
    with PathTracer(w, h, max_depth=depth) as pt, Rasterizer(w, h) as r, Svgf(w, h) as s:
        s.set_params(*params)
        pt.upload_packet(sc.build_packet())
        r.upload_scene(sc)
        for cam, launches, spp in views:
            pt.set_camera(align_camera(cam))              # what the renderer and the CLI give it
            pt.reset()
            r.set_camera(cam)
            s.begin_view_raster(r)
            for _ in range(launches):
                pt.render(spp)
            s.resolve_ctx(pt)
            out.append((pt.read()[1].reshape(h, w, 4), s.read()[1], s.stats()))
    return out


def test_renderer_svgf_block(require_gpu, tmp_path):
    exe = _build.SVGF_FACADE_TEST_PATH
    assert exe.exists()
    paths = [tmp_path / n for n in ("plain.ppm", "svgf_a.ppm", "svgf_b.ppm")]
    res = subprocess.run([str(exe), *map(str, paths)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["ok"] is True and out["plain_ppm_equal"] is True and out["accumulator_equal"] is True
    w, h = 96, 54
    # the PPMs are what Svgf makes of the same two cameras with the tool's parameters
    views = [(make_camera(w, h), out["launches_a"], 1), (make_camera(w, h, fovh=50.0), out["launches_b"], 1)]
    (_, want_a, stats_a), (_, want_b, stats_b) = sequence("cornell_lit", w, h, 8, views,
                                                          (0.9, 0.01, 256, 2, 3, 5, 1024.0, 4.0, 1e-6))
    assert stats_a == (stats_a[0], 0, out["spatial_a"]) and stats_a[0] == out["spatial_a"]
    assert stats_b == (out["guided_b"], out["valid_b"], out["spatial_b"]) and 0 < out["spatial_b"] < out["guided_b"] // 2
    assert np.array_equal(ppm_pixels(paths[1], w, h), want_a[:, :, 2::-1])
    assert np.array_equal(ppm_pixels(paths[2], w, h), want_b[:, :, 2::-1])
    assert not np.array_equal(want_a, want_b)


def test_cli_svgf(require_gpu, tmp_path):
    last, filtered, kept = tmp_path / "last.ppm", tmp_path / "filtered.ppm", tmp_path / "kept.ppm"
    w, h, k, step = 64, 36, 3, 0.05
    base = [str(_build.CLI_PATH), "--preset", "cornell_lit", "--width", str(w), "--height", str(h), "--spp", "2",
            "--max-depth", "8", "--views", str(k), "--step-x", str(step), "--out", str(last)]
    res = subprocess.run([*base, "--svgf", "--out-svgf", str(filtered)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert info["views"] == k and info["frames"] == 2
    from iqpt.svgf import PARAM_NAMES, default_params
    p = default_params()
    views = [(make_camera(w, h, position=[np.float32(step) * np.float32(i), 0.5, -3.0, 0.0]), 1, 2) for i in range(k)]
    raw, want, stats = sequence("cornell_lit", w, h, 8, views, [p[name] for name in PARAM_NAMES])[-1]
    assert (info["guided"], info["valid"], info["spatial"]) == stats     # whatever the defaults are: they are read above
    assert np.array_equal(ppm_pixels(last, w, h), raw[:, :, 2::-1])
    assert np.array_equal(ppm_pixels(filtered, w, h), want[:, :, 2::-1])
    assert not np.array_equal(ppm_pixels(last, w, h), ppm_pixels(filtered, w, h))
    # with --temporal as well: the same filtered frame, and the temporal frame next to it
    res = subprocess.run([*base, "--svgf", "--out-svgf", str(filtered), "--temporal", "--out-temporal", str(kept)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = [json.loads(line) for line in res.stdout.strip().splitlines()[-2:]]
    assert "out_svgf" in lines[0] and "out_temporal" in lines[1]
    assert np.array_equal(ppm_pixels(filtered, w, h), want[:, :, 2::-1]) and kept.exists()
    # --svgf needs its output path; --views and --step-x need --temporal or --svgf
    for args in (["--svgf", "--out", str(last)], ["--views", "2", "--out", str(last)],
                 ["--step-x", "0.1", "--out", str(last)], ["--out-svgf", str(filtered), "--out", str(last)],
                 ["--svgf", "--denoise", "--out-denoised", str(kept), "--out-svgf", str(filtered)]):
        assert subprocess.run([str(_build.CLI_PATH), *args], capture_output=True, text=True, timeout=60).returncode == 2
