"""The renderer facade's temporal block (csrc/raster/rasterizer.hpp: renderer_options::temporal, iqpt::temporal in
csrc/temporal/temporal.hpp) and the CLI's --temporal, on the GPU."""
import json
import subprocess

import numpy as np
import pytest

from iqpt import Denoiser, PathTracer, Rasterizer, Scene, Temporal, _build, align_camera, make_camera

pytestmark = pytest.mark.gpu


def ppm_pixels(path, w, h):
    data = path.read_bytes()
    head = f"P6\n{w} {h}\n255\n".encode()
    assert data.startswith(head) and len(data) == len(head) + w * h * 3
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 3)


def sequence(preset, w, h, depth, views, params, denoise=None):
    """The frames of a sequence of views, each (camera, launches, spp): the path tracer is reset and the temporal
    view begun from the rasterizer's G-buffer at every view. Returns per view (path tracer bgra, temporal bgra,
    denoised bgra or None, (guided, valid)), each [H,W,4]."""
    sc = Scene()
    sc.add_preset(preset)
    out = []
    with PathTracer(w, h, max_depth=depth) as pt, Rasterizer(w, h) as r, Temporal(w, h) as t, Denoiser(w, h) as d:
        t.set_params(*params)
        pt.upload_packet(sc.build_packet())
        r.upload_scene(sc)
        for cam, launches, spp in views:
            pt.set_camera(align_camera(cam))              # what the renderer and the CLI give it
            pt.reset()
            r.set_camera(cam)
            t.begin_view_raster(r)
            for _ in range(launches):
                pt.render(spp)
            t.resolve_ctx(pt)
            den = None
            if denoise is not None:
                d.set_params(*denoise)
                d.set_guides_device(*r.gbuffer_device())
                t.sync()
                d.run_device(t.output_device())
                den = d.read()[1]
            out.append((pt.read()[1].reshape(h, w, 4), t.read()[1], den, t.stats()))
    return out


def test_renderer_temporal_block(require_gpu, tmp_path):
    exe = _build.TEMPORAL_FACADE_TEST_PATH
    assert exe.exists()
    paths = [tmp_path / n for n in ("plain.ppm", "temporal_a.ppm", "temporal_b.ppm", "denoised_b.ppm")]
    res = subprocess.run([str(exe), *map(str, paths)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["ok"] is True and out["plain_ppm_equal"] is True and out["accumulator_equal"] is True
    w, h = 96, 54
    assert out["pixels_carried"] > w * h // 4
    # the PPMs are what Temporal and Denoiser make of the same two cameras
    views = [(make_camera(w, h), out["launches_a"], 1), (make_camera(w, h, fovh=50.0), out["launches_b"], 1)]
    (_, want_a, _, _), (_, want_b, den_b, (guided, valid)) = sequence("cornell_lit", w, h, 8, views, (0.9, 0.01, 256),
                                                                      denoise=(2, 5, 1024.0, 1.0))
    assert valid > guided // 2
    assert np.array_equal(ppm_pixels(paths[1], w, h), want_a[:, :, 2::-1])
    assert np.array_equal(ppm_pixels(paths[2], w, h), want_b[:, :, 2::-1])
    assert np.array_equal(ppm_pixels(paths[3], w, h), den_b[:, :, 2::-1])
    assert not np.array_equal(want_a, want_b)


def test_cli_temporal(require_gpu, tmp_path):
    last, kept = tmp_path / "last.ppm", tmp_path / "kept.ppm"
    w, h, k, step = 64, 36, 3, 0.05
    res = subprocess.run([str(_build.CLI_PATH), "--preset", "cornell_lit", "--width", str(w), "--height", str(h), "--spp", "2",
                          "--max-depth", "8", "--temporal", "--views", str(k), "--step-x", str(step), "--out", str(last),
                          "--out-temporal", str(kept)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert info["views"] == k and info["frames"] == 2
    from iqpt.temporal import default_params
    p = default_params()
    views = [(make_camera(w, h, position=[np.float32(step) * np.float32(i), 0.5, -3.0, 0.0]), 1, 2) for i in range(k)]
    frames = sequence("cornell_lit", w, h, 8, views, (p["normal_min"], p["plane_tolerance"], p["max_history"]))
    raw, want, _, (guided, valid) = frames[-1]
    assert (info["guided"], info["valid"]) == (guided, valid)      # whatever the defaults are: they are read above
    assert np.array_equal(ppm_pixels(last, w, h), raw[:, :, 2::-1])
    assert np.array_equal(ppm_pixels(kept, w, h), want[:, :, 2::-1])
    assert not np.array_equal(ppm_pixels(last, w, h), ppm_pixels(kept, w, h))
    # --temporal needs its output path, and its options need --temporal
    for args in (["--temporal", "--out", str(last)], ["--views", "2", "--out", str(last)],
                 ["--temporal", "--denoise", "--out-denoised", str(kept), "--out-temporal", str(kept)]):
        assert subprocess.run([str(_build.CLI_PATH), *args], capture_output=True, text=True, timeout=60).returncode == 2
