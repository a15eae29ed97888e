"""What temporal reprojection costs, next to the two engines it sits between.

For each scene at one frame size, in one process: the camera alternates between two views of the 8-view test
sequence (0.05 along x and a yaw per view), and every iteration sets it on the rasterizer, takes the G-buffer, begins
a temporal view (the view kernel gathers its history from the other view's result) and resolves the path tracer's
1-spp accumulator into it. Reported are the medians over --runs iterations after warm-up of the library's own HIP
events: the view kernel and the resolve kernel, each in ms and in GB/s over its compulsory bytes (104 and 52 per
pixel), the G-buffer pass, and the render-kernel time of one 1-spp iqpt_render launch of the same scene as the
yardstick: what carrying the history costs in samples. Needs the GPU; prints one JSON line per scene and, with --out,
writes them to a file.

    python tools/temporal_bench.py --width 1920 --height 1080 --scenes cornell_lit,mixed --runs 30
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "path-tracer-and-rasterizer-engine_amd"))
import iqpt  # noqa: E402
from iqpt.scene import Scene, make_camera  # noqa: E402
from iqpt.temporal import default_params  # noqa: E402

VIEW_BYTES = 104        # coalesced: normal_z 16 + id 4 in, pos 16 + hist 16 out; gathered: out 16, pos 16, normal_z 16, id 4
RESOLVE_BYTES = 52      # hist 16 + colour 16 in, out 16 + bgra 4 out


def median(v):
    return float(statistics.median(v))


def bench(preset, w, h, max_depth, params, warmup, runs):
    sc = Scene()
    sc.add_preset(preset)
    cams = [make_camera(w, h, position=[0.05 * k, 0.5, -3.0, 0.0], forward=[-0.02 * k, -0.5, 3.0, 0.0]) for k in (0, 1)]
    with iqpt.PathTracer(w, h, max_depth=max_depth) as pt, iqpt.Rasterizer(w, h, samples=1) as r, \
            iqpt.Temporal(w, h) as t:
        pt.set_camera(cams[0])
        pt.upload_packet(sc.build_packet())
        pt.prepare()
        r.upload_scene(sc)
        t.set_params(*params)

        # the yardstick: one 1-spp launch
        for _ in range(warmup):
            pt.render(1)
        pt.sync()
        pt.kernel_time()
        ker = []
        for _ in range(runs):
            pt.render(1)
            pt.sync()
            ker.append(pt.kernel_time()[0])
        pt.reset()
        pt.render(1)
        pt.sync()

        view, resolve, guide, wall, valid = [], [], [], [], []
        for k in range(warmup + runs):
            r.set_camera(cams[k & 1])
            r.gbuffer_device()
            gms, gn = r.gbuffer_time()
            t0 = time.perf_counter()
            t.begin_view_raster(r)
            t.resolve_ctx(pt)
            t.sync()
            ms = 1e3 * (time.perf_counter() - t0)
            vms, nv, rms, nr = t.time()
            assert gn == 1 and nv == 1 and nr == 1
            if k >= warmup:
                view.append(vms)
                resolve.append(rms)
                guide.append(gms)
                wall.append(ms)
                valid.append(t.stats())
    npix = w * h
    guided, val = valid[-1]
    return {"scene": preset, "width": w, "height": h, "normal_min": params[0], "plane_tolerance": params[1],
            "max_history": params[2], "runs": runs, "guided_fraction": guided / npix, "valid_of_guided": val / max(guided, 1),
            "view_ms": median(view), "view_ms_min": min(view), "view_ms_max": max(view),
            "view_gbps": VIEW_BYTES * npix / (1e6 * median(view)),
            "resolve_ms": median(resolve), "resolve_ms_min": min(resolve), "resolve_ms_max": max(resolve),
            "resolve_gbps": RESOLVE_BYTES * npix / (1e6 * median(resolve)),
            "view_and_resolve_call_wall_ms": median(wall), "gbuffer_ms": median(guide),
            "pt_1spp_kernel_ms": median(ker), "temporal_in_samples": (median(view) + median(resolve)) / median(ker)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    dp = default_params()
    ap.add_argument("--scenes", default="cornell_lit,mixed")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--normal-min", type=float, default=dp["normal_min"])
    ap.add_argument("--plane-tolerance", type=float, default=dp["plane_tolerance"])
    ap.add_argument("--max-history", type=int, default=dp["max_history"])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    params = (a.normal_min, a.plane_tolerance, a.max_history)
    lines = []
    for preset in a.scenes.split(","):
        line = json.dumps(bench(preset, a.width, a.height, a.max_depth, params, a.warmup, a.runs))
        print(line, flush=True)
        lines.append(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
