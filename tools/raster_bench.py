"""The rasterized preview against the only preview the path tracer offers, one 1-spp launch.

For each scene at one frame size: the median over --draws iqpt_raster_draw calls after warm-up (the library's
own HIP events, first kernel to last, and the per-stage split), the host wall time of a draw that ends in a
synchronise, and next to them the median render-kernel time and wall time of one 1-spp iqpt_render launch of the
same scene, frame and camera in the same process. Needs the GPU; prints one JSON line per scene and, with
--out, writes them to a file.

    python tools/raster_bench.py --width 1920 --height 1080 --samples 4 --draws 30
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

STAGES = ("vertex", "setup", "bin", "sort", "tiles")


def median(v):
    return float(statistics.median(v))


def bench_raster(preset, w, h, samples, warmup, draws):
    sc = Scene()
    sc.add_preset(preset)
    with iqpt.Rasterizer(w, h, samples=samples) as r:
        r.set_camera(make_camera(w, h))
        t0 = time.perf_counter()
        r.upload_scene(sc)
        r.sync()
        upload_ms = 1e3 * (time.perf_counter() - t0)
        r.draw()
        r.sync()
        first_vertex = r.stage_time()[0]          # the vertex stage runs once per camera or scene change
        r.time()
        for _ in range(warmup):
            r.draw()
        r.sync()
        r.time()
        ev, wall, stages = [], [], []
        for _ in range(draws):
            t1 = time.perf_counter()
            r.draw()
            r.sync()
            wall.append(1e3 * (time.perf_counter() - t1))
            stages.append(r.stage_time())
            ms, n = r.time()
            assert n == 1
            ev.append(ms)
        return {"draw_ms": median(ev), "draw_ms_min": min(ev), "draw_ms_max": max(ev), "draw_wall_ms": median(wall),
                "stage_ms": {k: median([s[i] for s in stages]) for i, k in enumerate(STAGES)},
                "vertex_ms_first_draw": first_vertex, "upload_ms": upload_ms, **r.stats()}


def bench_path_tracer(preset, w, h, max_depth, warmup, launches):
    sc = Scene()
    sc.add_preset(preset)
    pk = sc.build_packet()
    pt = iqpt.PathTracer(w, h, max_depth=max_depth)
    pt.set_camera(make_camera(w, h))
    pt.upload_packet(pk)
    pt.prepare()
    for _ in range(warmup):
        pt.render(1)
    pt.sync()
    pt.kernel_time()
    ker, wall = [], []
    for _ in range(launches):
        t1 = time.perf_counter()
        pt.render(1)
        pt.sync()
        wall.append(1e3 * (time.perf_counter() - t1))
        ms, n = pt.kernel_time()
        assert n == 1
        ker.append(ms)
    pt.close()
    return {"pt_1spp_kernel_ms": median(ker), "pt_1spp_kernel_ms_min": min(ker), "pt_1spp_kernel_ms_max": max(ker),
            "pt_1spp_wall_ms": median(wall), "pt_max_depth": max_depth}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="cornell,mesh10k,mixed")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--draws", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.draws < 20:
        ap.error("--draws must be at least 20")
    lines = []
    for preset in a.scenes.split(","):
        res = {"scene": preset, "width": a.width, "height": a.height, "samples": a.samples, "draws": a.draws}
        res.update(bench_raster(preset, a.width, a.height, a.samples, a.warmup, a.draws))
        res.update(bench_path_tracer(preset, a.width, a.height, a.max_depth, a.warmup, a.draws))
        res["pt_over_raster"] = res["pt_1spp_kernel_ms"] / res["draw_ms"]
        res["pt_over_raster_wall"] = res["pt_1spp_wall_ms"] / res["draw_wall_ms"]
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
