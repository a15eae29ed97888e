"""The motion view kernel's two forms next to temporal reprojection's view kernel, in one process.

C2's scene (the Cornell box) at 1920x1080: the rasterizer's G-buffers of two cameras (0.05 along x and a yaw apart)
stay on the device; every round begins one view per object, each object gathering from its own last result, and
resolves a fixed colour plane into it. The objects are iqpt.Temporal (libiqpt.so's iqt_view_kernel: the code the
parent commit has), iqpt.Motion of libiqpt_motion.so (every lane gathers its entry) and iqpt.Motion of
libiqpt_motion_uniform.so (wave-uniform entry loads, the gather as the fallback); within a round they run one after the other, and the two
libraries swap places from round to round. Two tables: every draw static, every draw moved (by a small translation).
Reported per object and table: the median, minimum and maximum over --runs rounds after --warmup rounds of the
library's own HIP events around the view kernel, and the four counts. Needs the GPU; prints one JSON line and, with
--out, writes it to a file.

    python tools/motion_bench.py --out profiles/r11/motion_ab_c2.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "path-tracer-and-rasterizer-engine_amd"))
import iqpt  # noqa: E402
from iqpt import _build  # noqa: E402
from iqpt.motion import identity_table  # noqa: E402
from iqpt.scene import CONFIGS, Scene, make_camera  # noqa: E402

VIEW_BYTES = 104        # compulsory bytes per pixel of either view kernel (tools/temporal_bench.py)


def summary(v):
    return {"median_ms": float(statistics.median(v)), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    cfg = CONFIGS["c2"]
    w, h = cfg.width, cfg.height
    sc = Scene()
    sc.add_preset(cfg.preset)
    ndraws = len(sc.draw_list())
    cams = [make_camera(w, h, position=[0.05 * k, 0.5, -3.0, 0.0], forward=[-0.02 * k, -0.5, 3.0, 0.0]) for k in (0, 1)]
    static = identity_table(ndraws)
    moved = identity_table(ndraws)
    moved["moved"] = 1
    moved["back"][:, 12] = 0.01                 # every model was 0.01 further along x
    tables = {"static": static, "moved": moved}

    planes = []
    with iqpt.Rasterizer(w, h, samples=1) as r:
        r.upload_scene(sc)
        for cam in cams:
            r.set_camera(cam)
            nz, ids = r.gbuffer()
            planes.append((torch.from_numpy(nz.copy()).cuda(), torch.from_numpy(ids.view(np.int32).copy()).cuda()))
    colour = torch.rand((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    result = {"config": "c2", "scene": cfg.preset, "width": w, "height": h, "draws": ndraws, "runs": a.runs,
              "warmup": a.warmup, "kernel_source_sha16": _build.kernel_source_sha16(), "view_bytes_per_pixel": VIEW_BYTES,
              "tables": {}}
    for tname, table in tables.items():
        with iqpt.Temporal(w, h) as t, iqpt.Motion(w, h) as mg, iqpt.Motion(w, h, lib=_build.MOTION_UNIFORM_LIB_PATH) as mu:
            objs = {"temporal": t, "motion_uniform": mu, "motion_gather": mg}
            times = {k: [] for k in objs}
            counts = {}
            for k in range(a.warmup + a.runs):
                cam, (nz, ids) = cams[k & 1], planes[k & 1]
                order = ["temporal", "motion_uniform", "motion_gather"] if k & 2 == 0 else \
                    ["temporal", "motion_gather", "motion_uniform"]
                for name in order:
                    o = objs[name]
                    if name == "temporal":
                        o.begin_view_device(cam, nz.data_ptr(), ids.data_ptr())
                    else:
                        o.begin_view_device(cam, nz.data_ptr(), ids.data_ptr(), motion=table)
                    o.resolve_device(colour.data_ptr(), 1)
                    o.sync()
                    vms, nv, _, _ = o.time()
                    assert nv == 1
                    if k >= a.warmup:
                        times[name].append(vms)
                    counts[name] = list(o.stats())
            assert counts["motion_uniform"] == counts["motion_gather"]
            entry = {name: dict(summary(v), gbps=VIEW_BYTES * w * h / (1e6 * statistics.median(v)), counts=counts[name])
                     for name, v in times.items()}
            for name in ("motion_uniform", "motion_gather"):
                entry[name]["vs_temporal"] = entry[name]["median_ms"] / entry["temporal"]["median_ms"]
            spread = max(entry[n]["max_ms"] - entry[n]["min_ms"] for n in ("motion_uniform", "motion_gather"))
            entry["uniform_minus_gather_ms"] = entry["motion_uniform"]["median_ms"] - entry["motion_gather"]["median_ms"]
            entry["spread_ms"] = spread
            entry["difference_outside_three_spreads"] = abs(entry["uniform_minus_gather_ms"]) > 3 * spread
            result["tables"][tname] = entry
    line = json.dumps(result)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
