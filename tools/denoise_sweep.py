"""Choose the denoiser's defaults: RMSE of the filtered low-sample frame against the GPU path
tracer's own many-sample frame of the same seed, over a grid of parameters.

For each scene, one context renders 1, 4, 16 and then --ref-spp samples in total (the low-sample frames are prefixes
of the reference's sample sequence, and the GPU frame is bit-identical to the CPU oracle's, so it is the reference);
the G-buffer comes from the rasterizer; every parameter set filters every low-sample frame. The measure is the
RMSE over xyz of all pixels, divided by the raw frame's. Prints a table per scene and the parameter set with the
lowest mean ratio over scenes and sample counts; with --out, writes every row as JSON lines. Needs the GPU.

    python tools/denoise_sweep.py --width 1920 --height 1080 --scenes cornell_lit,app_default --ref-spp 4096
"""
from __future__ import annotations

import argparse
import itertools
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "path-tracer-and-rasterizer-engine_amd"))
import iqpt  # noqa: E402
from iqpt.scene import Scene, make_camera  # noqa: E402

SPP = (1, 4, 16)


def rmse(a, ref):
    d = a[..., :3].astype(np.float64) - ref
    return float(np.sqrt(np.mean(d * d)))


def frames(preset, w, h, max_depth, ref_spp):
    """({spp: accumulator [H,W,4]}, the reference's xyz as float64, the G-buffer)."""
    sc = Scene()
    sc.add_preset(preset)
    cam = make_camera(w, h)
    low, done = {}, 0
    with iqpt.PathTracer(w, h, max_depth=max_depth) as pt, iqpt.Rasterizer(w, h, samples=1) as r:
        pt.set_camera(cam)
        pt.upload_packet(sc.build_packet())
        for spp in SPP + (ref_spp,):
            while done < spp:
                step = min(64, spp - done)
                pt.render(step)
                done += step
            frame = pt.read()[0].reshape(h, w, 4)
            if spp == ref_spp:
                ref = frame[..., :3].astype(np.float64)
            else:
                low[spp] = frame.copy()
        r.set_camera(cam)
        r.upload_scene(sc)
        guides = r.gbuffer()
    return low, ref, guides


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="cornell_lit,app_default")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--levels", default="3,4,5")
    ap.add_argument("--normal-squarings", default="0,5")
    ap.add_argument("--depth-sharpness", default="0,1024")
    ap.add_argument("--colour-sharpness", default="0,1,2,4")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    grid = list(itertools.product([int(v) for v in a.levels.split(",")], [int(v) for v in a.normal_squarings.split(",")],
                                  [float(v) for v in a.depth_sharpness.split(",")],
                                  [float(v) for v in a.colour_sharpness.split(",")]))
    rows, score = [], {p: [] for p in grid}
    for preset in a.scenes.split(","):
        low, ref, (nz, ids) = frames(preset, a.width, a.height, a.max_depth, a.ref_spp)
        raw = {spp: rmse(low[spp], ref) for spp in SPP}
        print(f"# {preset} {a.width}x{a.height}: raw RMSE " + ", ".join(f"{s} spp {raw[s]:.4f}" for s in SPP) +
              f"; guided pixels {np.mean(ids != 0xFFFFFFFF):.3f}", flush=True)
        with iqpt.Denoiser(a.width, a.height) as d:
            d.set_guides(nz, ids)
            for p in grid:
                d.set_params(*p)
                ratio = {}
                for spp in SPP:
                    d.run(low[spp])
                    ratio[spp] = rmse(d.read()[0], ref) / raw[spp]
                    score[p].append(ratio[spp])
                row = {"scene": preset, "levels": p[0], "normal_squarings": p[1], "depth_sharpness": p[2],
                       "colour_sharpness": p[3], "raw_rmse": raw, "ratio": ratio}
                rows.append(row)
                print(f"{preset} L={p[0]} q={p[1]} s_z={p[2]:g} s_c={p[3]:g}: " +
                      " ".join(f"{s}spp {ratio[s]:.3f}" for s in SPP), flush=True)
    best = min(grid, key=lambda p: float(np.mean(score[p])))
    print(json.dumps({"best": {"levels": best[0], "normal_squarings": best[1], "depth_sharpness": best[2],
                               "colour_sharpness": best[3]}, "mean_ratio": float(np.mean(score[best])),
                      "ratios": score[best]}), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
