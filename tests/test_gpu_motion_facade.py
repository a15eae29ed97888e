"""csrc/tools/test_motion_facade.cpp (iqpt::motion, the header-only C++ facade over libiqpt_motion.so) against
tests/motion_ref.py: the program's four counts and the FNV-1a hashes of its float4 and BGRA8 results equal the
reference's on the G-buffers and accumulators the Python objects make of the same two scenes."""
import json
import subprocess

import numpy as np
import pytest

import iqpt
import motion_cases as mc
import motion_ref as mr
from iqpt import PathTracer, Rasterizer, _build, align_camera

pytestmark = pytest.mark.gpu


def fnv1a_64(data: bytes) -> int:
    """FNV-1a, 64 bits, byte by byte (8-byte words at a time would be another hash)."""
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_motion_facade(require_gpu):
    assert _build.MOTION_FACADE_TEST_PATH.exists()
    proc = subprocess.run([str(_build.MOTION_FACADE_TEST_PATH)], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    w, h, spp = got["width"], got["height"], got["spp"]
    assert got["ok"] and (w, h) == (96, 54)

    cam = mc.movers_camera(w, h)
    scenes = [mc.movers(0, materials=False), mc.movers(1, materials=False)]
    ref = mr.Motion(w, h, 0.9, 0.01, 256)
    with PathTracer(w, h, max_depth=8) as pt, Rasterizer(w, h) as r:
        pt.set_camera(align_camera(cam))
        r.set_camera(cam)
        for k, sc in enumerate(scenes):
            pt.upload_packet(sc.build_packet())
            pt.reset()
            r.upload_scene(sc)
            nz, ids = r.gbuffer()
            ref.begin_view(cam, nz, ids, iqpt.motion_table(scenes[0], sc) if k else None)
            pt.render(spp)
            lin, bgra = ref.resolve(pt.read()[0], spp)
    guided, valid, moved, moved_valid = ref.stats()
    assert moved > 50 and moved_valid > moved // 2
    assert (got["guided"], got["valid"], got["moved"], got["moved_valid"]) == (guided, valid, moved, moved_valid)
    assert got["lin_fnv1a"] == f"{fnv1a_64(np.ascontiguousarray(lin, np.float32).tobytes()):016x}"
    assert got["bgra_fnv1a"] == f"{fnv1a_64(np.ascontiguousarray(bgra, np.uint8).tobytes()):016x}"
