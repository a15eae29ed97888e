#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — builds the reference engine's own hot-path source as a host library.

``build_ref()`` reads the reference (IoniqRE) from its directory, compiles its translation units verbatim behind
the stand-in headers of ``oracle/ref/shim/`` together with ``oracle/ref/ref_driver.cpp``, and links
``oracle/_ref/libref_a.so`` and ``oracle/_ref/libref_b.so`` (git-ignored). Nothing of the reference is committed:
its text is only ever read from its directory and, for the kernel ranges of ``path_tracer.cu`` (which cannot be
compiled whole), cut into ``oracle/_ref/`` at build time.

* Reference directory: ``$IQPT_REFERENCE`` (the directory holding ``path_tracer.cu``), default
  ``reference/IoniqRE`` next to the repository. When it, g++ or clang++ is absent, ``build_ref()`` returns
  ``None`` quietly and the live comparisons of tests/test_ref_*.py skip; the recorded ones
  (tests/golden/ref_*.npz) still run.
* Every reference file consumed is checked against ``reference_sha256.json`` first. A file that differs fails the
  build loudly, so that a moved line range is never silently compiled. ``python build_ref.py --record`` rewrites
  the table (hashes are recorded results, not reference text).
* Flavours, both ``-O2 -ffp-contract=off -fno-fast-math``: **a** = glibc libm; **b** = the
  reference's sinf / cosf / tanf / acosf / asinf / atan2f redirected to csrc/iq_fp.h (shim/cuda_runtime.h).
* ``max_depth`` is a literal in the reference's ray_color; each depth in ``DEPTHS`` is one extracted copy with that
  line substituted and one compile of the driver's kernel part.
* The random generator is this project's restatement of cuRAND's XORWOW (csrc/iq_xorwow.h, behind
  shim/curand_kernel.h): the one part the reference does not contain, pinned only by rocRAND's jump tables and
  SURVEY.md §8c's known-answer vector.
"""
from __future__ import annotations

import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

HERE = Path(__file__).resolve().parent                 # oracle/ref
REPO = HERE.parent.parent
OUT = HERE.parent / "_ref"                             # oracle/_ref (git-ignored)
SHIM = HERE / "shim"
DRIVER = HERE / "ref_driver.cpp"
HASHES = HERE / "reference_sha256.json"
CSRC = REPO / "path-tracer-and-rasterizer-engine_amd" / "csrc"

DEFAULT_REFERENCE = str(REPO.parent / "reference" / "IoniqRE")
FLAVOURS = {"a": [], "b": ["-DREF_FLAVOUR_B"]}
DEPTHS = (1, 2, 5, 8)

# translation units compiled verbatim: plain g++, and the three that need clang's MSVC leniency
GXX_UNITS = ["matrix.cu", "ray.cu", "random.cu", "onb.cu", "camera.cu", "material.cu", "shape.cu", "model.cu"]
MS_UNITS = ["mesh.cu", "scene.cu", "ioniq_exception.cu"]
HEADERS = ["camera.h", "core.h", "ioniq_exception.h", "ioniq_windows.h", "iqmath.h", "material.h", "matrix.h", "mesh.h",
           "model.h", "onb.h", "path_tracer.h", "random.h", "ray.h", "renderer.h", "renderer_base.h",
           "renderer_template.h", "scene.h", "shader.h", "shape.h", "vector.h", "window.h"]
KERNEL_SOURCE = "path_tracer.cu"
# 1-based inclusive line ranges of path_tracer.cu: includes + `threads`, renderer_init_kernel, then pixel_shader,
# ray_color and render_kernel
KERNEL_RANGES = ((1, 10), (36, 46), (212, 366))
MAX_DEPTH_LINE = 240
MAX_DEPTH_RE = re.compile(r"^(\s*const int max_depth = )5(;\s*)$")

FP_FLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math"]
MS_FLAGS = ["-fms-extensions", "-fms-compatibility", "-fms-compatibility-version=19.29",
            "-D__GCC_ATOMIC_TEST_AND_SET_TRUEVAL=1",
            "-D__extern_always_inline=extern inline __attribute__((always_inline,gnu_inline))",
            "-Wno-everything"]


class ReferenceChanged(RuntimeError):
    """A consumed reference file does not match reference_sha256.json."""


def reference_dir() -> Path | None:
    d = Path(os.environ.get("IQPT_REFERENCE", DEFAULT_REFERENCE) or "/nonexistent")
    try:
        if (d / KERNEL_SOURCE).is_file() and os.access(d / KERNEL_SOURCE, os.R_OK):
            return d
    except OSError:
        pass
    return None


def _clangxx() -> str | None:
    for cand in (os.environ.get("IQPT_CLANGXX"), shutil.which("clang++"),
                 str(Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "lib/llvm/bin/clang++"),
                 str(Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm/bin/clang++")):
        if cand and Path(cand).exists():
            return cand
    return None


def _gxx() -> str | None:
    return os.environ.get("CXX") or shutil.which("g++")


def consumed_files() -> list[str]:
    return sorted(GXX_UNITS + MS_UNITS + HEADERS + [KERNEL_SOURCE])


def _sha256(path: Path) -> str:
    return hashlib.sha256(path.read_bytes()).hexdigest()


def record_hashes(ref: Path) -> None:
    table = {name: _sha256(ref / name) for name in consumed_files()}
    HASHES.write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")


def check_hashes(ref: Path) -> None:
    table = json.loads(HASHES.read_text())
    bad = [n for n in consumed_files() if table.get(n) != _sha256(ref / n)]
    if bad:
        raise ReferenceChanged(f"reference files differ from {HASHES.name}: {', '.join(bad)}; the line ranges of "
                               f"{KERNEL_SOURCE} may have moved. Check them, then run build_ref.py --record")


def extract_kernel_text(ref: Path, depth: int) -> Path:
    """The kernel ranges of path_tracer.cu with max_depth set to ``depth``, written into oracle/_ref/."""
    lines = (ref / KERNEL_SOURCE).read_text().splitlines(keepends=True)
    m = MAX_DEPTH_RE.match(lines[MAX_DEPTH_LINE - 1].rstrip("\r\n"))
    if not m:
        raise ReferenceChanged(f"{KERNEL_SOURCE}:{MAX_DEPTH_LINE} is not the max_depth line")
    lines[MAX_DEPTH_LINE - 1] = f"{m.group(1)}{depth}{m.group(2)}\n"
    out = OUT / f"path_tracer_kernel_d{depth}.inc"
    out.write_text("".join("".join(lines[a - 1:b]) + "\n" for a, b in KERNEL_RANGES))
    return out


def _run(cmd: list[str]) -> None:
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f"build_ref failed ({proc.returncode}): {' '.join(cmd)}\n{proc.stdout}\n{proc.stderr}")


def _stamp(ref: Path) -> str:
    h = hashlib.sha256()
    for p in [Path(__file__), DRIVER, HASHES, CSRC / "iq_fp.h", CSRC / "iq_xorwow.h", *sorted(SHIM.iterdir())]:
        h.update(p.name.encode())
        h.update(p.read_bytes())
    h.update(str(ref).encode())
    return h.hexdigest()


def lib_path(flavour: str) -> Path:
    return OUT / f"libref_{flavour}.so"


def build_ref(force: bool = False) -> Path | None:
    """Builds oracle/_ref/libref_a.so and libref_b.so; returns oracle/_ref, or None when the reference directory or a
    compiler is absent."""
    ref = reference_dir()
    gxx, clangxx = _gxx(), _clangxx()
    if ref is None or not gxx or not clangxx:
        return None
    try:
        if not all(os.access(ref / n, os.R_OK) for n in consumed_files()):
            return None
    except OSError:
        return None
    check_hashes(ref)
    stamp = _stamp(ref)
    stamp_file = OUT / "stamp"
    if (not force and stamp_file.exists() and stamp_file.read_text() == stamp
            and all(lib_path(f).exists() for f in FLAVOURS)):
        return OUT
    OUT.mkdir(parents=True, exist_ok=True)
    texts = {d: extract_kernel_text(ref, d) for d in DEPTHS}
    common = ["-std=c++17", "-x", "c++", *FP_FLAGS, "-fPIC", f"-I{SHIM}", f"-I{CSRC}", "-iquote", str(ref)]
    cmds, objs = [], {f: [] for f in FLAVOURS}
    for flavour, defs in FLAVOURS.items():
        odir = OUT / f"obj_{flavour}"
        odir.mkdir(exist_ok=True)

        def add(compiler, extra, src, name):
            o = odir / f"{name}.o"
            cmds.append([compiler, *common, *defs, *extra, "-c", str(src), "-o", str(o)])
            objs[flavour].append(o)
        for unit in GXX_UNITS:
            add(gxx, ["-w"], ref / unit, Path(unit).stem)
        for unit in MS_UNITS:
            add(clangxx, MS_FLAGS, ref / unit, Path(unit).stem)
        add(clangxx, MS_FLAGS, DRIVER, "ref_driver")
        for d, text in texts.items():
            add(clangxx, [*MS_FLAGS, f"-I{OUT}", f"-DREF_KERNEL_DEPTH={d}", f'-DREF_KERNEL_TEXT="{text.name}"'],
                DRIVER, f"ref_kernel_d{d}")
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(_run, cmds))
    for flavour in FLAVOURS:
        tmp = lib_path(flavour).with_suffix(".so.tmp")
        _run([gxx, "-shared", "-fPIC", *map(str, objs[flavour]), "-o", str(tmp), "-lm"])
        os.replace(tmp, lib_path(flavour))
    stamp_file.write_text(stamp)
    return OUT


if __name__ == "__main__":
    if "--record" in sys.argv:
        r = reference_dir()
        if r is None:
            sys.exit("no reference directory")
        record_hashes(r)
        print("recorded", len(consumed_files()), "hashes in", HASHES)
    t0 = time.perf_counter()
    print("build_ref:", build_ref(force="--force" in sys.argv), f"{time.perf_counter() - t0:.1f} s")
