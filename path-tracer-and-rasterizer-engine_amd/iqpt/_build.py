"""Build recipes for the native parts (no cmake/ninja needed).

* ``libiqpt.so`` — the product: HIP kernels for gfx950 + the C-ABI runtime + the scene builder,
  built in-tree next to this package so it travels to the GPU box with the snapshot.
* ``oracle/liboracle.so`` (+ ``liboracle_glibc.so``) — TEST INFRASTRUCTURE: the plain-C CPU
  restatement of the reference hot path (see oracle/iqpt_oracle.c).
* ``iqpt_cli`` / ``test_facade`` — C++ programs over the ``path_tracer`` facade.

Every translation unit on the hot path is compiled with ``-ffp-contract=off``.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent            # .../path-tracer-and-rasterizer-engine_amd/iqpt
PROJ_DIR = PKG_DIR.parent                            # .../path-tracer-and-rasterizer-engine_amd
REPO = PROJ_DIR.parent
CSRC = PROJ_DIR / "csrc"
INCLUDE = REPO / "include"
ORACLE_DIR = REPO / "oracle"
BUILD_DIR = PROJ_DIR / "build"

LIB_PATH = PKG_DIR / "libiqpt.so"
STATS_LIB_PATH = PKG_DIR / "libiqpt_stats.so"  # + the instrumented kOptStats variants (tools/work_counters.py)
ORACLE_LIB = ORACLE_DIR / "liboracle.so"
ORACLE_GLIBC_LIB = ORACLE_DIR / "liboracle_glibc.so"
ORACLE_FMA_LIB = ORACLE_DIR / "liboracle_fma.so"      # informational: contraction on + glibc libm (nvcc-like)
CLI_PATH = PKG_DIR / "iqpt_cli"
FACADE_TEST_PATH = PKG_DIR / "test_facade"
RASTER_FACADE_TEST_PATH = PKG_DIR / "test_raster_facade"
DENOISE_FACADE_TEST_PATH = PKG_DIR / "test_denoise_facade"
TEMPORAL_FACADE_TEST_PATH = PKG_DIR / "test_temporal_facade"
SVGF_FACADE_TEST_PATH = PKG_DIR / "test_svgf_facade"
UPSCALE_FACADE_TEST_PATH = PKG_DIR / "test_upscale_facade"
MOTION_LIB_PATH = PKG_DIR / "libiqpt_motion.so"              # moving-model reprojection: links libiqpt.so
MOTION_UNIFORM_LIB_PATH = PKG_DIR / "libiqpt_motion_uniform.so"  # its wave-uniform-entry form (A/B and test only)
MOTION_FACADE_TEST_PATH = PKG_DIR / "test_motion_facade"

ARCH = os.environ.get("IQPT_OFFLOAD_ARCH", "gfx950")
HIPCC = os.environ.get("HIPCC", shutil.which("hipcc") or "/opt/rocm/bin/hipcc")
CC = os.environ.get("CC", "gcc")

FP_FLAGS = ["-ffp-contract=off", "-fno-fast-math"]
HIP_FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", *FP_FLAGS,
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-Wno-unused-function",
             f"-I{INCLUDE}", f"-I{CSRC}"]

LIB_SOURCES = ["iqpt_kernels.hip", "iqpt_runtime.cpp", "iq_scene.cpp", "path_tracer.cpp",
               # the rest of the C ABI by concern; runtime/iq_ctx.hpp is theirs alone, outside
               # kernel_source_sha16's identity
               "runtime/iq_cull.cpp", "runtime/iq_launch.cpp", "runtime/iq_comm.cpp", "runtime/iq_checkpoint.cpp",
               "runtime/iq_debug.cpp",
               # the rasterizer: its own directory, outside kernel_source_sha16's path-tracing identity
               "raster/iq_raster_kernels.hip", "raster/iq_raster.cpp", "raster/rasterizer.cpp",
               # the rasterizer-guided denoiser, likewise outside that identity
               "denoise/iq_denoise_kernels.hip", "denoise/iq_denoise.cpp",
               # temporal reprojection, likewise
               "temporal/iq_temporal_kernels.hip", "temporal/iq_temporal.cpp",
               # variance-guided filtering, likewise
               "svgf/iq_svgf_kernels.hip", "svgf/iq_svgf.cpp",
               # what those three share, likewise
               "post/iq_post_kernels.hip", "post/iq_post.cpp",
               # guided upsampling, likewise
               "upscale/iq_upscale_kernels.hip", "upscale/iq_upscale.cpp"]


def _run(cmd: list[str], cwd: Path | None = None, stderr_to: Path | None = None) -> None:
    proc = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f"build failed ({proc.returncode}): {' '.join(map(str, cmd))}\n"
                           f"{proc.stdout}\n{proc.stderr}")
    if stderr_to is not None:
        stderr_to.write_text(proc.stderr)


KERNELS_SOURCE = "iqpt_kernels.hip"
REMARKS_FLAG = "-Rpass-analysis=kernel-resource-usage"


def _build_dir(target: Path, stats: bool, flags: bool) -> Path:
    return BUILD_DIR / (target.stem if flags else ("stats" if stats else "prod"))


def _remarks_path(bdir: Path) -> Path:
    return bdir / (KERNELS_SOURCE + ".remarks.txt")


def _newer(target: Path, deps: list[Path]) -> bool:
    if not target.exists():
        return False
    t = target.stat().st_mtime
    return all(d.stat().st_mtime <= t for d in deps if d.exists())


def _headers() -> list[Path]:
    return sorted(CSRC.glob("*.h")) + sorted(CSRC.glob("*.hpp")) + sorted(INCLUDE.glob("*.h"))


SUBDIRS = ("runtime", "raster", "denoise", "temporal", "svgf", "post", "upscale")


def _deps() -> list[Path]:
    """Every header a library object or a tool may include."""
    return _headers() + [h for d in SUBDIRS
                         for h in sorted((CSRC / d).glob("*.hpp")) + sorted((INCLUDE / d).glob("*.h"))]


def kernel_source_sha16() -> str:
    """16 hex digits of SHA-256 over the device-code sources (the .hip kernels and every header they include):
    the identity of the kernels a measurement profile describes (tools/work_counters.py writes it, bench.py
    refuses a profile of other sources)."""
    import hashlib
    h = hashlib.sha256()
    for p in sorted(CSRC.glob("*.hip")) + _headers():
        h.update(p.name.encode())
        h.update(p.read_bytes())
    return h.hexdigest()[:16]


def build_lib(force: bool = False, stats: bool = False, flags: tuple[str, ...] = (),
              target: Path | None = None) -> Path:
    """Compile the HIP kernels + runtime into libiqpt.so (gfx950); stats=True adds the instrumented
    kOptStats variants (a separate library: measurement only).
    ``flags``/``target``: extra compiler flags into another library (compiler-option A/B runs)."""
    target = target or (STATS_LIB_PATH if stats else LIB_PATH)
    srcs = [CSRC / s for s in LIB_SOURCES]
    if not force and _newer(target, srcs + _deps() + [Path(__file__)]):
        return target
    bdir = _build_dir(target, stats, bool(flags))
    bdir.mkdir(parents=True, exist_ok=True)
    objs = []
    cmds = []
    extra = (["-DIQPT_STATS_VARIANTS"] if stats else []) + list(flags)
    for s in srcs:
        o = bdir / (s.name + ".o")
        # an object is rebuilt when its source, a header or this recipe is newer (force: always)
        if force or not _newer(o, [s] + _deps() + [Path(__file__)]):
            cmd = [HIPCC, *HIP_FLAGS, *extra, "-x", "hip", "-c", str(s), "-o", str(o)]
            # the path-tracing kernels' resource remarks are kept beside the object (kernel_resources)
            cmds.append((cmd + [REMARKS_FLAG], _remarks_path(bdir)) if s.name == KERNELS_SOURCE else (cmd, None))
        objs.append(o)
    if cmds:
        with ThreadPoolExecutor(max_workers=min(4, len(cmds))) as ex:
            list(ex.map(lambda c: _run(c[0], stderr_to=c[1]), cmds))
    tmp = target.with_suffix(".so.tmp")
    _run([HIPCC, "-shared", "-fPIC", f"--offload-arch={ARCH}", *map(str, objs), "-o", str(tmp)])
    os.replace(tmp, target)
    return target


# Moving-model reprojection: a library of its own over libiqpt.so's exports, so that library's
# dynamic symbol table stays what tests/golden/libiqpt_exports.txt pins.
MOTION_LIB_SOURCES = ["motion/iq_motion_kernels.hip", "motion/iq_motion.cpp"]
MOTION_KERNELS_SOURCE = "iq_motion_kernels.hip"
MOTION_UNIFORM_FLAGS = ("-DIQM_UNIFORM_ENTRY=1",)


def _motion_deps() -> list[Path]:
    """_deps() and the motion directory's own headers, which no source of libiqpt.so includes."""
    return _deps() + sorted((CSRC / "motion").glob("*.hpp")) + sorted((INCLUDE / "motion").glob("*.h"))


def motion_remarks_path(target: Path = MOTION_LIB_PATH) -> Path:
    """The view and stats kernels' resource remarks of the motion library `target`, kept beside its objects."""
    return BUILD_DIR / target.stem / (MOTION_KERNELS_SOURCE + ".remarks.txt")


def build_motion_lib(force: bool = False, flags: tuple[str, ...] = (), target: Path | None = None) -> Path:
    """libiqpt_motion.so: the main library's flags, linked against libiqpt.so in the package directory."""
    target = target or MOTION_LIB_PATH
    lib = build_lib(force)
    srcs = [CSRC / s for s in MOTION_LIB_SOURCES]
    if not force and _newer(target, srcs + _motion_deps() + [lib, Path(__file__)]):
        return target
    bdir = BUILD_DIR / target.stem
    bdir.mkdir(parents=True, exist_ok=True)
    objs = []
    for s in srcs:
        o = bdir / (s.name + ".o")
        cmd = [HIPCC, *HIP_FLAGS, *flags, "-x", "hip", "-c", str(s), "-o", str(o)]
        if s.name == MOTION_KERNELS_SOURCE:
            _run(cmd + [REMARKS_FLAG], stderr_to=motion_remarks_path(target))
        else:
            _run(cmd)
        objs.append(o)
    tmp = target.with_suffix(".so.tmp")
    _run([HIPCC, "-shared", "-fPIC", f"--offload-arch={ARCH}", *map(str, objs), f"-L{PKG_DIR}", "-liqpt",
          "-Wl,-rpath,$ORIGIN", "-o", str(tmp)])
    os.replace(tmp, target)
    return target


def build_motion_libs(force: bool = False) -> list[Path]:
    """The default motion library (every lane gathers its entry) and the one with wave-uniform entry loads that
    tests/test_gpu_motion.py and tools/motion_bench.py compare it with."""
    return [build_motion_lib(force),
            build_motion_lib(force, flags=MOTION_UNIFORM_FLAGS, target=MOTION_UNIFORM_LIB_PATH)]


def build_tools(force: bool = False) -> list[Path]:
    """C++ programs over the facades: the headless CLI, the path_tracer facade test, the two-engine renderer test,
    the tests of the renderer's denoise, temporal and svgf blocks, the test of iqpt::upscaler and, over both
    libraries, the test of iqpt::motion."""
    lib = build_lib(force)
    out = []
    src, dst = CSRC / "tools" / "test_motion_facade.cpp", MOTION_FACADE_TEST_PATH
    if src.exists():
        mlib = build_motion_lib(force)
        if force or not _newer(dst, [src, lib, mlib] + _motion_deps()):
            _run([HIPCC, "-O2", "-std=c++17", *FP_FLAGS, f"-I{INCLUDE}", f"-I{CSRC}", str(src),
                  f"-L{PKG_DIR}", "-liqpt_motion", "-liqpt", "-Wl,-rpath,$ORIGIN", "-o", str(dst)])
        out.append(dst)
    for src, dst in ((CSRC / "tools" / "iqpt_cli.cpp", CLI_PATH),
                     (CSRC / "tools" / "test_facade.cpp", FACADE_TEST_PATH),
                     (CSRC / "tools" / "test_raster_facade.cpp", RASTER_FACADE_TEST_PATH),
                     (CSRC / "tools" / "test_denoise_facade.cpp", DENOISE_FACADE_TEST_PATH),
                     (CSRC / "tools" / "test_temporal_facade.cpp", TEMPORAL_FACADE_TEST_PATH),
                     (CSRC / "tools" / "test_svgf_facade.cpp", SVGF_FACADE_TEST_PATH),
                     (CSRC / "tools" / "test_upscale_facade.cpp", UPSCALE_FACADE_TEST_PATH)):
        if not src.exists():
            continue
        if force or not _newer(dst, [src, lib] + _deps()):
            _run([HIPCC, "-O2", "-std=c++17", *FP_FLAGS, f"-I{INCLUDE}", f"-I{CSRC}", str(src),
                  f"-L{PKG_DIR}", "-liqpt", f"-Wl,-rpath,$ORIGIN", "-o", str(dst)])
        out.append(dst)
    return out


def build_oracle(force: bool = False) -> list[Path]:
    """TEST INFRASTRUCTURE: the C restatement of the reference hot path (plain gcc, OpenMP)."""
    src = ORACLE_DIR / "iqpt_oracle.c"
    deps = [src, CSRC / "iq_fp.h", CSRC / "iq_xorwow.h", INCLUDE / "iqpt.h", Path(__file__)]
    base = [CC, "-O3", "-std=gnu11", "-fPIC", "-shared", "-fopenmp", *FP_FLAGS, "-fno-builtin-sinf",
            f"-I{INCLUDE}", f"-I{CSRC}", str(src)]
    built = []
    # flavours: B = the parity target (iq_fp.h, contraction off); A = glibc libm;
    # FMA = contraction on (-ffp-contract=fast -mfma) with glibc libm, the closest this image gets to
    # nvcc's default (contraction on, libdevice): an estimate of how far the reference binary may sit
    for target, extra in ((ORACLE_LIB, []), (ORACLE_GLIBC_LIB, ["-DIQO_GLIBC_LIBM"]),
                          (ORACLE_FMA_LIB, ["-DIQO_GLIBC_LIBM", "-ffp-contract=fast", "-mfma"])):
        if force or not _newer(target, deps):
            tmp = target.with_suffix(".so.tmp")
            cmd = [*base, *extra, "-o", str(tmp), "-lm"]
            if "-ffp-contract=fast" in extra:
                cmd.remove("-ffp-contract=off")
            _run(cmd)
            os.replace(tmp, target)
        built.append(target)
    return built


ORACLE_NATIVE_FLAGS = ["-O3", "-march=native", "-std=gnu11", "-fPIC", "-shared", "-fopenmp", *FP_FLAGS,
                       "-fno-builtin-sinf"]


def build_oracle_native() -> tuple[Path, str]:
    """TEST INFRASTRUCTURE (bench.py's CPU baseline only): flavour B of the oracle compiled for THIS host's CPU
    (-O3 -march=native, contraction off as every flavour-B build), into oracle/_native/. Built where
    the baseline runs (the GPU box's CPU is not this container's), a few seconds with gcc. Returns (path, the
    command line as a string)."""
    src = ORACLE_DIR / "iqpt_oracle.c"
    dst = ORACLE_DIR / "_native" / "liboracle_native.so"
    dst.parent.mkdir(parents=True, exist_ok=True)
    cmd = [CC, *ORACLE_NATIVE_FLAGS, f"-I{INCLUDE}", f"-I{CSRC}", str(src), "-o", str(dst.with_suffix(".so.tmp")), "-lm"]
    _run(cmd)
    os.replace(dst.with_suffix(".so.tmp"), dst)
    return dst, " ".join([Path(CC).name, *ORACLE_NATIVE_FLAGS, "-lm"])


# The two-ray kernel with every pair through the two-ray body (the form before the per-pair body choice, DESIGN.md
# §3.14): an A/B library for bench.py --lib and the tools' --lib, and the other side of tests/test_gpu_pair_bodies.py.
PAIR2_BOTH_FLAGS = ("-DIQPT_PAIR2_BOTH=1",)
PAIR2_BOTH_LIB = PKG_DIR / "libiqpt_pair2both.so"
PAIR2_BOTH_STATS_LIB = PKG_DIR / "libiqpt_stats_pair2both.so"


def build_pair_body_libs(force: bool = False) -> list[Path]:
    """The libraries tests/test_gpu_pair_bodies.py compares (measurement and test only): the instrumented build and
    the IQPT_PAIR2_BOTH=1 builds of the production and the instrumented library, compiled side by side."""
    jobs = [dict(stats=True), dict(flags=PAIR2_BOTH_FLAGS, target=PAIR2_BOTH_LIB),
            dict(stats=True, flags=PAIR2_BOTH_FLAGS, target=PAIR2_BOTH_STATS_LIB)]
    with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        return list(ex.map(lambda kw: build_lib(force, **kw), jobs))


# The Oren–Nayar scatter on the branch-free transcendental pairs alone (the form before the wave vote for the lean
# paths): an A/B library for bench.py --lib and the tools' --lib, and the other side of
# tests/test_gpu_scatter_lean.py. The instrumented form of it is built on demand (build_lib with these flags).
SCATTER_FULL_FLAGS = ("-DIQPT_SCATTER_LEAN=0",)
SCATTER_FULL_LIB = PKG_DIR / "libiqpt_scatterfull.so"
SCATTER_FULL_STATS_LIB = PKG_DIR / "libiqpt_stats_scatterfull.so"


def build_scatter_libs(force: bool = False) -> list[Path]:
    """The library tests/test_gpu_scatter_lean.py compares the default one with (measurement and test only)."""
    return [build_lib(force, flags=SCATTER_FULL_FLAGS, target=SCATTER_FULL_LIB)]


# The sky kernel with one sample per loop trip in every variant (the form before the paired body):
# an A/B library for bench.py --lib and the tools' --lib, and the other side of tests/test_gpu_sky_pairs.py.
SKY_SINGLE_FLAGS = ("-DIQPT_SKY_PAIRS=0",)
SKY_SINGLE_LIB = PKG_DIR / "libiqpt_skysingle.so"


def build_sky_libs(force: bool = False) -> list[Path]:
    """The library tests/test_gpu_sky_pairs.py compares the default one with (measurement and test only)."""
    return [build_lib(force, flags=SKY_SINGLE_FLAGS, target=SKY_SINGLE_LIB)]


# iqpt_certain_kernel without the beside-a-sphere rule (the folded hit masks equal the tile rule's: the form before
# it): an A/B library for bench.py --lib and the tools' --lib, and the other side of
# tests/test_gpu_certain_beside_sphere.py.
CERTAIN_TILE_RULE_FLAGS = ("-DIQPT_CERTAIN_BESIDE_SPHERE=0",)
CERTAIN_TILE_RULE_LIB = PKG_DIR / "libiqpt_certaintile.so"


def build_certain_libs(force: bool = False) -> list[Path]:
    """The library tests/test_gpu_certain_beside_sphere.py compares the default one with (measurement and test only)."""
    return [build_lib(force, flags=CERTAIN_TILE_RULE_FLAGS, target=CERTAIN_TILE_RULE_LIB)]


def kernel_resources(target: Path = LIB_PATH, stats: bool = False) -> dict[str, dict[str, int]]:
    """Per kernel of iqpt_kernels.hip as compiled into `target` (a library build_lib has built): the compiler's
    resource remarks (-Rpass-analysis=kernel-resource-usage, kept beside the object), as
    {mangled name: {"VGPRs": .., "ScratchSize [bytes/lane]": .., "SGPRs Spill": .., "Occupancy [waves/SIMD]": ..}}."""
    import re
    text = _remarks_path(_build_dir(target, stats, flags=target not in (LIB_PATH, STATS_LIB_PATH))).read_text()
    out: dict[str, dict[str, int]] = {}
    name = None
    for line in text.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark: [^\[]*?\s{2,}([A-Za-z][^:]*): (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def build_ref(force: bool = False) -> Path | None:
    """TEST INFRASTRUCTURE: the reference's own source as a host library (oracle/ref/build_ref.py), into the
    git-ignored oracle/_ref/. None, quietly, where the reference directory or a compiler is absent: the build is
    then what it is without it, and the live comparisons of tests/test_ref_*.py skip. The same where the recipe
    itself is not in the tree (the package used with an oracle/ directory that has no ref/)."""
    import importlib.util
    recipe = ORACLE_DIR / "ref" / "build_ref.py"
    if not recipe.is_file():
        return None
    spec = importlib.util.spec_from_file_location("iqpt_build_ref", recipe)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_ref(force)


def build_all(force: bool = False) -> None:
    build_lib(force)
    build_motion_libs(force)
    build_tools(force)
    build_oracle(force)
    build_ref(force)
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(lambda f: f(force), (build_pair_body_libs, build_scatter_libs, build_sky_libs,
                                         build_certain_libs)))


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
    print("built", LIB_PATH, ORACLE_LIB)
