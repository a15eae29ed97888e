"""The dynamic symbol table of libiqpt.so is pinned: the C ABI, the kernels' launchers and the facade, no more.

tests/golden/libiqpt_exports.txt lists the names `nm -D --defined-only` gave for the library before the runtime
was split into csrc/runtime/ (one per line, sorted), without iqpt::take_launch_events, which left with the split,
and without the `__hip_cuid_<hash>` names: hipcc emits one per translation unit from the source's path and
contents, so they differ between any two checkouts. Helpers the runtime sources share are hidden
(IQPT_RT_LOCAL in csrc/runtime/iq_ctx.hpp) and must not show up here.
"""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

from iqpt import _build

FIXTURE = Path(__file__).resolve().parent / "golden" / "libiqpt_exports.txt"


def exported_names(lib: Path) -> set[str]:
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path=str(Path(_build.HIPCC).parent))
    if nm is None:
        pytest.fail("neither nm nor llvm-nm found: cannot list the library's exports")
    out = subprocess.run([nm, "-D", "--defined-only", str(lib)], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    return {n for n in names if not n.startswith("__hip_cuid_")}


def test_exports_match_fixture():
    want = set(FIXTURE.read_text().split())
    got = exported_names(_build.build_lib())
    assert got == want, f"new exports: {sorted(got - want)}; missing exports: {sorted(want - got)}"


def test_lib_sources_exist_with_unique_object_names():
    paths = [_build.CSRC / s for s in _build.LIB_SOURCES]
    assert [str(p) for p in paths if not p.is_file()] == []
    # build_lib names each object after its source's base name, whatever its directory
    bases = [p.name for p in paths]
    assert sorted(set(bases)) == sorted(bases)
