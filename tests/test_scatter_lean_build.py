"""The IQPT_SCATTER_LEAN knob (csrc/iqpt_kernels.hip, iqpt/_build.py) builds both libraries, and the production
variants of the two-ray kernel keep their register budget in both: 128 VGPRs, no scratch, 4 waves per SIMD (the
compiler's -Rpass-analysis=kernel-resource-usage remarks, kept by build_lib beside the kernels' object)."""
import ctypes as C

import pytest

from iqpt import _build

# MAXD 8 and 16 of the production option sets 0x2e4b2f (overlapped launches) and 0x264b2f
PRODUCTION = [(maxd, opt) for maxd in (8, 16) for opt in (0x2e4b2f, 0x264b2f)]


def production_kernels(res):
    out = {}
    for maxd, opt in PRODUCTION:
        names = [n for n in res if f"iqpt_render_kernelILi{maxd}ELb0ELi{opt}EE" in n]
        assert len(names) == 1, (maxd, hex(opt), names)
        out[(maxd, opt)] = res[names[0]]
    return out


@pytest.mark.parametrize("form", ["lean", "full"])
def test_knob_builds_the_library_within_the_budget(form):
    if form == "lean":
        lib = _build.build_lib()
        assert lib == _build.LIB_PATH
    else:
        lib = _build.build_lib(flags=_build.SCATTER_FULL_FLAGS, target=_build.SCATTER_FULL_LIB)
        assert lib == _build.SCATTER_FULL_LIB and lib != _build.LIB_PATH
    assert lib.exists()
    h = C.CDLL(str(lib))
    assert h.iqpt_abi_version() > 0 and hasattr(h, "iqpt_debug_read_stats_ext")
    for key, r in production_kernels(_build.kernel_resources(lib)).items():
        print(form, key[0], hex(key[1]), r)
        assert r["VGPRs"] == 128, (form, key, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (form, key, r)
        assert r["VGPRs Spill"] == 0, (form, key, r)
        assert r["Occupancy [waves/SIMD]"] == 4, (form, key, r)


def test_the_two_forms_differ():
    """The knob reaches the kernels: the two libraries' kernels are not the same code."""
    assert _build.LIB_PATH.read_bytes() != _build.SCATTER_FULL_LIB.read_bytes()
