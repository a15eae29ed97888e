"""The CPU half of tests/test_gpu_scatter_probe.py: what the device comparison rests on, shown without a GPU.

(a) iqo_oren_nayar_batch with sigma 1 and albedo .5 returns the bits of iqo_oren_nayar on all of
    ref_cases.scatter_inputs, so the pin of the oracle's scatter to the reference carries over to the batch export;
(b) crafted_state gives states whose next two draws are the chosen words;
(c) the case set holds every kind of case the comparison is meant to see, stated from the oracle alone;
(d) the oracle's outputs are NaN-free in every case whose inputs hold no NaN, so a NaN can match a NaN only there."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ref_cases
import scatter_probe as sp

F32 = np.float32
UP = C.POINTER(C.c_uint32)


def test_batch_export_returns_the_old_exports_bits():
    inp = ref_cases.scatter_inputs(ref_cases.N_LIVE)
    old = ref_cases.oracle_units({**ref_cases.unit_inputs(8), "scatter": inp}, "b")
    new = sp.oracle_scatter(inp["p"], inp["n"], inp["d"], inp["states"], 1.0, 0.5)
    assert len(inp["p"]) == ref_cases.N_LIVE + 99
    for k in ("att", "pdf", "cosw", "ro", "rd"):
        assert np.array_equal(new[k].view(np.uint32), old[f"oren_nayar.{k}"].view(np.uint32)), k
    assert np.array_equal(new["states"], old["oren_nayar.states"])
    assert np.all(old["oren_nayar.ret"] == 1)


def test_batch_export_clamps_sigma_and_takes_the_albedo():
    inp = {k: v[:64] for k, v in ref_cases.scatter_inputs(64).items()}
    one = sp.oracle_scatter(inp["p"], inp["n"], inp["d"], inp["states"], 1.0, 0.5)
    above = sp.oracle_scatter(inp["p"], inp["n"], inp["d"], inp["states"], 7.0, 0.5)
    assert np.array_equal(one["att"].view(np.uint32), above["att"].view(np.uint32))
    # sigma 0: A = 1, B = 0, so att = (albedo * 1) * (1 / pi) whatever the angles
    flat = sp.oracle_scatter(inp["p"], inp["n"], inp["d"], inp["states"], 0.0, 0.25)
    want = F32(F32(0.25) * (F32(1.0) / F32(np.pi)))
    assert np.all(flat["att"][:, :3] == want) and np.all(flat["att"][:, 3] == 0)
    assert np.array_equal(flat["rd"].view(np.uint32), one["rd"].view(np.uint32))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_crafted_states_draw_the_chosen_words(seed):
    lib = oracle.load()
    rng = np.random.default_rng(seed)
    xs = (0, 1, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF, 0x80000000)
    for x1 in xs:
        for x2 in xs:
            st = sp.crafted_state(x1, x2, rng.integers(0, 1 << 32, 4, dtype=np.uint64))
            a = st.copy()
            assert lib.iqo_xorwow_next(a.ctypes.data_as(UP)) == x1
            assert lib.iqo_xorwow_next(a.ctypes.data_as(UP)) == x2
            b = st.copy()
            u1 = lib.iqo_real(b.ctypes.data_as(UP), 0.0, 1.0)
            u2 = lib.iqo_real(b.ctypes.data_as(UP), 0.0, 1.0)
            assert F32(u1).view(np.uint32) == sp.draw_unit(x1).view(np.uint32)
            assert F32(u2).view(np.uint32) == sp.draw_unit(x2).view(np.uint32)
            assert np.array_equal(a, b)
    # the draws the cases are named after
    assert sp.draw_unit(sp.R_ZERO) == 0 and sp.draw_unit(sp.R_MIN) == F32(2.0 ** -32)
    assert sp.draw_unit(sp.R_BELOW_ONE) == np.nextafter(F32(1), F32(0))
    assert sp.draw_unit(sp.R_ONE) == 1 and sp.draw_unit(sp.R_MAX) == 1 and sp.draw_unit(sp.R_ONE - 1) < 1


def first_draws(states):
    """(r1, r2): the next two generator outputs of every state."""
    lib = oracle.load()
    out = np.zeros((len(states), 2), np.uint64)
    for i, s in enumerate(states):
        s = np.array(s, np.uint32)
        out[i, 0] = lib.iqo_xorwow_next(s.ctypes.data_as(UP))
        out[i, 1] = lib.iqo_xorwow_next(s.ctypes.data_as(UP))
    return out


def test_case_set_covers_every_kind_from_the_reference_alone():
    c = sp.main_cases()
    ref = sp.main_reference(*sp.SIGMAS[0])
    obj = sp.objections(c["n"], c["d"], ref["rd"])
    real = ~c["has_nan"] & ~c["nonunit"]                     # what a kernel can meet, NaN-free
    r = first_draws(c["states"])
    u1 = np.array([sp.draw_unit(int(v)) for v in r[:, 0]], F32)
    u2 = np.array([sp.draw_unit(int(v)) for v in r[:, 1]], F32)
    replaced = (ref["pdf"] == F32(1.0) / F32(np.pi)) & np.all(ref["rd"].view(np.uint32) == c["n"].view(np.uint32), 1)
    n3 = c["n"][:, :3].astype(np.float64)
    with np.errstate(all="ignore"):
        wx = np.abs(n3[:, 0] / np.sqrt((n3 ** 2).sum(1)))
    kinds = {
        "pdf replaced": replaced & real,
        "cto > 1": (obj["cto_value"] > 1) & real,
        "cti = 0": (obj["cti_value"] == 0) & real,
        "refused: atan2(woy, wox)": obj["wo"] & real,
        "refused: atan2(dy, dx)": obj["d"] & real,
        "refused: acos(cto)": obj["cto"] & real,
        "refused: acos(cti)": obj["cti"] & real,
        "|w.x| > 0.9": (wx > 0.9001) & real,
        "|w.x| <= 0.9": (wx < 0.8999) & real,
        "u2 = 0": (u2 == 0) & real,
        "u2 = 1": (u2 == 1) & real,
        "phi = RN(2 pi)": (u1 == 1) & real,
        "a NaN in the inputs": c["has_nan"],
        "a non-unit normal": c["nonunit"],
    }
    counts = {k: int(v.sum()) for k, v in kinds.items()}
    print(len(c["p"]), "cases;", counts)
    assert all(v >= 1 for v in counts.values()), counts
    # non-unit: the nine 2.5 a of ref_cases.scatter_inputs (its nine 1e-6 a are null normals) and the 18 short axis
    # normals that put the pdf at its threshold; all of them are compared like every other case
    thr = np.array([t.startswith("pdf threshold") for t in c["tag"]])
    assert counts["a non-unit normal"] == 9 + 18 and (c["nonunit"] & thr).sum() == 18
    at = np.array([t == "pdf threshold +0" for t in c["tag"]])
    below = np.array([t == "pdf threshold -1" for t in c["tag"]])
    assert at.sum() == 6 and np.all(ref["pdf"][at] == sp.PDF_MIN) and not replaced[at].any()
    assert below.sum() == 6 and replaced[below].all()
    # u2 = 1 replaces the pdf (lz = 0: n . d is rounding noise), and for an axis-aligned normal d = n then has dx = 0
    assert np.all(replaced[(u2 == 1) & real & (np.abs(obj["cti_value"]) > 0)])
    # the placement cases exist: in-domain waves and one case per kind that objects for that kind alone
    base, pick = sp.placement_cases()
    assert len(base) == sp.PLACEMENT_N and not sp.objects(obj)[base].any()
    assert set(pick) == set(sp.KINDS)
    # and more than one wave of the main set stays lean while others fall back
    bad = sp.objects(obj)
    waves = [bad[w:w + 64].any() for w in range(0, len(bad), 64)]
    assert sum(waves) >= 2 and len(waves) - sum(waves) >= 2, (sum(waves), len(waves))


@pytest.mark.parametrize("sigma,albedo", sp.SIGMAS)
def test_reference_is_nan_free_where_the_inputs_are(sigma, albedo):
    c = sp.main_cases()
    ref = sp.main_reference(sigma, albedo)
    clean = ~c["has_nan"]
    for k in ("att", "pdf", "cosw", "q", "ro", "rd"):
        assert not np.isnan(ref[k][clean]).any(), (k, np.flatnonzero(np.isnan(ref[k]).reshape(len(clean), -1).any(1) & clean)[:8])
    assert c["has_nan"].sum() >= 3


def test_sphere_cases_from_the_reference_alone():
    s, ref = sp.sphere_cases()
    assert len(s["t"]) == 3 * 24 * len(sp.SPHERE_RADII)
    for rad in sp.SPHERE_RADII:
        for kind in ("outside", "inside", "grazing"):
            assert sum(1 for k, r in zip(s["kind"], s["r"]) if k == kind and r == F32(rad)) == 24, (rad, kind)
    for k in ("value", "ro", "rd", "q"):
        assert not np.isnan(ref[k]).any(), k
    # grazing: the incoming ray is within a few degrees of the tangent plane
    graz = np.array([k == "grazing" for k in s["kind"]])
    cosi = np.abs((s["d"][:, :3].astype(np.float64) * s["n"][:, :3]).sum(1))
    assert np.all(cosi[graz] < 0.2), cosi[graz].max()
    # the radii stay inside the range the runtime admits to kOptFastDiv's reciprocal (iq_rcp: [2^-126, 2^126])
    assert s["r"].min() == F32(2.0 ** -20) and s["r"].max() == F32(2.0 ** 20)
