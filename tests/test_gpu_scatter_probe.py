"""The Oren-Nayar scatter on the device, lane by lane, against the oracle: the device probe
(iqpt_debug_scatter -> iqpt_scatter_probe_kernel) calls or_scatter_core, or sphere_hit and oren_nayar_scatter, exactly
as the render kernels do, one case per lane, in each of its forms: kOptScatter2 | kOptSinCos with and without
kOptFastDiv, each with the wave vote for the lean transcendentals and on the branch-free forms alone, and the plain
transliteration. tests/scatter_probe.py builds the cases and the reference, tests/test_scatter_probe_cases.py shows on
the CPU what the comparison rests on.

Per case the continuation ray, att = (albedo * coeff) * (1 / pi), q = cos / pdf and the six generator words must equal
the oracle's bits; a NaN matches a NaN only where the inputs hold one. No case is left out: the list of cases with a
non-unit normal that a kOptFastDiv form may differ on (NONUNIT_MAY_DIFFER) is empty, because no form differs there.

The vote is predicted on the CPU first (scatter_probe.objections: the oracle's outgoing direction, binary32 dot
products in the kernel's order): case i is lane i % 64 of wave i / 64, every active lane of a wave reports the
fallback exactly when an active lane of that wave objects, and a lane that skips the scatter neither votes nor writes."""
import numpy as np
import pytest

import scatter_probe as sp

pytestmark = pytest.mark.gpu

F32 = np.float32
# Cases with a non-unit normal (scatter_probe.main_cases()["nonunit"]) on which a kOptFastDiv form may differ from the
# oracle: none. Every form returns the oracle's bits on all of them.
NONUNIT_MAY_DIFFER = ()


def describe(i, rows, what):
    return (f"{what}: case {i} ({rows['tag'][i]}) n={rows['n'][i, :3].tolist()} d={rows['d'][i, :3].tolist()} "
            f"state={[hex(int(v)) for v in rows['states'][i]]}")


def same_bits(got_u32, want_f32, nan_ok):
    """Per row: equal bits in every column, or, where nan_ok, NaN on both sides."""
    want = np.ascontiguousarray(want_f32, F32)
    want_u = want.view(np.uint32).reshape(got_u32.shape)
    eq = got_u32 == want_u
    both_nan = np.isnan(got_u32.view(F32)) & np.isnan(want.reshape(got_u32.shape))
    eq = eq | (both_nan & np.reshape(nan_ok, (-1,) + (1,) * (got_u32.ndim - 1)))
    return eq.reshape(len(got_u32), -1).all(1)


def check(form, got, rows, ref, active, objecting, albedo, what):
    """Every active case against the oracle and the predicted vote; every inactive one against the sentinel."""
    act = active.astype(bool)
    nan_ok = rows["has_nan"]
    parts = {
        "origin": same_bits(got["ray"][:, 0:3], ref["ro"][:, :3], nan_ok),
        "direction": same_bits(got["ray"][:, 3:6], ref["rd"][:, :3], nan_ok),
        "q": same_bits(got["vals"][:, 1], ref["q"], nan_ok),
        "att": same_bits(got["vals"][:, 2], ref["att"][:, 0], nan_ok),
        "state": (got["states"] == ref["states"]).all(1),
    }
    for name, ok in parts.items():
        bad = np.flatnonzero(act & ~ok)
        assert bad.size == 0, f"{form} {name}: {bad.size} cases differ; " + describe(int(bad[0]), rows, what) + \
            f" got ray {got['ray'][bad[0]].view(F32).tolist()} vals {got['vals'][bad[0]].view(F32).tolist()}" \
            f" want ro {ref['ro'][bad[0], :3].tolist()} rd {ref['rd'][bad[0], :3].tolist()} q {ref['q'][bad[0]]!r}" \
            f" att {ref['att'][bad[0], 0]!r} cosw {ref['cosw'][bad[0]]!r} pdf {ref['pdf'][bad[0]]!r}"
    want_fb = sp.predicted_fallback(form, objecting, active)
    bad = np.flatnonzero(got["fell_back"] != want_fb)
    assert bad.size == 0, f"{form} fell_back: {bad.size} lanes differ, first lane {bad[0] % 64} of wave " \
        f"{bad[0] // 64}: got {got['fell_back'][bad[0]]} want {want_fb[bad[0]]}; " + describe(int(bad[0]), rows, what)
    off = ~act
    for k in ("ray", "vals", "states"):
        assert np.all(got[k][off] == sp.SENTINEL_WORD), f"{form} {k}: an inactive lane wrote ({what})"
    assert np.all(got["fell_back"][off] == sp.SENTINEL_BYTE), f"{form}: an inactive lane wrote its flag ({what})"
    # att is the call sites' expression of the coeff the probe returns
    coeff = got["vals"][:, 0].view(F32)
    with np.errstate(all="ignore"):
        att_of_coeff = ((F32(albedo) * coeff).astype(F32) * (F32(1.0) / F32(np.pi))).astype(F32)
    bad = np.flatnonzero(act & ~same_bits(got["vals"][:, 2], att_of_coeff, np.ones(len(act), bool)))
    assert bad.size == 0, f"{form}: att is not (albedo * coeff) * (1 / pi); " + describe(int(bad[0]), rows, what)


def take(d, idx):
    return {k: (v[idx] if isinstance(v, np.ndarray) else [v[i] for i in idx]) for k, v in d.items()}


# ------------------------------------------------------------------ the whole case set, every form, every material
@pytest.mark.parametrize("sigma,albedo", sp.SIGMAS, ids=[f"sigma{s:g}" for s, _ in sp.SIGMAS])
@pytest.mark.parametrize("form", list(sp.FORMS))
def test_every_case_equals_the_oracle(require_gpu, form, sigma, albedo):
    c = sp.main_cases()
    ref = sp.main_reference(sigma, albedo)
    obj = sp.objections(c["n"], c["d"], ref["rd"])
    active = np.ones(len(c["p"]), np.uint8)
    got = sp.gpu_scatter(form, sp.probe_inputs(c["p"], c["n"], c["d"]), c["states"], active, sigma, albedo)
    assert NONUNIT_MAY_DIFFER == ()                    # nothing is set aside: all of c is compared
    check(form, got, c, ref, active, sp.objects(obj), albedo, f"sigma {sigma} albedo {albedo}")
    if form in sp.LEAN_FORMS:                          # both paths ran, in different waves of one launch
        fb = got["fell_back"].reshape(-1)
        waves = [int(fb[w]) for w in range(0, len(fb), 64)]
        assert 0 in waves and 1 in waves


# ------------------------------------------------------------------ placement of one objecting lane
def placement_run(form, at, kind, active_objector, inactive_wave=None):
    c = sp.main_cases()
    ref = sp.main_reference(*sp.SIGMAS[0])
    base, pick = sp.placement_cases()
    idx = base.copy()
    idx[at] = pick[kind]
    rows, r = take(c, idx), take(ref, idx)
    objecting = sp.objects(sp.objections(rows["n"], rows["d"], r["rd"]))
    assert objecting.sum() == 1 and objecting[at]      # on the CPU, before the GPU is asked
    active = np.ones(len(idx), np.uint8)
    if not active_objector:
        active[at] = 0
    if inactive_wave is not None:
        active[64 * inactive_wave:64 * inactive_wave + 64] = 0
    sigma, albedo = sp.SIGMAS[0]
    got = sp.gpu_scatter(form, sp.probe_inputs(rows["p"], rows["n"], rows["d"]), rows["states"], active, sigma, albedo)
    what = f"objector ({kind}) at {at}, {'active' if active_objector else 'inactive'}, wave off: {inactive_wave}"
    check(form, got, rows, r, active, objecting, albedo, what)
    return got


@pytest.mark.parametrize("form", list(sp.FORMS))
def test_one_objecting_lane_moves_its_wave_and_no_other(require_gpu, form):
    for kind in sp.KINDS:
        for at in sp.PLACEMENT_AT:
            got = placement_run(form, at, kind, True)
            if form in sp.LEAN_FORMS:                  # stated once more without the helper: its wave, whole, alone
                fb = got["fell_back"]
                w = at // 64
                assert np.all(fb[64 * w:64 * w + 64] == 1) and fb.sum() == min(64, sp.PLACEMENT_N - 64 * w)
            got = placement_run(form, at, kind, False)
            if form in sp.LEAN_FORMS:                  # an inactive lane does not vote: every wave stays lean
                assert np.all(np.delete(got["fell_back"], at) == 0)


@pytest.mark.parametrize("form", list(sp.FORMS))
def test_a_whole_wave_inactive(require_gpu, form):
    placement_run(form, 70, "cto", True, inactive_wave=1)      # the objector sits in the wave that is off
    got = placement_run(form, 0, "d", True, inactive_wave=1)   # the wave before it falls back, the ones after do not
    if form in sp.LEAN_FORMS:
        fb = got["fell_back"]
        assert np.all(fb[:64] == 1) and np.all(fb[64:128] == sp.SENTINEL_BYTE) and np.all(fb[128:] == 0)


# ------------------------------------------------------------------ sphere mode: sphere_hit + oren_nayar_scatter
@pytest.mark.parametrize("form", list(sp.SPHERE_FORMS))
def test_sphere_hit_and_scatter_equal_the_oracle(require_gpu, form):
    s, ref = sp.sphere_cases()
    m = len(s["t"])
    objecting = sp.objects(sp.objections(s["n"], s["d"], ref["rd"]))
    active = np.ones(m, np.uint8)
    got = sp.gpu_scatter(form, sp.sphere_probe_inputs(s), s["states"], active, sphere=True)
    no = np.zeros(m, bool)
    parts = {"origin": same_bits(got["ray"][:, 0:3], ref["ro"][:, :3], no),
             "direction": same_bits(got["ray"][:, 3:6], ref["rd"][:, :3], no),
             "att * q": same_bits(got["vals"][:, 0], ref["value"], no),
             "state": (got["states"] == ref["states"]).all(1)}
    for name, ok in parts.items():
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, f"{form} {name}: {bad.size} cases differ, first {bad[0]} ({s['kind'][bad[0]]}, radius " \
            f"{s['r'][bad[0]]!r}, t {s['t'][bad[0]]!r}): got ray {got['ray'][bad[0]].view(F32).tolist()} value " \
            f"{got['vals'][bad[0], 0:1].view(F32)[0]!r} want ro {ref['ro'][bad[0], :3].tolist()} rd " \
            f"{ref['rd'][bad[0], :3].tolist()} value {ref['value'][bad[0]]!r}"
    assert np.all(got["vals"][:, 1:] == sp.SENTINEL_WORD)          # sphere mode writes the scalar alone
    assert np.array_equal(got["fell_back"], sp.predicted_fallback(form, objecting, active))
