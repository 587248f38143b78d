"""CPU: the definition of the multi-trait fit and of the colocalisation of its traits (tests/coloc_ref.py).  Every case of
tests/test_gpu_coloc.py: each trait's two statements of the fit agree (susie_ref), the two statements of the colocalisation agree, and
no decision -- of a fit, or the hit of a pair -- is borderline, so that the GPU test may compare sizes, sets, kept flags, sweeps and
hits exactly.  The planted claims hold for the reference alone."""
import numpy as np
import pytest

import coloc_ref as cr
import susie_ref as sr
from cond_ref import window_mats

E_REF_MAX = 1e-10          # tests/test_susie_ref.py's bound on the gap between the fit's two statements
DIRECT_TOL = 1e-9          # the two statements of the colocalisation share no sum: what separates them is the rounding of some thousand
                           # terms of size <= 1 each (n^2 of them in the direct H3), carried through one division


def vet(B, C, z1, z_more, k, kw, what, direct=True):
    """Every trait's fit by both statements, then the pairs by both; returns (fits, tolerances, pairs)"""
    fits, tols = [], []
    for t in range(k + 1):
        z = z1 if t == 0 else z_more[t - 1]
        a, b = sr.fit_textbook(B, C, z, **kw), sr.fit_w(B, C, z, **kw)
        e_ref = sr.gap(a, b)
        assert e_ref <= E_REF_MAX, (what, t, e_ref)
        for key in sr.EXACT_KEYS:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (what, t, key)
        fits.append(b)
        tols.append(sr.value_tol(b, e_ref))
    bl = cr.borderline(fits, kw, tols)
    assert bl == [], (what, bl)
    want = cr.pairs(fits)
    n_kept = int(np.sum(want["hit"] >= 0))
    print(f"coloc {what}: traits {k + 1}  sweeps {[f['sweeps'] for f in fits]}  kept {[int(f['kept'].sum()) for f in fits]}  "
          f"pairs of kept effects {n_kept}  tol {max(tols):.2e}")
    if direct:
        other = cr.pairs(fits, statement=cr.coloc_direct)
        assert np.array_equal(want["hit"], other["hit"]) and np.array_equal(want["n"], other["n"]), what
        for key in ("pp", "hit_pp"):
            assert np.array_equal(np.isnan(want[key]), np.isnan(other[key])), (what, key)
            assert float(np.nanmax(np.abs(want[key] - other[key]), initial=0.0)) <= DIRECT_TOL, (what, key)
    return fits, tols, want


@pytest.mark.parametrize("case", cr.CASE_MODES, ids=lambda c: f"M{c[0]}-U{c[1]}-L{c[2].get('L', 10)}-k{c[3]}-mode{c[5]}")
def test_cases_are_committable(case):
    M, U, kw, k, seed, mode = case
    p, gm, gu, z1, z_more = cr.case_window(M, U, k, seed)
    B, C = window_mats(mode, gm, gu, p["off"], p["w"] if mode else None)
    fits, _, want = vet(B, C, z1, z_more, k, kw, f"M={M} U={U} mode={mode}", direct=M + U <= 600)
    if (M, U) == (1, 1):
        assert want["n"][0] == 1 and fits[0]["kept"][0] and fits[1]["kept"][0] and want["pp"][0, 0, 0, 3] == 0.0 and want["hit"][0, 0, 0] == 0
    else:
        assert np.any(want["hit"] >= 0)                          # some pair of kept effects exists: the case tests the kernel


def test_the_traits_of_one_case_stop_at_different_sweeps():
    p, gm, gu, z1, z_more, kw = cr.sweeps_window()
    B, C = window_mats(0, gm, gu, p["off"], None)
    fits, _, want = vet(B, C, z1, z_more, 1, kw, "different sweeps")
    assert fits[0]["converged"] and fits[1]["converged"] and fits[0]["sweeps"] != fits[1]["sweeps"]
    assert not fits[1]["kept"].any() and np.all(np.isnan(want["pp"])) and np.all(want["hit"] == -1)      # a null trait: no pair


def test_the_planted_claims_hold_for_the_reference():
    def one(which):
        p, gm, gu, z1, z_more = cr.planted_window(which)
        B, C = window_mats(0, gm, gu, p["off"], None)
        return vet(B, C, z1, z_more, 1, {}, which)
    fits, _, want = one("shared")
    (la,), (lb,) = np.flatnonzero(fits[0]["kept"]), np.flatnonzero(fits[1]["kept"])
    assert int(np.argmax(want["pp"][0, la, lb])) == 4 and want["hit"][0, la, lb] == 52
    fits, _, want = one("distinct")
    (la,), (lb,) = np.flatnonzero(fits[0]["kept"]), np.flatnonzero(fits[1]["kept"])
    assert int(np.argmax(want["pp"][0, la, lb])) == 3
    fits, _, want = one("unmeasured")
    (la,), (lb,) = np.flatnonzero(fits[0]["kept"]), np.flatnonzero(fits[1]["kept"])
    assert int(np.argmax(want["pp"][0, la, lb])) == 4 and want["hit"][0, la, lb] == 100 + 7
    fits, _, want = one("null")
    assert fits[0]["kept"].any() and not fits[1]["kept"].any() and np.all(np.isnan(want["pp"])) and np.all(want["hit"] == -1)


def test_n_is_one_and_the_two_statements_on_hand_made_rows():
    """n = 1: S1 S2 = S12 to the bit, PP.H3 an exact 0.  Ties go to the smaller index.  Nothing admissible in both: NaN / -1."""
    l1, l2 = np.array([3.0, -np.inf, 1.0]), np.array([2.5, 0.5, -np.inf])
    r = cr.coloc(l1, l2, np.array([True, False, False]), **cr.PRIORS)
    assert r["n"] == 1 and r["pp"][3] == 0.0 and r["hit"] == 0 and r["hit_pp"] == 1.0 and abs(r["pp"].sum() - 1.0) < 1e-15
    l1, l2 = np.array([1.0, 4.0, 4.0, 0.0]), np.array([2.0, 3.0, 3.0, 0.0])
    a, b = cr.coloc(l1, l2, np.ones(4, bool), **cr.PRIORS), cr.coloc_direct(l1, l2, np.ones(4, bool), **cr.PRIORS)
    assert a["hit"] == b["hit"] == 1 and np.allclose(a["pp"], b["pp"], rtol=0, atol=1e-14) and abs(a["hit_pp"] - b["hit_pp"]) < 1e-15
    r = cr.coloc(l1, l2, np.zeros(4, bool), **cr.PRIORS)
    assert r["n"] == 0 and r["hit"] == -1 and np.all(np.isnan(r["pp"]))


@pytest.mark.parametrize("mix", [False, True])
def test_the_study_of_the_end_to_end_test_is_committable(tmp_path, mix):
    """The window the host calls build from the three study files: no fit and no hit is borderline, trait 2 shares a signal with trait 1"""
    import cs_ref
    st = cr.study(tmp_path)
    fw = cs_ref.feeder_window(mix, st["files"])
    B, C = window_mats(1 if mix else 0, fw["gm"], fw["gu"], fw["off"], fw["w"])
    z1 = np.array([s.z for s in fw["meas"]])
    fits, _, want = vet(B, C, z1, cr.study_z_more(fw["meas"], st["more"]), 2, cr.STUDY_ARGS, f"study mix={mix}", direct=False)
    assert fits[0]["kept"].any() and fits[1]["kept"].any() and np.any(np.argmax(want["pp"][0][want["hit"][0] >= 0], axis=1) == 4)
