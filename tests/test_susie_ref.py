"""CPU: the multi-causal fit's definition (tests/susie_ref.py) -- the textbook statement with R formed explicitly against the W form the
kernels evaluate, an independent plain SuSiE-RSS loop for measured_only, the two planted windows the feature rests on, and every case
of tests/test_gpu_susie.py: the two statements agree (their gap is the case's e_ref) and no decision is borderline, so that the GPU
test may compare sizes, sets, kept flags and sweeps exactly."""
import numpy as np
import pytest

import cs_ref
import susie_ref as sr
from cond_ref import window_mats
from slct_ref import min_var_frac, slct_by_definition

E_REF_MAX = 1e-10         # the two statements share no product: what separates them is rounding carried through the sweeps.  A committed
                          # case stays a factor of ten or more below this (a seed whose gap came close, 7e-10, was replaced): it must hold
                          # with another BLAS too


def vet(B, C, z, what, **kw):
    """Both statements; returns (W-form result, e_ref).  Exact outputs must agree and nothing may be borderline."""
    a, b = sr.fit_textbook(B, C, z, **kw), sr.fit_w(B, C, z, **kw)
    e_ref = sr.gap(a, b)
    tol = sr.value_tol(b, e_ref)
    print(f"susie {what}: T {b['alpha'].shape[1]}  sweeps {b['sweeps']}  kept {int(b['kept'].sum())}  sizes {b['size'].tolist()}  "
          f"e_ref {e_ref:.2e}  tol {tol:.2e}  r_max {b['rmax']:.2f}")
    assert e_ref <= E_REF_MAX, (what, e_ref)
    for k in sr.EXACT_KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)
    assert np.array_equal(a["member"], b["member"]), what
    assert sr.borderline(b, kw, tol) == [], (what, sr.borderline(b, kw, tol))
    return b, e_ref


def _case(M, U, kw, seed, mode=0):
    p, gm, gu, z1 = sr.small_window(M, U, seed)
    B, C = window_mats(mode, gm, gu, p["off"], p["w"] if mode else None)
    return B, C, z1


@pytest.mark.parametrize("case", sr.SMALL_CASE_MODES, ids=lambda c: f"M{c[0]}-U{c[1]}-L{c[2].get('L', 10)}-s{c[2].get('max_sweeps')}-mode{c[4]}")
def test_small_cases_are_committable(case):
    M, U, kw, seed, mode = case
    res, _ = vet(*_case(M, U, kw, seed, mode), f"M={M} U={U} mode={mode} {kw}", **kw)
    assert res["sweeps"] == kw["max_sweeps"]                   # tol = 0 runs them all


def test_the_other_cases_are_committable():
    M, U, kw, seed = sr.CONVERGENCE_CASE
    res, _ = vet(*_case(M, U, kw, seed), "convergence", **kw)
    assert res["converged"] and 1 < res["sweeps"] < sr.DEFAULTS["max_sweeps"]
    M, U, kw, seed = sr.NOCONV_CASE
    res, _ = vet(*_case(M, U, kw, seed), "no convergence", **kw)
    assert not res["converged"] and res["sweeps"] == kw["max_sweeps"] and np.all(np.isfinite(res["alpha"]))
    M, U, seed = sr.COVERAGE_WINDOW
    sizes = []
    for kw in sr.COVERAGE_CASES:
        res, _ = vet(*_case(M, U, kw, seed, mode=1), f"coverage {kw}", **kw)
        sizes.append(res["size"])
    assert np.all(sizes[0] <= sizes[1])
    admissible = int(res["adm"].sum())
    assert np.all(sizes[1] == admissible)                      # rho = 1 takes every alpha > 0
    # pure noise: nothing beats the null
    B, C, _ = _case(65, 40, {}, 9)
    z = np.random.default_rng(5).multivariate_normal(np.zeros(65), B) * 0.7
    res, _ = vet(B, C, z, "null window")
    assert np.all(res["V"] == 0) and np.all(res["pip"] == 0) and not res["kept"].any()
    # a NaN in z1: that SNP and every unmeasured SNP are no candidates
    B, C, z = _case(12, 11, {}, 14)
    z[5] = np.nan
    res, _ = vet(B, C, z, "NaN in z1", L=3)
    assert not res["adm"][5] and not res["adm"][12:].any() and res["adm"].sum() == 11
    assert np.all(res["alpha"][:, 5] == 0) and np.all(res["alpha"][:, 12:] == 0) and np.all(np.isfinite(res["pip"]))


def test_no_admissible_candidate():
    """Every z1 non-finite: alpha = mu = 0, pip 0, lse NaN, V 0 after the first sweep's null check, no set, one sweep"""
    B, C, _ = _case(12, 11, {}, 14)
    res, e_ref = vet(B, C, np.full(12, np.nan), "every z1 NaN", L=3)
    assert not res["adm"].any() and np.all(res["alpha"] == 0) and np.all(res["mu"] == 0) and np.all(res["pip"] == 0)
    assert np.all(np.isnan(res["lse"])) and np.all(res["V"] == 0) and np.all(res["size"] == 0) and not res["kept"].any()
    assert res["sweeps"] == 1 and e_ref == 0.0


def test_the_large_case_is_committable():
    M, U, kw, seed = sr.LARGE_CASE
    p, gm, gu = cs_ref.window(M, U, scale=0.1)
    B, C = window_mats(1, gm, gu, p["off"], p["w"])
    vet(B, C, cs_ref.planted(gm, seed=seed), "chr22's largest shape", **kw)


def test_measured_only_is_plain_susie_rss():
    """With measured_only the fit is SuSiE-RSS on (z, B): an independent loop that shares no helper returns the same alpha"""
    for (M, U, seed, ev) in ((12, 11, 14, True), (40, 9, 4, False), (65, 20, 10, True)):
        B, C, z = _case(M, U, {}, seed)
        kw = dict(L=4, tol=0.0, max_sweeps=6, estimate_var=ev, measured_only=True)
        res, _ = vet(B, C, z, f"measured_only M={M}", **kw)
        want = sr.plain_rss(z, B, 4, 25.0, 6, 0.0, ev)
        err = float(np.max(np.abs(res["alpha"][:, :M] - want)))
        print(f"susie measured_only M={M}: |alpha - plain SuSiE-RSS| {err:.2e}")
        assert err <= 1e-10 and np.all(res["alpha"][:, M:] == 0)


def test_the_tag_window():
    """(a) One measured tag of two causal SNPs has the largest marginal |z|: the stepwise selection takes the tag first; the fit
    returns two kept sets, one around each causal SNP, and neither holds the tag."""
    p, gm, gu, z1, (c1, c2, tag) = sr.tag_window()
    B, C = window_mats(0, gm, gu, p["off"], None)
    assert int(np.argmax(np.abs(z1))) == tag
    sel = slct_by_definition(B, z1, 5, cs_ref.CHI2_GWS, min_var_frac(0.9, 0.1))
    assert sel["n"] >= 1 and int(sel["idx"][0]) == tag
    res, _ = vet(B, C, z1, "tag window")
    kept = np.flatnonzero(res["kept"])
    assert len(kept) == 2
    leads = sorted(int(np.argmax(res["alpha"][l])) for l in kept)
    assert leads == sorted((c1, c2))
    for l in kept:
        assert not res["member"][l][tag] and res["purity"][l] >= 0.5
    assert res["pip"][tag] < 0.05 and res["pip"][c1] > 0.9 and res["pip"][c2] > 0.9


def test_the_claim_window():
    """(b) cs_ref.claim_window(): the unmeasured causal SNP leads its set ahead of the measured lead SNP"""
    p, gm, gu, z1, u = cs_ref.claim_window()
    B, C = window_mats(0, gm, gu, p["off"], None)
    M = gm.shape[0]
    res, _ = vet(B, C, z1, "claim window")
    kept = np.flatnonzero(res["kept"])
    assert len(kept) == 3
    sets = [l for l in kept if res["member"][l][M + u]]
    assert len(sets) == 1
    l = sets[0]
    assert int(np.argmax(res["alpha"][l])) == M + u
    measured = res["alpha"][l][:M]
    assert res["alpha"][l][M + u] > measured.max()
