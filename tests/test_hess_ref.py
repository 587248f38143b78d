"""CPU: the two numpy statements of the hess rule (tests/hess_ref.py) against each other, against a planted truth and against
api.hess_estimates; the repair of non-finite entries; the var_frac -> k rule at ties; the refusals of api.hess_estimates.  No GPU."""
import os

import numpy as np
import pytest

import hess_ref as hr
from gauss_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spd(M, seed):
    """a full-rank correlation matrix with neighbours in LD"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((4 * M + 50, M))
    for j in range(1, M):
        X[:, j] = 0.6 * X[:, j - 1] + 0.8 * X[:, j]
    return np.atleast_2d(np.corrcoef(X, rowvar=False))


def test_the_header_states_the_rule_and_the_limits():
    text = open(os.path.join(ROOT, "include", "gauss_hip.h")).read()
    for line in ("int gauss_ld_hess_rows(", "#define GAUSS_HESS_MAX_M      4096", "#define GAUSS_HESS_MAX_TRAITS 64",
                 "#define GAUSS_HESS_MAX_K      1024", "#define GAUSS_ST_HESS_NOCONV      512", "does not depend on it"):
        assert line in text, line
    assert (_lib.HESS_MAX_M, _lib.HESS_MAX_TRAITS, _lib.HESS_MAX_K, _lib.ST_HESS_NOCONV) == (4096, 64, 1024, 512)
    assert "gauss_ld_hess_rows" in _lib.SYMBOLS


@pytest.mark.parametrize("M,T,k", [(1, 1, None), (7, 3, 4), (40, 5, None), (40, 2, 40)])
def test_the_two_statements_and_the_api_agree_on_the_estimators(M, T, k):
    rng = np.random.default_rng(M + T)
    R = _spd(M, M)
    z = rng.standard_normal((T, M)) * 3
    n = rng.integers(5_000, 90_000, size=T).astype(float)
    s = rng.uniform(-0.2, 0.2, size=(T, T))
    s = (s + s.T) / 2
    ref = hr.rule(R, z, k_max=M)
    a = hr.estimates(ref["lam"], ref["proj"], n, k=k, overlap=s)
    b = hr.estimates_loops(ref["lam"], ref["proj"], n, k=k, overlap=s)
    got = api.hess_estimates(ref["lam"], ref["proj"], n, k=k, overlap=s)
    assert a["k"] == b["k"] == got["k"] and 1 <= a["k"] <= M
    for name in ("H", "h2", "se"):
        np.testing.assert_allclose(a[name], b[name], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(got[name], b[name], rtol=1e-12, atol=1e-15)
    for name in ("C", "cov", "rg"):
        np.testing.assert_allclose(a[name], b[name], rtol=1e-11, atol=1e-14, equal_nan=True)
    ia, ib = got["pairs"]["a"], got["pairs"]["b"]
    assert len(ia) == T * (T - 1) // 2 and np.all(ia < ib)
    for name in ("C", "cov", "rg"):
        np.testing.assert_allclose(got["pairs"][name], b[name][ia, ib], rtol=1e-11, atol=1e-14, equal_nan=True)
    np.testing.assert_array_equal(got["pairs"]["s"], s[ia, ib])
    # the curve holds H at every k, and its column k - 1 is H
    assert got["curve"].shape == (T, M) and np.array_equal(got["curve"][:, got["k"] - 1], got["H"])
    assert abs(got["var_curve"][-1] - 1.0) < 1e-12 and got["var_kept"] == got["var_curve"][got["k"] - 1]


def test_a_planted_truth_is_recovered():
    """z = R b exactly, R of full rank, k = M: H = b^T R b and C_ab = b_a^T R b_b"""
    M, T = 30, 3
    rng = np.random.default_rng(3)
    R = _spd(M, 11)
    b = rng.standard_normal((T, M))
    z = b @ R
    ref = hr.rule(R, z, k_max=M, eig_min=0.0)
    assert ref["n_pos"] == M
    truth = b @ R @ b.T
    for est in (hr.estimates(ref["lam"], ref["proj"], 1e5, k=M, eig_min=0.0), hr.estimates_loops(ref["lam"], ref["proj"], 1e5, k=M, eig_min=0.0)):
        np.testing.assert_allclose(est["H"], np.diag(truth), rtol=1e-10)
        np.testing.assert_allclose(est["C"], truth, rtol=1e-10, atol=1e-10 * np.abs(truth).max())
    got = api.hess_estimates(ref["lam"], ref["proj"], 1e5, k=M, eig_min=0.0)
    np.testing.assert_allclose(got["H"], np.diag(truth), rtol=1e-10)
    # flipping the sign of any eigenvector changes nothing
    flipped = ref["proj"] * np.where(np.arange(M) % 2, -1.0, 1.0)[None, :]
    again = api.hess_estimates(ref["lam"], flipped, 1e5, k=M, eig_min=0.0)
    assert np.array_equal(again["H"], got["H"]) and np.array_equal(again["pairs"]["C"], got["pairs"]["C"])


def test_the_repair_of_non_finite_entries():
    M = 9
    R = _spd(M, 5)
    R[4, :] = R[:, 4] = np.nan
    R[4, 4] = 1.0                                           # a monomorphic SNP: every off-diagonal entry NaN, the diagonal 1
    R[1, 7] = R[7, 1] = np.inf                              # any other non-finite entry: 0, counted once per pair
    R[2, 3] = R[3, 2] = np.nan
    Rp, mono, n_bad = hr.repair(R)
    assert list(np.flatnonzero(mono)) == [4] and n_bad == 2
    assert np.all(Rp[4] == 0) and np.all(Rp[:, 4] == 0) and Rp[4, 4] == 0 and Rp[1, 7] == 0 and Rp[2, 3] == 0 and np.all(np.isfinite(Rp))
    assert Rp[0, 0] == 1.0 and Rp[0, 1] == R[0, 1]
    z = np.arange(1.0, 2 * M + 1).reshape(2, M)
    z[0, 2], z[1, 4] = np.nan, np.inf
    zr = hr.repair_z(z, mono)
    assert zr[0, 2] == 0 and np.all(zr[:, 4] == 0) and zr[1, 2] == z[1, 2]
    ref = hr.rule(R, z, k_max=M)
    assert ref["n_pos"] <= M - 1 and np.all(np.isnan(ref["proj"][:, ref["n_pos"]:])) and np.all(np.isfinite(ref["proj"][:, :ref["n_pos"]]))
    # the monomorphic SNP's z does not matter
    z2 = z.copy()
    z2[:, 4] = 1e6
    assert np.array_equal(hr.rule(R, z2, k_max=M)["proj"], ref["proj"], equal_nan=True)
    # M = 1 is no monomorphic SNP
    one = hr.rule(np.array([[1.0]]), np.array([[3.0]]), k_max=2)
    assert one["n_pos"] == 1 and one["proj"][0, 0] == 3.0 and np.isnan(one["proj"][0, 1]) and not one["mono"][0]


def test_var_frac_takes_the_smallest_k_that_reaches_it_ties_included():
    lam = np.array([4.0, 2.0, 1.0, 1.0, 0.0, 0.0])        # shares 0.5, 0.75, 0.875, 1
    proj = np.ones((1, 6))
    for frac, k in ((0.5, 1), (0.50001, 2), (0.75, 2), (0.875, 3), (0.9, 4), (1.0, 4), (0.01, 1)):
        assert api.hess_estimates(lam, proj, 100, var_frac=frac)["k"] == k, frac
        assert hr.choose_k(lam, 6, 4, None, frac) == k, frac
    # capped at n_pos = 4 and at k_max
    assert api.hess_n_pos(lam) == 4 and api.hess_estimates(lam, proj, 100, k=6)["k"] == 4
    assert api.hess_estimates(lam, proj[:, :2], 100, var_frac=0.99)["k"] == 2
    assert api.hess_n_pos([1.0, 1e-7]) == 1 and api.hess_n_pos([1.0, 1e-7], eig_min=0.0) == 2 and api.hess_n_pos([0.0, 0.0]) == 0
    none = api.hess_estimates(np.zeros(3), np.full((2, 3), np.nan), 100)
    assert none["k"] == 0 and np.all(none["H"] == 0) and np.all(np.isnan(none["h2"])) and np.all(np.isnan(none["pairs"]["rg"]))


def test_rg_is_nan_unless_both_h2_are_positive():
    lam = np.array([2.0, 1.0])
    proj = np.array([[30.0, 20.0], [0.5, 0.5], [25.0, -10.0]])
    got = api.hess_estimates(lam, proj, [1000, 1000, 2000], k=2)
    assert got["h2"][0] > 0 and got["h2"][1] < 0 and got["h2"][2] > 0
    rg = dict(zip(zip(got["pairs"]["a"], got["pairs"]["b"]), got["pairs"]["rg"]))
    assert np.isnan(rg[(0, 1)]) and np.isnan(rg[(1, 2)]) and np.isfinite(rg[(0, 2)])
    assert got["pairs"]["C"][1] == 30.0 * 25.0 + 20.0 * -10.0


def test_hess_estimates_refusals():
    lam, proj = np.array([2.0, 1.0, 0.5]), np.ones((2, 3))
    for text, kw in (("lam has shape", dict(lam=np.ones((2, 2)))), ("lam has shape", dict(lam=np.zeros(0))), ("proj has shape", dict(proj=np.ones(3))),
                     ("not in descending order", dict(lam=np.array([1.0, 2.0, 0.5]))), ("n has 3 entries for 2 traits", dict(n=[1e4, 1e4, 1e4])),
                     ("every n must be positive", dict(n=[1e4, 0])), ("every n must be positive", dict(n=np.nan)),
                     ("k = 0; it must be", dict(k=0)), ("k = 1.5; it must be", dict(k=1.5)), ("var_frac = 0 is outside (0, 1]", dict(var_frac=0)),
                     ("var_frac = 1.2 is outside (0, 1]", dict(var_frac=1.2)), ("is not above k = 3", dict(n=3, k=3)),
                     ("eig_min = 1.0 is outside [0, 1)", dict(eig_min=1.0)), ("overlap has shape (3, 3)", dict(overlap=np.zeros((3, 3)))),
                     ("overlap has shape", dict(overlap=np.nan))):
        a = dict(lam=lam, proj=proj, n=1e4)
        a.update(kw)
        with pytest.raises(api.GaussError) as e:
            api.hess_estimates(**a)
        assert text in str(e.value), (text, str(e.value))
