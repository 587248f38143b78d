"""CPU suite: zmix's constrained quadratic program (gauss_host_zmix_qp, the Goldfarb-Idnani method of quadprog::solve.QP) against
a KKT certificate, the reduced solve on the free set and scipy's SLSQP; permutation, a singular D and the rounding step."""
import numpy as np
import pytest

from gauss_amd import api

from zmix_ref import finish, kkt, reduced_solve


def _spd(P, rng, cond=1e3):
    Q, _ = np.linalg.qr(rng.standard_normal((P, P)))
    ev = np.exp(rng.uniform(0, np.log(cond), P))
    D = (Q * ev) @ Q.T
    return (D + D.T) / 2


def _problem(P, kind, rng):
    """D, d and the known optimum w* (strict complementarity: the multipliers of the zero weights are clear of 0)."""
    D = _spd(P, rng)
    w = np.zeros(P)
    if kind == "interior":
        w = rng.dirichlet(np.ones(P))
    elif kind == "boundary":
        sup = rng.choice(P, size=max(1, P // 2), replace=False)
        w[sup] = rng.dirichlet(np.ones(len(sup)))
    else:                                                       # vertex: w = e_k, every other w >= 0 active with w_k <= 1
        w[rng.integers(P)] = 1.0
    nu = rng.normal()
    lam = np.where(w > 0, 0.0, rng.uniform(0.1, 1.0, P))
    d = D @ w - nu - lam                                        # D w - d = nu 1 + lam
    return D, d, w


def _slsqp(D, d):
    from scipy.optimize import minimize
    P = len(d)
    res = minimize(lambda w: 0.5 * w @ D @ w - d @ w, np.full(P, 1.0 / P), jac=lambda w: D @ w - d, method="SLSQP",
                   bounds=[(0.0, 1.0)] * P, constraints=[dict(type="eq", fun=lambda w: np.sum(w) - 1.0, jac=lambda w: np.ones(P))],
                   options=dict(ftol=1e-15, maxiter=1000))
    return res.x


@pytest.mark.parametrize("P", [1, 2, 6, 21, 26, 29, 64])
@pytest.mark.parametrize("kind", ["interior", "boundary", "vertex"])
def test_qp_optimum(P, kind):
    rng = np.random.default_rng(1000 * P + len(kind))
    D, d, w_star = _problem(P, kind, rng)
    w_unr, w_fin = api.zmix_qp(D, d)
    assert kkt(D, d, w_unr) == []
    F = w_unr > 1e-10
    assert np.max(np.abs(w_unr - reduced_solve(D, d, F))) <= 1e-10
    assert np.max(np.abs(w_unr - w_star)) <= 1e-10
    assert np.array_equal(w_fin, finish(w_unr)[1]) or np.max(np.abs(w_fin - finish(w_unr)[1])) <= 1e-15
    if P <= 29:
        assert np.max(np.abs(w_unr - _slsqp(D, d))) <= 1e-6


def test_qp_permutation():
    rng = np.random.default_rng(5)
    for kind in ("interior", "boundary", "vertex"):
        D, d, _ = _problem(12, kind, rng)
        perm = rng.permutation(12)
        w, _ = api.zmix_qp(D, d)
        wp, _ = api.zmix_qp(D[np.ix_(perm, perm)], d[perm])
        assert np.max(np.abs(wp - w[perm])) <= 1e-12


def test_qp_not_positive_definite():
    rng = np.random.default_rng(8)
    X = rng.integers(-3, 4, (12, 5)).astype(np.float64)
    X[:, 1] = X[:, 3]                                           # a repeated column: D singular
    D = X.T @ X
    with pytest.raises(api.GaussError, match="matrix D in quadratic function is not positive definite!"):
        api.zmix_qp(D, rng.standard_normal(5))
    X[:, 3] = 0.0
    X[[0, 1, 2], 3] = [1.0, 2.0, 2.0]
    X[:, 0] = X[:, 3]                                           # exact arithmetic: the second pivot is 9 - 3^2 = 0
    with pytest.raises(api.GaussError, match="not positive definite"):
        api.zmix_qp(X.T @ X, np.ones(5))


@pytest.mark.parametrize("w_star,want", [
    ([0.123456, 0.234561, 0.641983], [0.12346, 0.23456, 0.64198]),
    ([0.333334, 0.333333, 0.333333], [1 / 3, 1 / 3, 1 / 3]),
    ([0.5, 0.25, 0.125, 0.125], [0.5, 0.25, 0.125, 0.125]),
    ([0.999996, 0.000004], [1.0, 0.0]),
    ([0.7000012, 0.1999982, 0.1000006, 0.0], [0.7, 0.2, 0.1, 0.0]),
    ([0.411112, 0.411112, 0.177776], [0.41111, 0.41111, 0.17778]),
])
def test_rounding_and_renormalisation(w_star, want):
    """D = I and d = w* + nu put the optimum at w* (all of it on the simplex): the final weights are w* / sum, rounded to five
    decimals (none of these values is near a half-way point) and normalised again, as zmix.R does."""
    w_star = np.array(w_star, dtype=np.float64)
    P = len(w_star)
    assert abs(w_star.sum() - 1.0) <= 1e-15
    D = np.eye(P)
    d = w_star + 0.3
    w_unr, w_fin = api.zmix_qp(D, d)
    assert np.max(np.abs(w_unr - w_star / w_star.sum())) <= 1e-12
    r = np.round(w_star / w_star.sum() * 1e5) / 1e5
    assert np.max(np.abs(w_fin - r / r.sum())) <= 1e-15
    assert np.max(np.abs(w_fin - np.array(want))) <= 1e-15
    assert abs(w_fin.sum() - 1.0) <= 1e-15


def test_qp_rejects_bad_shapes():
    with pytest.raises(ValueError):
        api.zmix_qp(np.eye(3), np.ones(2))
