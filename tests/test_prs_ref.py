"""CPU: the two numpy statements of the polygenic score weights (tests/prs_ref.py) against each other and against what the model says
in closed form, and the vetting of the cases tests/test_gpu_prs.py runs: none of them may hold a decision that rounding could turn."""
import numpy as np
import pytest

import prs_ref as pr

N = pr.N_STUDY


def _mats(M, U, seed, mode):
    p, gm, gu, z1 = pr.small_window(M, U, seed)
    B, _ = pr.mats(mode, gm, gu, p["off"], p["w"] if mode else None)
    return B, z1


@pytest.fixture(scope="module")
def window():
    """(B, z1, fit_cov's result on the default grid) of the pooled 65-SNP window: computed once, shared, left unchanged"""
    B, z1 = _mats(65, 3, 165, 0)
    return B, z1, pr.fit_cov(B, z1, N)


@pytest.mark.parametrize("case", pr.SMALL_CASES + [pr.NOCONV_CASE + (0,)], ids=pr.case_id)
def test_the_two_statements_agree_and_no_case_is_borderline(case):
    M, U, kw, seed, mode = case
    B, z1 = _mats(M, U, seed, mode)
    bl, want, e = pr.borderline(B, z1, N, **kw)
    assert bl == [], bl
    assert e <= 1e-12 and pr.value_tol(want, e) == 1e-8 * max(1.0, np.abs(want["beta"]).max())


def test_the_frozen_case_is_not_borderline():
    M, U, kw, seed, bad = pr.FROZEN_CASE
    B, z1 = _mats(M, U, seed, 0)
    z1[bad[0]], z1[bad[1]] = np.nan, np.inf
    bl, want, e = pr.borderline(B, z1, N, **kw)
    assert bl == [] and np.all(want["beta"][:, :, list(bad)] == 0) and np.all(want["r"][list(bad)] == 0) and want["nnz"].max() > 10


def test_s_equal_one_is_the_soft_threshold_whatever_b_is(window):
    B, z1, want = window
    r, _ = pr.p2cor(z1, N)
    i_s = pr.DEFAULT_S.index(1.0)
    junk = np.random.default_rng(1).standard_normal(B.shape)
    other = pr.fit_cov(junk, z1, N, s=(1.0,))
    for i_l, lam in enumerate(pr.DEFAULT_LAM):
        soft = np.sign(r) * np.maximum(np.abs(r) - lam, 0.0)
        assert np.array_equal(want["beta"][i_s, i_l], soft) and np.array_equal(other["beta"][0, i_l], soft)
    assert np.all(want["sweeps"][i_s] <= 2)


def test_a_penalty_of_r_max_or_more_gives_zero_in_one_sweep(window):
    B, z1, want = window
    got = pr.fit_cov(B, z1, N, lam=(want["rmax"], 1.0))
    assert np.all(got["beta"] == 0) and np.all(got["sweeps"] == 1) and np.all(got["nnz"] == 0) and not got["noconv"].any()
    none = pr.fit_cov(B, np.full(len(z1), np.nan), N)                  # r_max = 0: one sweep everywhere, no flag
    assert np.all(none["beta"] == 0) and np.all(none["sweeps"] == 1) and not none["noconv"].any() and none["rmax"] == 0.0


def test_no_penalty_meets_the_linear_solve_within_the_kkt_bound(window):
    B, z1, _ = window
    r, _ = pr.p2cor(z1, N)
    a = pr.args_of()
    got = pr.fit_cov(B, z1, N, lam=(0.0,), max_sweeps=1000)
    assert not got["noconv"].any()
    rowsum = np.abs(B).sum(axis=1)
    for i_s, s in enumerate(a["s"]):
        beta = got["beta"][i_s, 0]
        top, res, mag = pr.kkt(B, r, s, 0.0, beta)
        assert np.all(res <= (1.0 - s) * a["tol"] * got["rmax"] * rowsum + len(r) * 2.0 ** -52 * mag)
        exact = np.linalg.solve((1.0 - s) * B + s * np.eye(len(r)), r)
        # the residual of the linear system IS the KKT residual at lam = 0: the distance to the solve is at most ||A^-1|| times it
        A = (1.0 - s) * B + s * np.eye(len(r))
        assert np.max(np.abs(beta - exact)) <= np.linalg.norm(np.linalg.inv(A), np.inf) * max(top, 1e-15) * 1.0000001


def test_later_penalties_and_other_chains_do_not_reach_a_cell(window):
    B, z1, want = window
    short = pr.fit_cov(B, z1, N, s=pr.DEFAULT_S[1:2], lam=pr.DEFAULT_LAM[:7])
    for k in ("beta", "nnz", "sweeps", "delta", "br", "bg", "kkt"):
        assert np.array_equal(short[k][0], want[k][1, :7]), k


def test_the_certificate_holds_for_the_reference(window):
    B, z1, want = window
    a = pr.args_of()
    rowsum = np.abs(B).sum(axis=1)
    for i_s, s in enumerate(a["s"]):
        for i_l, lam in enumerate(a["lam"]):
            top, res, mag = pr.kkt(B, want["r"], s, lam, want["beta"][i_s, i_l])
            rnd = len(z1) * 2.0 ** -52 * mag
            assert np.all(res <= (1.0 - s) * a["tol"] * want["rmax"] * rowsum + rnd)
            assert abs(want["kkt"][i_s, i_l] - top) <= rnd.max()
