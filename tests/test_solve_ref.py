"""CPU side of the ill-conditioned window-solve tests (tests/test_gpu_solve_illcond.py holds the kernels): every case is well
posed, the truth is the truth, the recorded levels are reproduced, and the bounds that follow from them reject five subtly
wrong versions of the kernel's algebra.

Why the GPU is compared with an exact-residual truth on its own matrices and not with the oracle: at the lam = 1.01e-5 cases
(cond(B11) 2e5 .. 3e5) the oracle's route -- the reference's full-pivot-LU inverse, whose entries reach 1e5 -- gets info wrong
by 4e-13 .. 6e-12, the Cholesky route by 4e-16 .. 3e-15: more than 100 times less at every one of them
(tests/golden/solve_levels.json, test_levels_are_reproduced asserts it).  A comparison with the oracle could therefore not
see a kernel that had lost three digits of info.  z is different: both routes get the numerator b21 B11^-1 z1 wrong by
1e-12 .. 4e-10, because the component of z1 along the small eigenvector is divided by lam and cancels only in exact
arithmetic; the bound for z follows that level, case by case.
"""
import numpy as np
import pytest

import clamp_ref as cr
import solve_ref as sr
from solve_ref import CASES, CLAMP_CHECKED, MUTATIONS, SMALL_LAM, UNCLAMPED

LEVELS = sr.load_levels()
NOISE = sr.FLOOR / sr.FACTOR          # a level below this cannot move a bound (bound() floors at FLOOR): it is a few ulps of noise


def test_the_case_list_covers_what_it_is_meant_to():
    assert set(LEVELS["solve"]) == set(UNCLAMPED) and set(LEVELS["clamp"]) == set(CLAMP_CHECKED)
    shapes = {(c.M, c.U) for c in CASES.values()}
    assert {(M, U) for M in (63, 64, 65, 129, 200) for U in (33, 130)} <= shapes and (640, 16) in shapes
    assert {c.place for c in CASES.values()} == {"first", "last", "straddle", "blockend", "three", "near"}
    assert {c.place for n, _ in sr.PAIRS for c in [CASES[n]]} == {"first", "last", "straddle", "blockend", "three", "near"}
    assert {c.lam for c in CASES.values() if c.eps == cr.EPS} == {1.01e-5, 1e-4, 1e-3, 0.99e-5, 0.0}
    assert {(c.lam, c.eps) for c in CASES.values() if c.eps != cr.EPS} == {(1.01e-3, 1e-3), (0.99e-3, 1e-3)}
    assert {c.mode for c in CASES.values()} == {0, 1} and {CASES[n].mode for n in sr.FORMS} == {0, 1}
    # every launch form sees every unclamped case of the three sizes: all placements, all three lam and the caller's own eps
    assert set(sr.FORMS) == {n for n in UNCLAMPED if CASES[n].M in (65, 129, 200)} and len(sr.FORMS) == 14
    assert {CASES[n].place for n in sr.FORMS} == {"last", "straddle", "blockend", "three", "near"}
    assert {CASES[n].lam for n in sr.FORMS} == {1.01e-5, 1e-4, 1e-3, 1.01e-3} and {CASES[n].eps for n in sr.FORMS} == {cr.EPS, 1e-3}
    assert len(sr.FORMS_BELOW) == 8 and all(CASES[n].lam < CASES[n].eps for n in sr.FORMS_BELOW)
    assert {CASES[n].place for n in sr.FORMS_BELOW} == {"last", "straddle", "blockend", "three", "near"}
    for M in (65, 129, 200):
        assert {CASES[n].lam for n in CLAMP_CHECKED if CASES[n].M == M and CASES[n].eps == cr.EPS} == {0.99e-5, 0.0}
    # the placements are what their names say, in terms of the factor block (NB rows) a tiny pivot falls into
    assert sr.NB == 64
    assert [r // sr.NB for r, _, _ in sr.duplicates("three", 129)] == [0, 1, 2]
    assert sr.duplicates("straddle", 129) == [(64, 63, 0)] and sr.duplicates("blockend", 129) == [(63, 62, 0)]
    assert sr.duplicates("first", 129) == [(1, 0, 0)] and sr.duplicates("last", 129) == [(128, 0, 0)]
    for name, lv in LEVELS["solve"].items():
        assert sr.FACTOR * lv["z"] <= sr.CEILING and sr.FACTOR * lv["info"] <= sr.CEILING, name
    for name, lv in LEVELS["clamp"].items():
        for what in ("b11", "cert", "info", "z", "info_own", "z_own"):
            assert cr.FACTOR * lv[what] <= cr.CEILING[what], (name, what)


@pytest.mark.parametrize("name", list(CASES))
def test_case_is_well_posed(name):
    c = CASES[name]
    win, o = sr.window(c), sr.oracle_run(name)
    dup = sr.duplicates(c.place, c.M)
    exact = [d for d in dup if d[2] == 0]
    for row, src, changed in dup:
        assert int(np.sum(win["geno_m"][row] != win["geno_m"][src])) == changed
    assert all(abs(win["z1"][row] - win["z1"][src]) > 1e-3 for row, src, _ in exact)      # z1 differs on a duplicate pair
    A, _ = cr.raw_b11(win)
    ev = np.linalg.eigvalsh(A)
    # the planted spectrum: one eigenvalue at lam for every exact duplicate, nothing else near eps or below
    assert np.max(np.abs(ev[:len(exact)] - c.lam)) <= 1e-12, ev[:4]
    assert ev[len(exact)] - c.lam > 1e-3 and ev[len(exact)] > 1.5 * c.eps
    if c.place == "near":
        assert int(np.sum((ev > c.lam + 1e-4) & (ev < 2e-2))) >= 6, ev[:12]
    clamps = c.lam < c.eps
    assert o["mpd"] == int(clamps)
    assert np.all(np.isfinite(o["z"])) and np.all(np.isfinite(o["info"])) and np.all(o["info"] > 0)
    evo = np.linalg.eigvalsh(o["b11"])
    assert abs(evo[0] - max(c.lam, c.eps)) <= 1e-12, evo[0]
    assert abs(c.lam / c.eps - 1.0) >= 0.0099          # never a coin toss: at least 1 % (1e-7 absolute) from eps, rounding moves it 1e-15


@pytest.mark.parametrize("name", [n for n in UNCLAMPED if CASES[n].M <= 65])
def test_truth_against_mpmath(name):
    """truth_solve against a plain 50-digit LU solve that shares nothing with it (no LAPACK, no refinement, no fixed point)."""
    import mpmath as mp
    o, t = sr.oracle_run(name), sr.oracle_truth(name)
    rhs = np.column_stack([o["b21"].T, sr.window(CASES[name])["z1"]])
    M, R = rhs.shape
    with mp.workdps(50):
        A = mp.matrix(M, M)
        for i in range(M):
            for j in range(M):
                A[i, j] = mp.mpf(float(o["b11"][i, j]))
        LU, perm = mp.mp.LU_decomp(A)
        worst = mp.mpf(0)
        for r in sorted(set(range(0, R, 8)) | {R - 1}):           # every 8th unmeasured row and z1
            b = mp.matrix([mp.mpf(float(v)) for v in rhs[:, r]])
            x = mp.mp.U_solve(LU, mp.mp.L_solve(LU, b, perm))
            mine = [mp.ldexp(mp.mpf(int(v)), -t["frac_bits"]) for v in t["x"][:, r]]
            scale = max(abs(v) for v in x)
            worst = max(worst, max(abs(a - b_) for a, b_ in zip(mine, x)) / scale)
    print(name, "truth vs mpmath", float(worst))
    assert worst <= mp.mpf("1e-25")


@pytest.mark.parametrize("name", UNCLAMPED)
def test_levels_are_reproduced(name):
    c, lv = CASES[name], LEVELS["solve"][name]
    o, t = sr.oracle_run(name), sr.oracle_truth(name)
    rhs = np.column_stack([o["b21"].T, sr.window(c)["z1"]])
    assert t["resid"] < 1e-30 and sr.exact_residual(o["b11"], rhs, t["x"], t["frac_bits"]) < 1e-30
    now = sr.solve_level(name)
    print(name, {k: now[k] for k in ("cond", "z", "info", "z_oracle", "info_oracle")})
    assert now["mpd"] == lv["mpd"] == 0 and abs(now["lam_min"] - c.lam) <= 1e-12
    assert 0.5 * lv["cond"] <= now["cond"] <= 2 * lv["cond"] and 1e3 < now["cond"] < 1e8
    # the file against this machine's BLAS, within a factor of 2 (levels under FLOOR / FACTOR move no bound and are a few
    # ulps: they count as that)
    for what in ("z", "info", "z_oracle", "info_oracle"):
        a, b = max(now[what], NOISE), max(lv[what], NOISE)
        assert 0.5 * b <= a <= 2 * b, (what, now[what], lv[what])
    if name in SMALL_LAM and c.eps == cr.EPS:
        assert now["info_oracle"] > 100 * now["info"] and lv["info_oracle"] > 100 * lv["info"]      # the module docstring's reason


def _reject(mutation, name):
    c, lv = CASES[name], LEVELS["solve"][name]
    o, t = sr.oracle_run(name), sr.oracle_truth(name)
    e = sr.errors(*sr.chol_route_blocked(o["b11"], o["b21"], sr.window(c)["z1"], mutation), t)
    return e, (e["z"] > sr.bound(lv["z"]) or e["info"] > sr.bound(lv["info"]))


def test_the_blocked_statement_itself_is_within_the_bounds():
    """Another valid operation order of the same algebra (factor blocks, explicit block inverses, k-block sums) stays within
    16 x the LAPACK route's error: what the factor is there to cover."""
    for name in UNCLAMPED:
        e, rejected = _reject(None, name)
        assert not rejected, (name, e, LEVELS["solve"][name])


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_bounds_reject_a_subtly_wrong_solve(mutation):
    hits = []
    for name in SMALL_LAM:
        e, rejected = _reject(mutation, name)
        print(mutation, name, e, "bounds", sr.bound(LEVELS["solve"][name]["z"]), sr.bound(LEVELS["solve"][name]["info"]))
        hits.append(rejected)
    assert any(hits)


@pytest.mark.parametrize("name", CLAMP_CHECKED)
def test_clamped_case_levels(name):
    c, lv = CASES[name], LEVELS["clamp"][name]
    now = sr.clamp_level(name)
    assert now["mpd"] == 1 and now["lifted"] == lv["lifted"] == len([d for d in sr.duplicates(c.place, c.M) if d[2] == 0])
    for what in ("b11", "cert", "info", "z", "info_own", "z_own"):
        assert now[what] <= cr.bound(lv[what], what), (what, now[what], lv[what])


def test_certificate_threshold_separates_the_mode_1_cases():
    """shift_cert_kernel's bound reaches eps at a lam of 1e-3 or so in mode 1 (W = 1.061), so every small-lam mode 1 case takes
    the exact branch and every mode 0 case the certified one; the GPU test straddles the threshold itself."""
    for name in UNCLAMPED:
        c = CASES[name]
        thr = sr.cert_threshold(sr.window(c))
        if c.mode == 0:
            assert c.eps < thr < c.lam
        else:
            assert c.lam < thr and 5e-4 < thr < 1e-2
