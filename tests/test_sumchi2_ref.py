"""CPU: tests/sumchi2_ref.py, the statement the GPU tests hold k_sumchi2.hip and gauss_host_sumchi2_pval to, against what it does not
share code with: `jacobi` against numpy.linalg.eigvalsh; `saddle` against three closed forms, against itself across its switch, and
against Imhof's numerical inversion (scipy.integrate.quad); `prune` against a plain double loop."""
import math

import numpy as np
import pytest

import sumchi2_ref as sr

EPS = 2.0 ** -52


def _ld_like(rng, k, n_samples, kind="plain"):
    """a correlation matrix of k genotype rows over n_samples samples (n_samples < k: rank-deficient)"""
    G = rng.binomial(2, rng.uniform(0.1, 0.9, size=(k, 1)), size=(k, n_samples)).astype(float)
    G[:, 0], G[:, 1] = 0, 2
    if kind == "block" and k >= 8:
        G[3:8] = G[3]                                  # a block of identical rows
    R = np.atleast_2d(np.corrcoef(G))
    np.fill_diagonal(R, 1.0)
    return R


JACOBI_CASES = [(1, 50, "plain"), (2, 50, "plain"), (3, 50, "plain"), (33, 200, "plain"), (33, 20, "plain"), (64, 200, "plain"), (64, 40, "block"),
                (127, 300, "plain"), (127, 60, "plain"), (128, 400, "block"), (128, 60, "plain")]


@pytest.mark.parametrize("k,n_samples,kind", JACOBI_CASES)
def test_jacobi_against_eigvalsh(k, n_samples, kind):
    R = _ld_like(np.random.default_rng(1000 + 7 * k + n_samples), k, n_samples, kind)
    ev, sweeps, ok = sr.jacobi(R)
    want = np.linalg.eigvalsh(R)[::-1]
    ratio = float(np.abs(ev - want).max()) / (k * EPS * want[0])
    print(f"REACHED jacobi k {k} samples {n_samples} {kind}: {sweeps} sweeps, max |dlambda| = {ratio:.2f} k 2^-52 lambda_max (bound 8)")
    assert ok and 1 <= sweeps <= 12
    assert np.all(np.diff(ev) <= 0)
    assert ratio <= 8.0
    if n_samples < k:
        assert ev[-1] < 1e-10                          # rank-deficient: zero (or slightly negative) eigenvalues


@pytest.mark.parametrize("r", [1.0, -1.0, 0.5, 0.0])
def test_jacobi_two_by_two(r):
    ev, sweeps, ok = sr.jacobi(np.array([[1.0, r], [r, 1.0]]))
    assert ok and np.abs(ev - np.array([1 + abs(r), 1 - abs(r)])).max() <= 4 * EPS
    assert sweeps == (1 if r == 0.0 else 2)


def test_prune_is_the_double_loop():
    rng = np.random.default_rng(3)
    for n in (1, 2, 5, 40):
        G = rng.binomial(2, 0.4, size=(n, 80)).astype(float)
        for s in range(1, n):
            if rng.random() < 0.6:
                G[s] = G[s - 1]
                G[s, rng.random(80) < 0.03] = 1
        if n >= 5:
            G[2] = 1                                   # monomorphic
        with np.errstate(invalid="ignore", divide="ignore"):
            R = np.atleast_2d(np.corrcoef(G))
        np.fill_diagonal(R, 1.0)
        kept, n_nan = sr.prune(R, 0.9)
        want, dropped = [], set()
        for i in range(n):
            if n > 1 and all(math.isnan(R[i, j]) for j in range(n) if j != i):
                want.append(0)
                continue
            if i in dropped:
                want.append(0)
                continue
            want.append(1)
            dropped |= {j for j in range(i + 1, n) if R[i, j] * R[i, j] > 0.9}
        assert kept.tolist() == want and n_nan == (1 if n >= 5 else 0)
        assert sr.prune(R, 1.0)[0].sum() >= kept.sum()
    assert sr.prune(np.ones((1, 1)), 0.9)[0].tolist() == [1]
    kept, n_nan = sr.prune(np.array([[1.0, np.nan], [np.nan, 1.0]]), 0.9)      # two SNPs, one monomorphic: both rows are NaN rows
    assert kept.tolist() == [0, 0] and n_nan == 2


def test_saddle_closed_forms():
    from scipy.stats import chi2
    # one lambda: the exact tail
    for lam, q in ((1.0, 3.84), (0.3, 7.0), (5.0, 0.01), (2.0, 900.0)):
        want = chi2.sf(q / lam, 1)
        assert abs(sr.saddle([lam], q) - want) <= 1e-12 * want
        assert sr.saddle([lam, -1e-9, np.nan, 0.0], q) == sr.saddle([lam], q)          # what is not positive is left out
    assert sr.saddle([1.0, 2.0], 0.0) == 1.0 and sr.saddle([1.0, 2.0], -3.0) == 1.0
    assert math.isnan(sr.saddle([], 1.0)) and math.isnan(sr.saddle([-1.0, np.nan], 1.0)) and math.isnan(sr.saddle([1.0, 2.0], np.nan))
    # monotone in q: below the switch window, inside it, above it (across its two edges the value steps by the gap between the two
    # formulas, which test_the_two_branches_agree_at_the_switch measures)
    lam = np.linspace(0.05, 2.5, 40)
    mean, sd = lam.sum(), math.sqrt(2 * (lam * lam).sum())
    for lo, hi in ((0.5, mean - 1.01 * sr.EDGE * sd), (mean - 0.99 * sr.EDGE * sd, mean + 0.99 * sr.EDGE * sd), (mean + 1.01 * sr.EDGE * sd, 300.0)):
        p = np.array([sr.saddle(lam, q) for q in np.linspace(lo, hi, 300)])
        assert np.all(np.diff(p) <= 0) and np.all(np.diff(p[p < 1 - 1e-9]) < 0) and 0 < p[-1] < p[0] <= 1, (lo, hi)
    # a tail far out is reachable
    assert 0 < sr.saddle(np.ones(4), 1400.0) < 1e-290


def _spectra():
    rng = np.random.default_rng(8)
    out = {"equal20": np.full(20, 0.7), "equal128": np.ones(128), "linear128": np.linspace(0.02, 3.0, 128), "geometric64": 4.0 * 0.93 ** np.arange(64)}
    R = _ld_like(rng, 128, 500)
    out["ld128"] = np.linalg.eigvalsh(R)[::-1]
    R = _ld_like(rng, 64, 40)
    out["ld64_rank39"] = np.linalg.eigvalsh(R)[::-1]
    out["dominant12"] = np.concatenate([[6.0], np.full(11, 0.5)])
    return out


def test_the_two_branches_agree_at_the_switch():
    """At |x| = 1e-3 the saddlepoint formula and the Edgeworth tail are both in their range: the gap between them is the step pval makes
    there.  Measured on every test spectrum (SWITCH_GAP, from the REACHED lines); twice the spectrum's own figure is asserted."""
    for name, lam in _spectra().items():
        l = lam[lam > 0]
        worst = 0.0
        for sign in (-1.0, 1.0):
            q = l.sum() + sign * sr.EDGE * math.sqrt(2 * (l * l).sum())
            a, b = sr.saddle(l, q, branch="saddle"), sr.saddle(l, q, branch="edgeworth")
            worst = max(worst, abs(a - b) / b)
        print(f"REACHED switch {name}: largest relative gap {worst:.2e} (recorded {SWITCH_GAP[name]:.2e})")
        assert worst <= 2 * SWITCH_GAP[name], name


def test_saddle_against_imhof_and_the_equal_lambda_closed_form():
    """p from 0.5 down to 1e-8.  The largest relative error measured on each spectrum is SADDLE_ACCURACY (from the REACHED lines); twice
    the spectrum's own figure is asserted.  A case where quad's own error estimate exceeds 1 % of p is left out; at most a tenth may be."""
    from scipy.stats import chi2
    n_cases, n_out = 0, 0
    for name, lam in _spectra().items():
        l = lam[lam > 0]
        s1, s2 = l.sum(), (l * l).sum()
        equal = float(l.max() - l.min()) == 0.0
        worst = 0.0
        for x in (0.0, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0):
            q = s1 + x * math.sqrt(2 * s2)
            got = sr.saddle(l, q)
            if equal:
                want, err = chi2.sf(q / l[0], len(l)), 0.0
            else:
                want, err = sr.imhof(l, q)
            if want < 1e-8 or want > 0.55:
                continue
            n_cases += 1
            if err > 0.01 * want:
                n_out += 1
                continue
            worst = max(worst, abs(got - want) / want)
        print(f"REACHED saddle {name}: largest relative error {worst:.3e} (recorded {SADDLE_ACCURACY[name]:.2e})")
        assert worst <= 2 * SADDLE_ACCURACY[name], name
    assert n_cases >= 30 and n_out * 10 <= n_cases


# measured by the two tests above, per spectrum (their REACHED lines); DESIGN.md quotes them.  The gap at the switch is the difference of
# the two approximations at the mean and does not shrink with the window (dominant12: 1.50e-2 at |x| = 1e-5); below |x| = 1e-4 the
# saddlepoint formula's own rounding takes over, so the switch stays at 1e-3
SWITCH_GAP = {"equal20": 1.77e-4, "equal128": 1.10e-5, "linear128": 2.27e-5, "geometric64": 2.52e-4, "ld128": 2.26e-5, "ld64_rank39": 1.04e-3,
              "dominant12": 1.51e-2}
SADDLE_ACCURACY = {"equal20": 1.37e-3, "equal128": 9.45e-5, "linear128": 7.97e-4, "geometric64": 2.77e-2, "ld128": 9.42e-3,
                   "ld64_rank39": 6.12e-2, "dominant12": 6.25e-2}
