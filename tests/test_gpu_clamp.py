"""GPU suite: the two device eigensolvers at real sizes and real spectra.

* k_misc.hip, launch_jacobi_clamp (one-sided Jacobi on G = B11 V): MakePosDef of a window's B11 and CountPC's count, at
  M = NB - 1, NB, NB + 1, 2 NB + 2, 640 and 1200 with 1-3 and with hundreds of eigenvalues to lift, in mode 0 and in mode 1 with
  weights summing to 1, 1.061 and 1.5 (the last one an indefinite B11 with finite output), and with an eigenvalue 1 % on either
  side of min_abs_eig.
* k_popwgt.hip, pw_solve_kernel (two-sided Jacobi, clamp, Cholesky solve): Balding-Nichols allele-frequency tables whose columns
  correlate above 0.99 inside a super-population, against mpmath at 40 digits.

The inputs, the references and the bounds live in tests/clamp_ref.py; tests/test_clamp_ref.py asserts on the CPU that every
input is well posed.  A bound is 16 x the disagreement of the two CPU statements of that case (tests/golden/clamp_levels.json),
at least 1e-13 and at most today's bound (1e-9 for b11, 1e-5 for z and info, 1e-8 x scale for w).

Levels reached on an MI355X (the worst case of each quantity, with that case's bound; every figure is printed before it is
asserted, the whole file takes 24 s):

    certificate                     6.3e-14  (many_1200, bound 2.8e-12)
    b11 vs numpy                    2.9e-15  (few_1200, bound 1e-13)
    b11 vs the oracle               7.3e-15  (many_1200, bound 1.1e-13)
    info on the GPU's own matrices  2.4e-11  (many_640, bound 3.9e-10)
    z on the GPU's own matrices     9.0e-10  (many_1200, bound 7.5e-09)
    info vs numpy / the oracle      5.1e-11 / 4.7e-11  (mix_w1500, bound 8.7e-11: the case nearest to its bound)
    z vs numpy                      9.5e-10  (many_640, bound 2.2e-08)
    z vs the oracle                 1.9e-09  (many_1200, bound 3.0e-08)
    w vs mpmath / numpy             2.4e-12 / 7.8e-12  (bn_twin, bound 8.7e-11); at most 1.5e-13 elsewhere (bounds 1e-13 .. 1.8e-12)
    CountPC                         79 of 130 and 199 of 640, as numpy and the oracle count

Sweeps of launch_jacobi_clamp (GAUSS_TRACE=job prints them): with 1-3 zero eigenvalues the 30 sweeps run out at n = 64, 128, 192
and 640 with about n rotations left in the last one -- every one of them a pair with a column of G that is rounding noise, where
"orthogonal to 1e-15 relative" cannot be reached -- and the result is as accurate as where the loop ends by itself (17 sweeps at
n = 1216; 19, 19, 19, 21, 26, 27 sweeps at n = 64 .. 1216 with hundreds of zero eigenvalues; 12 with the eigenvalues at 0.99 eps).
"""
import numpy as np
import pytest

import clamp_ref as cr
from clamp_ref import CASES, EPS, NB, PW_CASES, QCAT_CASES
from gauss_amd import hotpath
from popwgt_ref import ST_CLAMPED, ST_NONFINITE

pytestmark = pytest.mark.gpu
LEVELS = cr.load_levels()


def _unclamped_neighbours(seed):
    rng = np.random.default_rng(seed)
    G = cr.rand_geno(rng, 90, 300)
    return [dict(mode=0, geno_m=np.ascontiguousarray(G[a:a + m]), geno_u=np.ascontiguousarray(G[60:90]), pop_off=np.array([0, 300], dtype=np.int32),
                 pop_wgt=None, z1=rng.standard_normal(m), lam=0.1) for a, m in ((0, 40), (10, 50))]


@pytest.mark.parametrize("name", list(CASES))
def test_makeposdef_against_the_references(name, ctx):
    _, clamps, _, _ = CASES[name]
    ref, lv = cr.reference(name), LEVELS["b11"][name]
    win, o = ref["win"], ref["oracle"]
    M = win["geno_m"].shape[0]
    assert M == lv["M"] and (M + NB - 1) // NB * NB >= M                      # the solver works on Mld = M padded to NB rows
    got = hotpath.impute_window(win["mode"], win["geno_m"], win["geno_u"], win["pop_off"], win["pop_wgt"], win["z1"], lam=win["lam"],
                                want_mats=True, ctx=ctx)
    # status bit 1 exactly when the reference says a clamp happens
    assert got["status"] == (1 if clamps else 0) and o["mpd"] == int(clamps)
    b11, b21 = got["b11"], got["b21"]
    assert np.all(np.isfinite(b11)) and np.all(np.isfinite(got["z"])) and np.all(np.isfinite(got["info"]))
    assert np.max(np.abs(b21 - ref["b21"])) <= 1e-12
    # the clamped matrix: basis-free certificate, then numpy's and the oracle's own result
    c = cr.clamp_certificate(ref["A"], b11)
    z_own, info_own = cr.solve_inv(b11, b21, win["z1"])
    reached = dict(cert=cr.certificate_level(c), b11=float(np.max(np.abs(b11 - ref["X"]))), b11_oracle=float(np.max(np.abs(b11 - o["b11"]))),
                   info_own=cr.relerr(got["info"], info_own), z_own=cr.zerr(got["z"], z_own),
                   info=cr.relerr(got["info"], ref["info"]), z=cr.zerr(got["z"], ref["z"]),
                   info_oracle=cr.relerr(got["info"], o["info"]), z_oracle=cr.zerr(got["z"], o["z"]))
    print("REACHED", name, "lifted", lv["lifted"], {k: float(f"{v:.2e}") for k, v in reached.items()},
          "bounds", {k: cr.bound(lv[k], k) for k in ("cert", "b11", "info", "z", "info_own", "z_own")})
    assert cr.certificate_ok(c, cr.bound(lv["cert"], "cert")), c
    assert reached["b11"] <= cr.bound(lv["b11"], "b11") and reached["b11_oracle"] <= cr.bound(lv["b11"], "b11")
    # the solve alone: numpy on the GPU's own b11 and b21
    assert reached["info_own"] <= cr.bound(lv["info_own"], "info_own") and reached["z_own"] <= cr.bound(lv["z_own"], "z_own")
    # the whole path against numpy and against the oracle
    assert reached["info"] <= cr.bound(lv["info"], "info") and reached["z"] <= cr.bound(lv["z"], "z")
    assert reached["info_oracle"] <= cr.bound(lv["info"], "info") and reached["z_oracle"] <= cr.bound(lv["z"], "z")
    # the same window between unclamped ones in a batch: the same bits
    before, after = _unclamped_neighbours(M)
    job = hotpath.Job([before, dict(win), after], ctx=ctx, want_mats=True)
    job.run()
    res = job.fetch()
    job.close()
    assert [r["status"] for r in res] == [0, 1 if clamps else 0, 0]
    for k in ("z", "info", "b11", "b21"):
        assert np.array_equal(res[1][k], got[k]), k


@pytest.mark.parametrize("name", list(QCAT_CASES))
def test_countpc_counts_hundreds_of_small_eigenvalues(name, ctx):
    lv = LEVELS["qcat"][name]
    win = cr.qcat_window(name)
    A, _ = cr.raw_b11(win)
    lam = np.linalg.eigvalsh(A)
    want = len(lam) - int(np.sum(lam < cr.QCAT_CUTOFF))
    got = hotpath.qcat_window(0, win["geno_m"], win["geno_u"], win["pop_off"], None, win["z1"], cr.QCAT_HEAD, cr.QCAT_PRED, lam=win["lam"],
                              eig_cutoff=cr.QCAT_CUTOFF, ctx=ctx)
    print("REACHED", name, "num_eig", got["num_eig"], "numpy", want, "below the cutoff", lv["below"])
    assert lv["below"] >= 50 and want == lv["num_eig"]
    assert got["status"] == 0 and got["num_eig"] == want
    assert np.all(np.isfinite(got["r"]))


@pytest.mark.parametrize("name", list(PW_CASES))
def test_pop_weights_on_correlated_populations(name, ctx):
    ref, lv = cr.pw_reference(name), LEVELS["popwgt"][name]
    x, off = ref["x"], ref["off"]
    got, st = hotpath.pop_weights(x, off, ctx=ctx)
    tol = cr.bound(lv["w"], "w")
    assert np.all((st & ST_NONFINITE) == 0) and np.all(np.isfinite(got))
    for which in ("mp", "np"):
        want, wst, lmin = ref[which]
        d = cr.werr(got, want)
        print("REACHED", name, which, "w", [float(f"{v:.2e}") for v in d], "bound", tol, "lambda_min", [float(f"{v:.3e}") for v in lmin])
        assert np.all(d <= tol), (which, d, tol)
        clear = (lmin < 0.5 * EPS) | (lmin > 2 * EPS)
        assert np.array_equal(st[clear] & ST_CLAMPED, wst[clear] & ST_CLAMPED)
    again, st2 = hotpath.pop_weights(x, off, ctx=ctx)
    assert got.tobytes() == again.tobytes() and np.array_equal(st, st2)
