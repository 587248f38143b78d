"""CPU side of the eigenvalue-clamp tests (tests/test_gpu_clamp.py holds the kernels): the references agree with each other at
the recorded levels, the certificate accepts a correct clamp and rejects five kinds of subtly wrong ones at the tolerance the
GPU tests use, and every input of the GPU tests is well posed -- finite, clamped exactly where it is meant to be, and with no
eigenvalue so close to a threshold that the predicate would be a coin toss."""
import numpy as np
import pytest

import clamp_ref as cr
from clamp_ref import CASES, EPS, PW_CASES, QCAT_CASES
from popwgt_ref import ST_CLAMPED, interval_weights

LEVELS = cr.load_levels()
MUTATED = ["many_65", "few_130", "mix_w1500", "near_below", "many_640"]


def test_every_case_has_a_recorded_level_under_todays_bounds():
    assert set(LEVELS["b11"]) == set(CASES) and set(LEVELS["qcat"]) == set(QCAT_CASES) and set(LEVELS["popwgt"]) == set(PW_CASES)
    for name, lv in LEVELS["b11"].items():
        for what in ("b11", "cert", "info", "z", "info_own", "z_own"):
            assert cr.FACTOR * lv[what] <= cr.CEILING[what], (name, what, lv[what])
    for name, lv in LEVELS["popwgt"].items():
        assert cr.FACTOR * lv["w"] <= cr.CEILING["w"], (name, lv["w"])


@pytest.mark.parametrize("name", list(CASES))
def test_case_is_well_posed_and_the_references_agree(name):
    _, clamps, margin, indefinite = CASES[name]
    ref, lv = cr.reference(name), LEVELS["b11"][name]
    o, lam = ref["oracle"], ref["lam"]
    M = ref["A"].shape[0]
    assert o["mpd"] == int(clamps) and (lam[0] < EPS) == clamps
    assert np.all(np.isfinite(ref["A"])) and np.all(np.isfinite(o["z"])) and np.all(np.isfinite(o["info"])) and np.all(o["info"] > 0)
    assert np.min(np.abs(lam / EPS - 1.0)) >= margin * 0.999, np.min(np.abs(lam / EPS - 1.0))
    assert int(np.sum(lam < EPS)) == lv["lifted"] and lv["M"] == M
    if name.startswith("many_"):
        assert lv["lifted"] == M - dict(cr.SIZES_MANY)[M] + 1
    if name.startswith("few_"):
        assert 1 <= lv["lifted"] <= 3
    if indefinite:
        assert lam[0] < -1e-4
    # the two CPU statements against each other, at what the GPU will be allowed
    now = cr.b11_level(name)
    print(name, {k: now[k] for k in ("b11", "cert", "info", "z", "info_own", "z_own")})
    for what in ("b11", "cert", "info", "z", "info_own", "z_own"):
        assert now[what] <= cr.bound(lv[what], what), (what, now[what], lv[what])
    tol = cr.bound(lv["cert"], "cert")
    for X in (ref["X"], o["b11"]):
        c = cr.clamp_certificate(ref["A"], X)
        assert cr.certificate_ok(c, tol), c


def _mutations(A, X, lam, V):
    """Subtly wrong clamps of A (X is the right one; lam, V its eigenpairs)."""
    low = np.nonzero(lam < EPS)[0]
    j = low[-1]                                              # the lifted eigenvalue nearest to eps: the smallest lift
    v, top = V[:, j], V[:, -1]
    kept = np.nonzero(lam >= EPS)[0][0]
    th = 1e-4
    vr = np.cos(th) * v + np.sin(th) * top
    wrong_row = X.copy()
    wrong_row[len(X) // 3] *= 1.0 + 1e-6
    return {
        "one eigenvalue left unlifted": X - (EPS - lam[j]) * np.outer(v, v),
        "one lifted to 2 eps": X + EPS * np.outer(v, v),
        "one lifted along a direction rotated by 1e-4 inside the kept subspace":
            X - (EPS - lam[j]) * np.outer(v, v) + (EPS - lam[j]) * np.outer(vr, vr),
        "one kept eigenvalue with its sign flipped": X - 2.0 * lam[kept] * np.outer(V[:, kept], V[:, kept]),
        "symmetrised from a result with one wrong row": 0.5 * (wrong_row + wrong_row.T),
    }


@pytest.mark.parametrize("name", MUTATED)
def test_certificate_rejects_wrong_clamps_at_the_gpu_tolerance(name):
    ref = cr.reference(name)
    A, X = ref["A"], ref["X"]
    lam, V = np.linalg.eigh(A)
    tol = cr.bound(LEVELS["b11"][name]["cert"], "cert")
    assert cr.certificate_ok(cr.clamp_certificate(A, X), tol)
    muts = _mutations(A, X, lam, V)
    assert len(muts) == 5
    for what, Xm in muts.items():
        c = cr.clamp_certificate(A, Xm)
        print(name, what, c)
        assert not cr.certificate_ok(c, tol), (what, c)
        # and the plain comparison with numpy's clamp, which the GPU tests make as well, sees all but the rotated one
        if "rotated" not in what and "wrong row" not in what:
            assert np.max(np.abs(Xm - X)) > cr.bound(LEVELS["b11"][name]["b11"], "b11")


def test_lam_for_places_the_spectrum():
    win = cr.window_duplicated(2 * cr.NB + 2, 300, 2, 77)
    A0, _ = cr.raw_b11(win, lam=0.0)
    with pytest.raises(ValueError):                          # two eigenvalues sit together at 0: one alone cannot be below eps
        cr.lam_for(A0, 1, 1e-2)
    for r, margin in ((0, 1e-2), (2, 1e-2), (2, 0.3), (0, 0.3)):
        lam = cr.lam_for(A0, r, margin)
        ev = np.linalg.eigvalsh(cr.raw_b11(win, lam=lam)[0])
        assert int(np.sum(ev < EPS)) == r
        assert abs(np.min(np.abs(ev / EPS - 1.0)) - margin) <= 1e-6


@pytest.mark.parametrize("name", list(QCAT_CASES))
def test_countpc_case_is_clear_of_the_cutoff(name):
    now, lv = cr.qcat_level(name), LEVELS["qcat"][name]
    assert now["below"] >= 50 and now["nearest"] >= 1e-6
    assert now["num_eig"] == now["oracle_num_eig"] == lv["num_eig"] and now["below"] == lv["below"]


def test_popwgt_mp_against_numpy_on_the_existing_inputs():
    from test_gpu_popwgt import _matrix
    for P in (1, 2, 26):
        small = max(2, P // 2)
        x, off = _matrix(P, [small, 2, 1, 40, 300, 200], seed=100 + P, dup=5)
        want, wst, lmin = interval_weights(x, off)
        got, st, lmp = cr.popwgt_mp(x, off)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        fin = ~np.isnan(want).any(1)
        assert np.max(cr.werr(want[fin], got[fin])) <= 1e-8
        clear = fin & ((lmp < 0.5 * EPS) | (lmp > 2 * EPS))
        assert np.array_equal(st[clear] & ST_CLAMPED, wst[clear] & ST_CLAMPED)
        assert np.allclose(lmin[fin], lmp[fin], atol=1e-12)


@pytest.mark.parametrize("name", list(PW_CASES))
def test_popwgt_case_is_well_posed(name):
    ref, lv = cr.pw_reference(name), LEVELS["popwgt"][name]
    w_np, st_np, _ = ref["np"]
    w_mp, st_mp, lmin = ref["mp"]
    assert np.all(np.isfinite(w_np)) and np.all(np.isfinite(w_mp))
    d = float(np.max(cr.werr(w_np, w_mp)))
    print(name, "w: numpy vs mpmath", d, "lambda_min", lmin)
    assert d <= cr.bound(lv["w"], "w")
    assert np.all((lmin < 0.5 * EPS) | (lmin > 2 * EPS))        # every interval's clamp bit is decided
    assert np.array_equal(st_np & ST_CLAMPED, st_mp & ST_CLAMPED)
    assert [int(v) for v in st_mp] == lv["clamped"]
    if name == "bn_twin":
        assert st_mp[0] & ST_CLAMPED and 0 < lmin[0] < 0.5 * EPS    # nearly, not exactly, collinear
    else:
        # the columns of a super-population are as correlated as real panels' are (P = 5: every population is a super-population
        # of its own, the columns share the ancestral frequency only)
        c = np.corrcoef(ref["x"][:1000, 1:].T)
        assert np.max(c - np.eye(len(c))) > (0.99 if name != "bn_P5" else 0.75)
