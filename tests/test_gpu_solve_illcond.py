"""GPU suite: the window solve on an ill-conditioned B11 -- factor_init / factor_panel / factor_update, solve_last and the riding
rows of the inverse, their k_solve_lite.hip twins, impute_gemm_kernel and the stand-alone solve_kernel -- with a tiny pivot in
the first factor block, the last one, on a block edge, in three blocks at once and beside a cluster of small eigenvalues, at lam
1 % above min_abs_eig and up to 1e-3 (cond(B11) 2e3 .. 3e5), and the MakePosDef decision 1 % on either side of min_abs_eig at the same places.

The inputs, the references and the bounds live in tests/solve_ref.py; tests/test_solve_ref.py asserts on the CPU that the cases
are well posed, that the truth is one, and that the bounds reject five subtly wrong solves.  z and info are compared with
truth_solve on the B11 and B21 that the GPU itself returns (at cond 1e5 the 1e-12 allowed between the GPU's LD and the oracle's
would move the answer by 1e-7: a truth on the oracle's matrices would measure the epilogue, not the solve).  A bound is 16 x the
error of the LAPACK statement of the same algebra on that case (tests/golden/solve_levels.json), at least 1e-13, at most 1e-8.
Every figure is printed before it is asserted.
"""
import os

import numpy as np
import pytest

import clamp_ref as cr
import solve_ref as sr
from gauss_amd import hotpath
from helpers import small_panel
from solve_ref import CASES, CLAMP_CHECKED, FORMS, FORMS_BELOW, PAIRS, UNCLAMPED

pytestmark = pytest.mark.gpu
LEVELS = sr.load_levels()
_TRUTH = {}


def _call(win, ctx):
    return hotpath.impute_window(win["mode"], win["geno_m"], win["geno_u"], win["pop_off"], win["pop_wgt"], win["z1"], lam=win["lam"],
                                 min_abs_eig=win["min_abs_eig"], want_mats=True, ctx=ctx)


def _job(wins, ctx):
    job = hotpath.Job(wins, ctx=ctx, want_mats=True)
    job.run()
    res = job.fetch()
    job.close()
    return res


def _same(a, b, keys=("z", "info", "b11", "b21")):
    return a["status"] == b["status"] and all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _truth(key, got, z1):
    """truth_solve on the matrices the GPU returned, computed once per distinct pair of matrices."""
    t = _TRUTH.get(key)
    if t is None or not (np.array_equal(t[0], got["b11"]) and np.array_equal(t[1], got["b21"])):
        t = _TRUTH[key] = (got["b11"].copy(), got["b21"].copy(), sr.truth_solve(got["b11"], got["b21"], z1))
    return t[2]


def _filler():
    """The filler of test_gpu_parity.py::test_solve_forms_agree: 27 windows at lam = 0.1 of 300 measured SNPs and 2 560
    unmeasured rows = 1 620 tiles of the closing product at 128 right-hand sides; with any window more the job is past
    OWN_PANEL_MAX_WINDOWS (20) and GEMM_SMALL_TILES (1 600)."""
    if "filler" not in _TRUTH:
        p = small_panel(n_snp=420, scale=0.03, seed=5)
        G, off = p["G"], p["off"]
        rng = np.random.default_rng(2)
        out = []
        for k in range(27):
            idx = rng.permutation(G.shape[0])
            gm = np.ascontiguousarray(G[np.sort(idx[:300])])
            gu = np.ascontiguousarray(G[rng.integers(0, G.shape[0], size=2560)])
            out.append(dict(mode=1, geno_m=gm, geno_u=gu, pop_off=off, pop_wgt=p["w"], z1=rng.standard_normal(300)))
        _TRUTH["filler"] = out
    return _TRUTH["filler"]


def _check_accuracy(name, got, win, what):
    lv = LEVELS["solve"][name]
    e = sr.errors(got["z"], got["info"], _truth(name, got, win["z1"]))
    bz, bi = sr.bound(lv["z"]), sr.bound(lv["info"])
    print("REACHED", name, what, "z", f"{e['z']:.2e}", "bound", f"{bz:.2e}", "info", f"{e['info']:.2e}", "bound", f"{bi:.2e}", "cond", f"{lv['cond']:.1e}")
    assert e["z"] <= bz and e["info"] <= bi, (name, what, e, bz, bi)


@pytest.mark.parametrize("name", UNCLAMPED)
def test_solve_against_the_truth_on_its_own_matrices(name, ctx):
    win, o = sr.window(CASES[name]), sr.oracle_run(name)
    got = _call(win, ctx)
    assert got["status"] == 0 and o["mpd"] == 0
    assert np.max(np.abs(got["b11"] - o["b11"])) <= 1e-12 and np.max(np.abs(got["b21"] - o["b21"])) <= 1e-12
    _check_accuracy(name, got, win, "fused")


@pytest.mark.parametrize("name", FORMS)
def test_launch_forms_give_the_same_bits(name, ctx, monkeypatch):
    """Every unclamped case at M = 65, 129 and 200 (all placements, all lam, the caller's own min_abs_eig): a window of its own
    job (no panel launches, 64-wide tiles of the closing product), first, in the middle and last in a job past both thresholds,
    under the int8 Gram kernel: the same bits, and those bits within the case's bound of the truth.  solve_kernel
    (GAUSS_FUSED_SOLVE=0): within the bound."""
    win = sr.window(CASES[name])
    call = _call(win, ctx)
    alone = _job([win], ctx)[0]
    assert alone["status"] == 0 and _same(call, alone)
    fill = _filler()
    res = _job([win] + fill[:14] + [win] + fill[14:] + [win], ctx)
    assert len(res) == 30 and all(r["status"] == 0 for r in res)
    for k in (0, 15, 29):
        assert _same(res[k], alone), k
    try:
        ctx.set_gram_dtype("i8")
        i8 = _job([win], ctx)[0]
    finally:
        ctx.set_gram_dtype(os.environ.get("GAUSS_GRAM_DTYPE", "f32"))
    assert _same(i8, alone)
    _check_accuracy(name, alone, win, "job")
    monkeypatch.setenv("GAUSS_FUSED_SOLVE", "0")
    plain = _job([win], ctx)[0]
    monkeypatch.delenv("GAUSS_FUSED_SOLVE")
    assert plain["status"] == 0 and np.array_equal(plain["b11"], alone["b11"]) and np.array_equal(plain["b21"], alone["b21"])
    _check_accuracy(name, plain, win, "solve_kernel")


def test_chain_beside_the_gram_kernel_same_bits(ctx, monkeypatch):
    """k_solve_lite.hip (GAUSS_CHAIN_ASIDE=2, as test_gpu_parity.py::test_chain_beside_the_gram_kernel_gives_the_same_bits forces
    it) on every window of FORMS and on those of them that the list also has just below min_abs_eig: the bits of the chain
    behind the Gram launch, as one merged launch (the context's counter shows it was queued that way) and as two."""
    names = FORMS + FORMS_BELOW
    wins = [sr.window(CASES[n]) for n in names]
    monkeypatch.setenv("GAUSS_CHAIN_ASIDE", "0")
    behind = _job(wins, ctx)
    assert [r["status"] & 1 for r in behind] == [0] * len(FORMS) + [1] * len(FORMS_BELOW)
    for n, w, r in zip(names, wins, behind):
        assert _same(r, _call(w, ctx)), n
    monkeypatch.setenv("GAUSS_CHAIN_ASIDE", "2")
    for merged in ("2", "0"):
        monkeypatch.setenv("GAUSS_CHAIN_MERGED", merged)
        c0 = ctx.counters()
        aside = _job(wins, ctx)
        c1 = ctx.counters()
        assert c1["merged"] - c0["merged"] == (1 if merged == "2" else 0) and c1["giveups"] == c0["giveups"], (c0, c1)
        for n, a, b in zip(names, behind, aside):
            assert _same(a, b), (n, merged)


def _decide(win, ctx, monkeypatch):
    got = _call(win, ctx)
    monkeypatch.setenv("GAUSS_NO_SHIFT_CERT", "1")
    exact = _call(win, ctx)
    monkeypatch.delenv("GAUSS_NO_SHIFT_CERT")
    assert _same(got, exact)
    return got


@pytest.mark.parametrize("above,below", PAIRS)
def test_decision_on_either_side_of_min_abs_eig(above, below, ctx, monkeypatch):
    """status & 1 is the oracle's MakePosDef decision 1 % above and 1 % below min_abs_eig, wherever the tiny pivot of
    B11 - eps I falls, with the shift certificate and with GAUSS_NO_SHIFT_CERT=1 (the same bits)."""
    res = {}
    for name in (above, below):
        res[name] = _decide(sr.window(CASES[name]), ctx, monkeypatch)
        assert (res[name]["status"] & 1) == sr.oracle_run(name)["mpd"], name
        assert (res[name]["status"] & ~1) == 0
        assert np.all(np.isfinite(res[name]["z"])) and np.all(np.isfinite(res[name]["info"])) and np.all(np.isfinite(res[name]["b11"]))
    assert res[above]["status"] == 0 and res[below]["status"] == 1


def test_decision_inside_a_large_job(ctx, monkeypatch):
    """All the pairs among the filler windows (panel launches, 128-wide tiles): the decisions and the bits of the single calls."""
    names = [n for pair in PAIRS for n in pair]
    wins = [sr.window(CASES[n]) for n in names]
    fill = _filler()
    batch, where = [], []
    for k, w in enumerate(wins):
        where.append(len(batch))
        batch.append(w)
        if k < len(fill):
            batch.append(fill[k])
    batch += fill[len(wins):]
    runs = []
    for no_cert in (False, True):
        if no_cert:
            monkeypatch.setenv("GAUSS_NO_SHIFT_CERT", "1")
        runs.append(_job(batch, ctx))
        if no_cert:
            monkeypatch.delenv("GAUSS_NO_SHIFT_CERT")
    for n, w, at in zip(names, wins, where):
        assert (runs[0][at]["status"] & 1) == sr.oracle_run(n)["mpd"], n
        assert _same(runs[0][at], runs[1][at]), n
        assert _same(runs[0][at], _call(w, ctx)), n


# one name for every distinct mode 1 window of FORMS (the lam of the case is replaced)
CERT_WINDOWS = list({(CASES[n].M, CASES[n].U, CASES[n].place): n for n in FORMS if CASES[n].mode == 1}.values())
CERT_STEPS = (0.5, 1.0 - 1e-3, 1.0 + 1e-3, 2.0)


@pytest.mark.parametrize("name", CERT_WINDOWS)
def test_certified_and_exact_branch_side_by_side(name, ctx, monkeypatch):
    """Mode 1: lam at 0.5, 0.999, 1.001 and 2 times the lam at which shift_cert_kernel's own bound reaches min_abs_eig, as
    neighbours in one job.  All four are unclamped like the oracle's and have the bits of GAUSS_NO_SHIFT_CERT=1; the inner two
    are within the bound of the truth -- the bound from the LAPACK route's error on the same matrices, by the rule of
    solve_levels.json.

    What this rests on: the library exports neither status[3] nor a counter of certified windows, and the two branches give
    the same bits by design, so no test can see which one a window took.  The threshold is sr.cert_threshold, the formula of
    the comment above shift_cert_kernel evaluated in numpy on the oracle's means and variances.  If it matches the kernel's
    rt_mu / rt_sd scaling to 0.1 %, the inner two windows sit on either side and are neighbours in one launch; if it is off
    by up to a factor of 2 either way, the outer two still do.  The guard below keeps the whole ladder unclamped, above the
    small-lam cases (which take the exact branch) and in the range the kernel's comment gives for real panels."""
    base = sr.window(CASES[name])
    thr = sr.cert_threshold(base)
    assert 5e-4 < thr < 5e-3 and CERT_STEPS[0] * thr > 10 * base["min_abs_eig"]
    wins = [dict(base, lam=thr * f) for f in CERT_STEPS]
    res = _job(wins, ctx)
    monkeypatch.setenv("GAUSS_NO_SHIFT_CERT", "1")
    exact = _job(wins, ctx)
    monkeypatch.delenv("GAUSS_NO_SHIFT_CERT")
    for f, w, r, x in zip(CERT_STEPS, wins, res, exact):
        o = sr.oracle.run_impute(w["mode"], w["geno_m"], w["geno_u"], w["pop_off"], w["pop_wgt"], w["z1"], lam=w["lam"],
                                 min_abs_eig=w["min_abs_eig"])
        assert o["mpd"] == 0 and r["status"] == 0 and _same(r, x) and _same(r, _decide(w, ctx, monkeypatch)), f
        assert np.all(np.isfinite(r["z"])) and np.all(np.isfinite(r["info"]))
        if abs(f - 1.0) > 0.01:
            continue
        t = sr.truth_solve(r["b11"], r["b21"], w["z1"])
        lv = sr.errors(*sr.chol_route(r["b11"], r["b21"], w["z1"]), t)
        e = sr.errors(r["z"], r["info"], t)
        print("REACHED", name, "lam", f"{w['lam']:.6e}", "z", f"{e['z']:.2e}", "bound", f"{sr.bound(lv['z']):.2e}", "info", f"{e['info']:.2e}",
              "bound", f"{sr.bound(lv['info']):.2e}")
        assert e["z"] <= sr.bound(lv["z"]) and e["info"] <= sr.bound(lv["info"])


@pytest.mark.parametrize("name", CLAMP_CHECKED)
def test_clamped_side_against_the_clamp_reference(name, ctx):
    """lam = 0.99 eps and lam = 0 on the same windows: the repaired B11 passes clamp_ref.py's certificate, z and info agree with
    numpy's clamp and with the oracle at the levels of these cases (solve_levels.json, clamp_ref.bound: never looser than the
    1e-9 / 1e-5 of the clamp tests)."""
    c, lv = CASES[name], LEVELS["clamp"][name]
    win, o = sr.window(c), sr.oracle_run(name)
    got = _call(win, ctx)
    assert got["status"] == 1 and o["mpd"] == 1
    b11, b21 = got["b11"], got["b21"]
    assert np.all(np.isfinite(b11)) and np.all(np.isfinite(got["z"])) and np.all(np.isfinite(got["info"]))
    A, b21_ref = cr.raw_b11(win)
    X, _ = cr.clamp_numpy(A, c.eps)
    z_ref, info_ref = cr.solve_inv(X, b21_ref, win["z1"])
    assert np.max(np.abs(b21 - b21_ref)) <= 1e-12
    cert = cr.clamp_certificate(A, b11, c.eps)
    z_own, info_own = cr.solve_inv(b11, b21, win["z1"])
    reached = dict(cert=cr.certificate_level(cert), b11=float(np.max(np.abs(b11 - X))), b11_oracle=float(np.max(np.abs(b11 - o["b11"]))),
                   info_own=cr.relerr(got["info"], info_own), z_own=cr.zerr(got["z"], z_own),
                   info=cr.relerr(got["info"], info_ref), z=cr.zerr(got["z"], z_ref),
                   info_oracle=cr.relerr(got["info"], o["info"]), z_oracle=cr.zerr(got["z"], o["z"]))
    print("REACHED", name, "lifted", lv["lifted"], {k: float(f"{v:.2e}") for k, v in reached.items()},
          "bounds", {k: cr.bound(lv[k], k) for k in ("cert", "b11", "info", "z", "info_own", "z_own")})
    assert cr.certificate_ok(cert, cr.bound(lv["cert"], "cert")), cert
    assert reached["b11"] <= cr.bound(lv["b11"], "b11") and reached["b11_oracle"] <= cr.bound(lv["b11"], "b11")
    assert reached["info_own"] <= cr.bound(lv["info_own"], "info_own") and reached["z_own"] <= cr.bound(lv["z_own"], "z_own")
    assert reached["info"] <= cr.bound(lv["info"], "info") and reached["z"] <= cr.bound(lv["z"], "z")
    assert reached["info_oracle"] <= cr.bound(lv["info"], "info") and reached["z_oracle"] <= cr.bound(lv["z"], "z")
    up = sr.twin(name, "above")
    if c.lam > 0 and up:                       # 1 % higher, the same window is left alone: another status, the same finiteness
        other = _call(sr.window(CASES[up]), ctx)
        assert other["status"] == 0 and np.all(np.isfinite(other["z"])) and np.all(np.isfinite(other["info"]))
