"""GPU: the multi-causal fine-mapping of a window (k_susie.hip) against its definition (tests/susie_ref.py) evaluated on the B11 / B21
the GPU returns.  alpha, mu, pip, set_pip, mass, lse, V and purity are held to max(10 e_ref, 2 max(1, r_max^2) 1e-8) absolute
(susie_ref.value_tol: e_ref is the gap between the reference's two statements on that case); sizes, set, kept and the sweeps are exact,
and no decision of a case may be borderline.  Every case prints a REACHED line."""
import os

import numpy as np
import pytest

import cs_ref
import susie_ref as sr
from gauss_amd import api, hotpath
from gauss_amd import panel as panel_mod
from helpers import small_panel, split_window

pytestmark = pytest.mark.gpu

ST_CLAMPED, ST_NONFINITE, ST_NOCONV, ST_NOFIT = 1, 2, 16, 32
VALUE = (("susie_alpha", "alpha"), ("susie_mu", "mu"), ("susie_pip", "pip"), ("susie_set_pip", "set_pip"), ("susie_mass", "mass"),
         ("susie_lse", "lse"), ("susie_V", "V"), ("susie_purity", "purity"))
SUSIE_KEYS = ("susie_pip", "susie_set", "susie_set_pip", "susie_V", "susie_lse", "susie_mass", "susie_purity", "susie_size", "susie_kept",
              "susie_sweeps", "susie_delta")


def _same(a, b, keys, own_bits=0):
    """own_bits: status bits of the rider that `b`, a call without it, cannot carry"""
    assert a["status"] & ~own_bits == b["status"]
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _check(got, z1, kw, what):
    """got: a window's result with b11, b21, susie_alpha and susie_mu.  The reference on the GPU's matrices, vetted again there."""
    tb, want = sr.fit_textbook(got["b11"], got["b21"], z1, **kw), sr.fit_w(got["b11"], got["b21"], z1, **kw)
    e_ref = sr.gap(tb, want)
    tol = sr.value_tol(want, e_ref)
    bl = sr.borderline(want, kw, tol)
    assert bl == [], (what, bl)
    e = {}
    for g, w in VALUE:
        p, q = np.asarray(got[g], dtype=np.float64), np.asarray(want[w], dtype=np.float64)
        assert p.shape == q.shape and np.array_equal(np.isnan(p), np.isnan(q)), (what, g)
        e[w] = float(np.nanmax(np.abs(p - q), initial=0.0))
    print(f"REACHED susie {what}: T {len(want['pip'])}  L {len(want['V'])}  sweeps {want['sweeps']}  kept {int(want['kept'].sum())}  "
          f"r_max {want['rmax']:.2f}  e_ref {e_ref:.2e}  " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"  (bound {tol:.2e})")
    assert max(e.values()) <= tol, (what, e, tol)
    assert np.array_equal(got["susie_size"], want["size"]), (what, got["susie_size"], want["size"])
    assert np.array_equal(got["susie_set"], want["set"]), what
    assert np.array_equal(got["susie_kept"] != 0, want["kept"]), (what, got["susie_kept"], want["kept"])
    assert got["susie_sweeps"] == want["sweeps"], (what, got["susie_sweeps"], want["sweeps"])
    assert abs(got["susie_delta"] - want["delta"]) <= tol
    conv = want["delta"] < sr.args_of(**kw)["tol"]
    assert bool(got["status"] & ST_NOCONV) == (not conv), (what, got["status"])
    return want


def _window(ctx, M, U, kw, seed, mode=0, **more):
    p, gm, gu, z1 = sr.small_window(M, U, seed)
    got = hotpath.impute_window(mode, gm, gu, p["off"], p["w"] if mode else None, z1, want_mats=True, ctx=ctx,
                                susie=dict(kw, want_alpha=True), **more)
    return got, z1


@pytest.mark.parametrize("case", sr.SMALL_CASE_MODES, ids=lambda c: f"M{c[0]}-U{c[1]}-L{c[2].get('L', 10)}-s{c[2].get('max_sweeps')}-mode{c[4]}")
def test_small_cases(ctx, case):
    """Every small case on pooled (mode 0) and on weighted (mode 1) LD"""
    M, U, kw, seed, mode = case
    got, z1 = _window(ctx, M, U, kw, seed, mode=mode)
    assert got["status"] & ~ST_NOCONV == 0
    _check(got, z1, kw, f"M={M} U={U} mode={mode} {kw}")


def test_the_largest_window_of_chr22(ctx):
    M, U, kw, seed = sr.LARGE_CASE
    p, gm, gu = cs_ref.window(M, U, scale=0.1)
    z1 = cs_ref.planted(gm, seed=seed)
    got = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, want_mats=True, ctx=ctx, susie=dict(kw, want_alpha=True))
    _check(got, z1, kw, f"M={M} U={U} weighted, 5 sweeps")


def test_the_gpu_stops_at_the_reference_s_sweep_and_a_short_fit_reports_it(ctx):
    M, U, kw, seed = sr.CONVERGENCE_CASE
    got, z1 = _window(ctx, M, U, kw, seed)
    want = _check(got, z1, kw, "convergence")
    assert got["status"] == 0 and 1 < want["sweeps"] < 100
    M, U, kw, seed = sr.NOCONV_CASE
    got, z1 = _window(ctx, M, U, kw, seed)
    _check(got, z1, kw, "max_sweeps hit")
    assert got["status"] == ST_NOCONV and got["susie_sweeps"] == 2 and np.all(np.isfinite(got["susie_pip"]))


def test_a_null_window_keeps_nothing(ctx):
    p, gm, gu, _ = sr.small_window(65, 40, 9)
    first = hotpath.impute_window(0, gm, gu, p["off"], None, np.zeros(65), want_mats=True, ctx=ctx)
    z1 = np.random.default_rng(5).multivariate_normal(np.zeros(65), first["b11"]) * 0.7
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, want_mats=True, ctx=ctx, susie=dict(want_alpha=True))
    _check(got, z1, {}, "null window")
    assert np.all(got["susie_V"] == 0) and np.all(got["susie_pip"] == 0) and not got["susie_kept"].any() and np.all(got["susie_set"] == -1)


@pytest.mark.parametrize("kw", sr.COVERAGE_CASES)
def test_coverage_reaches_the_kernel(ctx, kw):
    M, U, seed = sr.COVERAGE_WINDOW
    got, z1 = _window(ctx, M, U, kw, seed, mode=1)
    want = _check(got, z1, kw, f"coverage {kw}")
    if kw["coverage"] >= 1.0:
        assert np.all(got["susie_size"] == int(want["adm"].sum()))


def test_nan_nonfinite_and_clamped_windows(ctx):
    """A NaN in z1: that SNP and every unmeasured SNP are no candidates, the rest is fitted.  A GAUSS_ST_NONFINITE window returns NaN,
    sizes 0, set -1.  A window MakePosDef repairs is not fitted (NOFIT) while z / info / selection / credible sets keep the bits of
    the call without the rider."""
    p, gm, gu, z1 = sr.small_window(12, 11, 14)
    z1[5] = np.nan
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, want_mats=True, ctx=ctx, susie=dict(L=3, want_alpha=True))
    assert got["status"] == 0 and np.all(np.isnan(got["z"]))
    _check(got, z1, dict(L=3), "NaN in z1")
    assert np.all(got["susie_alpha"][:, 12:] == 0) and np.all(got["susie_alpha"][:, 5] == 0) and np.all(np.isfinite(got["susie_pip"]))
    # no admissible candidate at all: alpha = mu = 0, pip 0, lse NaN, sizes 0, purity NaN, nothing kept, no status bit
    got = hotpath.impute_window(0, gm, gu, p["off"], None, np.full(12, np.nan), want_mats=True, ctx=ctx, susie=dict(L=3, want_alpha=True))
    _check(got, np.full(12, np.nan), dict(L=3), "every z1 NaN")
    assert got["status"] == 0 and np.all(got["susie_alpha"] == 0) and np.all(got["susie_mu"] == 0) and np.all(got["susie_pip"] == 0)
    assert np.all(np.isnan(got["susie_lse"])) and np.all(got["susie_size"] == 0) and not got["susie_kept"].any() and np.all(got["susie_V"] == 0)
    gm2 = gm.copy()
    gm2[3, :] = 1                                      # zero variance: CalCor returns 0 / 0
    got = hotpath.impute_window(0, gm2, gu, p["off"], None, np.nan_to_num(z1, nan=1.0), ctx=ctx, susie=dict(L=3, want_alpha=True))
    assert got["status"] & ST_NONFINITE and not got["status"] & (ST_NOFIT | ST_NOCONV)
    for k in ("susie_pip", "susie_set_pip", "susie_V", "susie_lse", "susie_mass", "susie_purity", "susie_alpha", "susie_mu"):
        assert np.all(np.isnan(got[k])), k
    assert np.all(got["susie_size"] == 0) and np.all(got["susie_kept"] == 0) and np.all(got["susie_set"] == -1) and got["susie_sweeps"] == 0
    p, gm, gu, z1 = cs_ref.clamped_window()
    slct = dict(max=32, chi2_stop=4.0, unmeasured=True, cs=dict(cs_ref.CS))
    keys = ("z", "info", "slct_idx", "slct_zin", "slct_joint", "slct_zc", "slct_var", "cond_z", "cond_var", "cs_pip", "cs_set", "cs_set_pip",
            "cs_size", "cs_mass", "cs_lse")
    plain = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, ctx=ctx, slct=slct)
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, ctx=ctx, slct=slct, susie=dict(want_alpha=True))
    assert plain["status"] == ST_CLAMPED and got["status"] == ST_CLAMPED | ST_NOFIT
    for k in keys:
        assert np.array_equal(got[k], plain[k], equal_nan=True), k
    assert np.all(np.isnan(got["susie_pip"])) and np.all(np.isnan(got["susie_V"])) and np.all(np.isnan(got["susie_alpha"]))
    assert np.all(got["susie_size"] == 0) and np.all(got["susie_kept"] == 0) and np.all(got["susie_set"] == -1) and got["susie_sweeps"] == 0


def test_the_two_planted_claims(ctx):
    """(a) the tag window: the fit returns one kept set around each causal SNP and neither holds the tag the stepwise selection takes
    first; (b) cs_ref.claim_window(): the unmeasured causal SNP leads its set."""
    p, gm, gu, z1, (c1, c2, tag) = sr.tag_window()
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, want_mats=True, ctx=ctx, slct=dict(max=5, chi2_stop=cs_ref.CHI2_GWS),
                                susie=dict(want_alpha=True))
    _check(got, z1, {}, "tag window")
    assert got["slct_idx"][0] == tag
    kept = np.flatnonzero(got["susie_kept"])
    assert len(kept) == 2 and sorted(int(np.argmax(got["susie_alpha"][l])) for l in kept) == sorted((c1, c2))
    assert got["susie_set"][tag] == -1 and got["susie_set"][c1] >= 0 and got["susie_set"][c2] >= 0 and got["susie_set"][c1] != got["susie_set"][c2]
    assert got["susie_pip"][tag] < 0.05
    p, gm, gu, z1, u = cs_ref.claim_window()
    M = gm.shape[0]
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, want_mats=True, ctx=ctx, susie=dict(want_alpha=True))
    _check(got, z1, {}, "claim window")
    l = got["susie_set"][M + u]
    assert l >= 0 and int(np.argmax(got["susie_alpha"][l])) == M + u and got["susie_alpha"][l][M + u] > got["susie_alpha"][l][:M].max()


def _store_windows(ctx, susie, **kw):
    """cs_ref.store_windows as windows over one resident 2-bit store and as byte rows in host memory, every window asking"""
    p, ws = cs_ref.store_windows(**kw)
    G = p["G"]
    rows2, src_off = panel_mod.pack2bit(G, p["off"])
    store = hotpath.RowStore(rows2, ctx=ctx)
    wins, host = [], []
    for w in ws:
        mi, ui = w["mi"], w["ui"]
        wins.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=w["z1"], dev=(store.ptr, store.ptr, len(mi), len(ui), store.ld),
                         packed=dict(fmt=1, rows_m=mi, rows_u=ui, pop_src_off=src_off), susie=susie))
        host.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=w["z1"], geno_m=np.ascontiguousarray(G[mi]),
                         geno_u=np.ascontiguousarray(G[ui]), susie=susie))
    return p, rows2, src_off, store, wins, host


def _run(ctx, wins, on_device=True, runs=1, want_mats=False):
    job = hotpath.Job(wins, ctx=ctx, on_device=on_device, want_mats=want_mats)
    for _ in range(runs):
        job.run()
    out = [job.fetch() for _ in range(runs)]
    cnt = job.counters()
    job.close()
    return out, cnt


ALL_KEYS = ("z", "info") + SUSIE_KEYS + ("susie_alpha", "susie_mu")
SUSIE = dict(L=5, max_sweeps=20, want_alpha=True)


def test_every_launch_form_and_source_format_returns_the_same_bits(ctx, monkeypatch):
    """The switches of tests/test_gpu_cs.py's test of the same name.  Under GAUSS_FUSED_SOLVE=0 the rider forces the fused form, as the
    leave-one-out values do: same bits there too, where a job in which nobody asks moves bits of z."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx, SUSIE)
    ref = _run(ctx, wins)[0][0]
    assert all(r["status"] & ~ST_NOCONV == 0 for r in ref) and any(r["susie_kept"].any() for r in ref)
    switches = [dict(GAUSS_CHAIN_ASIDE="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2"),
                dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2", GAUSS_EPI_EARLY="0"),
                dict(GAUSS_SHARE_MEASURED="0"), dict(GAUSS_SHARE_MEASURED="2"), dict(GAUSS_NO_SHIFT_CERT="1"),
                dict(GAUSS_FUSED_SOLVE="0", GAUSS_CHAIN_ASIDE="0")]
    for sw in switches:
        with monkeypatch.context() as m:
            for k, v in sw.items():
                m.setenv(k, v)
            for r, w in zip(_run(ctx, wins)[0][0], ref):
                _same(r, w, ALL_KEYS)
    with monkeypatch.context() as m:                   # ... where the plain job does take the stand-alone solver
        m.setenv("GAUSS_FUSED_SOLVE", "0")
        m.setenv("GAUSS_CHAIN_ASIDE", "0")
        alone = _run(ctx, [dict(w, susie=None) for w in wins])[0][0]
        assert any(not np.array_equal(a["z"], w["z"]) for a, w in zip(alone, ref))
    try:                                               # int8 Gram
        ctx.set_gram_dtype("i8")
        for r, w in zip(_run(ctx, wins)[0][0], ref):
            _same(r, w, ALL_KEYS)
    finally:
        ctx.set_gram_dtype(os.environ.get("GAUSS_GRAM_DTYPE", "f32"))
    for r, w in zip(_run(ctx, host, on_device=False)[0][0], ref):      # byte rows from host memory
        _same(r, w, ALL_KEYS)
    h2 = host[2]                                       # the blocking window call: streamed (default) and upload-then-run
    _same(hotpath.impute_window(1, h2["geno_m"], h2["geno_u"], p["off"], p["w"], h2["z1"], ctx=ctx, susie=SUSIE), ref[2], ALL_KEYS)
    with monkeypatch.context() as m:
        m.setenv("GAUSS_STREAM_WINDOW", "0")
        _same(hotpath.impute_window(1, h2["geno_m"], h2["geno_u"], p["off"], p["w"], h2["z1"], ctx=ctx, susie=SUSIE), ref[2], ALL_KEYS)
    with monkeypatch.context() as m:                   # read when a context is made: one queue
        m.setenv("GAUSS_SIDE_STREAM", "0")
        c = hotpath.Context(0)
        try:
            st2 = hotpath.RowStore(rows2, ctx=c)
            w2 = [dict(w, dev=(st2.ptr, st2.ptr) + w["dev"][2:]) for w in wins]
            for r, w in zip(_run(c, w2)[0][0], ref):
                _same(r, w, ALL_KEYS)
            st2.close()
        finally:
            c.close()
    store.close()


def test_three_windows_of_which_two_ask_and_a_job_in_which_nobody_asks(ctx):
    """Windows of one job may mix, with different L and sweeps.  The asking windows return what their stand-alone calls return, two
    runs in flight return the same values, and a job in which nobody asks has the counters and the bits of the same job built
    without the key."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx, SUSIE, seed=43, spans=((0, 131), (97, 340), (211, 560)))
    other = dict(L=2, max_sweeps=3, tol=0.0, want_alpha=True)
    ask = [SUSIE, None, other]
    mixed, c1 = _run(ctx, [dict(w, susie=ask[k]) for k, w in enumerate(wins)], runs=2)
    nobody, c0 = _run(ctx, [dict(w, susie=None) for w in wins], runs=2)
    plain, c2 = _run(ctx, [{k: v for k, v in w.items() if k != "susie"} for w in wins], runs=2)
    assert c0 == c1 == c2, (c0, c1, c2)
    for run in mixed:
        for k, r in enumerate(run):
            assert r["status"] & ~ST_NOCONV == plain[0][k]["status"]      # (window 2 runs its three sweeps out: tol = 0)
            assert np.array_equal(r["z"], plain[0][k]["z"]) and np.array_equal(r["info"], plain[0][k]["info"])
            assert ("susie_pip" in r) == (k != 1)
            if k != 1:
                h = host[k]
                _same(r, hotpath.impute_window(1, h["geno_m"], h["geno_u"], p["off"], p["w"], h["z1"], ctx=ctx, susie=ask[k]), ALL_KEYS)
    assert mixed[0][2]["susie_sweeps"] == 3 and mixed[0][2]["susie_V"].shape == (2,)
    for r, w in zip(nobody[1], plain[0]):
        _same(r, w, ("z", "info"))
        assert "susie_pip" not in r
    store.close()


def test_all_riders_on_one_window_at_once(ctx):
    """Leave-one-out values, the selection, the conditioned imputed SNPs, the credible sets, further traits, a mask of missing SNPs
    and the multi-causal fit on one window: each output has the bits of the call that asks for it alone."""
    p, gm, gu = cs_ref.window(129, 140, seed=77)
    M = 129
    z1 = cs_ref.planted(gm, seed=6)
    rng = np.random.default_rng(12)
    z_more = rng.standard_normal((3, M)) * 2
    mask = np.zeros((3, M), dtype=np.uint8)
    mask[0, [3, 50]] = 1
    mask[2, [7]] = 1
    slct = dict(max=32, chi2_stop=cs_ref.CHI2_GWS, unmeasured=True, cs=dict(cs_ref.CS))
    run = lambda **kw: hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, **kw)
    both = run(loo=True, slct=slct, z_more=z_more, miss_more=mask, susie=SUSIE)
    _same(both, run(susie=SUSIE), ALL_KEYS)
    _same(both, run(slct=slct), ("z", "info", "slct_idx", "slct_zin", "slct_joint", "slct_zc", "slct_var", "cond_z", "cond_var", "cs_pip", "cs_set",
                                 "cs_set_pip", "cs_size", "cs_mass", "cs_lse"), own_bits=ST_NOCONV)
    _same(both, run(loo=True), ("z", "info", "loo_z", "loo_info", "loo_t"), own_bits=ST_NOCONV)
    _same(both, run(z_more=z_more, miss_more=mask), ("z", "info", "z_more", "info_more", "z_miss", "info_miss"), own_bits=ST_NOCONV)
    assert both["susie_kept"].sum() >= 1


def test_refusals(ctx):
    p = small_panel(n_snp=120, scale=0.02, n_pops=5)
    gm, gu, z1 = split_window(p, 50)
    base = dict(mode=0, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=None, z1=z1, susie=dict(L=3))
    with pytest.raises(Exception, match="susie_L.*imputation windows only.*QCAT"):
        hotpath.Job([dict(base, qcat=(10, 30, 0.01))], ctx=ctx)
    with pytest.raises(Exception, match="susie_L.*imputation windows only.*LD"):
        hotpath.Job([dict(base, ld_codings=1)], ctx=ctx)
    run = lambda **kw: hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, susie=dict(dict(L=3), **kw))
    for bad in (-1, 33):
        with pytest.raises(Exception, match="susie_L = "):
            run(L=bad)
    for bad in (0.0, 1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(Exception, match="susie_coverage"):
            run(coverage=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(Exception, match="susie_prior_var"):
            run(prior_var=bad)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(Exception, match="susie_tol"):
            run(tol=bad)
    for bad in (0, -3, 1001, 10 ** 6):                 # (a run queues max_sweeps x L x 2 launches up front: capped)
        with pytest.raises(Exception, match="susie_max_sweeps = .*1 .. 1000 sweeps"):
            run(max_sweeps=bad)
    with pytest.raises(Exception, match="has no unmeasured SNPs"):      # refused as without the fit, with measured_only too
        hotpath.impute_window(0, gm, None, p["off"], None, z1, ctx=ctx, susie=dict(L=3, measured_only=True))
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(Exception, match="susie_min_abs_corr"):
            run(min_abs_corr=bad)
    ok = hotpath.Job([dict(base, qcat=(10, 30, 0.01), susie=None), base], ctx=ctx)      # a QCAT window beside one that asks
    ok.run()
    res = ok.fetch()
    ok.close()
    assert "r" in res[0] and "susie_pip" in res[1]


# ---- the host entry points, files -> table -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def study(tmp_path_factory):
    files = cs_ref.study_files(tmp_path_factory.mktemp("susie_study"))
    packed = os.path.join(os.path.dirname(files[2]), "panel.gpk")
    assert api.pack_panel(files[1], files[2], files[3], packed) > 0
    return dict(files=files, packed=packed)


def _same_column(a, b, c):
    if a[c].dtype.kind == "f":
        assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
    else:
        assert list(a[c]) == list(b[c]), c


@pytest.mark.parametrize("mix", [False, True])
def test_dist_susie_and_distmix_susie_end_to_end(ctx, study, mix, monkeypatch):
    """Text panel, packed panel and the packed panel through the full SNP map: the same table.  Its shared columns are dist() /
    distmix() of the same call bit for bit on the call's own rows; pip, cs and `effects` are the hotpath's result for the window the
    oracle's data layer builds, by rsid."""
    win = cs_ref.STUDY_WINDOW
    fw = cs_ref.feeder_window(mix, study["files"])
    meas, unme, gm, gu, off, w, who, cutoff = (fw[k] for k in ("meas", "unme", "gm", "gu", "off", "w", "who", "cutoff"))
    fn, fn_plain = (api.distmix_susie, api.distmix) if mix else (api.dist_susie, api.dist)
    inp, idx, dat, desc = study["files"]
    z1 = np.array([s.z for s in meas])
    M = len(meas)
    args = dict(L=6, coverage=0.9, max_sweeps=40)
    kw = dict(af1_cutoff=cutoff, ctx=ctx, **args)
    df = fn(*win, who, inp, idx, dat, desc, **kw)
    plain = fn_plain(*win, who, inp, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
    assert list(df.columns) == list(plain.columns) + ["wing", "pip", "cs", "cs_pip"]
    own = df.iloc[: len(plain)].reset_index(drop=True)
    for c in plain.columns:
        _same_column(own, plain, c)
    assert np.all(df["wing"].to_numpy()[: len(plain)] == 0) and np.all(df["wing"].to_numpy()[len(plain):] != 0)
    hp = hotpath.impute_window(1 if mix else 0, gm, gu, off, w, z1, want_mats=True, ctx=ctx, susie=dict(args, want_alpha=True))
    want = _check(hp, z1, args, f"table window mix={mix}")
    tol = sr.value_tol(want, 0.0)
    by = {r: k for k, r in enumerate(df["rsid"])}
    rows = np.array([by[s.rsid] for s in meas] + [by[s.rsid] for s in unme])          # every candidate has a row
    assert len(set(rows.tolist())) == len(rows) == len(df)
    assert np.array_equal(df["pip"].to_numpy()[rows], hp["susie_pip"]) and np.array_equal(df["cs_pip"].to_numpy()[rows], hp["susie_set_pip"])
    assert np.array_equal(df["cs"].to_numpy()[rows], hp["susie_set"] + 1)
    eff, fit = df.attrs["effects"], df.attrs["fit"]
    assert np.array_equal(eff["size"], hp["susie_size"]) and np.array_equal(eff["kept"], hp["susie_kept"] != 0)
    assert np.array_equal(eff["row"], rows[np.argmax(hp["susie_alpha"], axis=1)])
    for k in ("V", "lse", "mass", "purity"):
        assert np.array_equal(eff[k], hp["susie_" + k], equal_nan=True), k
    assert fit["sweeps"] == hp["susie_sweeps"] and fit["converged"] == (not hp["status"] & ST_NOCONV) and fit["delta"] == hp["susie_delta"]
    assert eff["kept"].any()
    print(f"REACHED susie table mix={mix}: kept {int(eff['kept'].sum())}  sweeps {fit['sweeps']}  (bound {tol:.3e})")
    forms = [fn(*win, who, inp, "(unused)", study["packed"], desc, **kw)]
    monkeypatch.setenv("GAUSS_HOST_FULL_MAP", "1")
    forms.append(fn(*win, who, inp, "(unused)", study["packed"], desc, **kw))
    forms.append(fn(*win, who, inp, idx, dat, desc, **kw))
    for other in forms:
        assert list(other.columns) == list(df.columns) and len(other) == len(df)
        for c in df.columns:
            _same_column(df, other, c)
        assert all(np.array_equal(other.attrs["effects"][k], df.attrs["effects"][k], equal_nan=True) for k in df.attrs["effects"])
        assert other.attrs["fit"] == df.attrs["fit"]
    with pytest.raises(Exception, match="susie_coverage"):
        fn(*win, who, inp, idx, dat, desc, af1_cutoff=cutoff, coverage=1.5, ctx=ctx)
    with pytest.raises(Exception, match="at most 32 effects"):
        fn(*win, who, inp, idx, dat, desc, af1_cutoff=cutoff, L=33, ctx=ctx)
