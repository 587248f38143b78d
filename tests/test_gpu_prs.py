"""GPU: the polygenic score weights of a window (k_prs.hip) against their definition (tests/prs_ref.py) evaluated on the B11 the GPU
returns.  beta, br, bg and delta are held to max(10 e_ref, 1e-8 max(1, max |beta_ref|)) absolute (prs_ref.value_tol: e_ref is the gap
between the reference's two statements on that case; 1e-8 is the project's fp64 bound); nnz, the support, the sweeps and the NOCONV bit
are exact, and no decision of a case may be borderline.  Independently of any statement of the algorithm every stored beta is held to
its KKT certificate.  Every case prints a REACHED line."""
import os

import numpy as np
import pytest

import cs_ref
import prs_ref as pr
from gauss_amd import api, hotpath
from gauss_amd import panel as panel_mod
from helpers import small_panel, split_window

pytestmark = pytest.mark.gpu

ST_CLAMPED, ST_NONFINITE, ST_NOCONV = 1, 2, 64
N = pr.N_STUDY
PRS_KEYS = ("prs_beta", "prs_nnz", "prs_sweeps", "prs_delta", "prs_br", "prs_bg", "prs_kkt")
EPS = 2.0 ** -52


def _same(a, b, keys, own_bits=0):
    """own_bits: status bits of the rider that `b`, a call without it, cannot carry"""
    assert a["status"] & ~own_bits == b["status"]
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _certificate(got, B, want, a, what):
    """Every stored beta against the KKT conditions of its (s, lam), from a fresh B beta in numpy.  Coordinate j was exactly optimal when
    last visited and no coordinate has moved by more than delta since: its residual is at most (1 - s) tol r_max sum_k |B_jk|, plus numpy's
    rounding of the gradient, M 2^-52 times the sum of its absolute terms.  The kernel's own prs_kkt lies within that rounding of the
    recomputed value."""
    M = B.shape[0]
    rowsum = np.abs(B).sum(axis=1)
    worst = 0.0
    for i_s, s in enumerate(a["s"]):
        for i_l, lam in enumerate(a["lam"]):
            beta = got["prs_beta"][i_s, i_l]
            top, res, mag = pr.kkt(B, want["r"], s, lam, beta, want["frozen"])
            rnd = M * EPS * mag
            bound = (1.0 - s) * a["tol"] * want["rmax"] * rowsum + rnd
            if not want["noconv"][i_s, i_l]:               # (a cell that ran its sweeps out promises nothing)
                assert np.all(res <= bound), (what, i_s, i_l, float(np.max(res - bound)))
                worst = max(worst, float(np.max(res / bound)))
            assert abs(got["prs_kkt"][i_s, i_l] - top) <= float(rnd.max()), (what, i_s, i_l, got["prs_kkt"][i_s, i_l], top)
    return worst


def _check(got, z1, kw, what, n=N):
    """got: a window's result with b11 and prs_*.  The reference on the GPU's matrix, vetted again there."""
    B = got["b11"]
    bl, want, e_ref = pr.borderline(B, z1, n, **kw)
    assert bl == [], (what, bl)
    tol = pr.value_tol(want, e_ref)
    a = pr.args_of(**kw)
    e = {k: float(np.max(np.abs(got["prs_" + k] - want[k]), initial=0.0)) for k in pr.VALUE_KEYS}
    share = _certificate(got, B, want, a, what)
    print(f"REACHED prs {what}: M {B.shape[0]}  cells {want['nnz'].size}  sweeps {int(want['sweeps'].sum())}  nnz <= {int(want['nnz'].max())}  "
          f"r_max {want['rmax']:.3f}  e_ref {e_ref:.2e}  " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"  (bound {tol:.2e})  kkt / bound <= {share:.2f}")
    assert max(e.values()) <= tol, (what, e, tol)
    assert np.array_equal(got["prs_nnz"], want["nnz"]), what
    assert np.array_equal(got["prs_beta"] != 0, want["beta"] != 0), what
    assert np.array_equal(got["prs_sweeps"], want["sweeps"]), (what, got["prs_sweeps"], want["sweeps"])
    assert bool(got["status"] & ST_NOCONV) == bool(want["noconv"].any()), (what, got["status"])
    return want


def _window(ctx, M, U, kw, seed, mode=0, **more):
    p, gm, gu, z1 = pr.small_window(M, U, seed)
    got = hotpath.impute_window(mode, gm, gu, p["off"], p["w"] if mode else None, z1, want_mats=True, ctx=ctx, prs=dict(kw, n=N), **more)
    return got, z1


@pytest.mark.parametrize("case", pr.SMALL_CASES, ids=pr.case_id)
def test_small_cases(ctx, case):
    """M on either side of a wave and of the workgroup, on pooled and on weighted LD, with the default grid and with one cell"""
    M, U, kw, seed, mode = case
    got, z1 = _window(ctx, M, U, kw, seed, mode=mode)
    assert got["status"] == 0
    want = _check(got, z1, kw, f"M={M} mode={mode} {'one cell' if kw else 'default grid'}")
    assert want["nnz"].max() >= min(M, 2) and (kw or np.all(np.diff(want["nnz"], axis=1) >= 0))      # the path opens up


def test_the_largest_window_of_chr22(ctx):
    M, U, kw, seed = pr.LARGE_CASE
    p, gm, gu = cs_ref.window(M, U, scale=0.1)
    z1 = cs_ref.planted(gm, seed=seed)
    got = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, want_mats=True, ctx=ctx, prs=dict(kw, n=N))
    _check(got, z1, kw, f"M={M} U={U} weighted, default grid")


def test_a_short_fit_reports_it(ctx):
    M, U, kw, seed = pr.NOCONV_CASE
    got, z1 = _window(ctx, M, U, kw, seed)
    want = _check(got, z1, kw, "max_sweeps = 2")
    assert got["status"] == ST_NOCONV and want["noconv"].any() and got["prs_sweeps"].max() == 2 and np.all(np.isfinite(got["prs_beta"]))


def test_frozen_nonfinite_and_clamped_windows(ctx):
    """A z1 that is not finite: that SNP is frozen at 0 and the rest is fitted.  Every z1 NaN: beta = 0 after one sweep, no status bit.
    A GAUSS_ST_NONFINITE window returns NaN / 0.  A window MakePosDef repairs is fitted on the repaired matrix, the one the selection
    runs on, and every other output keeps the bits of the call without the rider."""
    M, U, kw, seed, bad = pr.FROZEN_CASE
    p, gm, gu, z1 = pr.small_window(M, U, seed)
    z1[bad[0]], z1[bad[1]] = np.nan, np.inf
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, want_mats=True, ctx=ctx, prs=dict(kw, n=N))
    assert got["status"] == 0
    want = _check(got, z1, kw, "two frozen SNPs")
    assert np.all(got["prs_beta"][:, :, list(bad)] == 0) and want["nnz"].max() > 10
    none = np.full(M, np.nan)
    got = hotpath.impute_window(0, gm, gu, p["off"], None, none, want_mats=True, ctx=ctx, prs=dict(kw, n=N))
    _check(got, none, kw, "every z1 NaN")
    assert got["status"] == 0 and np.all(got["prs_beta"] == 0) and np.all(got["prs_sweeps"] == 1) and np.all(got["prs_nnz"] == 0)
    assert np.all(got["prs_br"] == 0) and np.all(got["prs_kkt"] == 0)
    gm2 = gm.copy()
    gm2[3, :] = 1                                      # zero variance: CalCor returns 0 / 0
    got = hotpath.impute_window(0, gm2, gu, p["off"], None, np.nan_to_num(z1, nan=1.0, posinf=1.0), ctx=ctx, prs=dict(kw, n=N))
    assert got["status"] & ST_NONFINITE and not got["status"] & ST_NOCONV
    for k in ("prs_beta", "prs_delta", "prs_br", "prs_bg", "prs_kkt"):
        assert np.all(np.isnan(got[k])), k
    assert np.all(got["prs_nnz"] == 0) and np.all(got["prs_sweeps"] == 0)
    p, gm, gu, z1 = cs_ref.clamped_window()
    slct = dict(max=32, chi2_stop=4.0, unmeasured=True, cs=dict(cs_ref.CS))
    keys = ("z", "info", "slct_idx", "slct_zin", "slct_joint", "slct_zc", "slct_var", "cond_z", "cond_var", "cs_pip", "cs_set", "cs_set_pip",
            "cs_size", "cs_mass", "cs_lse")
    plain = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, ctx=ctx, slct=slct)
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, want_mats=True, ctx=ctx, slct=slct, prs=dict(n=N))
    assert plain["status"] == ST_CLAMPED and got["status"] & ~ST_NOCONV == ST_CLAMPED
    for k in keys:
        assert np.array_equal(got[k], plain[k], equal_nan=True), k
    _check(got, z1, {}, "clamped window, on the repaired B11")      # (b11 is the repaired matrix)


def test_a_wave_per_chain_returns_the_bits_of_a_workgroup_per_chain(ctx, monkeypatch):
    """The fit has no reductions: how the row update is spread over lanes does not reach the result"""
    M, U, kw, seed, mode = 300, 3, {}, 400, 0
    ref, _ = _window(ctx, M, U, kw, seed, mode=mode)
    monkeypatch.setenv("GAUSS_PRS_T", "64")
    got, _ = _window(ctx, M, U, kw, seed, mode=mode)
    _same(got, ref, PRS_KEYS)


def _store_windows(ctx, prs, **kw):
    """cs_ref.store_windows as windows over one resident 2-bit store and as byte rows in host memory, every window asking"""
    p, ws = cs_ref.store_windows(**kw)
    G = p["G"]
    rows2, src_off = panel_mod.pack2bit(G, p["off"])
    store = hotpath.RowStore(rows2, ctx=ctx)
    wins, host = [], []
    for w in ws:
        mi, ui = w["mi"], w["ui"]
        wins.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=w["z1"], dev=(store.ptr, store.ptr, len(mi), len(ui), store.ld),
                         packed=dict(fmt=1, rows_m=mi, rows_u=ui, pop_src_off=src_off), prs=prs))
        host.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=w["z1"], geno_m=np.ascontiguousarray(G[mi]),
                         geno_u=np.ascontiguousarray(G[ui]), prs=prs))
    return p, rows2, src_off, store, wins, host


def _run(ctx, wins, on_device=True, runs=1, want_mats=False):
    job = hotpath.Job(wins, ctx=ctx, on_device=on_device, want_mats=want_mats)
    for _ in range(runs):
        job.run()
    out = [job.fetch() for _ in range(runs)]
    cnt = job.counters()
    job.close()
    return out, cnt


ALL_KEYS = ("z", "info") + PRS_KEYS
PRS = dict(n=N, s=(0.3, 1.0, 0.7), lam=(0.05, 0.02, 0.03, 0.0), max_sweeps=30)      # (a path in the caller's order, ridge at its end)


def test_every_launch_form_and_source_format_returns_the_same_bits(ctx, monkeypatch):
    """The switches of tests/test_gpu_cs.py's test of the same name.  The rider needs B11 and z1 only: under GAUSS_FUSED_SOLVE=0 the
    job takes the stand-alone solver as it does without the rider, and the weights keep their bits there too."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx, PRS)
    ref = _run(ctx, wins)[0][0]
    assert all(r["status"] & ~ST_NOCONV == 0 for r in ref) and all(r["prs_nnz"].max() > 0 for r in ref)
    switches = [dict(GAUSS_CHAIN_ASIDE="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2"),
                dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2", GAUSS_EPI_EARLY="0"),
                dict(GAUSS_SHARE_MEASURED="0"), dict(GAUSS_SHARE_MEASURED="2"), dict(GAUSS_NO_SHIFT_CERT="1")]
    for sw in switches:
        with monkeypatch.context() as m:
            for k, v in sw.items():
                m.setenv(k, v)
            for r, w in zip(_run(ctx, wins)[0][0], ref):
                _same(r, w, ALL_KEYS)
    with monkeypatch.context() as m:                   # the stand-alone solver: z moves as it does without the rider, the weights do not
        m.setenv("GAUSS_FUSED_SOLVE", "0")
        m.setenv("GAUSS_CHAIN_ASIDE", "0")
        alone = _run(ctx, [dict(w, prs=None) for w in wins])[0][0]
        for r, w, q in zip(_run(ctx, wins)[0][0], ref, alone):
            _same(r, w, PRS_KEYS)
            _same(r, q, ("z", "info"), own_bits=ST_NOCONV)
    try:                                               # int8 Gram
        ctx.set_gram_dtype("i8")
        for r, w in zip(_run(ctx, wins)[0][0], ref):
            _same(r, w, ALL_KEYS)
    finally:
        ctx.set_gram_dtype(os.environ.get("GAUSS_GRAM_DTYPE", "f32"))
    for r, w in zip(_run(ctx, host, on_device=False)[0][0], ref):      # byte rows from host memory
        _same(r, w, ALL_KEYS)
    h2 = host[2]                                       # the blocking window call: streamed (default) and upload-then-run
    _same(hotpath.impute_window(1, h2["geno_m"], h2["geno_u"], p["off"], p["w"], h2["z1"], ctx=ctx, prs=PRS), ref[2], ALL_KEYS)
    with monkeypatch.context() as m:
        m.setenv("GAUSS_STREAM_WINDOW", "0")
        _same(hotpath.impute_window(1, h2["geno_m"], h2["geno_u"], p["off"], p["w"], h2["z1"], ctx=ctx, prs=PRS), ref[2], ALL_KEYS)
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
    # a prefix of the path: the cells it shares keep their bits (the order of the lam inside a chain is the only ordering)
    short = dict(PRS, lam=PRS["lam"][:2], s=PRS["s"][:2])
    got = hotpath.impute_window(1, h2["geno_m"], h2["geno_u"], p["off"], p["w"], h2["z1"], ctx=ctx, prs=short)
    for k in PRS_KEYS:
        assert np.array_equal(got[k], ref[2][k][:2, :2]), k
    store.close()


def test_three_windows_of_which_two_ask_and_a_job_in_which_nobody_asks(ctx):
    """Windows of one job may mix, with different grids.  The asking windows return what their stand-alone calls return, two runs in
    flight return the same values, and a job in which nobody asks has the counters and the bits of the same job built without the key."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx, PRS, seed=43, spans=((0, 131), (97, 340), (211, 560)))
    other = dict(n=900.0, s=(1.0,), lam=(0.01,), max_sweeps=1, tol=0.0)
    ask = [PRS, None, other]
    mixed, c1 = _run(ctx, [dict(w, prs=ask[k]) for k, w in enumerate(wins)], runs=2)
    nobody, c0 = _run(ctx, [dict(w, prs=None) for w in wins], runs=2)
    plain, c2 = _run(ctx, [{k: v for k, v in w.items() if k != "prs"} for w in wins], runs=2)
    assert c0 == c1 == c2, (c0, c1, c2)
    for run in mixed:
        for k, r in enumerate(run):
            assert r["status"] & ~ST_NOCONV == plain[0][k]["status"]
            assert np.array_equal(r["z"], plain[0][k]["z"]) and np.array_equal(r["info"], plain[0][k]["info"])
            assert ("prs_beta" in r) == (k != 1)
            if k != 1:
                h = host[k]
                _same(r, hotpath.impute_window(1, h["geno_m"], h["geno_u"], p["off"], p["w"], h["z1"], ctx=ctx, prs=ask[k]), ALL_KEYS)
    assert mixed[0][2]["prs_beta"].shape == (1, 1, len(host[2]["z1"])) and mixed[0][2]["status"] & ST_NOCONV      # tol = 0: never below
    for r, w in zip(nobody[1], plain[0]):
        _same(r, w, ("z", "info"))
        assert "prs_beta" not in r
    store.close()


def test_all_riders_on_one_window_at_once(ctx):
    """Leave-one-out values, the selection with its conditioned SNPs and credible sets, the multi-causal fit and the score weights on one
    window: each output has the bits of the call that asks for it alone."""
    p, gm, gu = cs_ref.window(129, 140, seed=77)
    z1 = cs_ref.planted(gm, seed=6)
    slct = dict(max=32, chi2_stop=cs_ref.CHI2_GWS, unmeasured=True, cs=dict(cs_ref.CS))
    susie = dict(L=5, max_sweeps=20)
    run = lambda **kw: hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, **kw)
    both = run(loo=True, slct=slct, susie=susie, prs=PRS)
    _same(both, run(prs=PRS), ALL_KEYS, own_bits=16)
    _same(both, run(slct=slct), ("z", "info", "slct_idx", "slct_zin", "slct_joint", "slct_zc", "slct_var", "cond_z", "cond_var", "cs_pip", "cs_set",
                                 "cs_set_pip", "cs_size", "cs_mass", "cs_lse"), own_bits=16 | ST_NOCONV)
    _same(both, run(loo=True), ("z", "info", "loo_z", "loo_info", "loo_t"), own_bits=16 | ST_NOCONV)
    _same(both, run(susie=susie), ("z", "info", "susie_pip", "susie_set", "susie_set_pip", "susie_V", "susie_lse", "susie_size", "susie_kept",
                                   "susie_sweeps", "susie_delta"), own_bits=ST_NOCONV)
    assert both["prs_nnz"].max() > 0


def test_refusals(ctx):
    p = small_panel(n_snp=120, scale=0.02, n_pops=5)
    gm, gu, z1 = split_window(p, 50)
    base = dict(mode=0, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=None, z1=z1, prs=dict(n=N))
    with pytest.raises(Exception, match="prs_n_s.*imputation windows only.*QCAT"):
        hotpath.Job([dict(base, qcat=(10, 30, 0.01))], ctx=ctx)
    with pytest.raises(Exception, match="prs_n_s.*imputation windows only.*LD"):
        hotpath.Job([dict(base, ld_codings=1)], ctx=ctx)
    run = lambda **kw: hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, prs=dict(dict(n=N), **kw))
    for bad in ([], [0.5] * 9):
        with pytest.raises(Exception, match="prs_n_s = "):
            run(s=bad)
    for bad in ([], [0.01] * 33):
        with pytest.raises(Exception, match="prs_n_lam = "):
            run(lam=bad)
    for bad in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(Exception, match=r"prs_s\[1\] = "):
            run(s=[0.5, bad])
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(Exception, match=r"prs_lam\[2\] = "):
            run(lam=[0.1, 0.05, bad])
    for bad in (2.0, 0.0, -5.0, float("nan"), float("inf")):
        with pytest.raises(Exception, match="prs_n = "):
            run(n=bad)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(Exception, match="prs_tol"):
            run(tol=bad)
    for bad in (0, -3, 1001, 10 ** 6):
        with pytest.raises(Exception, match="prs_max_sweeps = .*1 .. 1000 sweeps"):
            run(max_sweeps=bad)
    ok = hotpath.Job([dict(base, qcat=(10, 30, 0.01), prs=None), base], ctx=ctx)      # a QCAT window beside one that asks
    ok.run()
    res = ok.fetch()
    ok.close()
    assert "r" in res[0] and "prs_beta" in res[1]


# ---- the host entry points, files -> table -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def study(tmp_path_factory):
    files = cs_ref.study_files(tmp_path_factory.mktemp("prs_study"))
    packed = os.path.join(os.path.dirname(files[2]), "panel.gpk")
    assert api.pack_panel(files[1], files[2], files[3], packed) > 0
    return dict(files=files, packed=packed)


def _same_column(a, b, c):
    if a[c].dtype.kind == "f":
        assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
    else:
        assert list(a[c]) == list(b[c]), c


@pytest.mark.parametrize("mix", [False, True])
def test_dist_prs_and_distmix_prs_end_to_end(ctx, study, mix, monkeypatch):
    """Text panel, packed panel and the packed panel through the full SNP map: the same table.  One row per measured SNP of the
    extended window, in the order of the window the oracle's data layer builds; r, wing, `beta` and `grid` are the hotpath's result for
    that window, which is held to fit_cov on the exported B11."""
    win = cs_ref.STUDY_WINDOW
    fw = cs_ref.feeder_window(mix, study["files"])
    meas, gm, gu, off, w, who, cutoff = (fw[k] for k in ("meas", "gm", "gu", "off", "w", "who", "cutoff"))
    fn = api.distmix_prs if mix else api.dist_prs
    inp, idx, dat, desc = study["files"]
    z1 = np.array([s.z for s in meas])
    args = dict(s=(0.5, 1.0), lam=(0.05, 0.02, 0.01), max_sweeps=50)
    kw = dict(af1_cutoff=cutoff, ctx=ctx, **args)
    df = fn(*win, who, inp, idx, dat, desc, N, **kw)
    assert list(df.columns) == ["rsid", "chr", "bp", "a1", "a2", "af1mix" if mix else "af1ref", "z", "r", "wing"]
    assert list(df["rsid"]) == [s.rsid for s in meas] and np.array_equal(df["z"].to_numpy(), z1)
    inside = np.array([win[1] <= s.bp <= win[2] for s in meas])
    assert np.array_equal(df["wing"].to_numpy() == 0, inside) and not inside.all()
    hp = hotpath.impute_window(1 if mix else 0, gm, gu, off, w, z1, want_mats=True, ctx=ctx, prs=dict(args, n=N))
    want = _check(hp, z1, args, f"table window mix={mix}")
    assert np.array_equal(df["r"].to_numpy(), want["r"])
    grid = df.attrs["grid"]
    assert np.array_equal(df.attrs["beta"], hp["prs_beta"].reshape(6, -1))
    assert np.array_equal(grid["s"], np.repeat(args["s"], 3)) and np.array_equal(grid["lam"], np.tile(args["lam"], 2))
    for k in ("nnz", "sweeps", "delta", "br", "bg", "kkt"):
        assert np.array_equal(grid[k], hp["prs_" + k].reshape(-1)), k
    assert np.array_equal(grid["converged"], ~want["noconv"].reshape(-1)) and grid["nnz"].max() > 0
    af = df["af1mix" if mix else "af1ref"].to_numpy()
    per = fn(*win, who, inp, idx, dat, desc, N, per_allele=True, **kw)
    assert np.array_equal(per.attrs["beta"], df.attrs["beta"] / np.sqrt(2.0 * af * (1.0 - af))[None, :])
    dflt = fn(*win, who, inp, idx, dat, desc, N, af1_cutoff=cutoff, ctx=ctx)      # lassosum's grid
    assert dflt.attrs["beta"].shape == (80, len(meas)) and np.array_equal(dflt.attrs["grid"]["s"], np.repeat(pr.DEFAULT_S, 20))
    assert np.allclose(dflt.attrs["grid"]["lam"], np.tile(pr.DEFAULT_LAM, 4), rtol=1e-14, atol=0)
    forms = [fn(*win, who, inp, "(unused)", study["packed"], desc, N, **kw)]
    monkeypatch.setenv("GAUSS_HOST_FULL_MAP", "1")
    forms.append(fn(*win, who, inp, "(unused)", study["packed"], desc, N, **kw))
    forms.append(fn(*win, who, inp, idx, dat, desc, N, **kw))
    for other in forms:
        assert list(other.columns) == list(df.columns) and len(other) == len(df)
        for c in df.columns:
            _same_column(df, other, c)
        assert np.array_equal(other.attrs["beta"], df.attrs["beta"])
        assert all(np.array_equal(other.attrs["grid"][k], grid[k]) for k in grid)
    with pytest.raises(Exception, match=r"prs_s\[0\]"):
        fn(*win, who, inp, idx, dat, desc, N, af1_cutoff=cutoff, s=[1.5], ctx=ctx)
    with pytest.raises(Exception, match="prs_n = "):
        fn(*win, who, inp, idx, dat, desc, 2.0, af1_cutoff=cutoff, ctx=ctx)
