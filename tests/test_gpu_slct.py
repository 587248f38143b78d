"""GPU: stepwise conditional signal selection (slct_* of gauss_window_desc, k_slct.hip) against tests/slct_ref.py.

Every case asks for out_b11 and is compared with slct_ref.slct_by_definition evaluated ON THE B11 THE GPU RETURNED (np.linalg.solve
on the selected submatrix at every step: no arithmetic shared with the kernel's recurrence).  n and the selected indices must be
exactly equal -- asserted only after the reference's margin says that no decision of the case sits within 1e-9 of a tie, a threshold
or a guard -- and zin, joint, zc and var_left agree within 1e-8 as |d| / max(1, |want|), the project's bound for solve outputs
(tests/test_gpu_parity.py), with NaNs in the same places.  Each case prints the level it reaches (REACHED lines)."""
import os

import numpy as np
import pytest

from gauss_amd import api, hotpath
from gauss_amd import panel as panel_mod
from helpers import small_panel, split_window
from loo_ref import window_b11
from slct_ref import min_var_frac, slct_by_definition

pytestmark = pytest.mark.gpu

TOL = 1e-8
MARGIN = 1e-9
CHI2_GWS = 29.716785
KEYS = ("slct_idx", "slct_zin", "slct_joint", "slct_zc", "slct_var")
THREADS = 512                      # SLCT_T of k_slct.hip: at M = 513 a thread owns two SNPs
LDS_M = 2048                       # SLCT_LDS_M: beyond it r and v leave LDS for the result block


def _err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaNs in different places"
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok])))) if ok.any() else 0.0


def _check(got, z1, slct, lam=0.1, what="", tol=TOL):
    """got: a window's result (with b11); slct: the dict the window was given."""
    mvf = min_var_frac(slct.get("collin", 0.9), lam)
    want = slct_by_definition(got["b11"], z1, slct["max"], slct["chi2_stop"], mvf, slct.get("forced", ()))
    print(f"slct {what}: n gpu {got['slct_n']} ref {want['n']}  idx {want['idx'].tolist()}  margin {want['min_margin']:.3e}")
    assert want["min_margin"] > MARGIN, (what, want["min_margin"])
    assert got["slct_n"] == want["n"] and np.array_equal(got["slct_idx"], want["idx"]), (what, got["slct_idx"], want["idx"])
    K, n = slct["max"], want["n"]
    raw = got["slct_raw"]
    assert np.all(raw["idx"][n:] == -1) and np.all(np.isnan(raw["zin"][n:])) and np.all(np.isnan(raw["joint"][n:])) and len(raw["idx"]) == K
    e = dict(zin=_err(got["slct_zin"], want["zin"]), joint=_err(got["slct_joint"], want["joint"]),
             zc=_err(got["slct_zc"], want["zc"]), var=_err(got["slct_var"], want["var"]))
    print(f"REACHED slct {what}: " + "  ".join(f"{k} {v:.3e}" for k, v in e.items()) + f"  (bound {tol:g})")
    assert max(e.values()) <= tol, (what, e)
    assert bool(got["status"] & 8) == bool(want["skipped"]), (what, got["status"], want["skipped"])
    return want


def _pooled(gm):
    from oracle import oracle_np
    return oracle_np.pooled_cor(gm)


def _planted(gm, seed, effect=(10.0, -9.0, 9.5)):
    """Z-scores with three signals spread through the window's (pooled) LD."""
    M = gm.shape[0]
    rng = np.random.default_rng(seed)
    causal = sorted({M // 7, M // 2, max(M - 9, 0)})
    B = _pooled(gm) if M > 1 else np.ones((1, 1))
    return B[:, causal] @ np.array(effect[: len(causal)]) + rng.standard_normal(M)


def _window(M, U=40, seed=None, scale=0.02):
    p = small_panel(n_snp=M + U + 30 + M // 20, scale=scale, seed=11 + M if seed is None else seed)
    gm, gu, _ = split_window(dict(G=p["G"][: M + U]), M)
    return p, gm, gu


def _same(a, b, keys=("z", "info") + KEYS):
    assert a["status"] == b["status"]
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _run(ctx, wins, on_device=True, runs=1, want_mats=False):
    job = hotpath.Job(wins, ctx=ctx, on_device=on_device, want_mats=want_mats)
    for _ in range(runs):
        job.run()
    out = [job.fetch() for _ in range(runs)]
    cnt = job.counters()
    job.close()
    return out, cnt


@pytest.mark.parametrize("M,mode", [(1, 0), (2, 0), (2, 1), (63, 0), (64, 1), (65, 0), (65, 1), (129, 0), (129, 1),
                                    (THREADS + 1, 0), (THREADS + 1, 1), (LDS_M + 52, 0)])
def test_selection_matches_the_definition_at_the_kernel_edges(ctx, M, mode):
    """M around the 64-row padding and panel edges, one above the workgroup's thread count (a thread owns two SNPs) and one above
    the LDS limit (r and v live in the result block); pooled and weighted; planted signals at the genome-wide threshold, then the
    same window at a low threshold so that many steps run.  z / info are the bits of the same call without the selection."""
    p, gm, gu = _window(M)
    w = p["w"] if mode else None
    z1 = _planted(gm, seed=M + mode)
    for k, slct in enumerate((dict(max=32, chi2_stop=CHI2_GWS), dict(max=12, chi2_stop=1.0))):
        got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, want_mats=True, ctx=ctx, slct=slct)
        assert got["status"] == 0
        want = _check(got, z1, slct, what=f"M={M} mode={mode} stop={slct['chi2_stop']:g}")
        if k == 0:
            plain = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx)
            _same(got, plain, ("z", "info"))
            assert want["n"] >= 1
        elif M >= 63:
            assert want["n"] == 12


def test_one_snp_enters_iff_its_chi2_reaches_the_threshold(ctx):
    p, gm, gu = _window(1)
    for z0, lam, n in ((6.0, 0.1, 1), (5.0, 0.1, 0), (6.0, 0.5, 0)):          # 36 / 1.1 = 32.7, 25 / 1.1 = 22.7, 36 / 1.5 = 24
        slct = dict(max=32, chi2_stop=CHI2_GWS)
        got = hotpath.impute_window(0, gm, gu, p["off"], None, np.array([z0]), lam=lam, want_mats=True, ctx=ctx, slct=slct)
        _check(got, np.array([z0]), slct, lam=lam, what=f"M=1 z={z0} lam={lam}")
        assert got["slct_n"] == n


def test_k_one_k_reached_and_nothing_selected(ctx):
    p, gm, gu = _window(120, seed=19)
    _, _, z1 = split_window(dict(G=p["G"][:160]), 120)
    for slct, n in ((dict(max=1, chi2_stop=0.05), 1), (dict(max=32, chi2_stop=0.05), 32), (dict(max=32, chi2_stop=1e3), 0)):
        got = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, want_mats=True, ctx=ctx, slct=slct)
        _check(got, z1, slct, what=f"K={slct['max']} stop={slct['chi2_stop']:g}")
        assert got["slct_n"] == n
    assert np.array_equal(got["slct_var"], np.ones(120))                    # nothing selected: nothing explained


def test_forced_snps_twins_and_the_skipped_bit(ctx):
    """Duplicated measured rows (rows 50, 51 repeat 7, 23): the guard excludes the twin of a selected SNP; forced SNPs enter first
    in the caller's order; a forced twin fails the guard, is left out and raises GAUSS_ST_SLCT_SKIPPED."""
    p = small_panel(n_snp=120, scale=0.02, seed=31)
    gm, gu, _ = split_window(dict(G=p["G"][:110]), 50)
    gm = np.ascontiguousarray(np.vstack([gm, gm[[7, 23]]]))
    B = _pooled(gm)
    rng = np.random.default_rng(3)
    z1 = B[:, [7, 23, 40]] @ np.array([9.0, -8.0, 7.0]) + 0.3 * rng.standard_normal(52)
    z1[50], z1[51] = z1[7] - 0.01, z1[23] + 0.01
    run = lambda slct: hotpath.impute_window(0, gm, gu, p["off"], None, z1, want_mats=True, ctx=ctx, slct=slct)
    slct = dict(max=32, chi2_stop=CHI2_GWS)
    got = run(slct)
    assert got["b11"][50, 7] == 1.0
    want = _check(got, z1, slct, what="duplicated rows")
    assert 7 in want["idx"] and 50 not in want["idx"] and np.isnan(got["slct_zc"][50]) and got["status"] == 0
    slct = dict(max=3, chi2_stop=CHI2_GWS, forced=[11, 2, 44])
    want = _check(run(slct), z1, slct, what="forced only")
    assert want["idx"].tolist() == [11, 2, 44]
    slct = dict(max=32, chi2_stop=CHI2_GWS, forced=[11, 2])
    want = _check(run(slct), z1, slct, what="forced then free")
    assert want["idx"].tolist()[:2] == [11, 2] and want["n"] > 2
    slct = dict(max=4, chi2_stop=CHI2_GWS, forced=[7, 50, 23])
    got = run(slct)
    want = _check(got, z1, slct, what="forced twin")
    assert got["status"] == 8 and want["idx"].tolist()[:2] == [7, 23] and 50 not in want["idx"]


def test_nan_in_z1_and_a_nonfinite_window(ctx):
    p, gm, gu = _window(65, seed=5)
    z1 = _planted(gm, seed=9)
    z1[13] = np.nan                                    # a NaN statistic never wins and stays NaN; the others are selected around it
    slct = dict(max=32, chi2_stop=CHI2_GWS)
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, want_mats=True, ctx=ctx, slct=slct)
    want = _check(got, z1, slct, what="NaN in z1")
    assert want["n"] >= 1 and 13 not in want["idx"] and np.isnan(got["slct_zc"][13]) and not np.isnan(got["slct_var"][13])
    gm = gm.copy()
    gm[3, :] = 1                                       # zero variance: CalCor returns 0 / 0
    got = hotpath.impute_window(0, gm, gu, p["off"], None, np.nan_to_num(z1, nan=1.0), ctx=ctx, slct=slct)
    assert got["status"] & 2 and got["slct_n"] == 0 and len(got["slct_idx"]) == 0
    assert np.all(got["slct_raw"]["idx"] == -1) and np.all(np.isnan(got["slct_raw"]["zin"])) and np.all(np.isnan(got["slct_raw"]["joint"]))
    assert got["slct_zc"].shape == (65,) and np.all(np.isnan(got["slct_zc"])) and np.all(np.isnan(got["slct_var"]))


def test_clamped_window_selects_on_the_repaired_matrix(ctx):
    """Duplicated measured SNPs at lambda = 0 (the construction of tests/test_gpu_clamp.py): MakePosDef rebuilds B11, the selection
    runs again inside the window's re-factorisation, and is compared on the repaired B11 the job returns."""
    p = small_panel(n_snp=70, scale=0.02, n_pops=6, seed=21)
    gm, gu, _ = split_window(p, 30)
    gm = np.ascontiguousarray(np.vstack([gm, gm[:3]]))
    z1 = _planted(gm, seed=2)
    z1[30:] = z1[:3] + 0.3
    slct = dict(max=32, chi2_stop=4.0)
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, want_mats=True, ctx=ctx, slct=slct)
    plain = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, ctx=ctx)
    assert got["status"] & 1
    _same(got, plain, ("z", "info"))
    want = _check(got, z1, slct, lam=0.0, what="clamped window")
    assert want["n"] >= 2


def _store_windows(ctx, seed=41, n_snp=2000, spans=((0, 131), (97, 340), (211, 560), (330, None), (400, 540))):
    """Windows over one resident 2-bit store, overlapping like a chromosome's (shared measured rows apply)."""
    p = small_panel(n_snp=n_snp, scale=0.05, seed=seed)
    G = p["G"]
    rows2, src_off = panel_mod.pack2bit(G, p["off"])
    store = hotpath.RowStore(rows2, ctx=ctx)
    rng = np.random.default_rng(5)
    n = G.shape[0]
    measured = np.sort(rng.choice(n, size=n // 3, replace=False))
    unmeasured = np.setdiff1d(np.arange(n), measured)
    wins, host = [], []
    for k, (a, b) in enumerate(spans):
        mi = measured[a:b]
        lo, hi = mi[len(mi) // 4], mi[3 * len(mi) // 4]
        ui = unmeasured[(unmeasured > lo) & (unmeasured < hi)]
        z1 = _planted(G[mi], seed=70 + k)
        slct = dict(max=32, chi2_stop=CHI2_GWS if k % 2 == 0 else 3.0, forced=[5, 1] if k == 1 else [])
        wins.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=z1, dev=(store.ptr, store.ptr, len(mi), len(ui), store.ld),
                         packed=dict(fmt=1, rows_m=mi.astype(np.int32), rows_u=ui.astype(np.int32), pop_src_off=src_off), slct=slct))
        host.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=z1, geno_m=np.ascontiguousarray(G[mi]),
                         geno_u=np.ascontiguousarray(G[ui]), slct=slct))
    return p, rows2, src_off, store, wins, host


def test_every_launch_form_and_source_format_returns_the_same_bits(ctx, monkeypatch):
    """The same job under each switch that changes a launch form or a source format: the selection bit for bit that of the default
    (B11 has the same bits in every form and the kernel's sums have a fixed order).  It needs B11, z1 and the status only, so under
    GAUSS_FUSED_SOLVE=0 the job does take the stand-alone solver -- z / info within 1e-8 of the fused ones -- and the selection
    is still the same bits."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx)
    ref = _run(ctx, wins, want_mats=True)[0][0]
    assert all(r["status"] == 0 for r in ref)
    for k, r in enumerate(ref):                        # against the definition once, so that "the same bits" are the right ones
        _check(r, wins[k]["z1"], wins[k]["slct"], what=f"store window {k}")
    switches = [dict(GAUSS_CHAIN_ASIDE="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2"),
                dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2", GAUSS_EPI_EARLY="0"),
                dict(GAUSS_SHARE_MEASURED="0"), dict(GAUSS_SHARE_MEASURED="2"), dict(GAUSS_NO_SHIFT_CERT="1")]
    for sw in switches:
        with monkeypatch.context() as m:
            for k, v in sw.items():
                m.setenv(k, v)
            for r, w in zip(_run(ctx, wins)[0][0], ref):
                _same(r, w)
    with monkeypatch.context() as m:
        m.setenv("GAUSS_FUSED_SOLVE", "0")
        for r, w in zip(_run(ctx, wins)[0][0], ref):
            _same(r, w, KEYS)
            assert _err(r["z"], w["z"]) <= TOL and _err(r["info"], w["info"]) <= TOL
    try:                                               # int8 Gram
        ctx.set_gram_dtype("i8")
        for r, w in zip(_run(ctx, wins)[0][0], ref):
            _same(r, w)
    finally:
        ctx.set_gram_dtype(os.environ.get("GAUSS_GRAM_DTYPE", "f32"))
    for r, w in zip(_run(ctx, host, on_device=False)[0][0], ref):      # byte rows from host memory
        _same(r, w)
    # the blocking window call: streamed (default) and upload-then-run
    h2 = host[2]
    _same(hotpath.impute_window(1, h2["geno_m"], h2["geno_u"], p["off"], p["w"], h2["z1"], ctx=ctx, slct=h2["slct"]), ref[2])
    with monkeypatch.context() as m:
        m.setenv("GAUSS_STREAM_WINDOW", "0")
        _same(hotpath.impute_window(1, h2["geno_m"], h2["geno_u"], p["off"], p["w"], h2["z1"], ctx=ctx, slct=h2["slct"]), ref[2])
    with monkeypatch.context() as m:                   # read when a context is made: one queue
        m.setenv("GAUSS_SIDE_STREAM", "0")
        c = hotpath.Context(0)
        try:
            st2 = hotpath.RowStore(rows2, ctx=c)
            w2 = [dict(w, dev=(st2.ptr, st2.ptr) + w["dev"][2:]) for w in wins]
            for r, w in zip(_run(c, w2)[0][0], ref):
                _same(r, w)
            st2.close()
        finally:
            c.close()
    store.close()


def test_three_windows_of_which_two_ask_and_a_job_in_which_nobody_asks(ctx):
    """Windows of one job may mix: nobody's z / info moves by a bit when some windows ask, the asking windows return what they
    return in a job where everybody asks, two runs in flight return the same values, and the job's counters are those of the
    job in which nobody asks (the descriptor fields zero: the code path of a library without the feature)."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx, seed=43, spans=((0, 131), (97, 340), (211, 560)))
    nobody, c0 = _run(ctx, [dict(w, slct=None) for w in wins], runs=2)
    mixed, c1 = _run(ctx, [dict(w, slct=(w["slct"] if k != 1 else None)) for k, w in enumerate(wins)], runs=2)
    everybody, c2 = _run(ctx, wins, runs=2)
    assert c0 == c1 == c2, (c0, c1, c2)
    for run in mixed:
        for k, (r, w) in enumerate(zip(run, nobody[0])):
            _same(r, w, ("z", "info"))
            assert ("slct_zc" in r) == (k != 1)
            if k != 1:
                _same(r, everybody[0][k])
    for r, w in zip(everybody[1], nobody[1]):
        _same(r, w, ("z", "info"))
    store.close()


def test_refusals(ctx):
    """Only imputation windows may ask; bad forced lists and slct_max > 32 are refused; a window without unmeasured SNPs solves
    nothing and is refused as before."""
    p = small_panel(n_snp=120, scale=0.02, n_pops=5)
    gm, gu, z1 = split_window(p, 50)
    slct = dict(max=8, chi2_stop=4.0)
    base = dict(mode=0, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=None, z1=z1, slct=slct)
    with pytest.raises(Exception, match="imputation windows only"):
        hotpath.Job([dict(base, qcat=(10, 30, 0.01))], ctx=ctx)
    with pytest.raises(Exception, match="imputation windows only"):
        hotpath.Job([dict(base, ld_codings=1)], ctx=ctx)
    with pytest.raises(Exception, match="slct_max = 33"):
        hotpath.Job([dict(base, slct=dict(max=33, chi2_stop=4.0))], ctx=ctx)
    with pytest.raises(Exception, match=r"slct_forced\[1\] = 50"):
        hotpath.Job([dict(base, slct=dict(slct, forced=[3, 50]))], ctx=ctx)
    with pytest.raises(Exception, match="not a measured SNP"):
        hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, slct=dict(slct, forced=[-1]))
    with pytest.raises(Exception, match="distinct"):
        hotpath.Job([dict(base, slct=dict(slct, forced=[3, 9, 3]))], ctx=ctx)
    with pytest.raises(Exception, match="n_slct_forced"):
        hotpath.Job([dict(base, slct=dict(max=2, chi2_stop=4.0, forced=[3, 9, 4]))], ctx=ctx)
    with pytest.raises(Exception, match="no unmeasured SNPs"):
        hotpath.Job([dict(base, geno_u=gu[:0])], ctx=ctx)
    with pytest.raises(Exception, match="unmeasured SNPs"):
        hotpath.impute_window(0, gm, gu[:0], p["off"], None, z1, ctx=ctx, slct=slct)
    ok = hotpath.Job([dict(base, qcat=(10, 30, 0.01), slct=None), base], ctx=ctx)      # a QCAT window beside one that asks
    ok.run()
    res = ok.fetch()
    ok.close()
    assert "r" in res[0] and "slct_zc" in res[1]


# ---- the host entry points, files -> table -----------------------------------------------------------------------
POPS = [("AAA", 160, "EUR"), ("BBB", 145, "EUR"), ("CCC", 170, "ASN"), ("DDD", 133, "AFR"), ("EEE", 152, "EUR"), ("FFF", 90, "ASN")]
WGT = (["aaa", "CCC", "eee", "FFF", "zzz"], [0.45, 0.2, 0.25, 0.161, 0.3])
COLS = ["z", "wing", "order", "z_entry", "z_joint", "z_cond", "pval_cond", "var_left"]


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    d = tmp_path_factory.mktemp("slct_study")
    st = panel_mod.make_synthetic_study(str(d), POPS, n_snp=700, bp_lo=1_000_000, bp_hi=2_400_000, n_genes=40, frac_measured=0.3, seed=17)
    q = st["paths"]
    packed = os.path.join(os.path.dirname(q["data.gz"]), "panel.gpk")
    assert api.pack_panel(q["index.gz"], q["data.gz"], q["desc.txt"], packed) > 0
    return dict(files=(q["gwas.txt"], q["index.gz"], q["data.gz"], q["desc.txt"]), packed=packed)


def _feeder_window(mix, chr_, start_bp, end_bp, wing, who, files, cutoff):
    """The window as oracle/feeder_py.py's dist / distmix build it: measured SNPs (reference order), their matrix, populations."""
    from oracle import feeder_py as fp
    inp, index, data, desc = files
    pops = fp.read_ref_desc(desc)
    flags, w = fp.pop_flags_wgt(pops, *who) if mix else (fp.pop_flags(pops, who), None)
    lo, hi = start_bp - wing, end_bp + wing
    m = fp.read_input_z(inp, chr_, lo, hi, False)
    fp.read_reference_index(m, index, chr_, lo, hi, False)
    vec = fp.make_snp_vec(m, data, flags, cutoff, w)
    meas = [s for s in vec if s.type == 1]
    return meas, fp._matrix(meas), fp._selected_off(pops, flags), (None if w is None else np.asarray(w, dtype=np.float64))


@pytest.mark.parametrize("mix", [False, True])
def test_dist_slct_and_distmix_slct_end_to_end(ctx, study, mix, monkeypatch):
    """Text panel, packed panel (lean window on the resident rows) and the packed panel through the full SNP map: the same table,
    one row per measured SNP of the extended window in the reference's order -- the wings too -- with the values of the definition
    on the oracle's B11 of the oracle's data layer; conditioning SNPs by rsid; a bad one is named."""
    import oracle
    win = (22, 1_500_000, 2_000_000, 300_000)
    who = WGT if mix else "EUR"
    cutoff = 0.02 if mix else 0.01
    fn = api.distmix_slct if mix else api.dist_slct
    inp, idx, dat, desc = study["files"]
    afcol = "af1mix" if mix else "af1ref"
    meas, gm, off, w = _feeder_window(mix, *win, who, study["files"], cutoff)
    z1 = np.array([s.z for s in meas])
    B = window_b11(1 if mix else 0, gm, off, w)
    p_cut = 0.05
    stop = api.slct_chi2(p_cut)
    cond = [meas[4].rsid, meas[len(meas) - 2].rsid]                       # the second one sits in the right wing
    for forced, kmax in (((), None), ((4, len(meas) - 2), None), ((4, len(meas) - 2), 2)):
        df = fn(*win, who, inp, idx, dat, desc, af1_cutoff=cutoff, p_cutoff=p_cut, max_signals=kmax,
                cond_rsids=[cond[k] for k in range(len(forced))], ctx=ctx)
        assert list(df.columns) == ["rsid", "chr", "bp", "a1", "a2", afcol] + COLS
        assert list(df["rsid"]) == [s.rsid for s in meas] and list(df["bp"]) == [s.bp for s in meas]
        assert list(df["a1"]) == [s.a1 for s in meas] and list(df["a2"]) == [s.a2 for s in meas]
        assert np.array_equal(df["z"].to_numpy(), z1)
        assert np.array_equal(df[afcol].to_numpy(), np.array([(s.af1mix if mix else s.af1ref) for s in meas]))
        wing = np.array([0 if win[1] <= s.bp <= win[2] else 1 for s in meas])
        assert 0 < wing.sum() < len(meas) and np.array_equal(df["wing"].to_numpy(), wing)
        want = slct_by_definition(B, z1, kmax or 32, stop, min_var_frac(0.9, 0.1), forced)
        print(f"slct table mix={mix} forced={forced} K={kmax}: n {want['n']}  idx {want['idx'].tolist()}  margin {want['min_margin']:.3e}")
        assert want["min_margin"] > MARGIN and want["n"] >= len(forced)
        order = np.zeros(len(meas), dtype=int)
        order[want["idx"]] = np.arange(1, want["n"] + 1)
        assert np.array_equal(df["order"].to_numpy(), order)
        entry, joint = np.full(len(meas), np.nan), np.full(len(meas), np.nan)
        entry[want["idx"]], joint[want["idx"]] = want["zin"], want["joint"]
        e = dict(z_entry=_err(df["z_entry"].to_numpy(), entry), z_joint=_err(df["z_joint"].to_numpy(), joint),
                 z_cond=_err(df["z_cond"].to_numpy(), want["zc"]), var_left=_err(df["var_left"].to_numpy(), want["var"]))
        print("REACHED slct table: " + "  ".join(f"{k} {v:.3e}" for k, v in e.items()))
        assert max(e.values()) <= TOL, e
        pv = df["pval_cond"].to_numpy()
        ok = ~np.isnan(want["zc"])
        wp = np.array([2 * oracle.pnorm_upper(abs(t)) for t in want["zc"][ok]])
        assert np.array_equal(np.isnan(pv), ~ok) and np.max(np.abs(pv[ok] - wp) / wp) <= 1e-6
        if forced and kmax is None:
            assert want["n"] > 2 and wing[want["idx"]].any()              # a signal in a wing is conditioned on, and listed
    forms = [fn(*win, who, inp, "(unused)", study["packed"], desc, af1_cutoff=cutoff, p_cutoff=p_cut, max_signals=2, cond_rsids=cond, ctx=ctx)]
    monkeypatch.setenv("GAUSS_HOST_FULL_MAP", "1")
    forms.append(fn(*win, who, inp, "(unused)", study["packed"], desc, af1_cutoff=cutoff, p_cutoff=p_cut, max_signals=2, cond_rsids=cond, ctx=ctx))
    for other in forms:
        assert list(other.columns) == list(df.columns) and len(other) == len(df)
        for c in df.columns:
            if df[c].dtype.kind == "f":
                assert np.array_equal(df[c].to_numpy(), other[c].to_numpy(), equal_nan=True), c
            else:
                assert list(df[c]) == list(other[c]), c
    with pytest.raises(Exception, match="rs_not_there"):
        fn(*win, who, inp, idx, dat, desc, af1_cutoff=cutoff, cond_rsids=[cond[0], "rs_not_there"], ctx=ctx)
    with pytest.raises(Exception, match="listed twice"):
        fn(*win, who, inp, idx, dat, desc, af1_cutoff=cutoff, cond_rsids=[cond[0], cond[0]], ctx=ctx)
