"""GPU: further traits on one window's LD (n_traits_more / z_more / out_z_more of gauss_window_desc, k_traits.hip) against the oracle.

Bounds are those of tests/test_gpu_loo.py: |d| / max(1, |want|) <= 1e-8, and 1e-5 where MakePosDef repaired the matrix (the test
asserts want["mpd"] == 1 there and == 0 everywhere else).  A numpy statement of the kernels' algebra against the LU-inverse form
gave <= 3e-13 on the CPU (M up to 1 213, duplicated SNPs, lambda = 0.1): an error anywhere near the bound is a finding.
References: tests/traits_ref.py (one oracle run per trait; the closed form in LAPACK)."""
import os

import numpy as np
import pytest

import oracle
from gauss_amd import api, hotpath, synth
from gauss_amd import panel as panel_mod
from helpers import small_panel, split_window
from traits_ref import traits_by_oracle, traits_closed_form

pytestmark = pytest.mark.gpu

Z_TOL = 1e-8
CLAMP_TOL = 1e-5


def _zerr(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if np.size(got) else 0.0


def _check(got, want, tol, what=""):
    """got, want: [T, U].  Prints the figure before it asserts."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    e = _zerr(got, want)
    print(f"traits {what}: z {e:.3e}  (bound {tol:g})")
    assert e <= tol, (what, e)


def _same(a, b, keys=("z", "info", "z_more")):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _window(M, U, seed=None, scale=0.02):
    p = small_panel(n_snp=M + U + 60, scale=scale, seed=(11 + M) if seed is None else seed)
    assert p["G"].shape[0] >= M + U
    gm, gu, z1 = split_window(dict(G=p["G"][: M + U]), M)
    assert gm.shape[0] == M and gu.shape[0] == U
    return p, gm, gu, z1


def _traits(T, M, seed=1):
    return np.random.default_rng(seed).standard_normal((T, M)) * 2.0


# M around the 64-row blocks of L^-1, U on both sides of the product's 64-row strip, T on both sides of its 16-column tiles
CASES = [(2, 63, 1), (63, 65, 15), (64, 130, 16), (65, 63, 17), (129, 65, 63), (300, 130, 17), (129, 130, 1)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M,U,T", CASES)
def test_every_trait_matches_its_own_oracle_run(ctx, mode, M, U, T):
    """One oracle run per trait (pooled and weighted LD); z, info and the status are the bits of the same call without z_more."""
    p, gm, gu, z1 = _window(M, U)
    w = p["w"] if mode else None
    Z = _traits(T, M, seed=M + T)
    got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, z_more=Z)
    plain = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx)
    assert got["status"] == plain["status"] == 0 and "z_more" not in plain
    _same(got, plain, ("z", "info"))
    want = traits_by_oracle(mode, gm, gu, p["off"], w, Z)
    assert want["mpd"] == 0
    _check(got["z_more"], want["z"], Z_TOL, f"M={M} U={U} T={T} mode={mode} oracle")
    mats = oracle.run_impute(mode, gm, gu, p["off"], w, z1, want_mats=True)
    _check(got["z_more"], traits_closed_form(mats["b11"], mats["b21"], Z)["z"], Z_TOL, f"M={M} U={U} T={T} mode={mode} closed form")


@pytest.mark.parametrize("M,U,T", [(129, 130, 63), (65, 63, 17)])
def test_product_puts_every_result_in_its_own_row_and_column(ctx, M, U, T):
    """The f64 MFMA's C/D map: Z's rows are distinct unit vectors scaled by distinct integers, so B^-1 Z^T is a selection of scaled
    columns of B^-1 and out_z_more sqrt(info) = b21 (B^-1 Z^T) has no two equal rows or columns -- a permuted result cannot pass."""
    p, gm, gu, z1 = _window(M, U)
    rng = np.random.default_rng(5)
    at = rng.choice(M, size=T, replace=False)
    Z = np.zeros((T, M))
    Z[np.arange(T), at] = np.arange(T) + 2.0
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, z_more=Z)
    mats = oracle.run_impute(0, gm, gu, p["off"], None, z1, want_mats=True)
    assert got["status"] == 0 and mats["mpd"] == 0
    want = mats["b21"] @ (np.linalg.inv(mats["b11"]) @ Z.T)                   # [U, T]
    raw = (got["z_more"] * np.sqrt(got["info"])[None, :]).T
    _check(raw, want, Z_TOL, f"M={M} U={U} T={T} raw product")
    assert len({tuple(np.round(r, 9)) for r in want}) == U and len({tuple(np.round(c, 9)) for c in want.T}) == T


def test_a_further_trait_equal_to_z1_agrees_with_z(ctx):
    p, gm, gu, z1 = _window(129, 65)
    Z = np.vstack([z1, _traits(3, 129)])
    for mode, w in ((0, None), (1, p["w"])):
        got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, z_more=Z)
        e = _zerr(got["z_more"][0], got["z"])
        print(f"traits z_more[0] = z1, mode {mode}: {e:.3e}")
        assert got["status"] == 0 and e <= Z_TOL


def test_a_trait_depends_on_its_own_scores_only(ctx):
    """Trait t alone (T = 1) and as any one of 63 gives the same bits; a NaN planted in one trait leaves every other trait's bits."""
    p, gm, gu, z1 = _window(129, 130)
    Z = _traits(63, 129, seed=9)
    full = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, z_more=Z)
    assert full["status"] == 0 and np.all(np.isfinite(full["z_more"]))
    for t in (0, 15, 16, 31, 47, 48, 62):
        alone = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, z_more=Z[t:t + 1])
        assert np.array_equal(alone["z_more"][0], full["z_more"][t]), t
        _same(alone, full, ("z", "info"))
    some = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, z_more=Z[[40, 3, 62, 17, 5]])      # another T, other places
    assert np.array_equal(some["z_more"], full["z_more"][[40, 3, 62, 17, 5]])
    for t, g in ((0, 0), (17, 128), (62, 64)):
        Zn = Z.copy()
        Zn[t, g] = np.nan if t != 17 else np.inf
        bad = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, z_more=Zn)
        keep = np.arange(63) != t
        assert bad["status"] == 0 and not np.any(np.isfinite(bad["z_more"][t]))
        assert np.array_equal(bad["z_more"][keep], full["z_more"][keep])
        _same(bad, full, ("z", "info"))


def _run(ctx, wins, on_device=True, runs=1):
    job = hotpath.Job(wins, ctx=ctx, on_device=on_device)
    for _ in range(runs):
        job.run()
    out = [job.fetch() for _ in range(runs)]
    job.close()
    return out


@pytest.mark.parametrize("mode,M0,dup", [(0, 30, [0, 1, 2]), (0, 150, [3, 70, 131, 140, 149]), (1, 150, [3, 70, 131, 140, 149])])
def test_clamped_window_uses_the_repaired_matrix(ctx, mode, M0, dup):
    """Duplicated measured SNPs at lambda = 0 (M = 33: one factor block; M = 155: three): MakePosDef rebuilds B11, the rows of L^-1
    of the REPAIRED matrix ride in the window's own re-factorisation, and the traits are those of the closed form on the oracle's
    repaired B11 -- alone and inside a job whose other windows need no repair (their bits do not move)."""
    p = small_panel(n_snp=M0 + 110, scale=0.02, seed=23 if M0 > 100 else 21)
    gm, gu, z1 = split_window(dict(G=p["G"][: M0 + 80]), M0)
    gm = np.ascontiguousarray(np.vstack([gm, gm[dup]]))
    z1 = np.concatenate([z1, z1[dup] - 0.2])
    M = gm.shape[0]
    w = p["w"] if mode else None
    Z = _traits(17, M, seed=3)
    got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, lam=0.0, ctx=ctx, z_more=Z)
    plain = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, lam=0.0, ctx=ctx)
    want = oracle.run_impute(mode, gm, gu, p["off"], w, z1, lam=0.0, want_mats=True)
    assert want["mpd"] == 1 and got["status"] & 1 and got["status"] == plain["status"]
    _same(got, plain, ("z", "info"))
    _check(got["z_more"], traits_closed_form(want["b11"], want["b21"], Z)["z"], CLAMP_TOL, f"clamped window, M = {M}, mode {mode}")
    by_oracle = traits_by_oracle(mode, gm, gu, p["off"], w, Z[:3], lam=0.0)
    assert by_oracle["mpd"] == 3
    _check(got["z_more"][:3], by_oracle["z"], CLAMP_TOL, f"clamped window, M = {M}, mode {mode}, oracle")
    ok = dict(mode=mode, geno_m=gm[:M0], geno_u=gu, pop_off=p["off"], pop_wgt=w, z1=z1[:M0], z_more=Z[:5, :M0])
    bad = dict(mode=mode, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=w, z1=z1, lam=0.0, z_more=Z)
    alone = _run(ctx, [ok], on_device=False)[0][0]
    assert alone["status"] == 0
    _check(alone["z_more"], traits_by_oracle(mode, gm[:M0], gu, p["off"], w, Z[:5, :M0])["z"], Z_TOL, f"its unrepaired neighbour, M = {M0}")
    for run in _run(ctx, [ok, bad, ok], on_device=False, runs=2):
        assert run[0]["status"] == 0 and run[1]["status"] & 1
        _same(run[0], alone)
        _same(run[2], alone)
        _same(run[1], got)


def test_nonfinite_window_is_all_nan(ctx):
    p = small_panel(n_snp=60, scale=0.01, n_pops=4)
    gm, gu, z1 = split_window(p, 25)
    gm = gm.copy()
    gm[3, :] = 1                                   # zero variance: CalCor returns 0 / 0
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, z_more=_traits(5, 25))
    assert got["status"] & 2
    assert got["z_more"].shape == (5, gu.shape[0]) and np.all(np.isnan(got["z_more"])) and np.all(np.isnan(got["z"]))


def _store_windows(ctx, seed=41, n_snp=2000, spans=((0, 131), (97, 340), (211, 560), (330, None), (400, 540)), T=(7, 0, 63, 16, 1)):
    """Windows over one resident 2-bit store, overlapping like a chromosome's (shared measured rows apply); window k carries T[k]
    further traits (0: it does not ask)."""
    p = small_panel(n_snp=n_snp, scale=0.05, seed=seed)
    G = p["G"]
    rows2, src_off = panel_mod.pack2bit(G, p["off"])
    store = hotpath.RowStore(rows2, ctx=ctx)
    rng = np.random.default_rng(5)
    n = G.shape[0]
    measured = np.sort(rng.choice(n, size=n // 3, replace=False))
    unmeasured = np.setdiff1d(np.arange(n), measured)
    z = rng.standard_normal(n)
    wins, host = [], []
    for k, (a, b) in enumerate(spans):
        mi = measured[a:b]
        lo, hi = mi[len(mi) // 4], mi[3 * len(mi) // 4]
        ui = unmeasured[(unmeasured > lo) & (unmeasured < hi)]
        more = dict(z_more=rng.standard_normal((T[k], len(mi))) * 2.0) if T[k] else {}
        wins.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=z[mi], dev=(store.ptr, store.ptr, len(mi), len(ui), store.ld),
                         packed=dict(fmt=1, rows_m=mi.astype(np.int32), rows_u=ui.astype(np.int32), pop_src_off=src_off), **more))
        host.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=z[mi], geno_m=np.ascontiguousarray(G[mi]),
                         geno_u=np.ascontiguousarray(G[ui]), **more))
    return p, rows2, src_off, store, wins, host


def _same_win(a, b):
    assert a["status"] == b["status"] and ("z_more" in a) == ("z_more" in b)
    _same(a, b, ("z", "info") + (("z_more",) if "z_more" in a else ()))


def test_every_launch_form_and_source_format_returns_the_same_bits(ctx, monkeypatch):
    """One job of overlapping windows, asking (T = 7, 63, 16, 1) and not asking mixed, two runs in flight, under each switch that
    changes a launch form or a source format: the further traits, z and info bit for bit those of the default.
    GAUSS_FUSED_SOLVE=0: a job with an asking window keeps the fused chain (the traits need the rows of L^-1)."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx)
    wins[4] = dict(wins[4], lam=1e-7)              # no certificate: the shifted matrix is factored too
    host[4] = dict(host[4], lam=1e-7)
    both = _run(ctx, wins, runs=2)
    ref = both[0]
    assert all(r["status"] == 0 for r in ref[:4]) and "z_more" not in ref[1]
    for r, w in zip(both[1], ref):
        _same_win(r, w)
    # against the oracle once, so that "the same bits" are the right ones
    want = traits_by_oracle(1, host[0]["geno_m"], host[0]["geno_u"], p["off"], p["w"], host[0]["z_more"])
    assert want["mpd"] == 0
    _check(ref[0]["z_more"], want["z"], Z_TOL, "store window 0")
    # nobody's z / info moves by a bit when some windows ask
    for r, w in zip(_run(ctx, [{k: v for k, v in w.items() if k != "z_more"} for w in wins])[0], ref):
        _same(r, w, ("z", "info"))
        assert r["status"] == w["status"] and "z_more" not in r
    switches = [dict(GAUSS_CHAIN_ASIDE="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2"),
                dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2", GAUSS_EPI_EARLY="0"),
                dict(GAUSS_SHARE_MEASURED="0"), dict(GAUSS_SHARE_MEASURED="2"), dict(GAUSS_NO_SHIFT_CERT="1"), dict(GAUSS_FUSED_SOLVE="0")]
    for sw in switches:
        with monkeypatch.context() as m:
            for k, v in sw.items():
                m.setenv(k, v)
            for run in _run(ctx, wins, runs=2):
                for r, w in zip(run, ref):
                    _same_win(r, w)
    # int8 Gram
    try:
        ctx.set_gram_dtype("i8")
        for r, w in zip(_run(ctx, wins)[0], ref):
            _same_win(r, w)
    finally:
        ctx.set_gram_dtype(os.environ.get("GAUSS_GRAM_DTYPE", "f32"))
    # byte rows from host memory instead of 2-bit rows of the resident store
    for run in _run(ctx, host, on_device=False, runs=2):
        for r, w in zip(run, ref):
            _same_win(r, w)
    # the blocking window call: streamed (default) and upload-then-run
    h = host[2]
    _same_win(hotpath.impute_window(1, h["geno_m"], h["geno_u"], p["off"], p["w"], h["z1"], ctx=ctx, z_more=h["z_more"]), ref[2])
    with monkeypatch.context() as m:
        m.setenv("GAUSS_STREAM_WINDOW", "0")
        _same_win(hotpath.impute_window(1, h["geno_m"], h["geno_u"], p["off"], p["w"], h["z1"], ctx=ctx, z_more=h["z_more"]), ref[2])
    # switches read when a context is made: one queue; one A row per lane in the f32 Gram kernel
    for sw in (dict(GAUSS_SIDE_STREAM="0"), dict(GAUSS_GRAM_PACKED="0")):
        with monkeypatch.context() as m:
            for k, v in sw.items():
                m.setenv(k, v)
            c = hotpath.Context(0)
            try:
                st2 = hotpath.RowStore(rows2, ctx=c)
                w2 = [dict(w, dev=(st2.ptr, st2.ptr) + w["dev"][2:]) for w in wins]
                for r, w in zip(_run(c, w2)[0], ref):
                    _same_win(r, w)
                st2.close()
            finally:
                c.close()
    store.close()


def test_give_up_rerun_inside_the_fetch_returns_the_same_values(ctx, monkeypatch):
    """A merged Gram launch whose chain queue gives up waiting (the library's test hook: a wait for a count that never comes,
    bounded at 2 ms) is queued again in the two-launch form inside gauss_job_fetch: the further traits come back with that
    re-run, bit for bit those of an undisturbed run, also with two such runs in flight."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx, seed=47)
    monkeypatch.setenv("GAUSS_CHAIN_ASIDE", "2")
    monkeypatch.setenv("GAUSS_CHAIN_MERGED", "2")
    ref = _run(ctx, wins)[0]
    job = hotpath.Job(wins, ctx=ctx, on_device=True)
    c0 = ctx.counters()
    monkeypatch.setenv("GAUSS_WAIT_COUNT_TIMEOUT_US", "-2000")
    job.run()
    a = job.fetch()
    job.run()
    job.run()
    b, c = job.fetch(), job.fetch()
    c1 = ctx.counters()
    monkeypatch.delenv("GAUSS_WAIT_COUNT_TIMEOUT_US")
    job.run()
    d = job.fetch()
    job.close()
    assert c1["giveups"] == c0["giveups"] + 3 and c1["rerun_failed"] == c0["rerun_failed"], (c0, c1)
    for res in (a, b, c, d):
        for r, w in zip(res, ref):
            assert r["status"] == w["status"] == 0
            _same_win(r, w)
    store.close()


def test_with_leave_one_out_and_selection_in_the_same_window(ctx):
    """Leave-one-out values and the signal selection stay statistics of z1: asked for beside further traits, their bits are those
    of the window without z_more, and the traits' bits those of the window that asks for nothing else."""
    p, gm, gu, z1 = _window(129, 65)
    Z = _traits(17, 129)
    slct = dict(max=4, chi2_stop=1.0)
    for mode, w in ((0, None), (1, p["w"])):
        every = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, loo=True, slct=slct, z_more=Z)
        stats = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, loo=True, slct=slct)
        only = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, z_more=Z)
        assert every["status"] == stats["status"] == only["status"] == 0 and every["slct_n"] == stats["slct_n"] > 0
        _same(every, stats, ("z", "info", "loo_z", "loo_info", "loo_t", "slct_idx", "slct_zin", "slct_joint", "slct_zc", "slct_var"))
        _same(every, only)


_RIDER_KEYS = ("z", "info", "loo_z", "loo_info", "loo_t", "z_more", "slct_idx", "slct_zin", "slct_joint", "slct_zc", "slct_var")
_LOO_KEYS = ("loo_z", "loo_info", "loo_t")
_SLCT_KEYS = ("slct_idx", "slct_zin", "slct_joint", "slct_zc", "slct_var")


def _same_riders(a, b, what):
    """Every output two results of the same window with the same asks carry, bit for bit (the unused tails of idx / zin / joint too)."""
    assert a["status"] == b["status"] and sorted(a) == sorted(b), (what, a["status"], b["status"], sorted(a), sorted(b))
    for k in _RIDER_KEYS:
        if k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    if "slct_n" in a:
        assert a["slct_n"] == b["slct_n"], what
        for k in ("idx", "zin", "joint"):
            assert np.array_equal(a["slct_raw"][k], b["slct_raw"][k], equal_nan=True), (what, "raw " + k)


def test_all_three_riders_share_one_result_block(ctx):
    """Leave-one-out, selection and further traits together where the result block's layout is used most intricately.
    (a) One job of four windows on shared store rows, two runs in flight, asking all three / the selection / nothing / loo + traits
    (T = 17, K = 4): a window's place in the block depends on the sections of the windows in front of it, and every output of
    every window is bit for bit that of the window run alone with the same asks.
    (b) The smallest clamped window of test_clamped_window_uses_the_repaired_matrix asking all three: each rider's outputs are the bits
    of the same clamped window asking for that rider alone: the riders read disjoint inputs, so the results are bit-equal.
    (c) The non-finite window of test_nonfinite_window_is_all_nan asking all three: status bit 2, every double NaN, nothing selected."""
    T, slct = 17, dict(max=4, chi2_stop=1.0)
    # (a)
    p, rows2, src_off, store, wins, host = _store_windows(ctx, spans=((0, 131), (97, 340), (211, 560), (330, None)), T=(T, 0, 0, T))
    wins = [dict(wins[0], loo=True, slct=slct), dict(wins[1], slct=slct), wins[2], dict(wins[3], loo=True)]
    alone = [_run(ctx, [w])[0][0] for w in wins]
    assert all(r["status"] == 0 for r in alone) and alone[0]["slct_n"] > 0 and alone[1]["slct_n"] > 0
    assert {"loo_z", "z_more", "slct_zc"} <= set(alone[0]) and "loo_z" not in alone[1] and "z_more" not in alone[1]
    assert not {"loo_z", "z_more", "slct_zc"} & set(alone[2]) and {"loo_z", "z_more"} <= set(alone[3]) and "slct_zc" not in alone[3]
    for r, run in enumerate(_run(ctx, wins, runs=2)):
        for k, (got, want) in enumerate(zip(run, alone)):
            _same_riders(got, want, f"store window {k}, run {r}")
    store.close()
    # (b)
    mode, M0, dup = 0, 30, [0, 1, 2]
    q = small_panel(n_snp=M0 + 110, scale=0.02, seed=21)
    gm, gu, z1 = split_window(dict(G=q["G"][: M0 + 80]), M0)
    gm = np.ascontiguousarray(np.vstack([gm, gm[dup]]))
    z1 = np.concatenate([z1, z1[dup] - 0.2])
    Z = _traits(T, gm.shape[0], seed=3)
    call = lambda **asks: hotpath.impute_window(mode, gm, gu, q["off"], None, z1, lam=0.0, ctx=ctx, **asks)
    every = call(loo=True, slct=slct, z_more=Z)
    assert every["status"] & 1 and every["slct_n"] > 0
    for keys, one in ((_LOO_KEYS, call(loo=True)), (_SLCT_KEYS, call(slct=slct)), (("z_more",), call(z_more=Z))):
        assert one["status"] == every["status"]
        for k in ("z", "info") + keys:
            assert np.array_equal(every[k], one[k], equal_nan=True), k
        if keys is _SLCT_KEYS:
            assert one["slct_n"] == every["slct_n"]
    # (c)
    q = small_panel(n_snp=60, scale=0.01, n_pops=4)
    gm, gu, z1 = split_window(q, 25)
    gm = gm.copy()
    gm[3, :] = 1                                   # zero variance: CalCor returns 0 / 0
    got = hotpath.impute_window(0, gm, gu, q["off"], None, z1, ctx=ctx, loo=True, slct=slct, z_more=_traits(T, 25))
    assert got["status"] & 2
    assert got["z"].shape == got["info"].shape == (gu.shape[0],) and got["z_more"].shape == (T, gu.shape[0])
    assert got["slct_zc"].shape == got["slct_var"].shape == got["loo_z"].shape == got["loo_info"].shape == got["loo_t"].shape == (25,)
    for k in ("z", "info", "loo_z", "loo_info", "loo_t", "z_more", "slct_zc", "slct_var"):
        assert np.all(np.isnan(got[k])), k
    raw = got["slct_raw"]
    assert raw["zin"].shape == raw["joint"].shape == raw["idx"].shape == (4,)
    assert np.all(np.isnan(raw["zin"])) and np.all(np.isnan(raw["joint"]))
    assert got["slct_n"] == 0 and np.all(raw["idx"] == -1)


def _rand_geno(rng, n, N):
    f = rng.uniform(0.05, 0.95, size=(n, 1))
    return ((rng.random((n, N)) < f).astype(np.uint8) + (rng.random((n, N)) < f).astype(np.uint8))


def test_full_size_window(ctx):
    """The shape of the largest chr22 window at reduced N: M = 1 213 = 19 factor blocks, U = 2 500, T = 63, against the closed form on
    the oracle's B11 / B21, and three traits against their own oracle runs."""
    rng = np.random.default_rng(99)
    N, M, U, T = 1500, 1213, 2500, 63
    off = np.array([0, N], dtype=np.int32)
    base = _rand_geno(rng, 220, N)
    G = base[rng.integers(0, 220, size=M + U)].copy()
    noise = rng.random(G.shape) < 0.4
    G[noise] = _rand_geno(rng, 1, N)[0][np.nonzero(noise)[1]]
    gm, gu = np.ascontiguousarray(G[:M]), np.ascontiguousarray(G[M:])
    z1 = rng.standard_normal(M) * 2
    Z = rng.standard_normal((T, M)) * 2
    got = hotpath.impute_window(0, gm, gu, off, None, z1, want_mats=True, ctx=ctx, z_more=Z)
    assert got["status"] == 0
    _check(got["z_more"], traits_closed_form(got["b11"], got["b21"], Z)["z"], Z_TOL, "full size, closed form on out_b11 / out_b21")
    from oracle import oracle_np
    want = traits_by_oracle(0, gm, gu, off, None, Z[[0, 31, 62]], run_impute=oracle_np.run_impute)
    assert want["mpd"] == 0
    _check(got["z_more"][[0, 31, 62]], want["z"], Z_TOL, "full size, three oracle runs")


def test_refusals(ctx):
    """Only imputation windows may ask, for at most 63 traits, with both arrays; a window without unmeasured SNPs is refused as before."""
    p = small_panel(n_snp=120, scale=0.02, n_pops=5)
    gm, gu, z1 = split_window(p, 50)
    Z = _traits(3, 50)
    base = dict(mode=0, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=None, z1=z1, z_more=Z)
    with pytest.raises(Exception, match="imputation windows only"):
        hotpath.Job([dict(base, qcat=(10, 30, 0.01))], ctx=ctx)
    with pytest.raises(Exception, match="imputation windows only"):
        hotpath.Job([dict(base, ld_codings=1)], ctx=ctx)
    with pytest.raises(Exception, match="0 .. 63 further traits"):
        hotpath.Job([dict(base, z_more=_traits(64, 50))], ctx=ctx)
    with pytest.raises(Exception, match="no unmeasured SNPs"):
        hotpath.Job([dict(base, geno_u=gu[:0])], ctx=ctx)
    with pytest.raises(Exception, match="unmeasured SNPs"):
        hotpath.impute_window(0, gm, gu[:0], p["off"], None, z1, ctx=ctx, z_more=Z)
    # the descriptor itself: a negative count, and a count without its arrays
    for field, value, msg in (("n_traits_more", -1, "0 .. 63 further traits"), ("z_more", None, "z_more is NULL"), ("out_z_more", None, "out_z_more is NULL")):
        desc = hotpath.WindowDesc()
        win = hotpath._Win(desc, dict(mode=0, geno_m=gm, geno_u=gu, pop_off=p["off"], z1=z1, lam=0.1, z_more=Z))
        setattr(desc, field, value)
        with pytest.raises(Exception, match=msg):
            hotpath.check(ctx.lib.gauss_impute_window(ctx.handle, hotpath.C.byref(desc)))
        del win
    ok = hotpath.Job([dict(base, qcat=(10, 30, 0.01), z_more=None), base, dict(base, z_more=None)], ctx=ctx)      # a QCAT window and a plain one beside one that asks
    ok.run()
    res = ok.fetch()
    ok.close()
    assert "r" in res[0] and res[1]["z_more"].shape == (3, gu.shape[0]) and "z_more" not in res[2]


# ---- the host entry points, files -> table -----------------------------------------------------------------------
POPS = [("AAA", 160, "EUR"), ("BBB", 145, "EUR"), ("CCC", 170, "ASN"), ("DDD", 133, "AFR"), ("EEE", 152, "EUR"), ("FFF", 90, "ASN")]
WGT = (["aaa", "CCC", "eee", "FFF", "zzz"], [0.45, 0.2, 0.25, 0.161, 0.3])
WIN = (22, 1_500_000, 2_000_000, 300_000)


def _write(path, rows):
    with open(path, "w") as f:
        f.write("rsid chr bp a1 a2 z\n")
        for r in rows:
            f.write(f"{r[0]} {r[1]} {r[2]} {r[3]} {r[4]} {float(r[5])!r}\n")
    return str(path)


@pytest.fixture(scope="module")
def study(tmp_path_factory, ctx):
    """Trait 1 is the synthetic study's own file.  Trait 2: other Z-scores, 10 % of its rows allele-swapped, rows for SNPs trait 1
    lacks (panel SNPs it does not measure, and positions the panel does not have), one key listed twice, rows shuffled.  Trait 3: other
    Z-scores, file order reversed.  `alone` holds, for traits 2 and 3, the file that is passed alone as input_file: the same rows
    without those of the SNPs trait 1 lacks (the swaps and the duplicate stay)."""
    d = tmp_path_factory.mktemp("traits_study")
    st = panel_mod.make_synthetic_study(str(d), POPS, n_snp=700, bp_lo=1_000_000, bp_hi=2_400_000, n_genes=40, frac_measured=0.3, seed=17)
    q = st["paths"]
    packed = os.path.join(os.path.dirname(q["data.gz"]), "panel.gpk")
    assert api.pack_panel(q["index.gz"], q["data.gz"], q["desc.txt"], packed) > 0
    rows = [l.split() for l in open(q["gwas.txt"]).read().splitlines()[1:]]
    rng = np.random.default_rng(3)
    plain = api.dist(*WIN, "EUR", q["gwas.txt"], q["index.gz"], q["data.gz"], q["desc.txt"], af1_cutoff=0.01, ctx=ctx)
    un = plain[plain["type"] == 0].iloc[:5]
    extra = [(r.rsid, r.chr, r.bp, r.a1, r.a2, 3.0 + k) for k, r in enumerate(un.itertuples())]       # panel SNPs trait 1 does not measure
    extra += [(f"rsx{k}", 22, int(rows[7 * k][2]) + 1, "A", "C", -2.0) for k in range(1, 6)]            # positions off the panel
    z2, z3 = rng.standard_normal(len(rows)) * 2.0, rng.standard_normal(len(rows)) * 2.0
    swap = rng.random(len(rows)) < 0.1
    t2 = [(r[0], r[1], r[2], r[4], r[3], z) if s else (r[0], r[1], r[2], r[3], r[4], z) for r, z, s in zip(rows, z2, swap)]
    inside = sorted((k for k, r in enumerate(rows) if WIN[1] <= int(r[2]) <= WIN[2]), key=lambda k: int(rows[k][2]))      # by position: the window's order
    twice = inside[len(inside) // 2]
    t2 = [t2[k] for k in rng.permutation(len(t2))]
    t2.insert(0, t2[[r[0] for r in t2].index(rows[twice][0])][:5] + (11.0,))         # the earlier row of a key listed twice: it loses
    t3 = [tuple(r[:5]) + (z,) for r, z in zip(rows, z3)][::-1]
    f2 = _write(d / "trait2.txt", t2[:50] + extra[:5] + t2[50:] + extra[5:])
    f2_alone = _write(d / "trait2_alone.txt", t2)
    f3 = _write(d / "trait3.txt", t3)
    lacking = [r for r in t3 if r[0] not in (rows[inside[0]][0], rows[inside[-1]][0])]
    return dict(files=(q["gwas.txt"], q["index.gz"], q["data.gz"], q["desc.txt"]), packed=packed, more=[f2, f3], alone=[f2_alone, f3],
                lacking=_write(d / "trait3_lacking.txt", lacking), n_swapped=int(swap.sum()), removed=(rows[inside[0]][0], rows[inside[-1]][0]))


@pytest.mark.parametrize("mix", [False, True])
def test_dist_traits_and_distmix_traits_end_to_end(ctx, study, mix, monkeypatch):
    """Three trait files on a text panel, a packed panel (lean window on the resident rows) and the packed panel through the full
    SNP map: trait 1's columns are the plain call's bits, and each further trait's columns are what the plain call returns when
    that trait's file, given the same SNP set, is passed alone."""
    who = WGT if mix else "EUR"
    cutoff = 0.02 if mix else 0.01
    fn, plain_fn = (api.distmix_traits, api.distmix) if mix else (api.dist_traits, api.dist)
    inp, idx, dat, desc = study["files"]
    assert study["n_swapped"] > 10
    df = fn(*WIN, who, [inp] + study["more"], idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
    one = plain_fn(*WIN, who, inp, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
    assert list(df.columns) == list(one.columns) + ["z_2", "pval_2", "z_3", "pval_3"] and len(df) == len(one)
    assert 0 < int((one["type"] == 1).sum()) < len(one)
    for c in one.columns:
        if one[c].dtype.kind == "f":
            assert np.array_equal(df[c].to_numpy(), one[c].to_numpy(), equal_nan=True), c
        else:
            assert list(df[c]) == list(one[c]), c
    for k, alone_file in zip((2, 3), study["alone"]):
        alone = plain_fn(*WIN, who, alone_file, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
        assert list(alone["rsid"]) == list(df["rsid"]) and list(alone["type"]) == list(df["type"])
        ez = _zerr(df[f"z_{k}"].to_numpy(), alone["z"].to_numpy())
        ep = float(np.max(np.abs(df[f"pval_{k}"].to_numpy() - alone["pval"].to_numpy()) / alone["pval"].to_numpy()))
        ei = float(np.max(np.abs(df["info"].to_numpy() - alone["info"].to_numpy())))
        print(f"{'distmix' if mix else 'dist'}_traits, trait {k}: z {ez:.3e}  pval rel {ep:.3e}  info {ei:.3e}")
        assert ez <= Z_TOL and ep <= 1e-6 and ei == 0.0
        meas = (df["type"] == 1).to_numpy()
        assert np.array_equal(df[f"z_{k}"].to_numpy()[meas], alone["z"].to_numpy()[meas])       # a measured SNP's own oriented study z
    assert list(fn(*WIN, who, [inp], idx, dat, desc, af1_cutoff=cutoff, ctx=ctx).columns) == list(one.columns)
    gone = [r for r in one["rsid"][one["type"] == 1] if r in study["removed"]]      # in the window's order; the AF filter may have dropped one
    assert gone
    with pytest.raises(Exception, match=f"trait3_lacking.txt lacks {len(gone)} of .* the first is {gone[0]}:"):
        fn(*WIN, who, [inp, study["lacking"]], idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
    with pytest.raises(Exception, match="at most 63"):
        fn(*WIN, who, [inp] + [study["more"][1]] * 64, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
    forms = [fn(*WIN, who, [inp] + study["more"], "(unused)", study["packed"], desc, af1_cutoff=cutoff, ctx=ctx)]
    monkeypatch.setenv("GAUSS_HOST_FULL_MAP", "1")
    forms.append(fn(*WIN, who, [inp] + study["more"], "(unused)", study["packed"], desc, af1_cutoff=cutoff, ctx=ctx))
    for other in forms:
        assert list(other.columns) == list(df.columns) and len(other) == len(df)
        for c in df.columns:
            if df[c].dtype.kind == "f":
                assert np.array_equal(df[c].to_numpy(), other[c].to_numpy(), equal_nan=True), c
            else:
                assert list(df[c]) == list(other[c]), c
