"""GPU: every trait of a window in one multi-causal fit (k_susie.hip's trait dimension) and the colocalisation of their signals
(k_coloc.hip) against the definition (tests/coloc_ref.py) evaluated on the B11 / B21 the GPU returns.  Per trait the values are held to
susie_ref.value_tol and sizes, sets, kept flags and sweeps are exact; PP and hit_pp of a pair are held to the sum of its two traits'
bounds (lH4 adds one lbf of each fit, and the softmax does not amplify), hit and n are exact.  No decision of a case may be
borderline.  Every case prints a REACHED line."""
import os

import numpy as np
import pytest

import coloc_ref as cr
import cs_ref
import susie_ref as sr
from gauss_amd import api, hotpath
from gauss_amd import panel as panel_mod
from helpers import small_panel, split_window

pytestmark = pytest.mark.gpu

ST_CLAMPED, ST_NONFINITE, ST_NOCONV, ST_NOFIT = 1, 2, 16, 32
VALUE = ("alpha", "mu", "pip", "set_pip", "mass", "lse", "V", "purity")
ONE = ("pip", "set", "set_pip", "V", "lse", "mass", "purity", "size", "kept", "sweeps", "delta", "alpha", "mu", "lbf")
SUSIE_KEYS = tuple("susie_" + k for k in ONE)
MORE_KEYS = tuple("susie_more_" + k for k in ONE + ("status",))
COLOC_KEYS = ("coloc_pp", "coloc_hit", "coloc_hit_pp", "coloc_n")


def _same(a, b, keys, own_bits=0):
    assert a["status"] & ~own_bits == b["status"] & ~own_bits
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _ask(kw, k, coloc=True):
    d = dict(kw, want_alpha=True, want_lbf=True, traits=k)
    if coloc:
        d["coloc"] = {}
    return d


def _trait(got, t):
    """Trait t of a result under the names of trait 0"""
    if t == 0:
        return {k: got["susie_" + k] for k in ONE}, got["status"]
    return {k: got["susie_more_" + k][t - 1] for k in ONE}, int(got["susie_more_status"][t - 1])


def _check(got, z1, z_more, k, kw, what, **priors):
    """got: a window's result with b11, b21, alpha, mu and lbf.  The reference on the GPU's matrices, vetted again there."""
    fits, tols = [], []
    for t in range(k + 1):
        z = z1 if t == 0 else z_more[t - 1]
        tb, want = sr.fit_textbook(got["b11"], got["b21"], z, **kw), sr.fit_w(got["b11"], got["b21"], z, **kw)
        e_ref = sr.gap(tb, want)
        tol = sr.value_tol(want, e_ref)
        fits.append(want)
        tols.append(tol)
        g, st = _trait(got, t)
        e = {}
        for key in VALUE:
            p, q = np.asarray(g[key], dtype=np.float64), np.asarray(want[key], dtype=np.float64)
            assert p.shape == q.shape and np.array_equal(np.isnan(p), np.isnan(q)), (what, t, key)
            e[key] = float(np.nanmax(np.abs(p - q), initial=0.0))
        # the Bayes factors themselves: -inf at the same candidates; a factor moves by half of what value_tol grants a pip, and is held to it
        fin = np.isfinite(want["lbf"])
        assert np.array_equal(np.isfinite(g["lbf"]), fin) and np.all(g["lbf"][~fin] == -np.inf), (what, t)
        e["lbf"] = float(np.max(np.abs(g["lbf"][fin] - want["lbf"][fin]), initial=0.0))
        print(f"REACHED coloc {what} trait {t}: T {len(want['pip'])}  L {len(want['V'])}  sweeps {want['sweeps']}  kept {int(want['kept'].sum())}  "
              f"e_ref {e_ref:.2e}  " + "  ".join(f"{key} {v:.2e}" for key, v in e.items()) + f"  (bound {tol:.2e})")
        assert max(e.values()) <= tol, (what, t, e, tol)
        assert np.array_equal(g["size"], want["size"]) and np.array_equal(g["set"], want["set"]), (what, t)
        assert np.array_equal(g["kept"] != 0, want["kept"]) and g["sweeps"] == want["sweeps"], (what, t, g["sweeps"], want["sweeps"])
        assert abs(g["delta"] - want["delta"]) <= tol
        assert bool(st & ST_NOCONV) == (not want["delta"] < sr.args_of(**kw)["tol"]), (what, t, st)
    bl = cr.borderline(fits, kw, tols)
    assert bl == [], (what, bl)
    if "coloc_pp" in got:
        want = cr.pairs(fits, **priors)
        assert np.array_equal(got["coloc_hit"], want["hit"]) and np.array_equal(got["coloc_n"], want["n"]), what
        gaps = []
        for q, (a, b) in enumerate(cr.pair_list(k)):
            bound = cr.pair_tol(fits, tols, a, b)
            for key in ("pp", "hit_pp"):
                x, y = got["coloc_" + key][q], want[key][q]
                assert np.array_equal(np.isnan(x), np.isnan(y)), (what, a, b, key)
                gap = float(np.nanmax(np.abs(x - y), initial=0.0))
                gaps.append(gap / bound)
                assert gap <= bound, (what, a, b, key, gap, bound)
        print(f"REACHED coloc {what} pairs: {len(cr.pair_list(k))}  pairs of kept effects {int(np.sum(want['hit'] >= 0))}  "
              f"largest gap / bound {max(gaps):.2e}")
    return fits


def _window(ctx, mode, p, gm, gu, z1, z_more, kw, k, coloc=True, **more):
    return hotpath.impute_window(mode, gm, gu, p["off"], p["w"] if mode else None, z1, want_mats=True, ctx=ctx, z_more=z_more,
                                 susie=_ask(kw, k, coloc), **more)


@pytest.mark.parametrize("case", cr.CASE_MODES, ids=lambda c: f"M{c[0]}-U{c[1]}-L{c[2].get('L', 10)}-k{c[3]}-mode{c[5]}")
def test_cases(ctx, case):
    """Every case on pooled (mode 0) and on weighted (mode 1) LD"""
    M, U, kw, k, seed, mode = case
    p, gm, gu, z1, z_more = cr.case_window(M, U, k, seed)
    got = _window(ctx, mode, p, gm, gu, z1, z_more, kw, k)
    assert got["status"] & ~ST_NOCONV == 0
    _check(got, z1, z_more, k, kw, f"M={M} U={U} mode={mode} k={k}")
    if (M, U) == (1, 1):                               # n = 1: S1 S2 = S12 to the bit
        assert got["coloc_n"][0] == 1 and got["coloc_pp"][0, 0, 0, 3] == 0.0 and got["coloc_hit"][0, 0, 0] == 0


def test_the_traits_stop_at_different_sweeps(ctx):
    p, gm, gu, z1, z_more, kw = cr.sweeps_window()
    got = _window(ctx, 0, p, gm, gu, z1, z_more, kw, 1)
    fits = _check(got, z1, z_more, 1, kw, "different sweeps")
    assert got["status"] == 0 and got["susie_more_status"][0] == 0
    assert got["susie_sweeps"] == fits[0]["sweeps"] != fits[1]["sweeps"] == got["susie_more_sweeps"][0]
    assert not got["susie_more_kept"].any() and np.all(np.isnan(got["coloc_pp"])) and np.all(got["coloc_hit"] == -1)


def test_the_planted_claims(ctx):
    """Shared measured SNP: H4 leads.  Two SNPs with r = 0.029: H3 leads.  A shared UNMEASURED SNP: H4 leads and the hit is the imputed
    candidate M + 7.  A null trait keeps no effect: its pairs are NaN."""
    def one(which):
        p, gm, gu, z1, z_more = cr.planted_window(which)
        got = _window(ctx, 0, p, gm, gu, z1, z_more, {}, 1)
        fits = _check(got, z1, z_more, 1, {}, f"planted {which}")
        want = cr.pairs(fits)
        return got, fits, want
    for which, lead, hit in (("shared", 4, 52), ("distinct", 3, None), ("unmeasured", 4, 100 + 7)):
        got, fits, want = one(which)
        (la,), (lb,) = np.flatnonzero(got["susie_kept"]), np.flatnonzero(got["susie_more_kept"][0])
        assert int(np.argmax(got["coloc_pp"][0, la, lb])) == int(np.argmax(want["pp"][0, la, lb])) == lead, which
        assert got["coloc_hit"][0, la, lb] == want["hit"][0, la, lb] and (hit is None or got["coloc_hit"][0, la, lb] == hit), which
    got, fits, want = one("null")
    assert got["susie_kept"].any() and not got["susie_more_kept"].any() and np.all(np.isnan(got["coloc_pp"])) and np.all(got["coloc_hit"] == -1)


def test_trait_one_and_every_further_trait_keep_their_bits(ctx):
    """Trait 1's outputs are those of a window without coloc_traits_more.  A further trait's bits depend on neither k, nor the other
    rows of z_more, nor its own place among them; the pairs of two traits do not depend on the traits beside them."""
    M, U, kw, seed = 65, 192, dict(L=5, max_sweeps=20), 10
    p, gm, gu, z1, z3 = cr.case_window(M, U, 3, seed)
    run = lambda z_more, k, **kw2: hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, z_more=z_more, susie=_ask(kw, k, **kw2))
    alone = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, susie=dict(kw, want_alpha=True, want_lbf=True))
    plain = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, susie=dict(kw, want_alpha=True))
    full = run(z3, 3)
    _same(full, alone, ("z", "info") + SUSIE_KEYS)
    _same(alone, plain, ("z", "info") + tuple(k for k in SUSIE_KEYS if k != "susie_lbf"))
    assert full["susie_more_kept"].any() and np.any(full["coloc_hit"] >= 0)
    moved = run(z3[[2, 0]], 1)                         # trait 3 first, alone in the fit; trait 1 unfitted behind it
    for k in MORE_KEYS:
        assert np.array_equal(moved[k][0], full[k][2], equal_nan=True), k
    _same(moved, alone, SUSIE_KEYS)
    pairs = cr.pair_list(3)
    for k in COLOC_KEYS:                               # the pair (0, 3) of the full fit is the pair (0, 1) of this one
        assert np.array_equal(moved[k][0], full[k][pairs.index((0, 3))], equal_nan=True), k
    noisy = z3.copy()
    noisy[1] = np.nan                                  # another row's NaN moves no bit of this one
    other = run(noisy, 3)
    for k in MORE_KEYS:
        assert np.array_equal(other[k][[0, 2]], full[k][[0, 2]], equal_nan=True), k
    nocoloc = run(z3, 3, coloc=False)                  # ... nor does asking for the pairs
    _same(nocoloc, full, SUSIE_KEYS + MORE_KEYS)
    assert "coloc_pp" not in nocoloc


def _store_windows(ctx, susie, k, **kw):
    """cs_ref.store_windows as windows over one resident 2-bit store and as byte rows in host memory, every window asking"""
    p, ws = cs_ref.store_windows(**kw)
    G = p["G"]
    rows2, src_off = panel_mod.pack2bit(G, p["off"])
    store = hotpath.RowStore(rows2, ctx=ctx)
    wins, host = [], []
    for n, w in enumerate(ws):
        mi, ui = w["mi"], w["ui"]
        z_more = cr.traits_z(np.ascontiguousarray(G[mi]), k, 50 + n)
        wins.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=w["z1"], dev=(store.ptr, store.ptr, len(mi), len(ui), store.ld),
                         packed=dict(fmt=1, rows_m=mi, rows_u=ui, pop_src_off=src_off), z_more=z_more, susie=susie))
        host.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=w["z1"], geno_m=np.ascontiguousarray(G[mi]),
                         geno_u=np.ascontiguousarray(G[ui]), z_more=z_more, susie=susie))
    return p, rows2, src_off, store, wins, host


def _run(ctx, wins, on_device=True, runs=1):
    job = hotpath.Job(wins, ctx=ctx, on_device=on_device)
    for _ in range(runs):
        job.run()
    out = [job.fetch() for _ in range(runs)]
    cnt = job.counters()
    job.close()
    return out, cnt


ALL_KEYS = ("z", "info", "z_more") + SUSIE_KEYS + MORE_KEYS + COLOC_KEYS
SUSIE = dict(L=5, max_sweeps=20, want_alpha=True, want_lbf=True, traits=2, coloc={})


def test_every_launch_form_and_source_format_returns_the_same_bits(ctx, monkeypatch):
    """The switches tests/test_gpu_susie.py's test of the same name drives"""
    p, rows2, src_off, store, wins, host = _store_windows(ctx, SUSIE, 2)
    ref = _run(ctx, wins)[0][0]
    assert all(r["status"] & ~ST_NOCONV == 0 for r in ref) and any(np.any(r["coloc_hit"] >= 0) for r in ref)
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
    try:                                               # int8 Gram
        ctx.set_gram_dtype("i8")
        for r, w in zip(_run(ctx, wins)[0][0], ref):
            _same(r, w, ALL_KEYS)
    finally:
        ctx.set_gram_dtype(os.environ.get("GAUSS_GRAM_DTYPE", "f32"))
    for r, w in zip(_run(ctx, host, on_device=False)[0][0], ref):      # byte rows from host memory
        _same(r, w, ALL_KEYS)
    h2 = host[2]                                       # the blocking window call: streamed (default) and upload-then-run
    call = lambda: hotpath.impute_window(1, h2["geno_m"], h2["geno_u"], p["off"], p["w"], h2["z1"], ctx=ctx, z_more=h2["z_more"], susie=SUSIE)
    _same(call(), ref[2], ALL_KEYS)
    with monkeypatch.context() as m:
        m.setenv("GAUSS_STREAM_WINDOW", "0")
        _same(call(), ref[2], ALL_KEYS)
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
    """Windows of one job may mix, with different k, L and sweeps.  The asking windows return what their stand-alone calls return, two
    runs in flight return the same values, and a job in which nobody asks has the counters and the bits of the job built without the
    keys -- and of the job whose windows fit trait 1 alone, as before."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx, SUSIE, 2, seed=43, spans=((0, 131), (97, 340), (211, 560)))
    other = dict(L=2, max_sweeps=3, tol=0.0, want_alpha=True, want_lbf=True, traits=1, coloc=dict(p1=1e-3, p2=2e-3, p12=1e-4))
    one = dict(L=5, max_sweeps=20, want_alpha=True)
    ask = [SUSIE, one, other]
    mixed, c1 = _run(ctx, [dict(w, susie=ask[k]) for k, w in enumerate(wins)], runs=2)
    nobody, c0 = _run(ctx, [dict(w, susie=one) for w in wins], runs=2)
    plain, c2 = _run(ctx, [{k: v for k, v in w.items() if k != "z_more"} | dict(susie=one) for w in wins], runs=2)
    assert c0 == c1 == c2, (c0, c1, c2)
    keys1 = tuple(k for k in SUSIE_KEYS if k != "susie_lbf")
    for run in mixed:
        for k, r in enumerate(run):
            _same(r, plain[0][k], ("z", "info"), own_bits=ST_NOCONV)
            assert ("coloc_pp" in r) == (k != 1) and ("susie_more_pip" in r) == (k != 1)
            h = host[k]
            alone = hotpath.impute_window(1, h["geno_m"], h["geno_u"], p["off"], p["w"], h["z1"], ctx=ctx, z_more=h["z_more"], susie=ask[k])
            _same(r, alone, ("z", "info", "z_more") + (keys1 if k == 1 else SUSIE_KEYS + MORE_KEYS + COLOC_KEYS))
    assert mixed[0][2]["susie_more_sweeps"][0] == 3 and mixed[0][2]["coloc_pp"].shape == (1, 2, 2, 5) and mixed[0][0]["coloc_pp"].shape == (3, 5, 5, 5)
    for r, w in zip(nobody[1], plain[0]):              # nobody asks for further traits in the fit: trait 1's job, bit for bit
        _same(r, w, ("z", "info") + keys1)
        assert "susie_more_pip" not in r and "coloc_pp" not in r
    store.close()


def test_all_riders_on_one_window_at_once(ctx):
    """Leave-one-out values, the selection, the conditioned imputed SNPs, the credible sets, further traits and the multi-trait fit with
    its pairs on one window: each output has the bits of the call that asks for it alone."""
    p, gm, gu = cs_ref.window(129, 140, seed=77)
    z1 = cs_ref.planted(gm, seed=6)
    z_more = cr.traits_z(gm, 3, 12)
    slct = dict(max=32, chi2_stop=cs_ref.CHI2_GWS, unmeasured=True, cs=dict(cs_ref.CS))
    run = lambda **kw: hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, **kw)
    both = run(loo=True, slct=slct, z_more=z_more, susie=SUSIE)
    _same(both, run(z_more=z_more, susie=SUSIE), ALL_KEYS)
    _same(both, run(slct=slct), ("z", "info", "slct_idx", "slct_zin", "slct_joint", "slct_zc", "slct_var", "cond_z", "cond_var", "cs_pip", "cs_set",
                                 "cs_set_pip", "cs_size", "cs_mass", "cs_lse"), own_bits=ST_NOCONV)
    _same(both, run(loo=True), ("z", "info", "loo_z", "loo_info", "loo_t"), own_bits=ST_NOCONV)
    _same(both, run(z_more=z_more), ("z", "info", "z_more"), own_bits=ST_NOCONV)
    assert both["susie_more_kept"].sum() >= 1 and both["susie_more_pip"].shape == (2, 269)


def test_nan_nonfinite_and_clamped_windows(ctx):
    """A NaN in a further trait's scores: that SNP and every unmeasured SNP are no candidates of that trait, the other traits keep
    their bits, and the pairs run over the candidates admissible in both.  A GAUSS_ST_NONFINITE window and a window MakePosDef repairs
    (NOFIT for every trait): NaN / 0 / -1 for every trait and every pair."""
    p, gm, gu, z1, z_more = cr.case_window(12, 11, 2, 14)
    kw = dict(L=3)
    clean = _window(ctx, 0, p, gm, gu, z1, z_more, kw, 2)
    z_nan = z_more.copy()
    z_nan[0, 5] = np.nan
    got = _window(ctx, 0, p, gm, gu, z1, z_nan, kw, 2)
    assert got["status"] == 0 and np.all(got["susie_more_status"] == 0) and not np.any(np.isfinite(got["z_more"][0]))
    _check(got, z1, z_nan, 2, kw, "NaN in a further trait")
    assert np.all(got["susie_more_alpha"][0][:, 12:] == 0) and np.all(got["susie_more_alpha"][0][:, 5] == 0)
    assert list(got["coloc_n"]) == [11, 23, 11]
    _same(got, clean, SUSIE_KEYS)
    for k in MORE_KEYS:
        assert np.array_equal(got[k][1], clean[k][1], equal_nan=True), k
    gm2 = gm.copy()
    gm2[3, :] = 1                                      # zero variance: CalCor returns 0 / 0
    got = hotpath.impute_window(0, gm2, gu, p["off"], None, z1, ctx=ctx, z_more=z_more, susie=_ask(kw, 2))
    assert got["status"] & ST_NONFINITE and not got["status"] & (ST_NOFIT | ST_NOCONV)
    assert np.all(got["susie_more_status"] == ST_NONFINITE)

    def nothing(got):
        for k in ("pip", "set_pip", "V", "lse", "mass", "purity", "alpha", "mu", "lbf"):
            assert np.all(np.isnan(got["susie_more_" + k])) and np.all(np.isnan(got["susie_" + k])), k
        assert np.all(got["susie_more_size"] == 0) and np.all(got["susie_more_kept"] == 0) and np.all(got["susie_more_set"] == -1)
        assert np.all(got["susie_more_sweeps"] == 0)
        assert np.all(np.isnan(got["coloc_pp"])) and np.all(np.isnan(got["coloc_hit_pp"])) and np.all(got["coloc_hit"] == -1) and np.all(got["coloc_n"] == 0)
    nothing(got)
    p, gm, gu, z1 = cs_ref.clamped_window()
    z_more = cr.traits_z(gm, 2, 3)
    plain = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, ctx=ctx, z_more=z_more)
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, ctx=ctx, z_more=z_more, susie=_ask({}, 2))
    assert plain["status"] == ST_CLAMPED and got["status"] == ST_CLAMPED | ST_NOFIT and np.all(got["susie_more_status"] == ST_NOFIT)
    _same(got, plain, ("z", "info", "z_more"), own_bits=ST_NOFIT)
    nothing(got)


def test_refusals(ctx):
    p = small_panel(n_snp=120, scale=0.02, n_pops=5)
    gm, gu, z1 = split_window(p, 50)
    z_more = np.random.default_rng(1).standard_normal((9, 50))
    run = lambda z=z_more, miss=None, **kw: hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, z_more=z, miss_more=miss,
                                                                 susie=dict(dict(L=3), **kw))
    for bad, z in ((-1, z_more), (8, z_more), (3, z_more[:2]), (1, None)):      # below 0, above the cap, above n_traits_more (twice)
        with pytest.raises(Exception, match="coloc_traits_more = "):
            run(z=z, traits=bad)
    with pytest.raises(Exception, match="coloc_traits_more.*susie_L"):
        run(L=0, traits=1)
    mask = np.zeros((9, 50), dtype=np.uint8)
    mask[4, 7] = 1
    with pytest.raises(Exception, match="coloc_traits_more.*miss_more"):
        run(miss=mask, traits=2)
    got = run(miss=mask)                               # the mask alone is no ground for a refusal
    assert "info_more" in got and "susie_more_pip" not in got
    for key in ("p1", "p2", "p12"):
        for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
            co = dict(dict(p1=1e-4, p2=1e-4, p12=1e-5), **{key: bad})
            with pytest.raises(Exception, match="coloc_" + key + " = "):
                run(traits=1, coloc=co)
    with pytest.raises(Exception, match="coloc_p12 = .*exceeds"):
        run(traits=1, coloc=dict(p1=1e-4, p2=1e-5, p12=5e-5))
    with pytest.raises(Exception, match="coloc_p1 / coloc_p2 / coloc_p12.*coloc_traits_more >= 1"):
        run(traits=0, coloc={})
    ok = run(traits=7, coloc={})                       # the cap itself: eight traits, 28 pairs
    assert ok["coloc_pp"].shape == (28, 3, 3, 5) and ok["susie_more_pip"].shape == (7, len(gm) + len(gu))


# ---- the host entry points, files -> table -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def study(tmp_path_factory):
    st = cr.study(tmp_path_factory.mktemp("coloc_study"))
    packed = os.path.join(os.path.dirname(st["files"][2]), "panel.gpk")
    assert api.pack_panel(st["files"][1], st["files"][2], st["files"][3], packed) > 0
    return dict(st, packed=packed)


def _same_column(a, b, c):
    if a[c].dtype.kind == "f":
        assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
    else:
        assert list(a[c]) == list(b[c]), c


def _same_frame(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for c in a.columns:
        _same_column(a, b, c)
    assert list(a.attrs["coloc"].columns) == list(b.attrs["coloc"].columns) and len(a.attrs["coloc"]) == len(b.attrs["coloc"])
    for c in a.attrs["coloc"].columns:
        _same_column(a.attrs["coloc"], b.attrs["coloc"], c)
    assert a.attrs["fit"] == b.attrs["fit"] and len(a.attrs["effects"]) == len(b.attrs["effects"])
    for x, y in zip(a.attrs["effects"], b.attrs["effects"]):
        assert all(np.array_equal(x[k], y[k], equal_nan=True) for k in x)


@pytest.mark.parametrize("mix", [False, True])
def test_dist_coloc_and_distmix_coloc_end_to_end(ctx, study, mix, monkeypatch):
    """Three study files on a text panel, a packed panel and the packed panel through the full SNP map: the same table.  Its rows and
    trait 1's columns are *_susie's on the first file bit for bit, the traits' columns are *_traits'; every trait's pip / cs / cs_pip,
    effects and fit, and the coloc frame are the hotpath's result for the window the oracle's data layer builds, by rsid."""
    win = cs_ref.STUDY_WINDOW
    fw = cs_ref.feeder_window(mix, study["files"])
    meas, unme, gm, gu, off, w, who, cutoff = (fw[k] for k in ("meas", "unme", "gm", "gu", "off", "w", "who", "cutoff"))
    fn, fn_susie, fn_traits = (api.distmix_coloc, api.distmix_susie, api.distmix_traits) if mix else (api.dist_coloc, api.dist_susie, api.dist_traits)
    inp, idx, dat, desc = study["files"]
    files = [inp] + study["more"]
    args, p12 = cr.STUDY_ARGS, cr.STUDY_P12
    kw = dict(af1_cutoff=cutoff, ctx=ctx, **args)
    df = fn(*win, who, files, idx, dat, desc, p12=p12, **kw)
    one = fn_susie(*win, who, inp, idx, dat, desc, **kw)
    tr = fn_traits(*win, who, files, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
    head = [c for c in one.columns if c not in ("wing", "pip", "cs", "cs_pip")]
    assert list(tr.columns) == head + ["z_2", "pval_2", "z_3", "pval_3"]
    assert list(df.columns) == list(tr.columns) + ["wing", "pip", "cs", "cs_pip", "pip_2", "cs_2", "cs_pip_2", "pip_3", "cs_3", "cs_pip_3"]
    assert len(df) == len(one)
    for c in one.columns:                              # *_susie on the first file: rows and bits
        _same_column(df, one, c)
    own = df.iloc[: len(tr)].reset_index(drop=True)
    for c in tr.columns:                               # *_traits on the call's own rows
        _same_column(own, tr, c)
    eff, fit, co = df.attrs["effects"], df.attrs["fit"], df.attrs["coloc"]
    assert len(eff) == len(fit) == 3 and fit[0] == one.attrs["fit"]
    assert all(np.array_equal(eff[0][k], one.attrs["effects"][k], equal_nan=True) for k in eff[0])
    # the hotpath on the oracle's window; the further traits' scores at its measured SNPs are the table's own z_t there (wings included)
    by = {r: k for k, r in enumerate(df["rsid"])}
    rows = np.array([by[s.rsid] for s in meas] + [by[s.rsid] for s in unme])          # every candidate has a row
    assert len(set(rows.tolist())) == len(rows) == len(df)
    M = len(meas)
    z1 = np.array([s.z for s in meas])
    z_more = np.array([df[f"z_{t}"].to_numpy()[rows[:M]] for t in (2, 3)])
    hp = hotpath.impute_window(1 if mix else 0, gm, gu, off, w, z1, want_mats=True, ctx=ctx, z_more=z_more,
                               susie=dict(args, traits=2, want_alpha=True, want_lbf=True, coloc=dict(p12=p12)))
    _check(hp, z1, z_more, 2, args, f"table window mix={mix}", p12=p12)
    assert np.array_equal(df["pip"].to_numpy()[rows], hp["susie_pip"]) and np.array_equal(df["cs"].to_numpy()[rows], hp["susie_set"] + 1)
    for t in (2, 3):
        assert np.array_equal(df[f"pip_{t}"].to_numpy()[rows], hp["susie_more_pip"][t - 2])
        assert np.array_equal(df[f"cs_{t}"].to_numpy()[rows], hp["susie_more_set"][t - 2] + 1)
        assert np.array_equal(df[f"cs_pip_{t}"].to_numpy()[rows], hp["susie_more_set_pip"][t - 2])
        e = eff[t - 1]
        assert np.array_equal(e["size"], hp["susie_more_size"][t - 2]) and np.array_equal(e["kept"], hp["susie_more_kept"][t - 2] != 0)
        assert np.array_equal(e["row"], rows[np.argmax(hp["susie_more_alpha"][t - 2], axis=1)])
        for k in ("V", "lse", "mass", "purity"):
            assert np.array_equal(e[k], hp["susie_more_" + k][t - 2], equal_nan=True), k
        assert fit[t - 1]["sweeps"] == hp["susie_more_sweeps"][t - 2] and fit[t - 1]["delta"] == hp["susie_more_delta"][t - 2]
        assert fit[t - 1]["converged"] == (not hp["susie_more_status"][t - 2] & ST_NOCONV)
    # the coloc frame: one row per pair of kept effects, in the order of the pairs, then la, then lb
    want = [(q, la, lb) for q in range(3) for la in range(6) for lb in range(6) if hp["coloc_hit"][q, la, lb] >= 0]
    pairs = cr.pair_list(2)
    assert len(co) == len(want) > 0 and eff[0]["kept"].any() and eff[1]["kept"].any()
    assert list(co.columns) == list(api.COLOC_COLUMNS) + ["hit_rsid"]
    for r, (q, la, lb) in zip(co.itertuples(index=False), want):
        assert (r.trait_a, r.trait_b, r.cs_a, r.cs_b, r.n) == (pairs[q][0] + 1, pairs[q][1] + 1, la + 1, lb + 1, hp["coloc_n"][q])
        assert np.array_equal([r.H0, r.H1, r.H2, r.H3, r.H4], hp["coloc_pp"][q, la, lb]) and r.hit_pp == hp["coloc_hit_pp"][q, la, lb]
        assert r.hit_row == rows[hp["coloc_hit"][q, la, lb]] and r.hit_rsid == df["rsid"][r.hit_row]
    shared = co[(co["trait_a"] == 1) & (co["trait_b"] == 2)]
    assert len(shared) and (shared[["H0", "H1", "H2", "H3", "H4"]].to_numpy().argmax(axis=1) == 4).any()      # trait 2 is trait 1 rescaled
    print(f"REACHED coloc table mix={mix}: kept {[int(e['kept'].sum()) for e in eff]}  pairs of kept effects {len(co)}  "
          f"sweeps {[f['sweeps'] for f in fit]}")
    forms = [fn(*win, who, files, "(unused)", study["packed"], desc, p12=p12, **kw)]
    monkeypatch.setenv("GAUSS_HOST_FULL_MAP", "1")
    forms.append(fn(*win, who, files, "(unused)", study["packed"], desc, p12=p12, **kw))
    forms.append(fn(*win, who, files, idx, dat, desc, p12=p12, **kw))
    for other in forms:
        _same_frame(df, other)
    with pytest.raises(Exception, match="trait3_lacking.txt lacks [12] of "):
        fn(*win, who, [inp, study["lacking"]], idx, dat, desc, **kw)
    with pytest.raises(Exception, match="at most 8 traits"):
        fn(*win, who, [inp] + [study["more"][1]] * 8, idx, dat, desc, **kw)
    with pytest.raises(Exception, match="at least two study files"):
        fn(*win, who, [inp], idx, dat, desc, **kw)
    with pytest.raises(Exception, match="coloc_p12 = .*exceeds"):
        fn(*win, who, files, idx, dat, desc, p1=1e-6, **kw)
    with pytest.raises(Exception, match="at most 32 effects"):
        fn(*win, who, files, idx, dat, desc, af1_cutoff=cutoff, L=33, ctx=ctx)
