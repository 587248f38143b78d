"""GPU: the imputed SNPs conditioned on the selected signals (out_cond_* of gauss_window_desc, k_cond.hip) against tests/cond_ref.py.

Every value case asks for out_b11 / out_b21 and is compared with cond_ref.cond_by_definition evaluated ON THE MATRICES THE GPU
RETURNED and on the indices the GPU selected -- which are first checked against slct_ref.slct_by_definition, as tests/test_gpu_slct.py
does.  cond_z and cond_var agree within 1e-8 as |d| / max(1, |want|), the project's bound for solve outputs, with NaNs in the same
places; where cond_z is NaN is asserted only after the reference's margin says that no imputed SNP sits within 1e-9 of its guard
and no info within 1e-9 of zero.  Each case prints the level it reaches (REACHED lines)."""
import os

import numpy as np
import pytest

from gauss_amd import api, hotpath
from gauss_amd import panel as panel_mod
from cond_ref import cond_by_definition, cond_by_residual, window_mats
from helpers import small_panel, split_window
from loo_ref import window_b11
from slct_ref import min_var_frac, slct_by_definition

pytestmark = pytest.mark.gpu

TOL = 1e-8
MARGIN = 1e-9
CHI2_GWS = 29.716785
BLOCK = 128                        # COND_T of k_cond.hip: unmeasured SNPs per workgroup
SLCT_KEYS = ("slct_idx", "slct_zin", "slct_joint", "slct_zc", "slct_var")
KEYS = SLCT_KEYS + ("cond_z", "cond_var")


def _err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaNs in different places"
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok])))) if ok.any() else 0.0


def _mvf_u(slct):
    return slct["min_var_frac_u"] if "min_var_frac_u" in slct else 1.0 - slct.get("collin", 0.9)


def _check(got, z1, slct, lam=0.1, what="", tol=TOL):
    """got: a window's result with b11 and b21; slct: the dict the window was given.  The selection against its definition (exact
    indices behind its margin), then the conditional statistics of the imputed SNPs on those indices."""
    sel = slct_by_definition(got["b11"], z1, slct["max"], slct["chi2_stop"], min_var_frac(slct.get("collin", 0.9), lam), slct.get("forced", ()))
    assert sel["min_margin"] > MARGIN, (what, sel["min_margin"])
    assert got["slct_n"] == sel["n"] and np.array_equal(got["slct_idx"], sel["idx"]), (what, got["slct_idx"], sel["idx"])
    want = cond_by_definition(got["b11"], got["b21"], z1, got["slct_idx"], _mvf_u(slct))
    assert want["margin"] > MARGIN, (what, want["margin"])
    e = dict(cond_z=_err(got["cond_z"], want["z"]), cond_var=_err(got["cond_var"], want["var"]))
    print(f"REACHED cond {what}: n {sel['n']}  U {len(want['z'])}  NaN {int(np.isnan(want['z']).sum())}  margin {want['margin']:.3e}  "
          + "  ".join(f"{k} {v:.3e}" for k, v in e.items()) + f"  (bound {tol:g})")
    assert max(e.values()) <= tol, (what, e)
    return sel, want


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
    p = small_panel(n_snp=M + U + 30 + (M + U) // 20, scale=scale, seed=11 + M + U if seed is None else seed)
    assert p["G"].shape[0] >= M + U
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


def _cond(slct, **kw):
    return dict(slct, unmeasured=True, **kw)


EDGES = [(65, u, mode) for u in (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1) for mode in (0, 1)] + \
        [(m, BLOCK + 1, mode) for m in (1, 2, 513, 2100) for mode in (0, 1)]


@pytest.mark.parametrize("M,U,mode", EDGES)
def test_conditional_statistics_match_the_definition_at_the_kernel_edges(ctx, M, U, mode):
    """U around the workgroup's 128 unmeasured SNPs (one thread each; the last block partly empty, three blocks), M from one SNP to
    above the selection's LDS limit (its r and v live in the result block, in front of this section), pooled and weighted; n = 1
    (max = 1), n = 32 (chi2_stop = 0: every step taken) and planted signals at the genome-wide threshold.  z / info are the bits of
    the same call without the rider, the selection's outputs the bits of the call without `unmeasured`.  The U values run at M = 65 and
    the M values at U = 129: the kernel's paths depend on U through the block count alone and on M through the selection's section
    alone.  The weighted M = 2 100 window takes a panel of 3 635 samples (scale 0.1): with the 1 190 of scale 0.02 its B11 has more SNPs
    than samples, an eigenvalue of -0.25, and is one MakePosDef repairs -- the clamped window has its own test."""
    p, gm, gu = _window(M, U, scale=0.1 if (mode and M > 2048) else 0.02)
    assert gm.shape[1] > M or not (mode and M > 2048)
    w = p["w"] if mode else None
    z1 = _planted(gm, seed=M + mode)
    plain = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx)
    for slct in (dict(max=1, chi2_stop=0.05), dict(max=32, chi2_stop=0.0), dict(max=32, chi2_stop=CHI2_GWS)):
        got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, want_mats=True, ctx=ctx, slct=_cond(slct))
        assert got["status"] == 0 and got["cond_z"].shape == (U,) and got["cond_var"].shape == (U,)
        sel, _ = _check(got, z1, slct, what=f"M={M} U={U} mode={mode} K={slct['max']} stop={slct['chi2_stop']:g}")
        _same(got, plain, ("z", "info"))
        _same(got, hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, slct=slct), SLCT_KEYS)
        if slct["max"] == 1:
            assert sel["n"] == 1
        elif slct["chi2_stop"] == 0.0 and M >= 65:
            assert sel["n"] == 32
        else:
            assert sel["n"] >= 1


def test_nothing_selected_returns_the_bits_of_z_and_ones(ctx):
    p, gm, gu = _window(120, 130, seed=19)
    _, _, z1 = split_window(dict(G=p["G"][:250]), 120)
    slct = dict(max=32, chi2_stop=1e3)
    got = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, want_mats=True, ctx=ctx, slct=_cond(slct))
    assert got["slct_n"] == 0 and got["status"] == 0
    assert np.array_equal(got["cond_z"], got["z"]) and np.array_equal(got["cond_var"], np.ones(130))
    _check(got, z1, slct, what="nothing selected")


def _near_twin(gm, j, p, lam, lo=0.11, hi=0.3):
    """A copy of measured row j with genotypes changed one sample at a time until SNP j leaves it a share of variance in (lo, hi): just
    inside the guard of 0.1.  Decided on the CPU's matrices; the GPU's are checked against the reference like every other case."""
    rng = np.random.default_rng(5)
    row = gm[j].copy()
    z = np.zeros(gm.shape[0])
    for col in rng.permutation(gm.shape[1]):
        row[col] = (row[col] + 1) % 3 if row[col] < 48 else 48 + (row[col] - 48 + 1) % 3
        B, b21 = window_mats(0, gm, row[None, :], p["off"], None, lam)
        v = cond_by_definition(B, b21, z, [j], 0.1)["var"][0]
        if v > lo:
            assert v < hi, v
            return row
    raise AssertionError("no near-duplicate found")


def test_unmeasured_twin_of_a_forced_snp_and_a_near_twin(ctx):
    """The ridge does not cap what a selected SNP explains of an imputed one.  For an unmeasured exact duplicate of measured SNP j,
    b_u = B_j - lambda e_j, so info_u = 1 - lambda + lambda^2 (B^-1)_jj, and S = {j} explains 1 / (1 + lambda) of it: what is left is
    lambda^2 ((B^-1)_jj - 1 / (1 + lambda)) -- exactly 0 where j is isolated ((B^-1)_jj = 1 / (1 + lambda)) and at lambda = 0.  Both
    are run: the one-SNP window at lambda = 0.1 (the only exactly isolated SNP a real panel offers) and a 50-SNP window at lambda = 0.
    cond_z is NaN there and cond_var below 1e-6, with the guard the host passes (1 - collin, no ridge correction).  A near-duplicate
    just inside the guard, in the 50-SNP window at lambda = 0.1, is finite and within the bound."""
    p, gm, gu = _window(1, 5, seed=8)
    gu2 = np.ascontiguousarray(np.vstack([gu, gm[0]]))
    slct = dict(max=1, chi2_stop=0.0, forced=[0])
    got = hotpath.impute_window(0, gm, gu2, p["off"], None, np.array([6.0]), ctx=ctx, slct=_cond(slct))
    assert got["slct_n"] == 1 and np.isnan(got["cond_z"][5]) and abs(got["cond_var"][5]) < 1e-6
    assert abs(got["info"][5] - 1 / 1.1) < 1e-12                               # info = q = 1 / (1 + lambda)
    p = small_panel(n_snp=120, scale=0.02, seed=31)
    gm, gu, _ = split_window(dict(G=p["G"][:110]), 50)
    j = 7
    z1 = _planted(gm, seed=4)
    gu2 = np.ascontiguousarray(np.vstack([gu, gm[j]]))
    slct = dict(max=1, chi2_stop=0.0, forced=[j])
    got = hotpath.impute_window(0, gm, gu2, p["off"], None, z1, lam=0.0, want_mats=True, ctx=ctx, slct=_cond(slct))
    assert got["status"] == 0 and got["slct_idx"].tolist() == [j]
    assert np.isnan(got["cond_z"][-1]) and abs(got["cond_var"][-1]) < 1e-6
    print(f"REACHED cond twin: var left {got['cond_var'][-1]:.3e} (bound 1e-6)")
    _check(got, z1, slct, lam=0.0, what="exact twin, lambda = 0")
    gu3 = np.ascontiguousarray(np.vstack([gu, _near_twin(gm, j, p, 0.1)]))
    got = hotpath.impute_window(0, gm, gu3, p["off"], None, z1, want_mats=True, ctx=ctx, slct=_cond(slct))
    _, want = _check(got, z1, slct, what="near twin")
    assert np.isfinite(got["cond_z"][-1]) and 0.1 < got["cond_var"][-1] < 0.3
    # and a guard of its own just above that share excludes it
    got = hotpath.impute_window(0, gm, gu3, p["off"], None, z1, want_mats=True, ctx=ctx, slct=_cond(slct, min_var_frac_u=float(want["var"][-1]) + 0.01))
    _check(got, z1, dict(slct, min_var_frac_u=float(want["var"][-1]) + 0.01), what="near twin, stricter guard")
    assert np.isnan(got["cond_z"][-1])


def test_pure_conditional_list(ctx):
    """max == len(forced): the imputed SNPs conditioned on a given list, in the caller's order."""
    p, gm, gu = _window(65, 70, seed=5)
    z1 = _planted(gm, seed=9)
    slct = dict(max=3, chi2_stop=CHI2_GWS, forced=[11, 2, 44])
    got = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, want_mats=True, ctx=ctx, slct=_cond(slct))
    sel, _ = _check(got, z1, slct, what="forced only")
    assert sel["idx"].tolist() == [11, 2, 44]
    rev = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, want_mats=True, ctx=ctx, slct=_cond(dict(slct, forced=[44, 2, 11])))
    assert _err(rev["cond_z"], got["cond_z"]) <= TOL and _err(rev["cond_var"], got["cond_var"]) <= TOL      # the set decides, not the order


@pytest.mark.parametrize("mode", [0, 1])
def test_second_route_through_the_oracle(ctx, mode):
    """cond_by_residual with the oracle as its imputer: the residual of z1 on the selected SNPs imputed by run_dist / run_distmix, the
    selection by its definition on the oracle's B11 -- nothing the GPU returned enters the expected values."""
    import oracle
    p, gm, gu = _window(65, 70, seed=23)
    w = p["w"] if mode else None
    z1 = _planted(gm, seed=3 + mode)
    slct = dict(max=32, chi2_stop=CHI2_GWS)
    o = oracle.run_impute(mode, gm, gu, p["off"], w, z1, want_mats=True)
    assert o["mpd"] == 0
    sel = slct_by_definition(o["b11"], z1, 32, CHI2_GWS, min_var_frac(0.9, 0.1))
    assert sel["min_margin"] > MARGIN and sel["n"] >= 1

    def impute(r):
        q = oracle.run_impute(mode, gm, gu, p["off"], w, r)
        return q["z"] * np.sqrt(q["info"]), q["info"]

    want = cond_by_residual(o["b11"], o["b21"], z1, sel["idx"], 0.1, impute=impute)
    assert want["margin"] > MARGIN
    got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, slct=_cond(slct))
    assert np.array_equal(got["slct_idx"], sel["idx"])
    e = dict(cond_z=_err(got["cond_z"], want["z"]), cond_var=_err(got["cond_var"], want["var"]))
    print(f"REACHED cond through the oracle mode={mode}: n {sel['n']}  " + "  ".join(f"{k} {v:.3e}" for k, v in e.items()) + f"  (bound {TOL:g})")
    assert max(e.values()) <= TOL, e


def test_clamped_nonfinite_and_nan_windows(ctx):
    """Duplicated measured SNPs at lambda = 0 (the construction of tests/test_gpu_slct.py's clamped window): MakePosDef rebuilds B11,
    selection and conditioning run again on the repaired matrix, which is the one the job returns.  A NaN in z1 makes every imputed
    mean NaN, and cond_z with it; the selection works around it as it does without the rider.  A GAUSS_ST_NONFINITE window returns
    NaN."""
    p = small_panel(n_snp=70, scale=0.02, n_pops=6, seed=21)
    gm, gu, _ = split_window(p, 30)
    gm = np.ascontiguousarray(np.vstack([gm, gm[:3]]))
    z1 = _planted(gm, seed=2)
    z1[30:] = z1[:3] + 0.3
    slct = dict(max=32, chi2_stop=4.0)
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, want_mats=True, ctx=ctx, slct=_cond(slct))
    plain = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, ctx=ctx)
    assert got["status"] & 1
    _same(got, plain, ("z", "info"))
    sel, _ = _check(got, z1, slct, lam=0.0, what="clamped window")
    assert sel["n"] >= 2
    p, gm, gu = _window(65, 70, seed=5)
    z1 = _planted(gm, seed=9)
    z1[13] = np.nan
    slct = dict(max=32, chi2_stop=CHI2_GWS)
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, want_mats=True, ctx=ctx, slct=_cond(slct))
    _same(got, hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, slct=slct), ("z", "info") + SLCT_KEYS)
    sel = slct_by_definition(got["b11"], z1, 32, CHI2_GWS, min_var_frac(0.9, 0.1))
    assert sel["min_margin"] > MARGIN and sel["n"] >= 1 and np.array_equal(got["slct_idx"], sel["idx"])
    assert np.all(np.isnan(got["z"])) and np.all(np.isnan(got["cond_z"]))
    fin = np.isfinite(got["info"])                     # (the share left is a function of info and the LD alone: given where info is)
    want = cond_by_definition(got["b11"], got["b21"], z1, sel["idx"], 0.1)
    assert np.all(np.isnan(got["cond_var"][~fin])) and _err(got["cond_var"][fin], want["var"][fin]) <= TOL
    gm = gm.copy()
    gm[3, :] = 1                                       # zero variance: CalCor returns 0 / 0
    got = hotpath.impute_window(0, gm, gu, p["off"], None, np.nan_to_num(z1, nan=1.0), ctx=ctx, slct=_cond(slct))
    assert got["status"] & 2 and got["slct_n"] == 0
    assert got["cond_z"].shape == (70,) and np.all(np.isnan(got["cond_z"])) and np.all(np.isnan(got["cond_var"]))


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
        slct = _cond(dict(max=32, chi2_stop=CHI2_GWS if k % 2 == 0 else 3.0, forced=[5, 1] if k == 1 else []))
        wins.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=z1, dev=(store.ptr, store.ptr, len(mi), len(ui), store.ld),
                         packed=dict(fmt=1, rows_m=mi.astype(np.int32), rows_u=ui.astype(np.int32), pop_src_off=src_off), slct=slct))
        host.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=z1, geno_m=np.ascontiguousarray(G[mi]),
                         geno_u=np.ascontiguousarray(G[ui]), slct=slct))
    return p, rows2, src_off, store, wins, host


def test_every_launch_form_and_source_format_returns_the_same_bits(ctx, monkeypatch):
    """The same job under each switch that changes a launch form or a source format (the list of tests/test_gpu_slct.py): the
    conditional statistics bit for bit those of the default -- z, info, the selection and B21 have the same bits in every form and
    the kernel's sums have a fixed order.  GAUSS_FUSED_SOLVE=0 (with the chain on the main queue, where the switch applies): z / info
    and with them the conditional statistics within 1e-8, the selection the same bits.  That the rider did not force the fused form
    cannot be read from the job's counters: gauss_job_counters counts merged / demoted runs, give-ups and failed re-runs and says
    nothing about which solver ran.  The counters are held equal to those of the same job with nobody asking, and the form is shown
    by the values instead: z / info are the bits of the nobody-asks job under the same switch, which takes the stand-alone solver,
    and some bit differs from the fused form's -- the rider rode behind the stand-alone solver."""
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
        m.setenv("GAUSS_CHAIN_ASIDE", "0")
        alone, cnt_alone = _run(ctx, [dict(w, slct=None) for w in wins])
        asked, cnt_asked = _run(ctx, wins)
        assert cnt_asked == cnt_alone, (cnt_asked, cnt_alone)
        differs = False
        for r, w, a in zip(asked[0], ref, alone[0]):
            _same(r, w, SLCT_KEYS)
            _same(r, a, ("z", "info"))
            differs = differs or not np.array_equal(r["z"], w["z"])
            e = [_err(r[k], w[k]) for k in ("z", "info", "cond_z", "cond_var")]
            print("REACHED cond behind the stand-alone solver: " + "  ".join(f"{v:.3e}" for v in e))
            assert max(e) <= TOL
        assert differs, "the stand-alone solver's sums have another order: some bit of z differs from the fused form's"
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
    """Windows of one job may mix: window 1 selects without conditioning its imputed SNPs.  The asking windows return what their
    stand-alone calls return, two runs in flight return the same values, and a job in which nobody asks has the counters and the
    z / info of the same job with the descriptor fields left zero."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx, seed=43, spans=((0, 131), (97, 340), (211, 560)))
    no_u = lambda s: {k: v for k, v in s.items() if k != "unmeasured"}
    nobody, c0 = _run(ctx, [dict(w, slct=None) for w in wins], runs=2)
    mixed, c1 = _run(ctx, [dict(w, slct=(w["slct"] if k != 1 else no_u(w["slct"]))) for k, w in enumerate(wins)], runs=2)
    only_slct, c2 = _run(ctx, [dict(w, slct=no_u(w["slct"])) for w in wins], runs=2)
    assert c0 == c1 == c2, (c0, c1, c2)
    for run in mixed:
        for k, (r, w) in enumerate(zip(run, nobody[0])):
            _same(r, w, ("z", "info"))
            _same(r, only_slct[0][k], SLCT_KEYS)
            assert ("cond_z" in r) == (k != 1)
            if k != 1:
                h = host[k]
                _same(r, hotpath.impute_window(1, h["geno_m"], h["geno_u"], p["off"], p["w"], h["z1"], ctx=ctx, slct=h["slct"]))
    for r, w in zip(only_slct[1], nobody[1]):
        _same(r, w, ("z", "info"))
    store.close()


def test_all_riders_on_one_window_at_once(ctx):
    """Leave-one-out values, the selection, the conditioned imputed SNPs, further traits and a mask of missing SNPs on one window:
    each output has the bits of the call that asks for it alone."""
    p, gm, gu = _window(129, 140, seed=77)
    M = 129
    z1 = _planted(gm, seed=6)
    rng = np.random.default_rng(12)
    z_more = rng.standard_normal((3, M)) * 2
    mask = np.zeros((3, M), dtype=np.uint8)
    mask[0, [3, 50]] = 1
    mask[2, [7]] = 1
    slct = _cond(dict(max=32, chi2_stop=CHI2_GWS))
    run = lambda **kw: hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, **kw)
    both = run(loo=True, slct=slct, z_more=z_more, miss_more=mask)
    _same(both, run(slct=slct))
    _same(both, run(loo=True), ("z", "info", "loo_z", "loo_info", "loo_t"))
    _same(both, run(z_more=z_more, miss_more=mask), ("z", "info", "z_more", "info_more", "z_miss", "info_miss"))
    assert both["slct_n"] >= 1 and np.isfinite(both["cond_z"]).any()


def test_refusals(ctx):
    """The conditional statistics condition on the selection: asking without slct_max is refused, and so are QCAT and LD windows; a
    window without unmeasured SNPs solves nothing and is refused as before."""
    p = small_panel(n_snp=120, scale=0.02, n_pops=5)
    gm, gu, z1 = split_window(p, 50)
    slct = _cond(dict(max=8, chi2_stop=4.0))
    base = dict(mode=0, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=None, z1=z1, slct=slct)
    with pytest.raises(Exception, match="need slct_max > 0"):
        hotpath.Job([dict(base, slct=_cond(dict(max=0, chi2_stop=4.0)))], ctx=ctx)
    with pytest.raises(Exception, match="need slct_max > 0"):
        hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, slct=_cond(dict(max=0)))
    with pytest.raises(Exception, match="imputation windows only"):
        hotpath.Job([dict(base, qcat=(10, 30, 0.01))], ctx=ctx)
    with pytest.raises(Exception, match="imputation windows only"):
        hotpath.Job([dict(base, ld_codings=1)], ctx=ctx)
    with pytest.raises(Exception, match="out_cond_z / out_cond_var.*QCAT"):        # also when the window does not select
        hotpath.Job([dict(base, qcat=(10, 30, 0.01), slct=_cond(dict(max=0)))], ctx=ctx)
    with pytest.raises(Exception, match="no unmeasured SNPs"):
        hotpath.Job([dict(base, geno_u=gu[:0])], ctx=ctx)
    with pytest.raises(Exception, match="unmeasured SNPs"):
        hotpath.impute_window(0, gm, gu[:0], p["off"], None, z1, ctx=ctx, slct=slct)
    ok = hotpath.Job([dict(base, qcat=(10, 30, 0.01), slct=None), base], ctx=ctx)      # a QCAT window beside one that asks
    ok.run()
    res = ok.fetch()
    ok.close()
    assert "r" in res[0] and "cond_z" in res[1]


# ---- the host entry points, files -> table -----------------------------------------------------------------------
POPS = [("AAA", 160, "EUR"), ("BBB", 145, "EUR"), ("CCC", 170, "ASN"), ("DDD", 133, "AFR"), ("EEE", 152, "EUR"), ("FFF", 90, "ASN")]
WGT = (["aaa", "CCC", "eee", "FFF", "zzz"], [0.45, 0.2, 0.25, 0.161, 0.3])
ADDED = ["wing", "order", "z_cond", "pval_cond", "var_left"]


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    d = tmp_path_factory.mktemp("cond_study")
    st = panel_mod.make_synthetic_study(str(d), POPS, n_snp=700, bp_lo=1_000_000, bp_hi=2_400_000, n_genes=40, frac_measured=0.3, seed=17)
    q = st["paths"]
    packed = os.path.join(os.path.dirname(q["data.gz"]), "panel.gpk")
    assert api.pack_panel(q["index.gz"], q["data.gz"], q["desc.txt"], packed) > 0
    return dict(files=(q["gwas.txt"], q["index.gz"], q["data.gz"], q["desc.txt"]), packed=packed)


def _feeder_window(mix, chr_, start_bp, end_bp, wing, who, files, cutoff):
    """The window as oracle/feeder_py.py's dist / distmix build it: measured and unmeasured SNPs (reference order), their matrices."""
    from oracle import feeder_py as fp
    inp, index, data, desc = files
    pops = fp.read_ref_desc(desc)
    flags, w = fp.pop_flags_wgt(pops, *who) if mix else (fp.pop_flags(pops, who), None)
    lo, hi = start_bp - wing, end_bp + wing
    m = fp.read_input_z(inp, chr_, lo, hi, False)
    fp.read_reference_index(m, index, chr_, lo, hi, False)
    vec = fp.make_snp_vec(m, data, flags, cutoff, w)
    meas = [s for s in vec if s.type == 1]
    unme = [s for s in vec if s.type == 0 and start_bp <= s.bp <= end_bp]
    return meas, unme, fp._matrix(meas), fp._matrix(unme), fp._selected_off(pops, flags), (None if w is None else np.asarray(w, dtype=np.float64))


def _same_column(a, b, c):
    if a[c].dtype.kind == "f":
        assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
    else:
        assert list(a[c]) == list(b[c]), c


@pytest.mark.parametrize("mix", [False, True])
def test_dist_cond_and_distmix_cond_end_to_end(ctx, study, mix, monkeypatch):
    """Text panel, packed panel (lean window on the resident rows) and the packed panel through the full SNP map: the same table.  Its
    first rows are dist() / distmix() of the same call bit for bit in the shared columns, the measured SNPs of the wings follow, the
    measured rows carry dist_slct()'s values by rsid bit for bit, and the imputed rows the values of the definition on the oracle's
    matrices of the oracle's data layer; conditioning SNPs by rsid."""
    import oracle
    win = (22, 1_500_000, 2_000_000, 300_000)
    who = WGT if mix else "EUR"
    cutoff = 0.02 if mix else 0.01
    fn, fn_slct, fn_plain = (api.distmix_cond, api.distmix_slct, api.distmix) if mix else (api.dist_cond, api.dist_slct, api.dist)
    inp, idx, dat, desc = study["files"]
    meas, unme, gm, gu, off, w = _feeder_window(mix, *win, who, study["files"], cutoff)
    z1 = np.array([s.z for s in meas])
    B, B21 = window_mats(1 if mix else 0, gm, gu, off, w)
    p_cut = 0.05
    stop = api.slct_chi2(p_cut)
    cond = [meas[4].rsid, meas[len(meas) - 2].rsid]                       # the second one sits in the right wing
    plain = fn_plain(*win, who, inp, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
    for forced, kmax in (((), None), ((4, len(meas) - 2), None), ((4, len(meas) - 2), 2)):
        kw = dict(af1_cutoff=cutoff, p_cutoff=p_cut, max_signals=kmax, cond_rsids=[cond[k] for k in range(len(forced))], ctx=ctx)
        df = fn(*win, who, inp, idx, dat, desc, **kw)
        sl = fn_slct(*win, who, inp, idx, dat, desc, **kw)
        assert list(df.columns) == list(plain.columns) + ADDED
        head = df.iloc[: len(plain)]
        for c in plain.columns:                                          # dist()'s rows, order and bits
            _same_column(head.reset_index(drop=True), plain, c)
        tail = df.iloc[len(plain):]
        wings = sl[sl["wing"] == 1]
        assert len(wings) > 0 and list(tail["rsid"]) == list(wings["rsid"]) and np.all(tail["type"] == 1) and np.all(tail["info"] == 1.0)
        by = {r: k for k, r in enumerate(df["rsid"])}
        at = np.array([by[r] for r in sl["rsid"]])                       # every measured SNP of the extended window has a row
        m_rows = df.iloc[at].reset_index(drop=True)
        for c in ["z", "wing", "order", "z_cond", "pval_cond", "var_left", "bp", "a1", "a2"]:
            _same_column(m_rows, sl, c)
        sig = df.attrs["signals"]
        n = int((sl["order"] > 0).sum())
        assert len(sig["row"]) == n and np.array_equal(df["order"].to_numpy()[sig["row"]], np.arange(1, n + 1))
        sel_rows = sl.iloc[[int(np.nonzero(sl["order"].to_numpy() == a)[0][0]) for a in range(1, n + 1)]]
        assert np.array_equal(sig["z_entry"], sel_rows["z_entry"].to_numpy()) and np.array_equal(sig["z_joint"], sel_rows["z_joint"].to_numpy())
        # the imputed rows against the definition on the oracle's window
        sel = slct_by_definition(B, z1, kmax or 32, stop, min_var_frac(0.9, 0.1), forced)
        assert sel["min_margin"] > MARGIN and sel["n"] == n and sel["n"] >= len(forced)
        want = cond_by_definition(B, B21, z1, sel["idx"], 0.1)
        assert want["margin"] > MARGIN
        u_rows = df.iloc[[by[s.rsid] for s in unme]]
        assert np.all(u_rows["type"] == 0) and np.all(u_rows["order"] == 0) and np.all(u_rows["wing"] == 0)
        e = dict(z_cond=_err(u_rows["z_cond"].to_numpy(), want["z"]), var_left=_err(u_rows["var_left"].to_numpy(), want["var"]))
        print(f"REACHED cond table mix={mix} forced={forced} K={kmax}: n {n}  U {len(unme)}  " + "  ".join(f"{k} {v:.3e}" for k, v in e.items()))
        assert max(e.values()) <= TOL, e
        pv, ok = u_rows["pval_cond"].to_numpy(), ~np.isnan(want["z"])
        wp = np.array([2 * oracle.pnorm_upper(abs(t)) for t in want["z"][ok]])
        assert np.array_equal(np.isnan(pv), ~ok) and np.max(np.abs(pv[ok] - wp) / wp) <= 1e-6
    forms = [fn(*win, who, inp, "(unused)", study["packed"], desc, af1_cutoff=cutoff, p_cutoff=p_cut, max_signals=2, cond_rsids=cond, ctx=ctx)]
    monkeypatch.setenv("GAUSS_HOST_FULL_MAP", "1")
    forms.append(fn(*win, who, inp, "(unused)", study["packed"], desc, af1_cutoff=cutoff, p_cutoff=p_cut, max_signals=2, cond_rsids=cond, ctx=ctx))
    for other in forms:
        assert list(other.columns) == list(df.columns) and len(other) == len(df)
        for c in df.columns:
            _same_column(df, other, c)
        assert all(np.array_equal(other.attrs["signals"][k], df.attrs["signals"][k]) for k in ("row", "z_entry", "z_joint"))
    with pytest.raises(Exception, match="rs_not_there"):
        fn(*win, who, inp, idx, dat, desc, af1_cutoff=cutoff, cond_rsids=[cond[0], "rs_not_there"], ctx=ctx)
    with pytest.raises(Exception, match="listed twice"):
        fn(*win, who, inp, idx, dat, desc, af1_cutoff=cutoff, cond_rsids=[cond[0], cond[0]], ctx=ctx)
