"""GPU: the credible sets of the selected signals (out_cs_* of gauss_window_desc, k_cs.hip) against tests/cs_ref.py.

Every value case asks for out_b11 / out_b21 and is compared with cs_ref.cs_by_definition evaluated ON THE MATRICES THE GPU RETURNED and
on the indices the GPU selected -- which are first checked against slct_ref.slct_by_definition, as tests/test_gpu_cond.py does.

Tolerances.  The project's bound for solve outputs is 1e-8 as |d| / max(1, |want|); it applies to the leave-one-out z, zc.  A log Bayes
factor then moves by at most |zc| dzc <= max(1, zc^2) 1e-8 and a pip by at most pip 2 |zc| dzc, so pip, set_pip, mass and lse are
held to 2 max(1, zmax^2) 1e-8 ABSOLUTE, zmax the case's largest |zc| in the reference (cs_ref.pip_tol: 2e-6 at zmax = 10).  size and
set are compared exactly on every SNP the reference does not call borderline (cs_ref.borderline with MARGIN = 1e-6 and that
tolerance); the committed seeds have NO borderline SNP (tests/test_cs_ref.py vets them on the CPU, and every case here asserts it
again on the GPU's matrices) -- the two identical measured rows of the twins' case, which are a tie built on purpose, are the one
exception: there alone `_check` is told to leave the SNPs the reference calls borderline out of the exact comparison.  At rho = 1
the mass ahead decides nothing and the members are compared with pip_ia > 0 directly.  Each case prints the level it reaches
(REACHED lines)."""
import os

import numpy as np
import pytest

import cs_ref
from gauss_amd import api, hotpath
from gauss_amd import panel as panel_mod
from cond_ref import window_mats
from cs_ref import CHI2_GWS, CS, borderline, cs_by_definition, pip_tol
from helpers import small_panel, split_window
from slct_ref import min_var_frac, slct_by_definition

pytestmark = pytest.mark.gpu

MARGIN = 1e-6
SEL_MARGIN = 1e-9
SLCT_KEYS = ("slct_idx", "slct_zin", "slct_joint", "slct_zc", "slct_var")
COND_KEYS = ("cond_z", "cond_var")
CS_KEYS = ("cs_pip", "cs_set", "cs_set_pip", "cs_size", "cs_mass", "cs_lse")


def _cs(slct, **kw):
    return dict(slct, cs=dict(CS, **kw))


def _same(a, b, keys):
    assert a["status"] == b["status"]
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _check(got, z1, slct, lam=0.1, what="", tie_built_on_purpose=False):
    """got: a window's result with b11 and b21; slct: the dict the window was given (with its cs key).  The selection against its
    definition (exact indices behind its margin), then the credible sets on those indices.  tie_built_on_purpose: the twins' case
    alone -- everywhere else a borderline SNP fails the test."""
    mvf_m, mvf_u = min_var_frac(slct.get("collin", 0.9), lam), slct.get("min_var_frac_u", 1.0 - slct.get("collin", 0.9))
    omega, rho = slct["cs"].get("prior_var", 25.0), slct["cs"].get("coverage", 0.95)
    sel = slct_by_definition(got["b11"], z1, slct["max"], slct["chi2_stop"], mvf_m, slct.get("forced", ()))
    assert sel["min_margin"] > SEL_MARGIN, (what, sel["min_margin"])
    assert got["slct_n"] == sel["n"] and np.array_equal(got["slct_idx"], sel["idx"]), (what, got["slct_idx"], sel["idx"])
    want = cs_by_definition(got["b11"], got["b21"], z1, got["slct_idx"], mvf_m, mvf_u, omega, rho)
    n, T, K = want["n"], len(want["pip"]), slct["max"]
    tol = pip_tol(want)
    bl = borderline(want, rho, MARGIN, tol)
    assert tie_built_on_purpose or not bl.any(), (what, np.argwhere(bl).tolist())
    for k in ("cs_pip", "cs_set", "cs_set_pip"):
        assert got[k].shape == (T,), (k, got[k].shape)
    raw = got["cs_raw"]
    assert raw["size"].shape == (K,) and np.all(raw["size"][n:] == 0) and np.all(np.isnan(raw["mass"][n:])) and np.all(np.isnan(raw["lse"][n:]))
    e = dict(pip=float(np.max(np.abs(got["cs_pip"] - want["pip"]), initial=0.0)),
             set_pip=float(np.max(np.abs(got["cs_set_pip"] - want["set_pip"])[~bl.any(axis=0)], initial=0.0)) if n else 0.0,
             mass=float(np.max(np.abs(got["cs_mass"] - want["mass"])[~bl.any(axis=1)], initial=0.0)) if n else 0.0,
             lse=float(np.max(np.abs(got["cs_lse"] - want["lse"]), initial=0.0)))
    print(f"REACHED cs {what}: n {n}  T {T}  sizes {want['size'].tolist()}  zmax {want['zmax']:.2f}  borderline {int(bl.sum())}  "
          + "  ".join(f"{k} {v:.3e}" for k, v in e.items()) + f"  (bound {tol:.3e})")
    assert max(e.values()) <= tol, (what, e, tol)
    firm = ~bl.any(axis=0)
    assert np.array_equal(got["cs_set"][firm], want["set"][firm]), (what, np.nonzero(got["cs_set"] != want["set"])[0])
    firm_a = ~bl.any(axis=1)
    assert np.array_equal(got["cs_size"][firm_a], want["size"][firm_a]), (what, got["cs_size"], want["size"])
    if n:
        assert np.all(got["cs_mass"][firm_a] >= rho - tol)
    else:
        assert np.array_equal(got["cs_pip"], np.zeros(T)) and np.all(got["cs_set"] == -1) and np.array_equal(got["cs_set_pip"], np.zeros(T))
    if n and rho >= 1.0 and not tie_built_on_purpose:
        # every candidate with pip > 0 is a member, whatever the rounded mass ahead of it: sizes and "in some set" from pip_ia alone
        live = want["pip_ia"] > 0
        assert np.array_equal(got["cs_size"], live.sum(axis=1)) and np.array_equal(got["cs_set"] >= 0, live.any(axis=0)), what
        assert np.array_equal(got["cs_set"], np.where(live.any(axis=0), np.argmax(want["pip_ia"], axis=0), -1)), what
    return sel, want


def _run(ctx, wins, on_device=True, runs=1, want_mats=False):
    job = hotpath.Job(wins, ctx=ctx, on_device=on_device, want_mats=want_mats)
    for _ in range(runs):
        job.run()
    out = [job.fetch() for _ in range(runs)]
    cnt = job.counters()
    job.close()
    return out, cnt


@pytest.mark.parametrize("M,U,mode,slct,zseed", cs_ref.EDGE_CASES)
def test_credible_sets_match_the_definition_at_the_kernel_edges(ctx, M, U, mode, slct, zseed):
    """T = M + U around the 128 candidates of a workgroup of cs_lbf_kernel (2, 5, 23, 255, 258, 553), the candidate blocks that
    straddle M, 4 096 and 4 119 candidates on either side of the row cs_set_kernel keeps in LDS, the chr22 study's largest window
    (M = 1 213, U = 2 512), pooled and weighted; n = 32 (chi2_stop = 0), a forced list, and planted signals at the genome-wide
    threshold.  z / info are the bits of the same call without the rider, the selection's and the conditional outputs the bits of
    the call without `cs`; asking without `unmeasured` (no out_cond_*) gives the same sets."""
    p, gm, gu, w, z1 = cs_ref.edge_window(M, U, mode, zseed)
    got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, want_mats=True, ctx=ctx, slct=_cs(slct))
    assert got["status"] == 0
    sel, want = _check(got, z1, _cs(slct), what=f"M={M} U={U} mode={mode} K={slct['max']} stop={slct['chi2_stop']:g}")
    if slct["chi2_stop"] == 0.0:
        assert sel["n"] == 32
    both = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, slct=dict(_cs(slct), unmeasured=True))
    _same(both, got, ("z", "info") + SLCT_KEYS + CS_KEYS)
    _same(both, hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, slct=dict(slct, unmeasured=True)), ("z", "info") + SLCT_KEYS + COND_KEYS)
    _same(got, hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx), ("z", "info"))


@pytest.mark.parametrize("cs", cs_ref.COVERAGE_CASES)
def test_coverage_and_prior_reach_the_kernel(ctx, cs):
    """rho = 0.5, rho = 1, omega = 4, and rho = 0.99 with omega = 100 on a window with nine signals: other sets than the defaults',
    each held to the definition with no borderline SNP.  At rho = 1 every candidate with pip > 0 is a member -- some 250 a set --
    although the rounded mass ahead of most of them is 1 (`_check` compares with pip_ia > 0 directly)."""
    M, U, mode, slct, zseed = cs_ref.COVERAGE_WINDOW
    p, gm, gu, w, z1 = cs_ref.edge_window(M, U, mode, zseed)
    got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, want_mats=True, ctx=ctx, slct=_cs(slct, **cs))
    sel, want = _check(got, z1, _cs(slct, **cs), what=f"{cs}")
    assert sel["n"] == 9
    if cs.get("coverage") == 1.0:
        assert got["cs_size"].min() > 100 and np.any(want["ahead"][want["member"]] >= 1.0)


def test_nothing_selected_returns_zeros_and_no_set(ctx):
    p, gm, gu = cs_ref.window(120, 130, seed=19)
    _, _, z1 = split_window(dict(G=p["G"][:250]), 120)
    slct = _cs(dict(max=32, chi2_stop=1e3))
    got = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, want_mats=True, ctx=ctx, slct=slct)
    assert got["slct_n"] == 0 and got["status"] == 0
    assert np.array_equal(got["cs_pip"], np.zeros(250)) and np.all(got["cs_set"] == -1) and np.array_equal(got["cs_set_pip"], np.zeros(250))
    assert got["cs_size"].shape == (0,) and np.all(got["cs_raw"]["size"] == 0) and np.all(np.isnan(got["cs_raw"]["mass"]))
    _check(got, z1, slct, what="nothing selected")


def test_twins(ctx):
    """An unmeasured exact copy of the lead SNP shares the set with it: with one signal nothing is conditioned on, the copy's zc is
    its imputed z and its share of variance its info, and its pip is the reference's.  Two identical measured rows that are not
    selected go through the same arithmetic: their pips have the same bits, and if exactly one of them is a member it is the one
    with the smaller index."""
    p, gm, gu2, z1, j = cs_ref.copy_of_the_lead_window()
    gu = np.ascontiguousarray(gu2[:-1])
    slct = _cs(dict(max=1, chi2_stop=0.0), coverage=0.99)
    got = hotpath.impute_window(0, gm, gu2, p["off"], None, z1, want_mats=True, ctx=ctx, slct=slct)
    sel, want = _check(got, z1, slct, what="unmeasured copy of the lead")
    assert sel["idx"].tolist() == [j]
    twin = 50 + gu2.shape[0] - 1
    assert want["member"][0, j] and want["member"][0, twin] and got["cs_set"][j] == 0 and got["cs_set"][twin] == 0
    assert abs(got["cs_pip"][twin] - want["pip"][twin]) <= pip_tol(want) and got["cs_pip"][twin] > 0.01
    print(f"REACHED cs twin: pip lead {got['cs_pip'][j]:.4f} copy {got['cs_pip'][twin]:.4f} (want {want['pip'][twin]:.4f})")
    # two identical measured rows beside the lead: the SNP most correlated with it (and admissible), duplicated at the end
    B, _ = window_mats(0, gm, gu, p["off"], None)
    r2 = B[j] ** 2
    r2[j] = 0
    k = int(np.argmax(np.where(r2 < 0.7, r2, 0)))
    gm2 = np.ascontiguousarray(np.vstack([gm, gm[k]]))
    z2 = np.append(z1, z1[k]) / 3.0                    # a weak lead (|z| about 3.5): the mass spreads over many SNPs
    cut = None                                         # a coverage that falls between the two: set from the reference at rho = 0.99
    for rho in (0.5, 0.99, 1.0, "cut"):
        rho = cut if rho == "cut" else rho
        slct = _cs(dict(max=1, chi2_stop=0.0, forced=[j]), coverage=rho)
        got = hotpath.impute_window(0, gm2, gu, p["off"], None, z2, want_mats=True, ctx=ctx, slct=slct)
        assert got["status"] == 0
        _, want = _check(got, z2, slct, what=f"measured twins rho={rho:.6f}", tie_built_on_purpose=True)
        if cut is None and rho == 0.99:
            assert want["ahead"][0, 50] == want["ahead"][0, k] + want["pip_ia"][0, k]
            cut = float(want["ahead"][0, k] + 0.5 * want["pip_ia"][0, k])
        elif rho == cut:
            assert got["cs_set"][k] == 0 and got["cs_set"][50] == -1, "exactly one of the two is a member: the smaller index"
        a, b = got["cs_pip"][k], got["cs_pip"][50]
        assert a == b and a > 0, (a, b)
        ina, inb = got["cs_set"][k] == 0, got["cs_set"][50] == 0
        assert not (inb and not ina), "of two tied SNPs the smaller index is ranked ahead"
        print(f"REACHED cs measured twins rho={rho}: pip {a:.3e} members {bool(ina)} {bool(inb)} size {got['cs_size'].tolist()}")


def test_clamped_nonfinite_and_nan_windows(ctx):
    """Duplicated measured SNPs at lambda = 0 (tests/test_gpu_cond.py's construction): MakePosDef rebuilds B11, selection and sets run
    again on the repaired matrix, which is the one the job returns.  A NaN in z1 makes every imputed z NaN: no unmeasured SNP is a
    candidate, nor is the measured SNP whose z is NaN; the others are.  A GAUSS_ST_NONFINITE window returns NaN, sizes 0, sets -1."""
    p, gm, gu, z1 = cs_ref.clamped_window()
    slct = _cs(dict(max=32, chi2_stop=4.0, unmeasured=True))
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, want_mats=True, ctx=ctx, slct=slct)
    assert got["status"] & 1
    _same(got, hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, ctx=ctx), ("z", "info"))
    no_cs = {k: v for k, v in slct.items() if k != "cs"}
    _same(got, hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, ctx=ctx, slct=no_cs), SLCT_KEYS + COND_KEYS)
    sel, _ = _check(got, z1, slct, lam=0.0, what="clamped window")
    assert sel["n"] >= 2
    p, gm, gu = cs_ref.window(65, 70, seed=5)
    z1 = cs_ref.planted(gm, seed=9)
    z1[13] = np.nan
    slct = _cs(dict(max=32, chi2_stop=CHI2_GWS))
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, want_mats=True, ctx=ctx, slct=slct)
    assert got["status"] == 0 and np.all(np.isnan(got["z"]))
    sel, want = _check(got, z1, slct, what="NaN in z1")
    assert sel["n"] >= 1 and np.all(got["cs_pip"][65:] == 0) and got["cs_pip"][13] == 0 and np.all(got["cs_set"][65:] == -1)
    assert np.all(np.isfinite(got["cs_pip"])) and np.all(np.isfinite(got["cs_lse"]))
    gm = gm.copy()
    gm[3, :] = 1                                       # zero variance: CalCor returns 0 / 0
    got = hotpath.impute_window(0, gm, gu, p["off"], None, np.nan_to_num(z1, nan=1.0), ctx=ctx, slct=slct)
    assert got["status"] & 2 and got["slct_n"] == 0
    assert got["cs_pip"].shape == (135,) and np.all(np.isnan(got["cs_pip"])) and np.all(np.isnan(got["cs_set_pip"])) and np.all(got["cs_set"] == -1)
    assert np.all(got["cs_raw"]["size"] == 0) and np.all(np.isnan(got["cs_raw"]["mass"])) and np.all(np.isnan(got["cs_raw"]["lse"]))


def _store_windows(ctx, **kw):
    """cs_ref.store_windows as windows over one resident 2-bit store (shared measured rows apply) and as byte rows in host memory."""
    p, ws = cs_ref.store_windows(**kw)
    G = p["G"]
    rows2, src_off = panel_mod.pack2bit(G, p["off"])
    store = hotpath.RowStore(rows2, ctx=ctx)
    wins, host = [], []
    for w in ws:
        mi, ui = w["mi"], w["ui"]
        wins.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=w["z1"], dev=(store.ptr, store.ptr, len(mi), len(ui), store.ld),
                         packed=dict(fmt=1, rows_m=mi, rows_u=ui, pop_src_off=src_off), slct=w["slct"]))
        host.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=w["z1"], geno_m=np.ascontiguousarray(G[mi]),
                         geno_u=np.ascontiguousarray(G[ui]), slct=w["slct"]))
    return p, rows2, src_off, store, wins, host


ALL_KEYS = ("z", "info") + SLCT_KEYS + COND_KEYS + CS_KEYS


def test_every_launch_form_and_source_format_returns_the_same_bits(ctx, monkeypatch):
    """The same job under each switch that changes a launch form or a source format (the list of tests/test_gpu_cond.py): the
    credible sets bit for bit those of the default -- z, info, the selection and B21 have the same bits in every form and the
    kernels' sums have a fixed order.  GAUSS_FUSED_SOLVE=0 (with the chain on the main queue, where the switch applies): z / info move
    within 1e-8, so the sets are held to the tolerance of their reference, not to bit equality; the job's counters are those of the
    same job with nobody asking (the rider does not force the fused form)."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx)
    ref = _run(ctx, wins, want_mats=True)[0][0]
    assert all(r["status"] == 0 for r in ref)
    wants = [_check(r, wins[k]["z1"], wins[k]["slct"], what=f"store window {k}")[1] for k, r in enumerate(ref)]
    switches = [dict(GAUSS_CHAIN_ASIDE="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2"),
                dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2", GAUSS_EPI_EARLY="0"),
                dict(GAUSS_SHARE_MEASURED="0"), dict(GAUSS_SHARE_MEASURED="2"), dict(GAUSS_NO_SHIFT_CERT="1")]
    for sw in switches:
        with monkeypatch.context() as m:
            for k, v in sw.items():
                m.setenv(k, v)
            for r, w in zip(_run(ctx, wins)[0][0], ref):
                _same(r, w, ALL_KEYS)
    with monkeypatch.context() as m:
        m.setenv("GAUSS_FUSED_SOLVE", "0")
        m.setenv("GAUSS_CHAIN_ASIDE", "0")
        alone, cnt_alone = _run(ctx, [dict(w, slct=None) for w in wins])
        asked, cnt_asked = _run(ctx, wins)
        assert cnt_asked == cnt_alone, (cnt_asked, cnt_alone)
        differs = False
        for r, w, a, want in zip(asked[0], ref, alone[0], wants):
            _same(r, w, SLCT_KEYS)
            _same(r, a, ("z", "info"))
            differs = differs or not np.array_equal(r["z"], w["z"])
            tol = pip_tol(want)
            e = [float(np.max(np.abs(r[k] - want[q]), initial=0.0)) for k, q in (("cs_pip", "pip"), ("cs_set_pip", "set_pip"), ("cs_mass", "mass"), ("cs_lse", "lse"))]
            print("REACHED cs behind the stand-alone solver: " + "  ".join(f"{v:.3e}" for v in e) + f"  (bound {tol:.3e})")
            assert max(e) <= tol
            assert np.array_equal(r["cs_set"], want["set"]) and np.array_equal(r["cs_size"], want["size"])
        assert differs, "the stand-alone solver's sums have another order: some bit of z differs from the fused form's"
    try:                                               # int8 Gram
        ctx.set_gram_dtype("i8")
        for r, w in zip(_run(ctx, wins)[0][0], ref):
            _same(r, w, ALL_KEYS)
    finally:
        ctx.set_gram_dtype(os.environ.get("GAUSS_GRAM_DTYPE", "f32"))
    for r, w in zip(_run(ctx, host, on_device=False)[0][0], ref):      # byte rows from host memory
        _same(r, w, ALL_KEYS)
    # the blocking window call: streamed (default) and upload-then-run
    h2 = host[2]
    _same(hotpath.impute_window(1, h2["geno_m"], h2["geno_u"], p["off"], p["w"], h2["z1"], ctx=ctx, slct=h2["slct"]), ref[2], ALL_KEYS)
    with monkeypatch.context() as m:
        m.setenv("GAUSS_STREAM_WINDOW", "0")
        _same(hotpath.impute_window(1, h2["geno_m"], h2["geno_u"], p["off"], p["w"], h2["z1"], ctx=ctx, slct=h2["slct"]), ref[2], ALL_KEYS)
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
    """Windows of one job may mix: window 1 selects and conditions without asking for sets.  The asking windows return what their
    stand-alone calls return, two runs in flight return the same values, the other outputs keep their bits, and a job in which
    nobody asks has the counters and the bits of the same job built without the key."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx, seed=43, spans=((0, 131), (97, 340), (211, 560)))
    no_cs = lambda s: {k: v for k, v in s.items() if k != "cs"}
    nobody, c0 = _run(ctx, [dict(w, slct=no_cs(w["slct"])) for w in wins], runs=2)
    mixed, c1 = _run(ctx, [dict(w, slct=(w["slct"] if k != 1 else no_cs(w["slct"]))) for k, w in enumerate(wins)], runs=2)
    plain, c2 = _run(ctx, [dict(w, slct=None) for w in wins], runs=2)
    assert c0 == c1 == c2, (c0, c1, c2)
    for run in mixed:
        for k, (r, w) in enumerate(zip(run, nobody[0])):
            _same(r, w, ("z", "info") + SLCT_KEYS + COND_KEYS)
            _same(r, plain[0][k], ("z", "info"))
            assert ("cs_pip" in r) == (k != 1)
            if k != 1:
                h = host[k]
                _same(r, hotpath.impute_window(1, h["geno_m"], h["geno_u"], p["off"], p["w"], h["z1"], ctx=ctx, slct=h["slct"]), ALL_KEYS)
    for r, w in zip(nobody[1], nobody[0]):
        _same(r, w, ("z", "info") + SLCT_KEYS + COND_KEYS)
    store.close()


def test_all_riders_on_one_window_at_once(ctx):
    """Leave-one-out values, the selection, the conditioned imputed SNPs, the credible sets, further traits and a mask of missing
    SNPs on one window: each output has the bits of the call that asks for it alone."""
    p, gm, gu = cs_ref.window(129, 140, seed=77)
    M = 129
    z1 = cs_ref.planted(gm, seed=6)
    rng = np.random.default_rng(12)
    z_more = rng.standard_normal((3, M)) * 2
    mask = np.zeros((3, M), dtype=np.uint8)
    mask[0, [3, 50]] = 1
    mask[2, [7]] = 1
    slct = _cs(dict(max=32, chi2_stop=CHI2_GWS, unmeasured=True))
    run = lambda **kw: hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, **kw)
    both = run(loo=True, slct=slct, z_more=z_more, miss_more=mask)
    _same(both, run(slct=slct), ALL_KEYS)
    _same(both, run(slct={k: v for k, v in slct.items() if k != "cs"}), ("z", "info") + SLCT_KEYS + COND_KEYS)
    _same(both, run(loo=True), ("z", "info", "loo_z", "loo_info", "loo_t"))
    _same(both, run(z_more=z_more, miss_more=mask), ("z", "info", "z_more", "info_more", "z_miss", "info_miss"))
    assert both["slct_n"] >= 1 and both["cs_size"].min() >= 1 and np.all(both["cs_mass"] >= 0.95 - 1e-5)


def test_refusals(ctx):
    """The sets are those of the selection: asking without slct_max is refused, and so are QCAT and LD windows, a coverage outside
    (0, 1] and a prior variance that is not positive and finite."""
    p = small_panel(n_snp=120, scale=0.02, n_pops=5)
    gm, gu, z1 = split_window(p, 50)
    slct = _cs(dict(max=8, chi2_stop=4.0))
    base = dict(mode=0, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=None, z1=z1, slct=slct)
    with pytest.raises(Exception, match="need slct_max > 0"):
        hotpath.Job([dict(base, slct=_cs(dict(max=0, chi2_stop=4.0)))], ctx=ctx)
    with pytest.raises(Exception, match="need slct_max > 0"):
        hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, slct=_cs(dict(max=0)))
    with pytest.raises(Exception, match="imputation windows only"):
        hotpath.Job([dict(base, qcat=(10, 30, 0.01))], ctx=ctx)
    with pytest.raises(Exception, match="imputation windows only"):
        hotpath.Job([dict(base, ld_codings=1)], ctx=ctx)
    with pytest.raises(Exception, match="out_cs_.*QCAT"):                  # also when the window does not select
        hotpath.Job([dict(base, qcat=(10, 30, 0.01), slct=_cs(dict(max=0)))], ctx=ctx)
    for bad in (0.0, 1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(Exception, match="cs_coverage"):
            hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, slct=_cs(dict(max=8, chi2_stop=4.0), coverage=bad))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(Exception, match="cs_prior_var"):
            hotpath.Job([dict(base, slct=_cs(dict(max=8, chi2_stop=4.0), prior_var=bad))], ctx=ctx)
    ok = hotpath.Job([dict(base, qcat=(10, 30, 0.01), slct=None), base], ctx=ctx)      # a QCAT window beside one that asks
    ok.run()
    res = ok.fetch()
    ok.close()
    assert "r" in res[0] and "cs_pip" in res[1] and "cond_z" not in res[1]


def test_an_imputed_causal_snp_leads_its_set_ahead_of_the_measured_lead(ctx):
    """The claim the rider rests on: a planted window whose causal SNP is unmeasured.  The selection takes a measured SNP for the
    signal; the signal's credible set ranks the imputed causal SNP first, ahead of that measured lead -- a set built from
    measured SNPs only would have missed it.  Asserted on the reference (tests/test_cs_ref.py, and here on the GPU's matrices) and
    on the GPU's output."""
    p, gm, gu, z1, u = cs_ref.claim_window()
    M = gm.shape[0]
    slct = _cs(dict(max=32, chi2_stop=CHI2_GWS))
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, want_mats=True, ctx=ctx, slct=slct)
    sel, want = _check(got, z1, slct, what="unmeasured causal SNP")
    k = int(want["set"][M + u])
    lead = int(sel["idx"][k])
    assert k >= 0 and int(np.argmax(want["pip_ia"][k])) == M + u and want["pip_ia"][k, M + u] > want["pip_ia"][k, lead]
    assert got["cs_set"][M + u] == k and got["cs_set"][lead] == k and got["cs_size"][k] == 2
    assert got["cs_set_pip"][M + u] > 0.9 > 0.1 > got["cs_set_pip"][lead] > 0
    assert np.all(got["cs_set_pip"][got["cs_set"] == k] <= got["cs_set_pip"][M + u])
    print(f"REACHED cs claim: set {k}  imputed SNP pip {got['cs_set_pip'][M + u]:.4f}  measured lead pip {got['cs_set_pip'][lead]:.4f}")


# ---- the host entry points, files -> table -----------------------------------------------------------------------
ADDED = ["pip", "cs", "cs_pip"]


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    files = cs_ref.study_files(tmp_path_factory.mktemp("cs_study"))
    packed = os.path.join(os.path.dirname(files[2]), "panel.gpk")
    assert api.pack_panel(files[1], files[2], files[3], packed) > 0
    return dict(files=files, packed=packed)


def _same_column(a, b, c):
    if a[c].dtype.kind == "f":
        assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
    else:
        assert list(a[c]) == list(b[c]), c


@pytest.mark.parametrize("mix", [False, True])
def test_dist_cs_and_distmix_cs_end_to_end(ctx, study, mix, monkeypatch):
    """Text panel, packed panel (lean window on the resident rows) and the packed panel through the full SNP map: the same table.  Its
    shared columns and `signals` are dist_cond() / distmix_cond() of the same call bit for bit; pip, cs, cs_pip and `sets` are the
    hotpath's result for the window the oracle's data layer builds, by rsid; coverage and prior reach the window."""
    win = cs_ref.STUDY_WINDOW
    fw = cs_ref.feeder_window(mix, study["files"])
    meas, unme, gm, gu, off, w, who, cutoff = (fw[k] for k in ("meas", "unme", "gm", "gu", "off", "w", "who", "cutoff"))
    fn, fn_cond = (api.distmix_cs, api.distmix_cond) if mix else (api.dist_cs, api.dist_cond)
    inp, idx, dat, desc = study["files"]
    z1 = np.array([s.z for s in meas])
    M = len(meas)
    p_cut = cs_ref.STUDY_P_CUT
    stop = api.slct_chi2(p_cut)
    cond = [meas[4].rsid, meas[M - 2].rsid]                               # the second one sits in the right wing
    for forced, kmax, cs in cs_ref.study_cases(M):
        kw = dict(af1_cutoff=cutoff, p_cutoff=p_cut, max_signals=kmax, cond_rsids=[cond[k] for k in range(len(forced))], ctx=ctx)
        df = fn(*win, who, inp, idx, dat, desc, **kw, **cs)
        dc = fn_cond(*win, who, inp, idx, dat, desc, **kw)
        assert list(df.columns) == list(dc.columns) + ADDED and len(df) == len(dc)
        for c in dc.columns:
            _same_column(df, dc, c)
        assert all(np.array_equal(df.attrs["signals"][k], dc.attrs["signals"][k]) for k in ("row", "z_entry", "z_joint"))
        slct = dict(max=kmax or 32, chi2_stop=stop, forced=list(forced), unmeasured=True, cs=dict(CS, **cs))
        hp = hotpath.impute_window(1 if mix else 0, gm, gu, off, w, z1, want_mats=True, ctx=ctx, slct=slct)
        _, want = _check(hp, z1, slct, what=f"table window mix={mix} forced={forced}")
        tol = pip_tol(want)
        by = {r: k for k, r in enumerate(df["rsid"])}
        rows = np.array([by[s.rsid] for s in meas] + [by[s.rsid] for s in unme])          # every candidate has a row
        assert len(set(rows.tolist())) == len(rows) == len(df)
        e = dict(pip=float(np.max(np.abs(df["pip"].to_numpy()[rows] - hp["cs_pip"]))), cs_pip=float(np.max(np.abs(df["cs_pip"].to_numpy()[rows] - hp["cs_set_pip"]))))
        assert np.array_equal(df["cs"].to_numpy()[rows], hp["cs_set"] + 1)
        sets, n = df.attrs["sets"], hp["slct_n"]
        assert len(sets["row"]) == n and np.array_equal(sets["row"], df.attrs["signals"]["row"]) and np.array_equal(sets["size"], hp["cs_size"])
        assert np.array_equal(df["order"].to_numpy()[sets["row"]], np.arange(1, n + 1))
        e.update(mass=float(np.max(np.abs(sets["mass"] - hp["cs_mass"]))), lse=float(np.max(np.abs(sets["lse"] - hp["cs_lse"]))))
        print(f"REACHED cs table mix={mix} forced={forced}: n {n}  " + "  ".join(f"{k} {v:.3e}" for k, v in e.items()) + f"  (bound {tol:.3e})")
        assert max(e.values()) <= tol, e
    forms = [fn(*win, who, inp, "(unused)", study["packed"], desc, **kw, **cs)]
    monkeypatch.setenv("GAUSS_HOST_FULL_MAP", "1")
    forms.append(fn(*win, who, inp, "(unused)", study["packed"], desc, **kw, **cs))
    forms.append(fn(*win, who, inp, idx, dat, desc, **kw, **cs))
    for other in forms:
        assert list(other.columns) == list(df.columns) and len(other) == len(df)
        for c in df.columns:
            _same_column(df, other, c)
        assert all(np.array_equal(other.attrs["sets"][k], df.attrs["sets"][k]) for k in ("row", "size", "mass", "lse"))
    with pytest.raises(Exception, match="cs_coverage"):
        fn(*win, who, inp, idx, dat, desc, af1_cutoff=cutoff, coverage=1.5, ctx=ctx)
