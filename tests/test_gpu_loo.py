"""GPU: leave-one-out re-imputation of the measured SNPs (out_loo_* of gauss_window_desc, k_loo.hip) against the oracle.

Bounds are those of tests/test_gpu_parity.py against the oracle: info relative <= 1e-8, z and t as |d| / max(1, |want|) <= 1e-8,
1e-5 for windows MakePosDef repaired.  References: tests/loo_ref.py (deletion through the oracle; closed form in LAPACK)."""
import numpy as np
import pytest

import oracle
from gauss_amd import api, hotpath, synth
from gauss_amd import panel as panel_mod
from helpers import relerr, small_panel, split_window
from loo_ref import loo_by_deletion, loo_closed_form, window_b11

pytestmark = pytest.mark.gpu

Z_TOL = 1e-8
CLAMP_TOL = 1e-5
KEYS = ("loo_z", "loo_info", "loo_t")


def _zerr(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _check(got, want, tol, what=""):
    """got: a window's result dict; want: dict(z, info, t) of loo_ref.  Prints every figure before it asserts."""
    e = (relerr(got["loo_info"], want["info"]), _zerr(got["loo_z"], want["z"]), _zerr(got["loo_t"], want["t"]))
    print(f"loo {what}: info rel {e[0]:.3e}  z {e[1]:.3e}  t {e[2]:.3e}  (bound {tol:g})")
    assert e[0] <= tol and e[1] <= tol and e[2] <= tol, (what, e)


def _same(a, b, keys=("z", "info") + KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M", [2, 63, 64, 65, 129, 300])
def test_loo_matches_deletion_on_both_sides_of_the_block_edges(ctx, mode, M):
    """Every measured SNP deleted in turn and imputed by the oracle (pooled and weighted LD), M around the 64-row block and
    panel edges of L^-1; z / info of the unmeasured SNPs are the bits of the same call without leave-one-out."""
    p = small_panel(n_snp=M + 90, scale=0.02, seed=11 + M)
    gm, gu, z1 = split_window(dict(G=p["G"][: M + 60]), M)
    w = p["w"] if mode else None
    got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, loo=True)
    plain = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx)
    assert got["status"] == 0
    _same(got, plain, ("z", "info"))
    idx = np.arange(0, M, 10) if (mode == 1 and M >= 300) else np.arange(M)       # (the weighted numpy oracle is slow at M = 300)
    want = loo_by_deletion(mode, gm, p["off"], w, z1, idx=idx)
    assert want["mpd"] == 0
    _check({k: got[k][idx] for k in KEYS}, want, Z_TOL, f"M={M} mode={mode} deletion")
    _check(got, loo_closed_form(window_b11(mode, gm, p["off"], w), z1), Z_TOL, f"M={M} mode={mode} closed form")


def test_one_measured_snp(ctx):
    p = small_panel(n_snp=60, scale=0.01, n_pops=4)
    gm, gu, z1 = split_window(p, 1)
    for lam in (0.1, 0.5):
        got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=lam, ctx=ctx, loo=True)
        assert got["loo_info"][0] == 0.0 and np.isnan(got["loo_z"][0])
        assert abs(got["loo_t"][0] - z1[0] / np.sqrt(1 + lam)) <= Z_TOL * max(1.0, abs(z1[0]))


def test_clamped_window_uses_the_repaired_matrix(ctx):
    """Duplicated measured SNPs at lambda = 0: MakePosDef rebuilds B11 (status bit), and the leave-one-out values are those of
    the closed form on the ORACLE's repaired B11."""
    p = small_panel(n_snp=70, scale=0.02, n_pops=6, seed=21)
    gm, gu, z1 = split_window(p, 30)
    gm = np.ascontiguousarray(np.vstack([gm, gm[:3]]))
    z1 = np.concatenate([z1, z1[:3] + 0.3])
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, ctx=ctx, loo=True)
    plain = hotpath.impute_window(0, gm, gu, p["off"], None, z1, lam=0.0, ctx=ctx)
    want = oracle.run_impute(0, gm, gu, p["off"], None, z1, lam=0.0, want_mats=True)
    assert want["mpd"] == 1 and got["status"] & 1
    _same(got, plain, ("z", "info"))
    _check(got, loo_closed_form(want["b11"], z1), CLAMP_TOL, "clamped window")


@pytest.mark.parametrize("mode", [0, 1])
def test_clamped_window_of_several_factor_blocks(ctx, mode):
    """The same repair at M = 155 = 3 factor blocks and 3 panels of [X | y]: the rows of L^-1 ride through the update launches
    of the window's own re-factorisation, alone and inside a job whose other windows need no repair (their bits do not move)."""
    p = small_panel(n_snp=260, scale=0.02, seed=23)
    gm, gu, z1 = split_window(dict(G=p["G"][:230]), 150)
    gm = np.ascontiguousarray(np.vstack([gm, gm[[3, 70, 131, 140, 149]]]))
    z1 = np.concatenate([z1, z1[[3, 70, 131, 140, 149]] - 0.2])
    w = p["w"] if mode else None
    got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, lam=0.0, ctx=ctx, loo=True)
    plain = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, lam=0.0, ctx=ctx)
    want = oracle.run_impute(mode, gm, gu, p["off"], w, z1, lam=0.0, want_mats=True)
    assert want["mpd"] == 1 and got["status"] & 1
    _same(got, plain, ("z", "info"))
    _check(got, loo_closed_form(want["b11"], z1), CLAMP_TOL, f"clamped window, M = 155, mode {mode}")
    ok = dict(mode=mode, geno_m=gm[:150], geno_u=gu, pop_off=p["off"], pop_wgt=w, z1=z1[:150], loo=True)
    bad = dict(mode=mode, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=w, z1=z1, lam=0.0, loo=True)
    alone = _run(ctx, [ok], on_device=False)[0][0]
    res = _run(ctx, [ok, bad, ok], on_device=False, runs=2)
    for run in res:
        assert run[0]["status"] == 0 and run[1]["status"] & 1
        _same(run[0], alone)
        _same(run[2], alone)
        _same(run[1], got)


def test_nonfinite_window_is_all_nan(ctx):
    p = small_panel(n_snp=60, scale=0.01, n_pops=4)
    gm, gu, z1 = split_window(p, 25)
    gm = gm.copy()
    gm[3, :] = 1                                   # zero variance: CalCor returns 0 / 0
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, loo=True)
    assert got["status"] & 2
    for k in KEYS:
        assert got[k].shape == (25,) and np.all(np.isnan(got[k])), k


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
    z = rng.standard_normal(n)
    wins, host = [], []
    for a, b in spans:
        mi = measured[a:b]
        lo, hi = mi[len(mi) // 4], mi[3 * len(mi) // 4]
        ui = unmeasured[(unmeasured > lo) & (unmeasured < hi)]
        wins.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=z[mi], dev=(store.ptr, store.ptr, len(mi), len(ui), store.ld),
                         packed=dict(fmt=1, rows_m=mi.astype(np.int32), rows_u=ui.astype(np.int32), pop_src_off=src_off)))
        host.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=z[mi], geno_m=np.ascontiguousarray(G[mi]),
                         geno_u=np.ascontiguousarray(G[ui])))
    return p, rows2, src_off, store, wins, host


def _run(ctx, wins, on_device=True, runs=1):
    job = hotpath.Job(wins, ctx=ctx, on_device=on_device)
    for _ in range(runs):
        job.run()
    out = [job.fetch() for _ in range(runs)]
    job.close()
    return out


def test_every_launch_form_and_source_format_returns_the_same_bits(ctx, monkeypatch):
    """The same job under each switch that changes a launch form or a source format: leave-one-out values, z and info bit for
    bit those of the default.  GAUSS_FUSED_SOLVE=0: a job with an asking window keeps the fused chain (the values are read off
    the rows of L^-1, which the stand-alone solver does not form), so that leg proves the switch is overridden -- the same
    bits, which the 1e-8 bound then holds trivially -- and that the job agrees within 1e-8 with the same windows NOT asking,
    which do take the stand-alone solver under the switch."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx)
    wins = [dict(w, loo=True) for w in wins]
    host = [dict(w, loo=True) for w in host]
    wins[4] = dict(wins[4], lam=1e-7)              # no certificate: the shifted matrix is factored too
    host[4] = dict(host[4], lam=1e-7)
    ref = _run(ctx, wins)[0]
    assert all(r["status"] == 0 for r in ref[:4])

    def _same(a, b):                               # (the status too: window 4 sits at the edge of MakePosDef's floor)
        assert a["status"] == b["status"]
        for k in ("z", "info") + KEYS:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    # against the oracle once, so that "the same bits" are the right ones
    _check(ref[0], loo_closed_form(window_b11(1, host[0]["geno_m"], p["off"], p["w"]), host[0]["z1"]), Z_TOL, "store window 0")
    switches = [dict(GAUSS_CHAIN_ASIDE="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2"),
                dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2", GAUSS_EPI_EARLY="0"),
                dict(GAUSS_SHARE_MEASURED="0"), dict(GAUSS_SHARE_MEASURED="2"), dict(GAUSS_NO_SHIFT_CERT="1")]
    for sw in switches:
        with monkeypatch.context() as m:
            for k, v in sw.items():
                m.setenv(k, v)
            for r, w in zip(_run(ctx, wins)[0], ref):
                _same(r, w)
    with monkeypatch.context() as m:
        m.setenv("GAUSS_FUSED_SOLVE", "0")
        for k, (r, w) in enumerate(zip(_run(ctx, wins)[0], ref)):
            _check(r, dict(z=w["loo_z"], info=w["loo_info"], t=w["loo_t"]), Z_TOL, f"GAUSS_FUSED_SOLVE=0 window {k}")
            assert relerr(r["info"], w["info"]) <= Z_TOL and _zerr(r["z"], w["z"]) <= Z_TOL
            _same(r, w)                                      # the asking job kept the fused chain
        standalone = _run(ctx, [dict(w, loo=False) for w in wins])[0]      # nobody asks: the stand-alone solver
        for k, (r, w) in enumerate(zip(standalone, ref)):
            e = (relerr(r["info"], w["info"]), _zerr(r["z"], w["z"]))
            print(f"stand-alone solver against the asking job, window {k}: info rel {e[0]:.3e}  z {e[1]:.3e}")
            assert r["status"] == w["status"] and e[0] <= Z_TOL and e[1] <= Z_TOL
    # int8 Gram
    try:
        ctx.set_gram_dtype("i8")
        for r, w in zip(_run(ctx, wins)[0], ref):
            _same(r, w)
    finally:
        import os
        ctx.set_gram_dtype(os.environ.get("GAUSS_GRAM_DTYPE", "f32"))
    # byte rows from host memory instead of 2-bit rows of the resident store
    for r, w in zip(_run(ctx, host, on_device=False)[0], ref):
        _same(r, w)
    # the blocking window call: streamed (default) and upload-then-run
    one = hotpath.impute_window(1, host[2]["geno_m"], host[2]["geno_u"], p["off"], p["w"], host[2]["z1"], ctx=ctx, loo=True)
    _same(one, ref[2])
    with monkeypatch.context() as m:
        m.setenv("GAUSS_STREAM_WINDOW", "0")
        _same(hotpath.impute_window(1, host[2]["geno_m"], host[2]["geno_u"], p["off"], p["w"], host[2]["z1"], ctx=ctx, loo=True), ref[2])
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
                    _same(r, w)
                st2.close()
            finally:
                c.close()
    store.close()


def test_asking_and_not_asking_windows_share_a_job_and_two_runs_in_flight(ctx):
    """Windows of one job may mix: nobody's z / info moves by a bit when some windows ask, and two runs in flight return the
    values of run-fetch-run-fetch."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx, seed=43)
    nobody = _run(ctx, wins)[0]
    mixed = [dict(w, loo=(k % 2 == 0)) for k, w in enumerate(wins)]
    got = _run(ctx, mixed, runs=2)
    everybody = _run(ctx, [dict(w, loo=True) for w in wins])[0]
    for run in got:
        for k, (r, w) in enumerate(zip(run, nobody)):
            _same(r, w, ("z", "info"))
            assert ("loo_t" in r) == (k % 2 == 0)
            if k % 2 == 0:
                _same(r, everybody[k])
    for r, w in zip(everybody, nobody):
        _same(r, w, ("z", "info"))
    _check(got[0][2], loo_closed_form(window_b11(1, host[2]["geno_m"], p["off"], p["w"]), host[2]["z1"]), Z_TOL, "mixed job window 2")
    store.close()


def test_give_up_rerun_inside_the_fetch_returns_the_same_values(ctx, monkeypatch):
    """A merged Gram launch whose chain queue gives up waiting (the library's test hook: a wait for a count that never comes,
    bounded at 2 ms) is queued again in the two-launch form inside gauss_job_fetch: the leave-one-out values come back with
    that re-run, bit for bit those of an undisturbed run, also with two such runs in flight."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx, seed=47)
    wins = [dict(w, loo=(k != 1)) for k, w in enumerate(wins)]
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
        for k, (r, w) in enumerate(zip(res, ref)):
            assert r["status"] == w["status"] == 0
            _same(r, w, ("z", "info") + (KEYS if k != 1 else ()))
    store.close()


def _rand_geno(rng, n, N):
    f = rng.uniform(0.05, 0.95, size=(n, 1))
    return ((rng.random((n, N)) < f).astype(np.uint8) + (rng.random((n, N)) < f).astype(np.uint8))


def test_full_size_window(ctx):
    """The dist(EUR) shape of the largest chr22 window (tests/test_gpu_edges.py): N = 20 281 pooled, M = 1 213 = 19 factor
    blocks, U = 2 583.  Closed form on the window's own exported B11 for every SNP, deletion through the oracle for 16."""
    pops = [q for q in synth.POPS_33KG if q[2] == "EUR"]
    off = synth.pop_offsets([q[1] for q in pops])
    N = int(off[-1])
    rng = np.random.default_rng(99)
    M, U = 1213, 2583
    base = _rand_geno(rng, 220, N)
    G = base[rng.integers(0, 220, size=M + U)].copy()
    noise = rng.random(G.shape) < 0.4
    G[noise] = _rand_geno(rng, 1, N)[0][np.nonzero(noise)[1]]
    gm, gu = np.ascontiguousarray(G[:M]), np.ascontiguousarray(G[M:])
    z1 = rng.standard_normal(M) * 2
    got = hotpath.impute_window(0, gm, gu, off, None, z1, want_mats=True, ctx=ctx, loo=True)
    assert got["status"] == 0
    _check(got, loo_closed_form(got["b11"], z1), Z_TOL, "full size, closed form on out_b11")
    idx = np.sort(rng.choice(M, size=16, replace=False))
    want = loo_by_deletion(0, gm, off, None, z1, idx=idx)
    assert want["mpd"] == 0
    _check({k: got[k][idx] for k in KEYS}, want, Z_TOL, "full size, 16 deletions")


def test_planted_sign_flip_has_the_largest_residual(ctx):
    """A block of SNPs in strong LD whose Z-scores follow the LD; one of them has its sign flipped (the allele mix-up the
    check is for): its |t| is the window's largest."""
    rng = np.random.default_rng(7)
    N, M, U = 1500, 90, 40
    off = np.array([0, N], dtype=np.int32)
    block = _rand_geno(rng, 1, N)[0]
    G = _rand_geno(rng, M + U, N)
    for r in list(range(20, 32)) + [M + 3, M + 4]:                    # twelve measured SNPs (and two unmeasured) copy the block, 3 % noise
        flip = rng.random(N) < 0.03
        G[r] = np.where(flip, G[r], block)
    gm, gu = np.ascontiguousarray(G[:M]), np.ascontiguousarray(G[M:])
    z1 = rng.standard_normal(M)
    z1[20:32] = 6.0 + 0.2 * rng.standard_normal(12)                   # a real signal shared by the block
    z1[25] = -z1[25]
    got = hotpath.impute_window(0, gm, gu, off, None, z1, ctx=ctx, loo=True)
    assert got["status"] == 0
    assert int(np.argmax(np.abs(got["loo_t"]))) == 25
    assert abs(got["loo_t"][25]) > 8 and got["loo_z"][25] > 3         # the others say +6 where the study says -6


def test_refusals(ctx):
    """Only imputation windows may ask; a window without unmeasured SNPs solves nothing and is refused as before."""
    p = small_panel(n_snp=120, scale=0.02, n_pops=5)
    gm, gu, z1 = split_window(p, 50)
    base = dict(mode=0, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=None, z1=z1, loo=True)
    with pytest.raises(Exception, match="imputation windows only"):
        hotpath.Job([dict(base, qcat=(10, 30, 0.01))], ctx=ctx)
    with pytest.raises(Exception, match="imputation windows only"):
        hotpath.Job([dict(base, ld_codings=1)], ctx=ctx)
    with pytest.raises(Exception, match="no unmeasured SNPs"):
        hotpath.Job([dict(base, geno_u=gu[:0])], ctx=ctx)
    with pytest.raises(Exception, match="unmeasured SNPs"):
        hotpath.impute_window(0, gm, gu[:0], p["off"], None, z1, ctx=ctx, loo=True)
    ok = hotpath.Job([dict(base, qcat=(10, 30, 0.01), loo=False), base], ctx=ctx)      # a QCAT window beside one that asks
    ok.run()
    res = ok.fetch()
    ok.close()
    assert "r" in res[0] and "loo_t" in res[1]


# ---- the host entry points, files -> table -----------------------------------------------------------------------
POPS = [("AAA", 160, "EUR"), ("BBB", 145, "EUR"), ("CCC", 170, "ASN"), ("DDD", 133, "AFR"), ("EEE", 152, "EUR"), ("FFF", 90, "ASN")]
WGT = (["aaa", "CCC", "eee", "FFF", "zzz"], [0.45, 0.2, 0.25, 0.161, 0.3])


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    d = tmp_path_factory.mktemp("loo_study")
    st = panel_mod.make_synthetic_study(str(d), POPS, n_snp=700, bp_lo=1_000_000, bp_hi=2_400_000, n_genes=40, frac_measured=0.3, seed=17)
    import os
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
def test_dist_loo_and_distmix_loo_end_to_end(ctx, study, mix, monkeypatch):
    """Text panel, packed panel (lean window on the resident rows) and the packed panel through the full SNP map: the same table,
    which lists the measured SNPs of [start_bp, end_bp] in the reference's order with the oracle's leave-one-out values."""
    win = (22, 1_500_000, 2_000_000, 300_000)
    who = WGT if mix else "EUR"
    cutoff = 0.02 if mix else 0.01
    fn = api.distmix_loo if mix else api.dist_loo
    inp, idx, dat, desc = study["files"]
    df = fn(*win, who, inp, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
    afcol = "af1mix" if mix else "af1ref"
    assert list(df.columns) == ["rsid", "chr", "bp", "a1", "a2", afcol, "z", "z_loo", "info_loo", "t", "pval"]
    meas, gm, off, w = _feeder_window(mix, *win, who, study["files"], cutoff)
    z1 = np.array([s.z for s in meas])
    inside = [k for k, s in enumerate(meas) if win[1] <= s.bp <= win[2]]
    assert 0 < len(inside) < len(meas)                       # the wings hold measured SNPs that are not listed
    assert list(df["rsid"]) == [meas[k].rsid for k in inside] and list(df["bp"]) == [meas[k].bp for k in inside]
    assert list(df["a1"]) == [meas[k].a1 for k in inside] and list(df["a2"]) == [meas[k].a2 for k in inside]
    assert np.array_equal(df["z"].to_numpy(), z1[inside])
    assert np.array_equal(df[afcol].to_numpy(), np.array([(meas[k].af1mix if mix else meas[k].af1ref) for k in inside]))
    want = loo_by_deletion(1 if mix else 0, gm, off, w, z1, idx=np.array(inside))
    assert want["mpd"] == 0
    _check(dict(loo_z=df["z_loo"].to_numpy(), loo_info=df["info_loo"].to_numpy(), loo_t=df["t"].to_numpy()), want, Z_TOL,
           f"{'distmix' if mix else 'dist'}_loo table")
    wp = np.array([2 * oracle.pnorm_upper(abs(t)) for t in df["t"].to_numpy()])
    assert np.max(np.abs(df["pval"].to_numpy() - wp) / wp) <= 1e-6
    forms = [fn(*win, who, inp, "(unused)", study["packed"], desc, af1_cutoff=cutoff, ctx=ctx)]
    monkeypatch.setenv("GAUSS_HOST_FULL_MAP", "1")
    forms.append(fn(*win, who, inp, "(unused)", study["packed"], desc, af1_cutoff=cutoff, ctx=ctx))
    for other in forms:
        assert list(other.columns) == list(df.columns) and len(other) == len(df)
        for c in df.columns:
            if df[c].dtype.kind == "f":
                assert np.array_equal(df[c].to_numpy(), other[c].to_numpy(), equal_nan=True), c
            else:
                assert list(df[c]) == list(other[c]), c
