"""GPU: further traits that lack some of the window's measured SNPs (miss_more / out_info_more / out_z_miss / out_info_miss of
gauss_window_desc, k_traits_miss.hip) against the oracle.

Bounds are those of tests/test_gpu_traits.py: |d| / max(1, |want|) <= 1e-8, and 1e-5 where MakePosDef repaired the matrix.  The
downdate in LAPACK against one oracle run per trait gave <= 4e-14 on the CPU (tests/test_traits_miss_host.py, the same windows): an
error anywhere near the bound is a finding.  References: tests/traits_miss_ref.py."""
import os

import numpy as np
import pytest

import oracle
from gauss_amd import hotpath
from gauss_amd import panel as panel_mod
from helpers import small_panel, split_window
from traits_miss_ref import cyclic_mask, miss_by_oracle, miss_closed_form, random_mask

pytestmark = pytest.mark.gpu

Z_TOL = 1e-8
CLAMP_TOL = 1e-5
KEYS = ("z_more", "info_more", "z_miss", "info_miss")


def _zerr(got, want):
    at = ~np.isnan(want)
    assert got.shape == want.shape and np.array_equal(at, ~np.isnan(got)), (got.shape, want.shape)
    return float(np.max(np.abs(got[at] - want[at]) / np.maximum(1.0, np.abs(want[at])))) if at.any() else 0.0


def _check(got, want, tol, what=""):
    """got: a window's result; want: a reference's dict(z, info, z_miss, info_miss).  Prints the figures before it asserts."""
    errs = {k: _zerr(got[k], want[r]) for k, r in zip(KEYS, ("z", "info", "z_miss", "info_miss"))}
    print(f"traits miss {what}: " + "  ".join(f"{k} {e:.3e}" for k, e in errs.items()) + f"  (bound {tol:g})")
    assert max(errs.values()) <= tol, (what, errs)


def _same(a, b, keys):
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


def _nested(M, E):
    """trait t lacks E[0 .. t]"""
    mask = np.zeros((len(E), M), dtype=np.uint8)
    for t in range(len(E)):
        mask[t, E[: t + 1]] = 1
    return mask


def _mixed_15(M):
    """0 / 1 / 5 mixed over a union of 15: three traits lack five each, five lack one of those, seven lack nothing"""
    E = np.sort(np.random.default_rng(4).choice(M, size=15, replace=False))
    mask = np.zeros((15, M), dtype=np.uint8)
    for a, t in enumerate((1, 6, 12)):
        mask[t, E[5 * a: 5 * a + 5]] = 1
    for a, t in enumerate((0, 3, 7, 9, 14)):
        mask[t, E[3 * a]] = 1
    return mask


# (M, U, T, mask, |E|): M around the 64-row blocks of L^-1, U on both sides of the 64-row strip, |E| on both sides of the 16-column tiles
# and of the 64-column groups, k up to the limit
def _cases():
    yield 12, 20, 1, random_mask(1, 12, [1], seed=1), 1
    yield 63, 65, 15, _mixed_15(63), 15
    yield 64, 130, 16, _nested(64, np.sort(np.random.default_rng(2).choice(64, size=16, replace=False))), 16
    yield 65, 63, 17, _nested(65, np.concatenate([[0], np.sort(np.random.default_rng(3).choice(np.arange(1, 63), size=14, replace=False)), [63, 64]])), 17
    for n in (63, 64, 65):
        yield 129, 65, 63, cyclic_mask(129, [31 + (t % 2) for t in range(63)], n, seed=n), n
    yield 300, 130, 17, cyclic_mask(300, [32] * 17, 128, seed=8), 128
    yield 129, 130, 1, random_mask(1, 129, [32], seed=6), 32


CASES = list(_cases())


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M,U,T,mask,n_union", CASES, ids=[f"M{c[0]}-U{c[1]}-T{c[2]}-E{c[4]}" for c in CASES])
def test_every_masked_trait_matches_its_own_oracle_run(ctx, mode, M, U, T, mask, n_union):
    """One oracle run per trait on its own measured set (pooled and weighted LD), and the downdate in LAPACK on the oracle's b11 / b21
    of the full set; MakePosDef acts on neither side."""
    assert mask.shape == (T, M) and int(mask.any(axis=0).sum()) == n_union and mask.sum(axis=1).max() <= 32
    p, gm, gu, z1 = _window(M, U)
    w = p["w"] if mode else None
    Z = _traits(T, M, seed=M + T)
    got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, z_more=Z, miss_more=mask)
    want = miss_by_oracle(mode, gm, gu, p["off"], w, Z, mask)
    mats = oracle.run_impute(mode, gm, gu, p["off"], w, z1, want_mats=True)
    assert got["status"] == 0 and want["mpd"] == 0 and mats["mpd"] == 0
    _check(got, want, Z_TOL, f"M={M} U={U} T={T} |E|={n_union} mode={mode} oracle")
    _check(got, miss_closed_form(mats["b11"], mats["b21"], Z, mask), Z_TOL, f"M={M} U={U} T={T} |E|={n_union} mode={mode} closed form")


@pytest.fixture(scope="module")
def placed():
    """One window and its oracle matrices, shared by the placement cases."""
    M, U = 200, 65
    p, gm, gu, z1 = _window(M, U)
    mats = oracle.run_impute(0, gm, gu, p["off"], None, z1, want_mats=True)
    assert mats["mpd"] == 0
    return p, gm, gu, z1, mats, _traits(63, M, seed=12)


@pytest.mark.parametrize("n_union", [15, 16, 17, 63, 64, 65, 128])
def test_every_column_of_the_inverse_lands_in_its_own_place(ctx, placed, n_union):
    """Up to 63 unions: every trait lacks a single SNP (n_union of them distinct, the other traits share one of those); above: every trait
    lacks three, walking round the union so that later traits share SNPs with earlier ones.  z_miss, info_miss and the info rows entry by entry against the closed
    form: the entries of A[:, E] differ from column to column, so a permuted column cannot pass."""
    p, gm, gu, z1, mats, Z = placed
    M = gm.shape[0]
    if n_union <= 63:
        E = np.random.default_rng(n_union).permutation(M)[:n_union]                 # not sorted: trait order is not SNP order
        mask = np.zeros((63, M), dtype=np.uint8)
        mask[np.arange(63), E[np.arange(63) % n_union]] = 1
    else:
        mask = cyclic_mask(M, [3] * 63, n_union, seed=n_union)
    assert int(mask.any(axis=0).sum()) == n_union
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, z_more=Z, miss_more=mask)
    assert got["status"] == 0
    want = miss_closed_form(mats["b11"], mats["b21"], Z, mask)
    _check(got, want, Z_TOL, f"placement |E|={n_union}")
    vals = want["info_miss"][mask != 0]
    assert len(np.unique(np.round(vals, 9))) >= min(n_union, 60)                     # the reference itself tells the columns apart


def test_nothing_else_moves(ctx):
    """z, info, the status, the leave-one-out values, the selection and every unmasked trait's row are the bits of the call without
    a mask; an all-zero mask gives those bits for every row, and the window's own info in every info row."""
    p, gm, gu, z1 = _window(129, 65)
    Z = _traits(17, 129)
    mask = random_mask(17, 129, [0, 3, 0, 32, 1, 0, 0, 7, 0, 0, 16, 0, 2, 0, 0, 0, 5], seed=2)
    slct = dict(max=4, chi2_stop=1.0)
    stat = ("z", "info", "loo_z", "loo_info", "loo_t", "slct_idx", "slct_zin", "slct_joint", "slct_zc", "slct_var")
    for mode, w in ((0, None), (1, p["w"])):
        base = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, loo=True, slct=slct, z_more=Z)
        got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, loo=True, slct=slct, z_more=Z, miss_more=mask)
        only = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, z_more=Z, miss_more=mask)
        assert got["status"] == base["status"] == only["status"] == 0 and got["slct_n"] == base["slct_n"] > 0
        assert "info_more" not in base and "z_miss" not in base
        _same(got, base, stat)
        _same(got, only, KEYS)
        plain = mask.sum(axis=1) == 0
        assert np.array_equal(got["z_more"][plain], base["z_more"][plain])
        assert not np.any(got["z_more"][~plain] == base["z_more"][~plain])
        assert np.array_equal(got["info_more"][plain], np.broadcast_to(base["info"], (int(plain.sum()), 65)))
        none = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, loo=True, slct=slct, z_more=Z, miss_more=np.zeros_like(mask))
        _same(none, base, stat + ("z_more",))
        assert none["status"] == 0 and np.array_equal(none["info_more"], np.broadcast_to(base["info"], (17, 65)))
        assert np.all(np.isnan(none["z_miss"])) and np.all(np.isnan(none["info_miss"]))


def test_a_trait_depends_on_its_own_scores_and_its_own_mask_only(ctx):
    """A masked trait alone (T = 1) and as any one of 63 beside other masks gives the same bits; another trait's mask moves none of them; a
    NaN at a masked entry is the 0.0 that stands there; a NaN at a present entry makes that trait's z values non-finite, leaves its info
    row finite and moves no other bit."""
    M, U = 129, 130
    p, gm, gu, z1 = _window(M, U)
    Z = _traits(63, M, seed=9)
    mask = cyclic_mask(M, [(5 * t) % 33 for t in range(63)], 100, seed=3)
    call = lambda Z, mask: hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx, z_more=Z, miss_more=mask)
    full = call(Z, mask)
    assert full["status"] == 0 and np.all(np.isfinite(full["z_more"])) and np.all(np.isfinite(full["info_more"]))
    for t in (0, 1, 15, 16, 32, 33, 47, 62):
        alone = call(Z[t:t + 1], mask[t:t + 1])
        for k in KEYS:
            assert np.array_equal(alone[k][0], full[k][t], equal_nan=True), (t, k)
        _same(alone, full, ("z", "info"))
    pick = [40, 3, 62, 17, 5]
    some = call(Z[pick], mask[pick])                                   # another T, other places, a smaller union
    for k in KEYS:
        assert np.array_equal(some[k], full[k][pick], equal_nan=True), k
    other = mask.copy()
    other[7] = random_mask(1, M, [32], seed=77)[0]
    other[8] = 0
    moved = call(Z, other)
    keep = ~np.isin(np.arange(63), (7, 8))
    for k in KEYS:
        assert np.array_equal(moved[k][keep], full[k][keep], equal_nan=True), k
    Zn = Z.copy()
    Zn[mask != 0] = np.nan
    _same(call(Zn, mask), full, KEYS + ("z", "info"))
    for t in (6, 33):
        Zb = Z.copy()
        Zb[t, np.nonzero(mask[t] == 0)[0][11]] = np.nan
        bad = call(Zb, mask)
        keep = np.arange(63) != t
        assert bad["status"] == 0 and not np.any(np.isfinite(bad["z_more"][t])) and not np.any(np.isfinite(bad["z_miss"][t][mask[t] != 0]))
        assert np.array_equal(bad["info_more"], full["info_more"]) and np.array_equal(bad["info_miss"], full["info_miss"], equal_nan=True)
        for k in ("z_more", "z_miss"):
            assert np.array_equal(bad[k][keep], full[k][keep], equal_nan=True), k
        _same(bad, full, ("z", "info"))


def test_one_missing_snp_on_a_copy_of_z1_is_its_leave_one_out_value(ctx):
    """k = 1: trait t is z1 without SNP m_t -- z_miss / info_miss there are loo_z / loo_info of that SNP."""
    M, U = 129, 65
    p, gm, gu, z1 = _window(M, U)
    at = np.random.default_rng(1).choice(M, size=63, replace=False)
    at[:4] = (0, 63, 64, M - 1)
    mask = np.zeros((63, M), dtype=np.uint8)
    mask[np.arange(63), at] = 1
    for mode, w in ((0, None), (1, p["w"])):
        got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, ctx=ctx, loo=True, z_more=np.tile(z1, (63, 1)), miss_more=mask)
        ez = _zerr(got["z_miss"][np.arange(63), at], got["loo_z"][at])
        ei = _zerr(got["info_miss"][np.arange(63), at], got["loo_info"][at])
        print(f"traits miss k = 1 against leave-one-out, mode {mode}: z {ez:.3e}  info {ei:.3e}")
        assert got["status"] == 0 and ez <= Z_TOL and ei <= Z_TOL


def _run(ctx, wins, on_device=True, runs=1, want_mats=False):
    job = hotpath.Job(wins, ctx=ctx, on_device=on_device, want_mats=want_mats)
    for _ in range(runs):
        job.run()
    out = [job.fetch() for _ in range(runs)]
    job.close()
    return out


@pytest.mark.parametrize("mode,M0,dup", [(0, 30, [0, 1, 2]), (1, 150, [3, 70, 131, 140, 149])])
def test_clamped_window_uses_the_repaired_matrix(ctx, mode, M0, dup):
    """Duplicated measured SNPs at lambda = 0 (as tests/test_gpu_traits.py makes the window): MakePosDef rebuilds B11 and the downdate is
    that of the REPAIRED matrix -- against the closed form on the b11 / b21 the GPU returns, alone and inside a job beside a window
    that needs no repair."""
    p = small_panel(n_snp=M0 + 110, scale=0.02, seed=23 if M0 > 100 else 21)
    gm, gu, z1 = split_window(dict(G=p["G"][: M0 + 80]), M0)
    gm = np.ascontiguousarray(np.vstack([gm, gm[dup]]))
    z1 = np.concatenate([z1, z1[dup] - 0.2])
    M = gm.shape[0]
    w = p["w"] if mode else None
    Z = _traits(17, M, seed=3)
    mask = random_mask(17, M, [(3 * t) % 12 for t in range(17)], seed=5)
    mask[16, dup[0]] = 1                                              # one of a duplicated pair among the missing
    got = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, lam=0.0, ctx=ctx, z_more=Z, miss_more=mask)
    mats = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, lam=0.0, ctx=ctx, z_more=Z, miss_more=mask, want_mats=True)
    plain = hotpath.impute_window(mode, gm, gu, p["off"], w, z1, lam=0.0, ctx=ctx)
    assert got["status"] & 1 and got["status"] == plain["status"] == mats["status"]
    _same(got, plain, ("z", "info"))
    _same(got, mats, KEYS)
    _check(got, miss_closed_form(mats["b11"], mats["b21"], Z, mask), CLAMP_TOL, f"clamped window, M = {M}, mode {mode}")
    ok = dict(mode=mode, geno_m=gm[:M0], geno_u=gu, pop_off=p["off"], pop_wgt=w, z1=z1[:M0], z_more=Z[:5, :M0], miss_more=mask[:5, :M0])
    bad = dict(mode=mode, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=w, z1=z1, lam=0.0, z_more=Z, miss_more=mask)
    alone = _run(ctx, [ok], on_device=False)[0][0]
    assert alone["status"] == 0
    for run in _run(ctx, [ok, bad, ok], on_device=False, runs=2):
        assert run[0]["status"] == 0 and run[1]["status"] & 1
        _same(run[0], alone, KEYS + ("z", "info"))
        _same(run[2], alone, KEYS + ("z", "info"))
        _same(run[1], got, KEYS + ("z", "info"))


def test_nonfinite_window_is_all_nan(ctx):
    p = small_panel(n_snp=60, scale=0.01, n_pops=4)
    gm, gu, z1 = split_window(p, 25)
    gm = gm.copy()
    gm[3, :] = 1                                   # zero variance: CalCor returns 0 / 0
    mask = random_mask(5, 25, [2, 0, 1, 5, 0], seed=1)
    got = hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, z_more=_traits(5, 25), miss_more=mask)
    assert got["status"] & 2
    assert got["z_more"].shape == got["info_more"].shape == (5, gu.shape[0]) and got["z_miss"].shape == got["info_miss"].shape == (5, 25)
    for k in KEYS + ("z", "info"):
        assert np.all(np.isnan(got[k])), k


def _store_windows(ctx, seed=41, n_snp=2000, spans=((0, 131), (97, 340), (211, 560), (330, None), (400, 540)), T=(7, 0, 63, 16, 1),
                   masked=(True, False, True, False, True)):
    """Windows over one resident 2-bit store, overlapping like a chromosome's (as tests/test_gpu_traits.py builds them); window k
    carries T[k] further traits (0: it does not ask), with a mask where masked[k]."""
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
        if T[k] and masked[k]:
            ks = [(7 * t + k) % 9 for t in range(T[k])]
            more["miss_more"] = cyclic_mask(len(mi), ks, min(sum(ks), 100), seed=k)
        wins.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=z[mi], dev=(store.ptr, store.ptr, len(mi), len(ui), store.ld),
                         packed=dict(fmt=1, rows_m=mi.astype(np.int32), rows_u=ui.astype(np.int32), pop_src_off=src_off), **more))
        host.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=z[mi], geno_m=np.ascontiguousarray(G[mi]),
                         geno_u=np.ascontiguousarray(G[ui]), **more))
    return p, rows2, src_off, store, wins, host


def _same_win(a, b):
    assert a["status"] == b["status"] and sorted(a) == sorted(b), (a["status"], b["status"], sorted(a), sorted(b))
    _same(a, b, [k for k in ("z", "info", "loo_z", "loo_info", "loo_t", "slct_zc", "slct_var") + KEYS if k in a])


def test_every_launch_form_and_source_format_returns_the_same_bits(ctx, monkeypatch):
    """One job of overlapping windows that mix masked (T = 7, 63, 1), unmasked (T = 16) and not asking, two runs in flight, under each
    switch that changes a launch form or a source format: every output bit for bit that of the default."""
    p, rows2, src_off, store, wins, host = _store_windows(ctx)
    wins[4] = dict(wins[4], lam=1e-7)              # no certificate: the shifted matrix is factored too
    host[4] = dict(host[4], lam=1e-7)
    both = _run(ctx, wins, runs=2)
    ref = both[0]
    assert all(r["status"] == 0 for r in ref[:4]) and "z_more" not in ref[1] and "info_more" in ref[0] and "info_more" not in ref[3]
    for r, w in zip(both[1], ref):
        _same_win(r, w)
    # against the oracle once, so that "the same bits" are the right ones
    want = miss_by_oracle(1, host[0]["geno_m"], host[0]["geno_u"], p["off"], p["w"], host[0]["z_more"], host[0]["miss_more"])
    assert want["mpd"] == 0
    _check(ref[0], want, Z_TOL, "store window 0")
    # the windows that pass no mask keep the bits of a job in which nobody does
    for r, w in zip(_run(ctx, [{k: v for k, v in w.items() if k != "miss_more"} for w in wins])[0], ref):
        _same(r, w, ("z", "info"))
        if "z_more" in w and "info_more" not in w:
            _same(r, w, ("z_more",))
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
    call = lambda: hotpath.impute_window(1, h["geno_m"], h["geno_u"], p["off"], p["w"], h["z1"], ctx=ctx, z_more=h["z_more"], miss_more=h["miss_more"])
    _same_win(call(), ref[2])
    with monkeypatch.context() as m:
        m.setenv("GAUSS_STREAM_WINDOW", "0")
        _same_win(call(), ref[2])
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
    """A merged Gram launch whose chain queue gives up waiting (the library's test hook, bounded at 2 ms) is queued again in the
    two-launch form inside gauss_job_fetch: the masked traits come back with that re-run, bit for bit those of an undisturbed run, also
    with two such runs in flight."""
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


def test_with_leave_one_out_and_selection_in_one_job(ctx):
    """The result block with every section in use: windows on shared store rows asking for loo + selection + masked traits / the selection /
    nothing / loo + masked traits, two runs in flight -- every output of every window is bit for bit that of the window run alone."""
    slct = dict(max=4, chi2_stop=1.0)
    p, rows2, src_off, store, wins, host = _store_windows(ctx, spans=((0, 131), (97, 340), (211, 560), (330, None)), T=(17, 0, 0, 17),
                                                          masked=(True, False, False, True))
    wins = [dict(wins[0], loo=True, slct=slct), dict(wins[1], slct=slct), wins[2], dict(wins[3], loo=True)]
    alone = [_run(ctx, [w])[0][0] for w in wins]
    assert all(r["status"] == 0 for r in alone) and {"loo_z", "z_more", "info_more", "slct_zc"} <= set(alone[0]) and "info_more" in alone[3]
    for run in _run(ctx, wins, runs=2):
        for got, want in zip(run, alone):
            _same_win(got, want)
            if "slct_n" in want:
                assert got["slct_n"] == want["slct_n"] and np.array_equal(got["slct_raw"]["idx"], want["slct_raw"]["idx"])
    store.close()


def _rand_geno(rng, n, N):
    f = rng.uniform(0.05, 0.95, size=(n, 1))
    return ((rng.random((n, N)) < f).astype(np.uint8) + (rng.random((n, N)) < f).astype(np.uint8))


def test_full_size_window(ctx):
    """M = 737 = 12 factor blocks, U = 2 407, T = 63, every trait lacks 32 SNPs, 128 distinct: against the closed form on the GPU's own
    B11 / B21 (the recipe of tests/test_gpu_traits.py's full-size window)."""
    rng = np.random.default_rng(99)
    N, M, U, T = 1500, 737, 2407, 63
    off = np.array([0, N], dtype=np.int32)
    base = _rand_geno(rng, 220, N)
    G = base[rng.integers(0, 220, size=M + U)].copy()
    noise = rng.random(G.shape) < 0.4
    G[noise] = _rand_geno(rng, 1, N)[0][np.nonzero(noise)[1]]
    gm, gu = np.ascontiguousarray(G[:M]), np.ascontiguousarray(G[M:])
    z1 = rng.standard_normal(M) * 2
    Z = rng.standard_normal((T, M)) * 2
    mask = cyclic_mask(M, [32] * T, 128, seed=4)
    got = hotpath.impute_window(0, gm, gu, off, None, z1, want_mats=True, ctx=ctx, z_more=Z, miss_more=mask)
    assert got["status"] == 0
    _check(got, miss_closed_form(got["b11"], got["b21"], Z, mask), Z_TOL, "full size, closed form on out_b11 / out_b21")


def test_refusals(ctx):
    """33 missing in a trait, 129 in the union, a trait with every SNP masked, missing output pointers, QCAT / LD windows, a mask without traits."""
    p = small_panel(n_snp=300, scale=0.02, n_pops=5)
    gm, gu, z1 = split_window(p, 200)
    M = gm.shape[0]
    Z = _traits(5, M)
    base = dict(mode=0, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=None, z1=z1, z_more=Z)
    ok = random_mask(5, M, [32, 0, 32, 32, 32], seed=1)
    with pytest.raises(Exception, match="further trait 2 lacks 33 .* at most 32"):
        m = ok.copy()
        m[2, np.nonzero(m[2] == 0)[0][0]] = 1
        hotpath.Job([dict(base, miss_more=m)], ctx=ctx)
    with pytest.raises(Exception, match="129 distinct .* at most 128"):
        hotpath.Job([dict(base, miss_more=cyclic_mask(M, [32, 32, 32, 32, 1], 129, seed=2))], ctx=ctx)
    hotpath.Job([dict(base, miss_more=cyclic_mask(M, [32, 32, 32, 32, 0], 128, seed=2))], ctx=ctx).close()      # the limits themselves pass
    with pytest.raises(Exception, match="further trait 1 lacks all 20 measured SNPs"):
        m = np.zeros((5, 20), dtype=np.uint8)
        m[1] = 1
        hotpath.Job([dict(base, geno_m=gm[:20], z1=z1[:20], z_more=Z[:, :20], miss_more=m)], ctx=ctx)
    with pytest.raises(Exception, match="imputation windows only"):
        hotpath.Job([dict(base, miss_more=ok, qcat=(10, 30, 0.01))], ctx=ctx)
    with pytest.raises(Exception, match="imputation windows only"):
        hotpath.Job([dict(base, miss_more=ok, ld_codings=1)], ctx=ctx)
    for field, msg in (("out_info_more", "out_info_more is NULL"), ("out_z_miss", "out_z_miss is NULL"), ("out_info_miss", "out_info_miss is NULL"),
                       ("n_traits_more", "needs n_traits_more > 0")):
        desc = hotpath.WindowDesc()
        win = hotpath._Win(desc, dict(mode=0, geno_m=gm, geno_u=gu, pop_off=p["off"], z1=z1, lam=0.1, z_more=Z, miss_more=ok))
        setattr(desc, field, 0 if field == "n_traits_more" else None)
        with pytest.raises(Exception, match=msg):
            hotpath.check(ctx.lib.gauss_impute_window(ctx.handle, hotpath.C.byref(desc)))
        del win
    with pytest.raises(ValueError, match="miss_more must be"):
        hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, miss_more=ok)
    with pytest.raises(ValueError, match="miss_more must be"):
        hotpath.impute_window(0, gm, gu, p["off"], None, z1, ctx=ctx, z_more=Z, miss_more=ok[:3])


# ---- the host entry points, files -> table -----------------------------------------------------------------------
POPS = [("AAA", 160, "EUR"), ("BBB", 145, "EUR"), ("CCC", 170, "ASN"), ("DDD", 133, "AFR"), ("EEE", 152, "EUR"), ("FFF", 90, "ASN")]
WGT = (["aaa", "CCC", "eee", "FFF", "zzz"], [0.45, 0.2, 0.25, 0.161, 0.3])
WIN = (22, 1_500_000, 2_000_000, 300_000)
WIDE_WIN = (22, 1_000_000, 2_400_000, 100_000)       # its prediction window holds every SNP of the study


def _write(path, rows):
    with open(path, "w") as f:
        f.write("rsid chr bp a1 a2 z\n")
        for r in rows:
            f.write(f"{r[0]} {r[1]} {r[2]} {r[3]} {r[4]} {float(r[5])!r}\n")
    return str(path)


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    """Trait 1 is the synthetic study's own file.  Traits 2 and 3: other Z-scores (trait 2 with 10 % of its rows allele-swapped and its
    rows shuffled) on trait 1's SNPs minus a few -- two in a wing, three in the prediction window, one of those lacking in both."""
    from gauss_amd import api
    d = tmp_path_factory.mktemp("traits_miss_study")
    st = panel_mod.make_synthetic_study(str(d), POPS, n_snp=700, bp_lo=1_000_000, bp_hi=2_400_000, n_genes=40, frac_measured=0.3, seed=17)
    q = st["paths"]
    packed = os.path.join(os.path.dirname(q["data.gz"]), "panel.gpk")
    assert api.pack_panel(q["index.gz"], q["data.gz"], q["desc.txt"], packed) > 0
    rows = sorted((l.split() for l in open(q["gwas.txt"]).read().splitlines()[1:]), key=lambda r: int(r[2]))
    rng = np.random.default_rng(3)
    inside = [r[0] for r in rows if WIN[1] <= int(r[2]) <= WIN[2]]
    wing = [r[0] for r in rows if WIN[1] - WIN[3] <= int(r[2]) < WIN[1] or WIN[2] < int(r[2]) <= WIN[2] + WIN[3]]
    assert len(inside) > 20 and len(wing) > 20
    gone = {2: {wing[3], wing[-2], inside[1], inside[len(inside) // 2], inside[-1]}, 3: {wing[5], wing[-4], inside[4], inside[len(inside) // 2], inside[-3]}}
    z2, z3 = rng.standard_normal(len(rows)) * 2.0, rng.standard_normal(len(rows)) * 2.0
    swap = rng.random(len(rows)) < 0.1
    t2 = [(r[0], r[1], r[2], r[4], r[3], z) if s else (r[0], r[1], r[2], r[3], r[4], z) for r, z, s in zip(rows, z2, swap)]
    t2 = [t2[k] for k in rng.permutation(len(t2)) if t2[k][0] not in gone[2]]
    t3 = [tuple(r[:5]) + (z,) for r, z in zip(rows, z3) if r[0] not in gone[3]][::-1]
    ext = [r for r in rows if WIN[1] - WIN[3] <= int(r[2]) <= WIN[2] + WIN[3]]
    assert len(ext) >= 60 and len(rows) >= 180
    many = lambda name, drop: _write(d / name, [tuple(r[:5]) + (1.0,) for r in rows if r[0] not in drop])
    # a narrow window of 36 of trait 1's SNPs, for the file that keeps 8 of them
    a = len(rows) // 2
    narrow = rows[a:a + 36]
    nwin = (22, int(narrow[0][2]) + 20_000, int(narrow[-1][2]) - 20_000, 20_000)
    return dict(files=(q["gwas.txt"], q["index.gz"], q["data.gz"], q["desc.txt"]), packed=packed, more=[_write(d / "trait2.txt", t2), _write(d / "trait3.txt", t3)],
                gone=gone, n_ext=len(ext), nwin=nwin,
                over=many("over.txt", {r[0] for r in ext[10:10 + 45]}),                                   # 45 of the extended window's: more than 32 whatever the AF filter drops
                rows=rows, dir=d,
                few=many("few.txt", {r[0] for r in narrow[4:32]}))


@pytest.mark.parametrize("mix", [False, True])
def test_dist_traits_and_distmix_traits_impute_what_a_file_lacks(ctx, study, mix):
    """Three trait files on a text panel and a packed panel: trait 1's columns are the plain call's bits; the columns z_k, pval_k, info_k,
    type_k are the plain call's table of file k alone (its SNPs are a subset of trait 1's) -- the SNPs it lacks imputed, type 0."""
    from gauss_amd import api
    who = WGT if mix else "EUR"
    cutoff = 0.02 if mix else 0.01
    fn, plain_fn = (api.distmix_traits, api.distmix) if mix else (api.dist_traits, api.dist)
    inp, idx, dat, desc = study["files"]
    one = plain_fn(*WIN, who, inp, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
    with pytest.raises(Exception, match="trait2.txt lacks .* every trait must be measured at the SNPs of the first"):
        fn(*WIN, who, [inp] + study["more"], idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
    df = fn(*WIN, who, [inp] + study["more"], idx, dat, desc, af1_cutoff=cutoff, ctx=ctx, missing="impute")
    assert list(df.columns) == list(one.columns) + [f"{c}_{k}" for k in (2, 3) for c in ("z", "pval", "info", "type")] and len(df) == len(one)
    for c in one.columns:
        if one[c].dtype.kind == "f":
            assert np.array_equal(df[c].to_numpy(), one[c].to_numpy(), equal_nan=True), c
        else:
            assert list(df[c]) == list(one[c]), c
    assert df.attrs["n_missing"][0] == 0 and 3 <= df.attrs["n_missing"][1] <= 5 and 3 <= df.attrs["n_missing"][2] <= 5
    for k, alone_file in zip((2, 3), study["more"]):
        alone = plain_fn(*WIN, who, alone_file, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
        assert list(alone["rsid"]) == list(df["rsid"])
        assert list(alone["type"]) == list(df[f"type_{k}"])
        lacked = [r for r, t1, tk in zip(df["rsid"], df["type"], df[f"type_{k}"]) if t1 == 1 and tk == 0]
        assert lacked and set(lacked) <= study["gone"][k]
        ez = _zerr(df[f"z_{k}"].to_numpy(), alone["z"].to_numpy())
        ei = _zerr(df[f"info_{k}"].to_numpy(), alone["info"].to_numpy())
        ep = float(np.max(np.abs(df[f"pval_{k}"].to_numpy() - alone["pval"].to_numpy()) / alone["pval"].to_numpy()))
        print(f"{'distmix' if mix else 'dist'}_traits missing=impute, trait {k}: z {ez:.3e}  info {ei:.3e}  pval rel {ep:.3e}  ({len(lacked)} imputed rows)")
        assert ez <= Z_TOL and ei <= Z_TOL and ep <= 1e-6
        meas = (df[f"type_{k}"] == 1).to_numpy()
        assert np.array_equal(df[f"z_{k}"].to_numpy()[meas], alone["z"].to_numpy()[meas])       # a measured SNP's own oriented study z
    other = fn(*WIN, who, [inp] + study["more"], "(unused)", study["packed"], desc, af1_cutoff=cutoff, ctx=ctx, missing="impute")
    assert list(other.columns) == list(df.columns) and len(other) == len(df)
    for c in df.columns:
        if df[c].dtype.kind == "f":
            assert np.array_equal(df[c].to_numpy(), other[c].to_numpy(), equal_nan=True), c
        else:
            assert list(df[c]) == list(other[c]), c
    # a file that lacks nothing: the same frame with the window's own info and type in its columns
    same = fn(*WIN, who, [inp, inp], idx, dat, desc, af1_cutoff=cutoff, ctx=ctx, missing="impute")
    assert np.array_equal(same["info_2"].to_numpy(), one["info"].to_numpy()) and list(same["type_2"]) == list(one["type"]) and same.attrs["n_missing"][1] == 0
    # the three limits, before any job is made.  Five files that lack 27 each of the measured SNPs WIDE_WIN's own table lists: 135 distinct
    all_m = list(plain_fn(*WIDE_WIN, who, inp, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx).query("type == 1")["rsid"])
    assert len(all_m) >= 150
    wide = [_write(study["dir"] / f"wide{k}_{int(mix)}.txt", [tuple(r[:5]) + (1.0,) for r in study["rows"] if r[0] not in set(all_m[27 * k: 27 * k + 27])])
            for k in range(5)]
    c0 = ctx.counters()
    with pytest.raises(Exception, match=r"over.txt lacks (3[3-9]|4[0-5]) of the window's \d+ measured SNPs: a trait may lack at most 32"):
        fn(*WIN, who, [inp, study["over"]], idx, dat, desc, af1_cutoff=cutoff, ctx=ctx, missing="impute")
    with pytest.raises(Exception, match=r"135 distinct measured SNPs .*wide4_[01].txt.* at most 128"):
        fn(*WIDE_WIN, who, [inp] + wide, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx, missing="impute")
    with pytest.raises(Exception, match=r"few.txt has ([0-9]|10) of the window's \d+ measured SNPs: a trait needs more than 10"):
        fn(*study["nwin"], who, [inp, study["few"]], idx, dat, desc, af1_cutoff=cutoff, ctx=ctx, missing="impute")
    assert ctx.counters() == c0


def test_missing_impute_gives_one_frame_on_every_panel_form(ctx, study, monkeypatch):
    """missing="impute" with three traits on WIN: the packed panel (a lean window), the packed panel with GAUSS_HOST_FULL_MAP=1 (the
    literal data layer on packed rows) and the text panel give the same frame, bit for bit, for dist_traits and distmix_traits"""
    from gauss_amd import api
    inp, idx, dat, desc = study["files"]
    for mix in (False, True):
        fn = api.distmix_traits if mix else api.dist_traits
        call = lambda index, data: fn(*WIN, WGT if mix else "EUR", [inp] + study["more"], index, data, desc, af1_cutoff=0.02 if mix else 0.01,
                                      ctx=ctx, missing="impute")
        packed = call("(unused)", study["packed"])
        with monkeypatch.context() as m:
            m.setenv("GAUSS_HOST_FULL_MAP", "1")
            full = call("(unused)", study["packed"])
        text = call(idx, dat)
        assert len(packed) > 0 and max(packed.attrs["n_missing"]) >= 3
        for other in (full, text):
            assert list(other.columns) == list(packed.columns) and len(other) == len(packed)
            for c in packed.columns:
                a, b = packed[c], other[c]
                assert np.array_equal(a.to_numpy(), b.to_numpy(), equal_nan=True) if a.dtype.kind == "f" else list(a) == list(b), (mix, c)
            assert list(other.attrs["n_missing"]) == list(packed.attrs["n_missing"])
