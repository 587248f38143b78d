"""GPU: simulateLD (simulateLD.cpp:34-252).  The resample-pack kernel (k_simld.hip) through gauss_ld_resampled_rows against the CPU
oracle's CalCor on the reference's geno_mat (drawn columns, then zero columns), for one-byte, 2-bit and resident rows; the entry
point end to end against the Python restatement of the reference driver on text and packed panels."""
import numpy as np
import pytest

import oracle
from gauss_amd import _lib, api, hotpath, panel
from oracle import feeder_py as fp
from oracle import oracle_np

import simld_ref

pytestmark = pytest.mark.gpu

LD_TOL = 1e-12
SIZES = [300, 77, 1000, 64, 129]          # blocks that end mid-chunk and one that fills its chunks
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)


def _geno(M, seed):
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.02, 0.6, size=(M, 1))
    G = (rng.random((M, OFF[-1])) < af).astype(np.uint8) + (rng.random((M, OFF[-1])) < af).astype(np.uint8)
    return np.ascontiguousarray(G)


def _draws(n, seed, repeat=False):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, len(SIZES), n)
    s = np.array([rng.integers(0, SIZES[k]) for k in q], dtype=np.int64)
    if repeat and n > 8:
        q[: n // 4], s[: n // 4] = 2, 17                       # one sample drawn many times
    return q.astype(np.int32), s.astype(np.int32)


def _want(G, q, s, n_cols):
    X = simld_ref.gathered(G, OFF, np.stack([q, s], 1).astype(np.int64), n_cols)
    return oracle.ld_pooled(X, np.array([0, n_cols], dtype=np.int32), 1.0)


def _same(got, want, tol=LD_TOL):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.max(np.abs(got[~nan] - want[~nan]), initial=0.0) <= tol
    assert np.mean((got == want) | nan) > 0.999


def _run(kind, G, q, s, n_cols, ctx, rows=None):
    if kind == "u8":
        return hotpath.ld_resampled(G, None, OFF, q, s, n_cols, fmt=_lib.GENO_U8, ctx=ctx)
    rows2, src = panel.pack2bit(G, OFF)
    idx = np.arange(G.shape[0], dtype=np.int32)
    # the window's rows are store rows in another order: stored reversed, asked for by index
    store = np.ascontiguousarray(rows2[::-1])
    ridx = (G.shape[0] - 1 - idx).astype(np.int32)
    if kind == "2bit":
        return hotpath.ld_resampled(store, ridx, OFF, q, s, n_cols, fmt=_lib.GENO_2BIT, pop_src_off=src, ctx=ctx)
    rs = hotpath.RowStore(store, ctx=ctx)
    try:
        return hotpath.ld_resampled(rs, ridx, OFF, q, s, n_cols, fmt=_lib.GENO_2BIT, pop_src_off=src, ctx=ctx)
    finally:
        rs.close()


CASES = [(2, 1, 1), (2, 63, 200), (127, 64, 64), (128, 65, 65), (129, 2047, 2100), (129, 2049, 2049), (300, 4097, 5000),
         (129, 20000, 20000), (128, 20011, 26000)]


@pytest.mark.parametrize("kind", ["u8", "2bit", "store"])
@pytest.mark.parametrize("M,n_drawn,n_cols", CASES)
def test_resampled_ld_matches_oracle(ctx, kind, M, n_drawn, n_cols):
    G = _geno(M, seed=M + n_drawn)
    q, s = _draws(n_drawn, seed=n_drawn, repeat=True)
    got = _run(kind, G, q, s, n_cols, ctx)
    _same(got, _want(G, q, s, n_cols))
    assert np.all(np.diag(got) == 1.0)


def test_draw_order_changes_no_bit(ctx):
    G = _geno(200, seed=3)
    q, s = _draws(5000, seed=4)
    perm = np.random.default_rng(5).permutation(len(q))
    for kind in ("u8", "2bit"):
        a = _run(kind, G, q, s, 6000, ctx)
        b = _run(kind, G, q[perm], s[perm], 6000, ctx)
        assert np.array_equal(a, b, equal_nan=True)


def test_constant_rows_and_no_draws(ctx):
    G = _geno(70, seed=8)
    G[3] = 1                                   # constant in every sample
    G[9] = 0                                   # all zero: constant even with zero columns
    q, s = _draws(500, seed=9)
    for n_cols in (500, 800):
        got = _run("2bit", G, q, s, n_cols, ctx)
        want = _want(G, q, s, n_cols)
        _same(got, want)
        assert np.all(np.isnan(np.delete(got[9], 9))) and got[9, 9] == 1.0
        if n_cols == 500:
            assert np.all(np.isnan(np.delete(got[3], 3))) and got[3, 3] == 1.0
    e = np.zeros(0, dtype=np.int32)
    got = hotpath.ld_resampled(G, None, OFF, e, e, 100, fmt=_lib.GENO_U8, ctx=ctx)
    assert np.all(np.diag(got) == 1.0)
    assert np.all(np.isnan(got[~np.eye(70, dtype=bool)]))


def test_bad_draws_are_refused(ctx):
    G = _geno(10, seed=1)
    with pytest.raises(_lib.GaussHipError, match="outside"):
        hotpath.ld_resampled(G, None, OFF, np.array([1], np.int32), np.array([77], np.int32), 10, fmt=_lib.GENO_U8, ctx=ctx)
    with pytest.raises(_lib.GaussHipError, match="n_drawn"):
        hotpath.ld_resampled(G, None, OFF, np.array([0, 0], np.int32), np.array([0, 1], np.int32), 1, fmt=_lib.GENO_U8, ctx=ctx)


def test_realistic_size_against_numpy(ctx):
    M, n_cols = 1200, 50_000
    G = _geno(M, seed=21)
    q, s = _draws(45_000, seed=22)
    got = _run("store", G, q, s, n_cols, ctx)
    X = simld_ref.gathered(G, OFF, np.stack([q, s], 1).astype(np.int64), n_cols)
    want = oracle_np.pooled_cor(X)
    np.fill_diagonal(want, 1.0)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.max(np.abs(got[~nan] - want[~nan])) <= LD_TOL


# ---- end to end -----------------------------------------------------------------------------------------------------------------
POPS = [("AAA", 160, "EUR"), ("BBB", 145, "EUR"), ("CCC", 170, "ASN"), ("DDD", 133, "AFR"), ("EEE", 152, "EUR"),
        ("FFF", 90, "ASN")]
W_FULL = (["fff", "aaa", "CCC", "eee", "zzz"], [0.15, 0.4, 0.2, 0.25, 0.3])     # panel order differs; an unknown name
W_PART = (["AAA", "DDD", "CCC"], [0.3, 0.25, 0.0])                              # sums to 0.55: zero columns; weight 0


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    d = tmp_path_factory.mktemp("simld_study")
    st = panel.make_synthetic_study(str(d), POPS, n_snp=600, bp_lo=1_000_000, bp_hi=2_400_000, frac_measured=0.35, seed=23)
    p = st["paths"]
    st["packed"] = str(d / "panel.gpk")
    assert api.pack_panel(p["index.gz"], p["data.gz"], p["desc.txt"], st["packed"]) > 0
    return st


def _files(st, packed=False):
    p = st["paths"]
    return p["gwas.txt"], p["index.gz"], st["packed"] if packed else p["data.gz"], p["desc.txt"]


def _feeder_rows(st, chr_, lo, hi, wgt):
    inp, idx, dat, desc = _files(st)
    pops = fp.read_ref_desc(desc)
    flags, w = fp.pop_flags_wgt(pops, *wgt)
    m = fp.read_input_z(inp, chr_, lo, hi, False)
    fp.read_reference_index(m, idx, chr_, lo, hi, False)
    vec = fp.make_snp_vec(m, dat, flags, 0.01, w)
    meas = [s for s in vec if s.type == 1]
    return fp._matrix(meas) & 0x0F, fp._selected_off(pops, flags)


@pytest.mark.parametrize("wgt,sim_size", [(W_FULL, 3000), (W_PART, 2000)])
def test_simulateLD_end_to_end(ctx, study, wgt, sim_size):
    win = (22, 1_200_000, 2_300_000)
    res = api.simulateLD(*win, wgt, sim_size, *_files(study), seed=2024, ctx=ctx, detail=True)
    ld = api.computeLD(*win, wgt, *_files(study), ctx=ctx)
    assert res["snplist"].equals(ld["snplist"])
    G, off = _feeder_rows(study, *win, wgt)
    assert G.shape[0] == len(res["snplist"])
    sizes = np.diff(off)
    dr = res["draws"]
    assert res["seed"] == 2024 and res["n_drawn"] == len(dr) <= sim_size
    np.testing.assert_array_equal(dr, simld_ref.draws(2024, list(sizes), list(res["counts"])))
    X = simld_ref.gathered(G, off, dr, sim_size)
    want = oracle.ld_pooled(X, np.array([0, sim_size], dtype=np.int32), 1.0)
    _same(res["cormat"], want)
    # the packed panel: same SNPs, same bits
    pk = api.simulateLD(*win, wgt, sim_size, *_files(study, packed=True), seed=2024, ctx=ctx)
    assert pk["snplist"].equals(res["snplist"])
    assert np.array_equal(pk["cormat"], res["cormat"], equal_nan=True)


def test_simulateLD_counts_in_panel_order(ctx, study):
    res = api.simulateLD(22, 1_200_000, 2_300_000, W_PART, 2000, *_files(study), seed=1, ctx=ctx, detail=True)
    assert list(res["counts"]) == [600, 0, 500]          # AAA, CCC, DDD in panel order; CCC has weight 0
    assert res["n_drawn"] == 1100


def test_simulateLD_errors(ctx, study):
    with pytest.raises(api.GaussError, match="Not enough number of SNPs loaded - computeLD not performed"):
        api.simulateLD(22, 1_000_000, 1_005_000, W_FULL, 1000, *_files(study), seed=1, ctx=ctx)
    with pytest.raises(api.GaussError, match="more than sim_size"):
        api.simulateLD(22, 1_200_000, 2_300_000, (["AAA", "BBB"], [0.7, 0.5]), 1000, *_files(study), seed=1, ctx=ctx)
    r1 = api.simulateLD(22, 1_200_000, 2_300_000, W_FULL, 500, *_files(study), ctx=ctx, detail=True)
    r2 = api.simulateLD(22, 1_200_000, 2_300_000, W_FULL, 500, *_files(study), seed=r1["seed"], ctx=ctx)
    assert np.array_equal(r1["cormat"], r2["cormat"], equal_nan=True)
