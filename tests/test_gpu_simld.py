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


# ---- the two forms of the resample-pack kernel: the source row staged in LDS, or gathered from global memory --------------------
# resample_pack_lds_bytes' rule (k_simld.hip), restated: a source row is staged while its length, rounded up to 16 bytes, is at
# most SIMLD_LDS_MAX = 60 KB; the library has no counter of the form it took, so the tests assert the rule on their own sizes.
LDS_MAX = 60 << 10
LONG = [20000, 1, 18000, 63, 23376]       # 61 440 one-byte samples: the longest staged row
SPARE = 4000                              # a further population nobody draws from: 65 440 bytes, the global form
SHORT = [700, 33, 1291]                   # a staged row for the codes above 2
WIDE2 = [120001, 63, 64, 125700]          # 245 828 2-bit samples in blocks of 64: 61 488 bytes, just past 60 KB


def _staged(row_bytes):
    return 0 < (row_bytes + 15) // 16 * 16 <= LDS_MAX


def _offs(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _geno_of(M, N, seed):
    """M rows of N codes 0..2 at a frequency of the row's own."""
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.05, 0.6, size=(M, 1))
    return np.ascontiguousarray((rng.random((M, N)) < af).astype(np.uint8) + (rng.random((M, N)) < af).astype(np.uint8))


def _draws_of(sizes, n, seed):
    """n draws from populations of `sizes`: the first and the last sample of every one (hence column 0 and the last column of
    the row), one sample drawn many times, the rest at random -- in shuffled order."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, len(sizes), n)
    s = np.array([rng.integers(0, sizes[k]) for k in q], dtype=np.int64)
    q[: n // 5], s[: n // 5] = len(sizes) - 1, sizes[-1] // 2
    for k, m in enumerate(sizes):
        q[n // 5 + 2 * k], s[n // 5 + 2 * k] = k, 0
        q[n // 5 + 2 * k + 1], s[n // 5 + 2 * k + 1] = k, m - 1
    perm = rng.permutation(n)
    return q[perm].astype(np.int32), s[perm].astype(np.int32)


def _with_spare(G, n_spare, seed):
    """G's rows with n_spare further columns: a population that is never drawn (it only lengthens the source row)."""
    return np.ascontiguousarray(np.hstack([G, np.random.default_rng(seed).integers(0, 3, (G.shape[0], n_spare)).astype(np.uint8)]))


def _ld_u8(G, sizes, q, s, n_cols, ctx, reverse=False):
    """One-byte host rows; reverse: the rows are stored in the opposite order and asked for through rows=."""
    assert G.shape[1] == sum(sizes)
    if not reverse:
        return hotpath.ld_resampled(G, None, _offs(sizes), q, s, n_cols, fmt=_lib.GENO_U8, ctx=ctx)
    ridx = np.arange(G.shape[0] - 1, -1, -1, dtype=np.int32)
    return hotpath.ld_resampled(np.ascontiguousarray(G[::-1]), ridx, _offs(sizes), q, s, n_cols, fmt=_lib.GENO_U8, ctx=ctx)


def _want_of(G, sizes, q, s, n_cols):
    X = simld_ref.gathered(G & 0x0F, _offs(sizes), np.stack([q, s], 1).astype(np.int64), n_cols)
    return oracle.ld_pooled(X, np.array([0, n_cols], dtype=np.int32), 1.0)


_LONG = {}


def _long():
    """The 70 rows of 61 440 samples, their draws (from the LONG populations only) and the oracle's LD; made once."""
    if not _LONG:
        G = _geno_of(70, sum(LONG), seed=61440)
        q, s = _draws_of(LONG, 3000, seed=61441)
        cols = _offs(LONG)[q] + s
        assert cols.min() == 0 and cols.max() == sum(LONG) - 1 and len(np.unique(cols)) < len(cols)
        _LONG.update(G=G, q=q, s=s, n_cols=3500, want=_want_of(G, LONG, q, s, 3500))
        _LONG["want"].setflags(write=False)
    return _LONG


def test_staged_and_global_forms_on_the_same_draws(ctx):
    """The longest staged row (61 440 bytes), the same rows with an undrawn population behind them (65 440 bytes: the global form)
    and with one undrawn sample behind them (61 441 bytes, 61 456 rounded: the first length past the rule): the same draws give the
    same bits, the oracle's LD, and so do the rows stored in another order."""
    L = _long()
    G, q, s, n_cols = L["G"], L["q"], L["s"], L["n_cols"]
    forms = {0: True, 1: False, SPARE: False}
    got = {}
    for spare, staged in forms.items():
        Gs, sizes = (G, LONG) if spare == 0 else (_with_spare(G, spare, seed=spare), LONG + [spare])
        assert Gs.shape[1] == 61440 + spare and _staged(Gs.shape[1]) == staged
        got[spare] = _ld_u8(Gs, sizes, q, s, n_cols, ctx)
        _same(got[spare], L["want"])
        assert np.all(np.diag(got[spare]) == 1.0)
        rev = _ld_u8(Gs, sizes, q, s, n_cols, ctx, reverse=True)
        assert np.array_equal(rev, got[spare], equal_nan=True), spare      # (window row i is store row M - 1 - i: G's row i again)
    assert np.isfinite(got[0]).all()
    for spare in (1, SPARE):
        assert np.array_equal(got[spare], got[0]), (spare, int(np.sum(got[spare] != got[0])))


def test_two_bit_global_form(ctx):
    """2-bit rows of 61 488 bytes (past 60 KB: gathered from global memory), as host rows and as a resident store, drawn at both
    ends of every block: the oracle's LD, and bit for bit the one-byte global form of the same matrix on the same draws."""
    M, n_cols = 40, 3300
    G = _geno_of(M, sum(WIDE2), seed=245828)
    q, s = _draws_of(WIDE2, 3000, seed=245829)
    rows2, src = panel.pack2bit(G, _offs(WIDE2))
    assert sum(WIDE2) >= 245824 and rows2.shape[1] == 61488 and not _staged(rows2.shape[1]) and _staged(rows2.shape[1] - 48)
    assert not _staged(G.shape[1])
    want = _want_of(G, WIDE2, q, s, n_cols)
    one = _ld_u8(G, WIDE2, q, s, n_cols, ctx)
    _same(one, want)
    store = np.ascontiguousarray(rows2[::-1])
    ridx = np.arange(M - 1, -1, -1, dtype=np.int32)
    host = hotpath.ld_resampled(store, ridx, _offs(WIDE2), q, s, n_cols, fmt=_lib.GENO_2BIT, pop_src_off=src, ctx=ctx)
    rs = hotpath.RowStore(store, ctx=ctx)
    try:
        res = hotpath.ld_resampled(rs, ridx, _offs(WIDE2), q, s, n_cols, fmt=_lib.GENO_2BIT, pop_src_off=src, ctx=ctx)
    finally:
        rs.close()
    _same(host, want)
    assert np.isfinite(one).all()
    assert np.array_equal(host, one) and np.array_equal(res, one)


def _codes_0_15(M, N, seed):
    """One-byte rows of codes 0..15: a third hold 0..7 only, the others at least one byte at 8 or above, the last row is all 15."""
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 16, size=(M, N)).astype(np.uint8)
    G[::3] &= 7
    G[-1] = 15
    assert (G[::3].max(1) <= 7).all() and (np.delete(G, np.s_[::3], 0).max(1) >= 8).all() and G[::3].min() == 0 and G[::3].max() == 7
    return np.ascontiguousarray(G)


# (row length, population sizes, the populations drawn from): a staged panel and the global layout of the long rows
CODE_LAYOUTS = {"staged": (SHORT, len(SHORT)), "global": (LONG + [SPARE], len(LONG))}
_CODES = {}


def _codes_case(layout, top):
    """Rows of codes 0..top (15, or 9: what an ASCII digit can hold) in `layout`, 5 000 draws, the oracle's LD; made once."""
    if (layout, top) not in _CODES:
        sizes, n_live = CODE_LAYOUTS[layout]
        M = 68
        G = _codes_0_15(M, sum(sizes), seed=15 + len(sizes))
        if top == 9:
            G = np.minimum(G, 9)
        q, s = _draws_of(sizes[:n_live], 5000, seed=16 + len(sizes))
        n_cols = 5600
        want = _want_of(G, sizes, q, s, n_cols)
        want.setflags(write=False)
        _CODES[(layout, top)] = dict(G=G, sizes=sizes, q=q, s=s, n_cols=n_cols, want=want)
    return _CODES[(layout, top)]


@pytest.mark.parametrize("layout", ["staged", "global"])
def test_one_byte_codes_above_two(ctx, layout):
    """Codes 3..7 (the byte-permute e4m3 table), 8..15 (the per-byte table behind x & 0x08080808) and a row of 15s, over 5 000
    draws: the oracle on the decoded matrix; the rows written as ASCII '0'..'9' give the bits of the numeric codes 0..9."""
    c = _codes_case(layout, 15)
    assert _staged(c["G"].shape[1]) == (layout == "staged")
    got = _ld_u8(c["G"], c["sizes"], c["q"], c["s"], c["n_cols"], ctx)
    _same(got, c["want"])
    assert np.isfinite(got).all() and np.all(np.diag(got) == 1.0)
    d = _codes_case(layout, 9)
    num = _ld_u8(d["G"], d["sizes"], d["q"], d["s"], d["n_cols"], ctx)
    _same(num, d["want"])
    txt = _ld_u8(d["G"] + np.uint8(ord("0")), d["sizes"], d["q"], d["s"], d["n_cols"], ctx)
    assert np.array_equal(txt, num)
    assert not np.array_equal(num, got)


def test_two_bit_rows_that_hold_code_three(ctx):
    """2-bit rows some of which hold code 3, host rows and resident: the oracle's LD and the bits of the one-byte rows."""
    sizes, M, n_cols = SHORT, 67, 5600
    rng = np.random.default_rng(33)
    G = rng.integers(0, 3, size=(M, sum(sizes))).astype(np.uint8)
    G[::4] = rng.integers(0, 4, size=G[::4].shape)
    G[-1] = 3
    assert (G[::4].max(1) == 3).all() and (np.delete(G, np.s_[::4], 0)[:-1].max(1) == 2).all()
    q, s = _draws_of(sizes, 5000, seed=34)
    want = _want_of(G, sizes, q, s, n_cols)
    rows2, src = panel.pack2bit(G, _offs(sizes))
    host = hotpath.ld_resampled(rows2, None, _offs(sizes), q, s, n_cols, fmt=_lib.GENO_2BIT, pop_src_off=src, ctx=ctx)
    _same(host, want)
    rs = hotpath.RowStore(rows2, ctx=ctx)
    try:
        ridx = np.arange(M, dtype=np.int32)
        res = hotpath.ld_resampled(rs, ridx, _offs(sizes), q, s, n_cols, fmt=_lib.GENO_2BIT, pop_src_off=src, ctx=ctx)
    finally:
        rs.close()
    assert np.array_equal(res, host)
    assert np.array_equal(_ld_u8(G, sizes, q, s, n_cols, ctx), host)


def test_int8_context_gives_the_same_bits(ctx, monkeypatch):
    """The resample-pack kernel's int8 operand (Prob::gram_i8: the codes as they are) on a context of its own: staged 0..2, global
    0..2 and staged 0..15 equal the default context bit for bit -- the sums are exact integers either way."""
    L = _long()
    Gp = _with_spare(L["G"], SPARE, seed=SPARE)
    c = _codes_case("staged", 15)
    cases = [(L["G"], LONG, L["q"], L["s"], L["n_cols"]), (Gp, LONG + [SPARE], L["q"], L["s"], L["n_cols"]),
             (c["G"], c["sizes"], c["q"], c["s"], c["n_cols"])]
    assert [_staged(a[0].shape[1]) for a in cases] == [True, False, True]
    want = [_ld_u8(*a, ctx) for a in cases]
    _same(want[0], L["want"])
    _same(want[2], c["want"])
    monkeypatch.setenv("GAUSS_GRAM_DTYPE", "i8")
    c8 = hotpath.Context(0)
    try:
        got = [_ld_u8(*a, c8) for a in cases]
    finally:
        c8.close()
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.isfinite(b).all()
        assert np.array_equal(a, b), (k, int(np.sum(a != b)))


def test_the_exact_integer_range_of_the_draws(ctx):
    """n_drawn * 225 >= 2^31 is refused before any draw is looked at; one draw fewer passes that gate (its first draw is then
    refused for its population): the bound is exact."""
    n = 9_544_372
    assert n * 225 >= 2 ** 31 > (n - 1) * 225
    G = _geno(4, seed=2)
    q = np.zeros(n, dtype=np.int32)
    q[0] = len(SIZES)                          # out of range, at index 0
    s = np.zeros(n, dtype=np.int32)
    with pytest.raises(_lib.GaussHipError, match="exact-integer range"):
        hotpath.ld_resampled(G, None, OFF, q, s, n, fmt=_lib.GENO_U8, ctx=ctx)
    with pytest.raises(_lib.GaussHipError, match=f"draw 0: population {len(SIZES)} is outside"):
        hotpath.ld_resampled(G, None, OFF, q[:-1], s[:-1], n, fmt=_lib.GENO_U8, ctx=ctx)


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
