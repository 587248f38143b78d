"""GPU: optimal LD-block boundaries on the device (k_ldsplit.hip, gauss_ld_split_rows) against tests/ldsplit_ref.py.

(i)   On the matrix gauss_ld_rows returns for the same rows: cost, prev, max_r2 and n_nonfinite equal replay() bit for bit (the float64
      bit patterns, +inf included), for shapes on both sides of every tile edge of the three kernels: 64 rows and 64 offsets a tile in
      ldsplit_band_kernel (offsets 1 .. max_size - 1: the chunk edge is at max_size = 65), 64 boundaries 0 .. M a workgroup in
      ldsplit_cost_kernel (M = 63), 64 boundaries 1 .. M a workgroup and 16 waves of block sizes in ldsplit_dp_kernel.
(ii)  The same bits from host bytes, a resident one-byte store, a resident 2-bit store, rows in permuted store order and one queue.
(iii) A planted region: three groups of SNPs in strong LD inside a group and none between groups give the planted boundaries at K = 3.
(iv)  On the CPU oracle's LD, M = 130: the GPU's split for each K, re-costed with math.fsum on the oracle's matrix, equals replay()'s
      optimum there within 4e-12 x (band pairs), the per-entry bound tests/test_gpu_ldscore.py holds summed r^2 to.
Then every refusal."""
import ctypes as C

import numpy as np
import pytest

import ldsplit_ref as lr
import oracle
from gauss_amd import _lib, hotpath
from gauss_amd import panel as panel_mod
from test_gpu_clump import _panel

pytestmark = pytest.mark.gpu

_ip, _dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
BIG = 1 << 32


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(got, ref, what):
    assert np.array_equal(_bits(got["cost"]), _bits(ref["cost"])), (what, "cost", got["cost"][:8], ref["cost"][:8])
    assert np.array_equal(got["prev"], ref["prev"]), (what, "prev")
    assert np.array_equal(_bits(got["max_r2"]), _bits(ref["max_r2"])), (what, "max_r2")
    assert got["n_nonfinite"] == ref["n_nonfinite"], (what, "n_nonfinite", got["n_nonfinite"], ref["n_nonfinite"])
    for K, ends in ref["splits"].items():
        assert (ends is None) == (got["splits"][K] is None) and (ends is None or np.array_equal(ends, got["splits"][K])), (what, K)


# (M, min_size, max_size, max_K, radius, thr_r2, max_r2): M and max_size below, at and above 64 and 128 (rows and offsets of a band tile,
# boundaries of a cost / DP workgroup); min(max_size, M) - 1 = 62 .. 65 and 126 .. 129 offsets, below, at and above a chunk; size ranges of 1, 8, 9, 16, 17 sizes (the DP's 16
# waves); min_size = 1 and = max_size; max_size > M; max_K = 1 and the limit; a radius of about 25 rows inside max_size
CASES = [
    (1, 1, 1, 3, BIG, 0.02, 1.0), (2, 1, 2, 3, BIG, 0.0, 1.0), (3, 1, 2, 128, BIG, 0.02, 0.9), (7, 2, 3, 5, BIG, 0.02, 1.0),
    (7, 1, 4096, 1, BIG, 0.02, 1.0),
    (63, 1, 63, 4, BIG, 0.02, 1.0), (63, 5, 64, 128, BIG, 0.0, 0.6), (64, 8, 16, 9, BIG, 0.02, 0.8), (64, 1, 65, 3, 5_000, 0.02, 1.0),
    (65, 5, 5, 14, BIG, 0.02, 1.0), (65, 10, 66, 4, BIG, 0.1, 0.7), (65, 1, 8, 70, BIG, 0.02, 1.0),
    (127, 20, 35, 6, BIG, 0.02, 0.5), (128, 60, 127, 3, BIG, 0.02, 1.0), (128, 1, 128, 2, 5_000, 0.0, 1.0),
    (129, 30, 129, 5, BIG, 0.02, 0.9), (129, 64, 130, 3, BIG, 0.02, 1.0), (129, 10, 26, 13, 2_000, 0.02, 0.6),
    (1030, 100, 300, 10, BIG, 0.02, 0.7), (1030, 40, 257, 12, 30_000, 0.05, 1.0),
    # M > max_size, so that W = min(max_size, M) is max_size: 65 and 129 offsets, the far chunk of the band holds one offset alone
    (130, 1, 66, 3, BIG, 0.02, 1.0), (200, 1, 130, 3, BIG, 0.0, 0.9), (130, 3, 64, 4, BIG, 0.02, 1.0), (200, 2, 129, 3, 9_000, 0.02, 1.0),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d-%d..%d-K%d-%s" % (c[0], c[1], c[2], c[3], "all" if c[4] == BIG else c[4]))
def test_the_bits_of_the_replay_on_the_gpus_own_ld(ctx, case):
    M, min_size, max_size, max_K, radius, thr, max_r2 = case
    k = CASES.index(case)
    mode, n_pop, n_samples = k % 2, 1 + k % 3, (200, 300, 450, 600)[k % 4]
    p = _panel(M, seed=900 + k, n_samples=n_samples, n_pop=n_pop)
    w = p["w"] if mode else None
    R = hotpath.ld_matrix_rows(p["G"], np.arange(M), p["off"], w, mode, 1.0, fmt=_lib.GENO_U8, ctx=ctx)
    got = hotpath.ld_split(p["G"], p["off"], p["bp"], w, mode, radius, thr, min_size, max_size, max_K, max_r2, ctx=ctx)
    ref = lr.replay(R, p["bp"], radius, thr, min_size, max_size, max_K, max_r2)
    n_ok = int(np.isfinite(ref["cost"]).sum())
    print(f"REACHED ldsplit M {M} sizes {min_size}..{max_size} max_K {max_K} radius {radius} mode {mode} P {n_pop}: {n_ok} feasible K, "
          f"cost[:3] {ref['cost'][:3]}, closed boundaries {int((ref['max_r2'] > max_r2).sum())}")
    _same(got, ref, case)
    assert got["cost"].shape == (max_K,) and got["prev"].shape == (max_K, M + 1) and got["max_r2"].shape == (M + 1,)
    for K, ends in got["splits"].items():
        if ends is not None:
            sizes = np.diff(np.concatenate([[0], ends]))
            assert len(ends) == K and ends[-1] == M and sizes.min() >= min_size and sizes.max() <= max_size
            assert np.all(got["max_r2"][ends[:-1]] <= max_r2)


def test_the_cases_reach_what_they_are_meant_to(ctx):
    """Some K feasible and some not, a boundary closed by max_r2, a radius that ends a band inside max_size: in at least one case each"""
    p = _panel(129, seed=900 + 17, n_samples=(200, 300, 450, 600)[17 % 4], n_pop=1 + 17 % 3)
    got = hotpath.ld_split(p["G"], p["off"], p["bp"], p["w"], 1, 2_000, 0.02, 10, 26, 13, 0.6, ctx=ctx)
    assert np.isfinite(got["cost"]).any() and np.isinf(got["cost"]).any()
    assert (got["max_r2"] > 0.6).any() and (got["max_r2"][1:-1] <= 0.6).any()
    span = np.searchsorted(p["bp"], p["bp"].astype(np.int64) + 2_000, side="right") - np.arange(129)
    assert span.min() < 26 and span.max() > 2


def test_a_monomorphic_snp_is_counted_and_costs_nothing(ctx):
    M, d = 130, 70
    p = _panel(M, seed=41, n_samples=260, n_pop=1)
    G = p["G"].copy()
    G[d, :] = 1                                            # pooled LD of a row without variance is 0 / 0
    R = hotpath.ld_matrix(G, p["off"], None, 0, 1.0, ctx=ctx)
    assert np.all(np.isnan(np.delete(R[d], d)))
    got = hotpath.ld_split(G, p["off"], p["bp"], None, 0, BIG, 0.02, 10, 40, 9, 0.9, ctx=ctx)
    _same(got, lr.replay(R, p["bp"], BIG, 0.02, 10, 40, 9, 0.9), "NaN row")
    assert got["n_nonfinite"] == 2 * 39 and np.all(np.isfinite(got["max_r2"])) and np.isfinite(got["cost"]).any()


def test_the_bits_do_not_depend_on_the_source_the_row_order_or_the_queue(ctx, monkeypatch):
    M = 257
    p = _panel(M, seed=77, n_samples=330, n_pop=3)
    G, bp = p["G"], p["bp"]
    args = dict(pop_wgt=p["w"], mode=1, radius=20_000, thr_r2=0.02, min_size=20, max_size=90, max_K=8, max_r2=0.8)
    ref = hotpath.ld_split(G, p["off"], bp, ctx=ctx, **args)
    R = hotpath.ld_matrix_rows(G, np.arange(M), p["off"], p["w"], 1, 1.0, fmt=_lib.GENO_U8, ctx=ctx)
    _same(ref, lr.replay(R, bp, 20_000, 0.02, 20, 90, 8, 0.8), "host bytes")
    assert np.isfinite(ref["cost"]).sum() >= 3
    rows2, src_off = panel_mod.pack2bit(G, p["off"])
    perm = np.random.default_rng(5).permutation(M)
    inv = np.argsort(perm).astype(np.int32)                # store row of SNP s when the store holds the rows in `perm` order

    def sources(c):
        _same(hotpath.ld_split_rows(G, np.arange(M), p["off"], bp, fmt=_lib.GENO_U8, ctx=c, **args), ref, "host rows by index")
        _same(hotpath.ld_split_rows(np.ascontiguousarray(G[perm]), inv, p["off"], bp, fmt=_lib.GENO_U8, ctx=c, **args), ref, "host rows, permuted store")
        for fmt, store_rows, src in ((_lib.GENO_U8, G, None), (_lib.GENO_2BIT, rows2, src_off)):
            for order, name in ((None, "store order"), (perm, "permuted store")):
                store = hotpath.RowStore(np.ascontiguousarray(store_rows if order is None else store_rows[order]), ctx=c)
                try:
                    got = hotpath.ld_split_rows(store, np.arange(M) if order is None else inv, p["off"], bp, fmt=fmt, pop_src_off=src, ctx=c, **args)
                finally:
                    store.close()
                _same(got, ref, (fmt, name))

    sources(ctx)
    with monkeypatch.context() as m:                       # read when a context is made: one queue
        m.setenv("GAUSS_SIDE_STREAM", "0")
        c = hotpath.Context(0)
        try:
            _same(hotpath.ld_split(G, p["off"], bp, ctx=c, **args), ref, "one queue, host bytes")
            sources(c)
        finally:
            c.close()


def _planted(n_samples=400):
    """Three groups of 20, 25 and 15 SNPs: inside a group every SNP is the group's founder with one genotype in sixteen redrawn (r^2
    about 0.8 to the founder), the founders are drawn independently"""
    rng = np.random.default_rng(2025)
    sizes = (20, 25, 15)
    rows = []
    for n in sizes:
        f = rng.binomial(2, 0.5, size=n_samples).astype(np.uint8)
        for _ in range(n):
            g = f.copy()
            flip = rng.random(n_samples) < 1 / 16
            g[flip] = rng.integers(0, 3, size=int(flip.sum()))
            rows.append(g)
    G = np.ascontiguousarray(np.array(rows, dtype=np.uint8))
    G[:, 0], G[:, 1] = 0, 2
    bp = (1_000_000 + 500 * np.arange(len(G))).astype(np.int32)
    return G, bp, np.cumsum(sizes)


def test_three_planted_groups_give_the_planted_boundaries(ctx):
    G, bp, ends = _planted()
    M = len(G)
    off, w = np.array([0, 240, 400], dtype=np.int32), np.array([0.6, 0.4])
    kw = dict(radius=BIG, thr_r2=0.02, min_size=5, max_size=40, max_K=6, max_r2=1.0)
    cpu = oracle.compute_ld(G, off, w)
    # on the oracle's LD the planted split is the best 3-block split by far more than the two LDs differ: every other admissible set of
    # two boundaries costs at least 1e-6 more
    ref = lr.replay(cpu, bp, BIG, 0.02, 5, 40, 6, 1.0)
    assert list(ref["splits"][3]) == list(ends)
    best = ref["cost"][2]
    second = min(lr.cross_cost(cpu, bp, e, BIG, 0.02, 40)[0] for e in lr.compositions(M, 3, 5, 40) if list(e) != list(ends))
    print(f"REACHED ldsplit planted: best {best:.6f}, second best {second:.6f}")
    assert second - best > 1e-6
    got = hotpath.ld_split(G, off, bp, w, 1, ctx=ctx, **kw)
    assert list(got["splits"][3]) == list(ends)
    assert np.isinf(got["cost"][0]) and got["cost"][2] < got["cost"][3]           # 60 SNPs are no one block; a fourth block cuts a group
    R = hotpath.ld_matrix(G, off, w, 1, 1.0, ctx=ctx)
    _same(got, lr.replay(R, bp, BIG, 0.02, 5, 40, 6, 1.0), "planted")


def test_the_splits_are_optimal_on_the_oracles_ld(ctx):
    M = 130
    p = _panel(M, seed=333, n_samples=450, n_pop=3)
    radius, thr, lo, hi, max_K = 12_000, 0.02, 8, 45, 14
    cpu = oracle.compute_ld(p["G"], p["off"], p["w"])
    got = hotpath.ld_split(p["G"], p["off"], p["bp"], p["w"], 1, radius, thr, lo, hi, max_K, 1.0, ctx=ctx)
    want = lr.replay(cpu, p["bp"], radius, thr, lo, hi, max_K, 1.0)
    n_pairs = lr.n_band_pairs(p["bp"], hi, radius)
    bound = 4e-12 * n_pairs
    # no in-band r^2 of the oracle's sits within the LD's own error of thr_r2, so the threshold cuts the same pairs under both LDs
    E0 = lr.pair_values(cpu, p["bp"], hi, radius, 0.0)[1]
    gap = np.abs(E0[E0 > 0] - thr)
    assert gap.min() > 1e-9, gap.min()
    assert np.array_equal(np.isfinite(got["cost"]), np.isfinite(want["cost"])) and np.isfinite(want["cost"]).sum() >= 8
    worst = 0.0
    for K in range(1, max_K + 1):
        if got["splits"][K] is None:
            continue
        c = lr.cross_cost(cpu, p["bp"], got["splits"][K], radius, thr, hi)[0]
        worst = max(worst, abs(c - want["cost"][K - 1]))
    print(f"REACHED ldsplit on the oracle's LD: M {M}, {n_pairs} band pairs, worst |cost - optimum| {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound


def _call(ctx, **change):
    """gauss_ld_split_rows on 20 SNPs of 200 samples with every argument in order but the changed ones: (rc, message, arguments)"""
    p = _panel(20, seed=5, n_samples=200, n_pop=1)
    G = p["G"]
    a = dict(store=G.ctypes.data, ld=G.strides[0], fmt=_lib.GENO_U8, n_snp=20, off=p["off"], n_pop=1, bp=p["bp"], radius=100_000, thr_r2=0.02,
             min_size=2, max_size=10, max_K=5, max_r2=1.0, cost=np.full(128, -1.0), mode=0)
    a.update(change)
    rc = ctx.lib.gauss_ld_split_rows(ctx.handle, a["mode"], a["store"], a["ld"], a["fmt"], None, a["n_snp"], _lib.ptr(a["off"], _ip), None, None,
                                     a["n_pop"], 0, _lib.ptr(a["bp"], _ip), a["radius"], a["thr_r2"], a["min_size"], a["max_size"], a["max_K"],
                                     a["max_r2"], _lib.ptr(a["cost"], _dp), None, None, None)
    return rc, ctx.lib.gauss_last_error().decode(), a


def test_every_refusal_is_invalid_with_its_limit_and_launches_nothing(ctx):
    rc, msg, a = _call(ctx)
    assert rc == 0, msg                                    # the optional outputs are NULL here: allowed
    p = _panel(20, 5, 200, 1)
    R = hotpath.ld_matrix(p["G"], [0, 200], None, 0, ctx=ctx)
    assert np.array_equal(_bits(a["cost"][:5]), _bits(lr.replay(R, a["bp"], 100_000, 0.02, 2, 10, 5, 1.0)["cost"]))
    down = a["bp"].copy()
    down[[3, 4]] = down[[4, 3]] + np.array([1, 0], dtype=np.int32)
    queued = ctx.counters()                                # runs queued so far: a refusal adds none (the kernels come behind a run)
    for text, change in (("bp is NULL", dict(bp=None)), ("out_cost is NULL", dict(cost=None)),
                         ("n_snp = 0; a region holds 1 .. 8192 SNPs", dict(n_snp=0)),
                         ("max_size = 4097; a block holds 1 .. 4096 SNPs", dict(max_size=4097)), ("max_size = 0; a block holds 1 .. 4096 SNPs", dict(max_size=0)),
                         ("min_size = 11 is outside 1 .. max_size = 10", dict(min_size=11)), ("min_size = 0 is outside 1 .. max_size = 10", dict(min_size=0)),
                         ("max_K = 129; a call splits into 1 .. 128 blocks", dict(max_K=129)), ("max_K = 0; a call splits into 1 .. 128 blocks", dict(max_K=0)),
                         ("bp decreases at row 4", dict(bp=down)), ("radius = -1 is negative", dict(radius=-1)),
                         ("thr_r2 = -0.1 is outside [0, 1]", dict(thr_r2=-0.1)), ("thr_r2 = 1.5 is outside [0, 1]", dict(thr_r2=1.5)),
                         ("thr_r2 = nan is outside [0, 1]", dict(thr_r2=np.nan)), ("max_r2 = -0.1 is outside [0, 1]", dict(max_r2=-0.1)),
                         ("max_r2 = 1.5 is outside [0, 1]", dict(max_r2=1.5)), ("max_r2 = nan is outside [0, 1]", dict(max_r2=np.nan)),
                         ("bad mode 7", dict(mode=7)), ("n_pop must be in 1..64 (got 0)", dict(n_pop=0)), ("ld (100) < n_samples (200)", dict(ld=100))):
        untouched = np.full(128, -7.0)
        rc, msg, _ = _call(ctx, **(change if "cost" in change else dict(change, cost=untouched)))
        assert rc == -1 and text in msg, (text, rc, msg)   # GAUSS_E_INVALID
        assert np.all(untouched == -7.0) and ctx.counters() == queued, text
    # one SNP too many is refused on a store of two rows: no row or position is read
    tiny = np.array([[0, 1, 2, 1], [2, 1, 0, 1]], dtype=np.uint8)
    rc, msg, _ = _call(ctx, store=tiny.ctypes.data, ld=4, off=np.array([0, 4], dtype=np.int32), n_snp=8193, bp=np.zeros(2, dtype=np.int32))
    assert rc == -1 and "n_snp = 8193; a region holds 1 .. 8192 SNPs" in msg, (rc, msg)
