"""GPU: LD clumping on the device (k_clump.hip, gauss_ld_clump_rows) against tests/clump_ref.py.

(i)   On the matrix gauss_ld_rows returns for the same rows: owner, rank and n_clumps equal, r2 the bits of R[owner, j] * R[owner, j].
(ii)  On the CPU oracle's LD of the same genotypes: owner, rank and n_clumps equal for every case -- the cases are seeded, and under the
      oracle's LD no in-band pair of any of them has an r^2 within 1e-9 of r2_min (asserted, never skipped: the project's LD entries are
      within 1e-12 of the oracle's, so no pair can fall on the other side); r2 within 1e-12, the tolerance the project holds its LD to.
Then the same bits from host bytes, a resident one-byte store, a resident 2-bit store, rows in permuted store order and one queue; the
extremes; a monomorphic row; every refusal; and the calls that ran before give their bits after."""
import ctypes as C

import numpy as np
import pytest

import clump_ref as cr
import oracle
from gauss_amd import _lib, hotpath
from gauss_amd import panel as panel_mod

pytestmark = pytest.mark.gpu

_ip, _dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
_cache = {}


def _panel(S, seed, n_samples, n_pop):
    """S SNPs with LD between neighbours (a row is, three times in four, its predecessor with a tenth of its genotypes redrawn), every
    row varying inside the first population; about one SNP per 200 bp, a few of them at their predecessor's position; keys z^2 of
    1, 3 and 64 traits, some tied, some NaN"""
    k = (S, seed, n_samples, n_pop)
    if k in _cache:
        return _cache[k]
    rng = np.random.default_rng(seed)
    G = np.empty((S, n_samples), dtype=np.uint8)
    for s in range(S):
        if s and rng.random() < 0.75:
            G[s] = G[s - 1]
            flip = rng.random(n_samples) < 0.1
            G[s, flip] = rng.integers(0, 3, size=int(flip.sum()))
        else:
            G[s] = rng.binomial(2, rng.uniform(0.1, 0.9), size=n_samples)
    G[:, 0], G[:, 1] = 0, 2
    cuts = np.sort(rng.choice(np.arange(40, n_samples - 40, 40), size=n_pop - 1, replace=False)) if n_pop > 1 else []
    off = np.array([0, *cuts, n_samples], dtype=np.int32)
    bp = np.sort(rng.integers(1, 200 * S + 2, size=S)).astype(np.int32)
    for s in range(1, S):
        if rng.random() < 0.05:
            bp[s] = bp[s - 1]
    bp = np.sort(bp)
    key = np.round(rng.chisquare(1, size=(64, S)) * 5, 1)
    key[rng.random((64, S)) < 0.02] = np.nan
    out = _cache[k] = dict(G=np.ascontiguousarray(G), off=off, w=rng.uniform(0.1, 0.6, size=n_pop), bp=bp, key=key)
    return out


def _ld(ctx, p, mode):
    """the matrix gauss_ld_rows returns for the panel's rows (host bytes), and the oracle's"""
    k = ("ld", id(p), mode)
    if k not in _cache:
        G = p["G"]
        gpu = hotpath.ld_matrix_rows(G, np.arange(len(G)), p["off"], p["w"] if mode else None, mode, 1.0, fmt=_lib.GENO_U8, ctx=ctx)
        cpu = oracle.compute_ld(G, p["off"], p["w"]) if mode else oracle.ld_pooled(G, p["off"], 1.0)
        _cache[k] = (gpu, cpu)
    return _cache[k]


def _same(a, b, what):
    assert np.array_equal(a["owner"], b["owner"]), (what, "owner")
    assert np.array_equal(a["rank"], b["rank"]), (what, "rank")
    assert np.array_equal(np.asarray(a["n_clumps"]), np.asarray(b["n_clumps"])), (what, "n_clumps")
    assert np.array_equal(a["r2"], b["r2"], equal_nan=True), (what, "r2")


R2_MIN, K_INDEX, K_MEMBER = 0.37, 6.0, 1.5
RADII = (0, 5_000, 10 ** 8)           # one position; bands of about 50 rows, which end inside a 64-row run; beyond the region
SHAPES = (1, 2, 63, 64, 65, 257, 1030)


@pytest.mark.parametrize("M", SHAPES)
def test_shapes_radii_and_traits_against_both_lds(ctx, M):
    k = SHAPES.index(M)
    mode, n_pop, n_samples = k % 2, 1 + k % 3, (200, 300, 450, 600)[k % 4]
    T = {65: 64, 257: 3, 64: 3}.get(M, 1)
    p = _panel(M, seed=500 + k, n_samples=n_samples, n_pop=n_pop)
    w = p["w"] if mode else None
    key = p["key"][:T] if T > 1 else p["key"][0]
    ki, km = (K_INDEX, K_MEMBER) if M > 2 else (0.0, 0.0)      # (one or two SNPs: everything with a key takes part)
    gpu, cpu = _ld(ctx, p, mode)
    assert np.all(np.abs(gpu - cpu) <= 1e-12)
    for radius in RADII:
        got = hotpath.ld_clump(p["G"], p["off"], p["bp"], key, w, mode, radius, R2_MIN, ki, km, ctx=ctx)
        ref = cr.replay(gpu, p["bp"], key, radius, R2_MIN, ki, km)
        _same(got, ref, (M, radius, "the GPU's own LD"))
        own = np.atleast_2d(got["owner"])
        r2 = np.atleast_2d(got["r2"])
        j = np.arange(M)
        for t in range(own.shape[0]):
            has = (own[t] >= 0) & (own[t] != j)
            r = gpu[own[t][has], j[has]]
            assert np.array_equal(r2[t][has], r * r), (M, radius, t)
        # (ii): no in-band pair sits on the threshold under the oracle's LD, so the oracle's LD gives the same clumps
        band = (np.abs(p["bp"].astype(np.int64)[:, None] - p["bp"][None, :]) <= radius) & ~np.eye(M, dtype=bool)
        gap = np.abs((cpu * cpu)[band] - R2_MIN)
        assert gap.size == 0 or float(gap.min()) > 1e-9, (M, radius, float(gap.min()))
        want = cr.replay(cpu, p["bp"], key, radius, R2_MIN, ki, km)
        for name in ("owner", "rank", "n_clumps"):
            assert np.array_equal(np.asarray(got[name]), np.asarray(want[name])), (M, radius, name, "the oracle's LD")
        assert np.array_equal(np.isnan(got["r2"]), np.isnan(want["r2"]))
        err = np.nanmax(np.abs(got["r2"] - want["r2"])) if np.any(~np.isnan(want["r2"])) else 0.0
        print(f"REACHED clump M {M} T {T} mode {mode} P {n_pop} N {n_samples} radius {radius}: clumps {np.atleast_1d(got['n_clumps']).tolist()[:3]} "
              f"r2 against the oracle's LD {float(err):.2e} (bound 1e-12), nearest in-band r^2 to r2_min {float(gap.min()) if gap.size else np.inf:.2e}")
        assert err <= 1e-12


def test_the_bits_do_not_depend_on_the_source_the_row_order_or_the_queue(ctx, monkeypatch):
    M = 257
    p = _panel(M, seed=77, n_samples=330, n_pop=3)
    G, bp, key = p["G"], p["bp"], p["key"][:3]
    args = dict(pop_wgt=p["w"], mode=1, radius=5_000, r2_min=R2_MIN, key_index=K_INDEX, key_member=K_MEMBER)
    ref = hotpath.ld_clump(G, p["off"], bp, key, ctx=ctx, **args)
    _same(ref, cr.replay(_ld(ctx, p, 1)[0], bp, key, 5_000, R2_MIN, K_INDEX, K_MEMBER), "host bytes")
    assert 1 < ref["n_clumps"].min() and ref["n_clumps"].max() < M
    rows2, src_off = panel_mod.pack2bit(G, p["off"])
    perm = np.random.default_rng(5).permutation(M)
    inv = np.argsort(perm).astype(np.int32)                # store row of SNP s when the store holds the rows in `perm` order

    def sources(c):
        _same(hotpath.ld_clump_rows(G, np.arange(M), p["off"], bp, key, fmt=_lib.GENO_U8, ctx=c, **args), ref, "host rows by index")
        _same(hotpath.ld_clump_rows(np.ascontiguousarray(G[perm]), inv, p["off"], bp, key, fmt=_lib.GENO_U8, ctx=c, **args), ref, "host rows, permuted store")
        for fmt, store_rows, src in ((_lib.GENO_U8, G, None), (_lib.GENO_2BIT, rows2, src_off)):
            for order, name in ((None, "store order"), (perm, "permuted store")):
                store = hotpath.RowStore(np.ascontiguousarray(store_rows if order is None else store_rows[order]), ctx=c)
                try:
                    got = hotpath.ld_clump_rows(store, np.arange(M) if order is None else inv, p["off"], bp, key, fmt=fmt, pop_src_off=src, ctx=c, **args)
                finally:
                    store.close()
                _same(got, ref, (fmt, name))

    sources(ctx)
    with monkeypatch.context() as m:                       # read when a context is made: one queue
        m.setenv("GAUSS_SIDE_STREAM", "0")
        c = hotpath.Context(0)
        try:
            _same(hotpath.ld_clump(G, p["off"], bp, key, ctx=c, **args), ref, "one queue, host bytes")
            sources(c)
        finally:
            c.close()


def test_the_extremes(ctx):
    """Every SNP its own clump at M = 1 030 (r2_min = 1 on distinct rows: M dependent steps), all SNPs in one clump (every row the
    same), nobody eligible"""
    M = 1030
    p = _panel(M, seed=506, n_samples=600, n_pop=1)
    key = np.nan_to_num(p["key"][0], nan=0.25)
    R = _ld(ctx, p, 0)[0]
    assert np.all((R * R)[~np.eye(M, dtype=bool)] < 1.0)
    got = hotpath.ld_clump(p["G"], p["off"], p["bp"], key, None, 0, 10 ** 8, 1.0, 0.0, 0.0, ctx=ctx)
    assert got["n_clumps"] == M and np.array_equal(got["owner"], np.arange(M)) and np.all(got["r2"] == 1.0)
    assert np.array_equal(got["rank"][np.lexsort((np.arange(M), -key))], np.arange(1, M + 1))
    same_rows = np.repeat(p["G"][:1], M, axis=0)
    got = hotpath.ld_clump(same_rows, p["off"], p["bp"], key, None, 0, 10 ** 8, 0.99, 0.0, 0.0, ctx=ctx)
    lead = int(np.lexsort((np.arange(M), -key))[0])
    assert got["n_clumps"] == 1 and np.all(got["owner"] == lead) and got["rank"][lead] == 1 and got["rank"].sum() == 1
    got = hotpath.ld_clump(p["G"], p["off"], p["bp"], key, None, 0, 10 ** 8, 0.5, float(key.max()) + 1.0, 0.0, ctx=ctx)
    assert got["n_clumps"] == 0 and np.all(got["owner"] == -1) and np.all(got["rank"] == 0) and np.all(np.isnan(got["r2"]))


def test_a_radius_beyond_any_position_is_no_limit(ctx):
    """Positions are 32-bit: a radius of 2^32 and above is every band already, up to INT64_MAX (bp +- radius does not wrap)"""
    p = _panel(257, seed=506, n_samples=300, n_pop=3)
    key = p["key"][:3]
    ref = hotpath.ld_clump(p["G"], p["off"], p["bp"], key, p["w"], 1, 10 ** 8, R2_MIN, K_INDEX, K_MEMBER, ctx=ctx)
    assert np.all(ref["n_clumps"] < (key >= K_INDEX).sum(axis=1))              # something joins a lead
    for radius in (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63 - 2 ** 31, 2 ** 63 - 1):
        _same(hotpath.ld_clump(p["G"], p["off"], p["bp"], key, p["w"], 1, radius, R2_MIN, K_INDEX, K_MEMBER, ctx=ctx), ref, radius)


def test_a_monomorphic_row_is_never_a_member_and_leads_alone(ctx):
    M, d = 130, 70
    p = _panel(M, seed=41, n_samples=260, n_pop=1)
    G = p["G"].copy()
    G[d, :] = 1                                            # pooled LD of a row without variance is 0 / 0
    R = hotpath.ld_matrix(G, p["off"], None, 0, 1.0, ctx=ctx)
    assert np.all(np.isnan(np.delete(R[d], d)))
    key = np.nan_to_num(p["key"][0], nan=0.5)
    for kd, ki in ((key.max() + 1.0, 0.0), (0.0, 0.0), (3.0, 4.0)):      # it leads first; it leads last; it may only be a member
        k = key.copy()
        k[d] = kd
        got = hotpath.ld_clump(G, p["off"], p["bp"], k, None, 0, 10 ** 8, 0.0, ki, 0.0, ctx=ctx)      # r2_min = 0: anything finite joins
        _same(got, cr.replay(R, p["bp"], k, 10 ** 8, 0.0, ki, 0.0), (kd, ki))
        assert np.all(np.delete(got["owner"], d) != d)
        if kd >= ki:
            assert got["owner"][d] == d and got["r2"][d] == 1.0 and (got["rank"][d] == 1 if kd > 1.0 else got["rank"][d] > 1)
        else:
            assert got["owner"][d] == -1 and np.isnan(got["r2"][d]) and got["rank"][d] == 0


def _call(ctx, **change):
    """gauss_ld_clump_rows on 20 SNPs of 200 samples with every argument in order but the changed ones: (rc, message)"""
    p = _panel(20, seed=5, n_samples=200, n_pop=1)
    G, bp, key = p["G"], p["bp"], np.ascontiguousarray(np.nan_to_num(p["key"][:2], nan=1.0))
    a = dict(store=G.ctypes.data, ld=G.strides[0], fmt=_lib.GENO_U8, n_snp=20, off=p["off"], n_pop=1, bp=bp, key=key, n_key=2, radius=1000,
             r2_min=0.5, key_index=2.0, key_member=1.0, owner=np.zeros((2, 20), dtype=np.int32), mode=0)
    a.update(change)
    rc = ctx.lib.gauss_ld_clump_rows(ctx.handle, a["mode"], a["store"], a["ld"], a["fmt"], None, a["n_snp"], _lib.ptr(a["off"], _ip), None, None,
                                     a["n_pop"], 0, _lib.ptr(a["bp"], _ip), _lib.ptr(a["key"], _dp), a["n_key"], a["radius"], a["r2_min"],
                                     a["key_index"], a["key_member"], _lib.ptr(a["owner"], _ip), None, None, None)
    return rc, ctx.lib.gauss_last_error().decode(), a


def test_every_refusal_is_invalid_with_its_message(ctx):
    rc, msg, a = _call(ctx)
    assert rc == 0, msg                                    # the optional outputs are NULL here: allowed
    assert np.array_equal(a["owner"], cr.replay(hotpath.ld_matrix(_panel(20, 5, 200, 1)["G"], [0, 200], None, 0, ctx=ctx), a["bp"], a["key"],
                                                1000, 0.5, 2.0, 1.0)["owner"])
    down = a["bp"].copy()
    down[[3, 4]] = down[[4, 3]] + np.array([1, 0], dtype=np.int32)
    for text, change in (("bp is NULL", dict(bp=None)), ("key is NULL", dict(key=None)), ("out_owner is NULL", dict(owner=None)),
                         ("n_key = 0; a call clumps 1 .. 64 traits", dict(n_key=0)), ("n_key = 65; a call clumps 1 .. 64 traits", dict(n_key=65)),
                         ("n_snp = 0; a region holds 1 .. 8192 SNPs", dict(n_snp=0)), ("bp decreases at row 4", dict(bp=down)),
                         ("radius = -1 is negative", dict(radius=-1)), ("r2_min = -0.1 is outside [0, 1]", dict(r2_min=-0.1)),
                         ("r2_min = 1.5 is outside [0, 1]", dict(r2_min=1.5)), ("r2_min = nan is outside [0, 1]", dict(r2_min=np.nan)),
                         ("both thresholds must be finite", dict(key_index=np.inf)), ("both thresholds must be finite", dict(key_member=-np.inf)),
                         ("both thresholds must be finite", dict(key_index=np.nan)), ("key_member = 3 is above key_index = 2", dict(key_member=3.0)),
                         ("bad mode 7", dict(mode=7)), ("n_pop must be in 1..64 (got 0)", dict(n_pop=0)), ("ld (100) < n_samples (200)", dict(ld=100))):
        rc, msg, _ = _call(ctx, **change)
        assert rc == -1 and text in msg, (text, rc, msg)   # GAUSS_E_INVALID
    # one SNP too many is refused on a store of two rows: no row, position or key is read
    tiny = np.array([[0, 1, 2, 1], [2, 1, 0, 1]], dtype=np.uint8)
    rc, msg, _ = _call(ctx, store=tiny.ctypes.data, ld=4, off=np.array([0, 4], dtype=np.int32), n_snp=8193, bp=np.zeros(2, dtype=np.int32),
                       key=np.zeros(2), n_key=1)
    assert rc == -1 and "n_snp = 8193; a region holds 1 .. 8192 SNPs" in msg, (rc, msg)


def test_the_calls_that_ran_before_give_their_bits_after(ctx):
    p = _panel(257, seed=12, n_samples=240, n_pop=2)
    G = p["G"]
    gm, gu = np.ascontiguousarray(G[::2][:70]), np.ascontiguousarray(G[1::2][:100])
    z1 = np.random.default_rng(1).normal(size=70)

    def before():
        ld = hotpath.ld_matrix_rows(G, np.arange(257), p["off"], p["w"], 1, 1.0, fmt=_lib.GENO_U8, ctx=ctx)
        imp = hotpath.impute_window(1, gm, gu, p["off"], p["w"], z1, ctx=ctx)
        return ld, imp

    ld0, imp0 = before()
    got = hotpath.ld_clump(G, p["off"], p["bp"], p["key"][:64], p["w"], 1, 5_000, R2_MIN, K_INDEX, K_MEMBER, ctx=ctx)
    _same(got, cr.replay(ld0, p["bp"], p["key"][:64], 5_000, R2_MIN, K_INDEX, K_MEMBER), "64 traits")
    ld1, imp1 = before()
    assert np.array_equal(ld0, ld1)
    for name in ("z", "info"):
        assert np.array_equal(imp0[name], imp1[name]), name
    assert imp0["status"] == imp1["status"]
