"""GPU: the gene-based sum-of-chi2 test on the device (k_sumchi2.hip, gauss_gene_sumchi2[_rows]) against tests/sumchi2_ref.py.

(i)   On the blocks gauss_gene_ld_batch_rows(diag = 1) returns for the same rows: kept, n_kept, status and top equal the replay's, q the
      bits of the ascending-order sum.
(ii)  lambda against the replay's Jacobi on the kept block: the bits are expected (no contraction; fp64 division and square root round
      correctly); asserted within 1e-12 max(1, lambda_max), sweeps equal.  Against numpy.linalg.eigvalsh within 8 k 2^-52 lambda_max.
(iii) On the CPU oracle's LD of the same genotypes: kept equal -- no pair of any case has an r^2 within 1e-9 of prune_r2 under the
      oracle's LD (asserted), and the project's LD entries are within 1e-12 of the oracle's -- and lambda within k 1e-12 plus (ii)'s bound.
(iv)  The same bits from host bytes, host rows by index, a resident one-byte store and a resident 2-bit store, on one queue too; a gene
      alone gives its bits of the batch; three traits in one call give the bits of three calls.
(v)   pval equals the replay's saddlepoint within 1e-10 relative.
(vi)  Every refusal with its message.
(vii) The calls that ran before give their bits after a 64-trait call."""
import ctypes as C

import numpy as np
import pytest

import oracle
import sumchi2_ref as sr
from gauss_amd import _lib, hotpath
from gauss_amd import panel as panel_mod

pytestmark = pytest.mark.gpu

_ip, _dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
_cache = {}
EPS = 2.0 ** -52


def _rows(rng, n, n_samples, chain=0.75, flip_p=0.1):
    """n SNPs with LD between neighbours (a row is, `chain` of the time, its predecessor with `flip_p` of its genotypes redrawn); every row
    varies inside the first 40 samples (the first population is never shorter)"""
    G = np.empty((n, n_samples), dtype=np.uint8)
    for s in range(n):
        if s and rng.random() < chain:
            G[s] = G[s - 1]
            flip = rng.random(n_samples) < flip_p
            G[s, flip] = rng.integers(0, 3, size=int(flip.sum()))
        else:
            G[s] = rng.binomial(2, rng.uniform(0.1, 0.9), size=n_samples)
    if n:
        G[:, 0], G[:, 1] = 0, 2
    return G


def _case(name):
    """dict(G, gene_off, off, w, mode, Z [64, S], r2): the genes of one call"""
    if name in _cache:
        return _cache[name]
    seed, n_samples, n_pop, mode, r2, sizes = {
        # fewer samples than SNPs from n = 64 on: zero and slightly negative eigenvalues
        "small60": (11, 60, 1, 0, 0.9, (0, 1, 2, 3, 31, 32, 33, 64, 127, 128)),
        "mid300": (12, 300, 2, 1, 0.9, (33, 0, 128, 1, 64, 2, 127, 3, 32, 31)),
        "noprune": (13, 200, 1, 1, 1.0, (129, 128, 33, 1)),                     # prune_r2 = 1: 129 kept is too many
        "big600": (14, 600, 3, 1, 0.9, (129, 300, 1024, 5)),
        "mono": (15, 240, 1, 0, 0.9, (40, 2, 1)),
    }[name]
    rng = np.random.default_rng(seed)
    parts = []
    for n in sizes:
        if name == "noprune":
            g = _rows(rng, n, n_samples, chain=0.0)                                 # independent rows: no r^2 near 1
        elif name == "big600" and n == 129:
            g = _rows(rng, 128, n_samples, chain=0.0)
            g = np.vstack([g[:57], g[56:]])                                         # rows 56 and 57 identical: k = 128
        elif name == "big600" and n == 300:
            g = np.repeat(_rows(rng, 100, n_samples, chain=0.0), 3, axis=0)        # 100 triples of identical rows: k = 100
        elif name == "big600" and n == 1024:
            g = _rows(rng, 1024, n_samples, chain=0.97, flip_p=0.004)               # long chains of near copies: heavy pruning
        else:
            g = _rows(rng, n, n_samples)
        parts.append(g)
    G = np.ascontiguousarray(np.vstack(parts))
    gene_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    if name == "mono":
        G[7, :] = 1                                                                 # gene 0, row 7: pooled LD 0 / 0
        G[41, :] = 1                                                                # gene 1 (two SNPs), its second: both rows are NaN rows
    cuts = np.sort(rng.choice(np.arange(40, n_samples - 40, 20), size=n_pop - 1, replace=False)) if n_pop > 1 else []
    off = np.array([0, *cuts, n_samples], dtype=np.int32)
    Z = np.round(rng.normal(size=(64, len(G))) * 1.5, 2)                            # (rounded: ties in z^2 happen)
    out = _cache[name] = dict(G=G, gene_off=gene_off, off=off, w=rng.uniform(0.1, 0.6, size=n_pop), mode=mode, Z=Z, r2=r2, sizes=sizes)
    return out


def _blocks(ctx, c):
    """the blocks gauss_gene_ld_batch_rows(diag = 1) returns for the case's genes (host bytes), and the oracle's"""
    k = ("blocks", id(c))
    if k not in _cache:
        G, mode = c["G"], c["mode"]
        gpu = hotpath.gene_ld_batch_rows(G, np.arange(len(G)), c["off"], c["gene_off"], c["w"] if mode else None, mode, 1.0, fmt=_lib.GENO_U8, ctx=ctx)
        cpu = []
        for g in range(len(c["sizes"])):
            rows = G[c["gene_off"][g]:c["gene_off"][g + 1]]
            if len(rows) == 0:
                cpu.append(np.zeros((0, 0)))
            elif len(rows) == 1:
                cpu.append(np.ones((1, 1)))
            else:
                cpu.append(oracle.compute_ld(rows, c["off"], c["w"]) if mode else oracle.ld_pooled(rows, c["off"], 1.0))
        _cache[k] = (gpu, cpu)
    return _cache[k]


def _replay(ctx, c, T):
    """the replay of every gene of the case on the GPU's own blocks, for the first T traits"""
    k = ("replay", id(c), T)
    if k not in _cache:
        gpu, _ = _blocks(ctx, c)
        go = c["gene_off"]
        _cache[k] = [sr.gene(gpu[g], c["Z"][:T, go[g]:go[g + 1]], c["r2"]) for g in range(len(gpu))]
    return _cache[k]


def _run(ctx, c, T, **kw):
    z = c["Z"][:T] if T > 1 else c["Z"][0]
    return hotpath.gene_sumchi2(c["G"], c["off"], c["gene_off"], z, c["w"] if c["mode"] else None, c["mode"], c["r2"], ctx=ctx, **kw)


def _same(a, b, what):
    for name in ("kept", "n_kept", "status", "sweeps", "top"):
        assert np.array_equal(a[name], b[name]), (what, name)
    for name in ("lam", "q", "pval"):
        assert np.array_equal(a[name], b[name], equal_nan=True), (what, name)


CASES = (("small60", 1), ("mid300", 3), ("noprune", 1), ("big600", 64), ("mono", 3))


@pytest.mark.parametrize("name,T", CASES)
def test_genes_against_the_replay_eigvalsh_and_the_oracles_ld(ctx, name, T):
    c = _case(name)
    go, r2 = c["gene_off"], c["r2"]
    gpu, cpu = _blocks(ctx, c)
    if name == "mono":
        assert np.all(np.isnan(np.delete(gpu[0][7], 7))) and np.isnan(gpu[1][0, 1])
    got = _run(ctx, c, T)
    ref = _replay(ctx, c, T)
    q, top, pval = (np.atleast_2d(got[n]) for n in ("q", "top", "pval"))
    worst_j = worst_e = worst_o = 0.0
    for g, want in enumerate(ref):
        n, k = int(go[g + 1] - go[g]), want["n_kept"]
        what = (name, "gene", g, "n", n, "k", k)
        # (i)
        assert np.array_equal(got["kept"][go[g]:go[g + 1]], want["kept"]), what
        assert got["n_kept"][g] == k and got["status"][g] == want["status"], what
        assert np.array_equal(top[:, g], want["top"]), what
        assert np.array_equal(q[:, g], want["q"], equal_nan=True), what
        # (ii)
        lam = got["lam"][g]
        assert np.all(np.isnan(lam[k if want["status"] == 0 else 0:])), what
        assert got["sweeps"][g] == want["sweeps"], (what, got["sweeps"][g], want["sweeps"])
        if want["status"] == 0:
            lmax = float(want["lam"][0])
            dj = float(np.abs(lam[:k] - want["lam"][:k]).max())
            worst_j = max(worst_j, dj / max(1.0, lmax))
            assert dj <= 1e-12 * max(1.0, lmax), (what, dj)
            idx = np.flatnonzero(want["kept"])
            ev = np.linalg.eigvalsh(gpu[g][np.ix_(idx, idx)])[::-1]
            de = float(np.abs(lam[:k] - ev).max())
            worst_e = max(worst_e, de / (k * EPS * lmax))
            assert de <= 8 * k * EPS * lmax, (what, de / (k * EPS * lmax))
            assert np.all(np.diff(lam[:k]) <= 0)
            # (v)
            for t in range(T):
                want_p = sr.saddle(want["lam"], want["q"][t])
                if np.isnan(want_p):
                    assert np.isnan(pval[t, g]), what
                else:
                    assert abs(pval[t, g] - want_p) <= 1e-10 * want_p, (what, t, pval[t, g], want_p)
        else:
            assert np.all(np.isnan(pval[:, g])), what
        # (iii)
        if n:
            assert np.all(np.abs(gpu[g] - cpu[g])[~np.isnan(cpu[g])] <= 1e-12) and np.array_equal(np.isnan(gpu[g]), np.isnan(cpu[g])), what
            with np.errstate(invalid="ignore"):
                gap = np.abs(cpu[g] * cpu[g] - r2)[~np.eye(n, dtype=bool)]
            gap = gap[~np.isnan(gap)]
            assert gap.size == 0 or float(gap.min()) > 1e-9, (what, float(gap.min()))
            kept_o, _ = sr.prune(cpu[g], r2)
            assert np.array_equal(kept_o, want["kept"]), what
            if want["status"] == 0:
                ev_o = np.linalg.eigvalsh(cpu[g][np.ix_(idx, idx)])[::-1]
                do = float(np.abs(lam[:k] - ev_o).max())
                worst_o = max(worst_o, do)
                assert do <= k * 1e-12 + 8 * k * EPS * lmax, (what, do)
    print(f"REACHED sumchi2 {name} T {T} mode {c['mode']} N {c['G'].shape[1]} prune_r2 {r2}: n {list(c['sizes'])} kept {got['n_kept'].tolist()} "
          f"status {got['status'].tolist()} sweeps {got['sweeps'].tolist()}; lambda against the replay {worst_j:.2e} of max(1, lambda_max) (bound 1e-12), "
          f"against eigvalsh {worst_e:.2f} of k 2^-52 lambda_max (bound 8), against the oracle's LD {worst_o:.2e}")
    # what the case is there for
    st = dict(zip(c["sizes"], got["status"].tolist()))
    kk = dict(zip(c["sizes"], got["n_kept"].tolist()))
    if name in ("small60", "mid300"):
        assert st[0] == _lib.ST_SUMCHI2_EMPTY and kk[0] == 0 and np.all(q[:, list(c["sizes"]).index(0)] == 0.0)
        assert all(st[n] == 0 for n in c["sizes"] if n) and kk[1] == 1 and got["lam"][list(c["sizes"]).index(1), 0] == 1.0
    if name == "small60":
        g128 = list(c["sizes"]).index(128)
        assert kk[128] > 60 and np.nanmin(got["lam"][g128]) < 1e-10                 # more kept SNPs than samples: a singular block
    if name == "noprune":
        assert st[129] == _lib.ST_SUMCHI2_TOOLARGE and kk[129] == 129 and kk[128] == 128 and st[128] == 0
        assert np.all(got["kept"] == 1)
    if name == "big600":
        assert (kk[129], st[129]) == (128, 0) and (kk[300], st[300]) == (100, 0) and 1 < kk[1024] < 1024
        g300 = list(c["sizes"]).index(300)
        assert np.array_equal(got["kept"][go[g300]:go[g300 + 1]], np.tile([1, 0, 0], 100))
    if name == "mono":
        assert got["kept"][7] == 0 and st[2] == _lib.ST_SUMCHI2_EMPTY and kk[2] == 0 and kk[1] == 1


def test_a_nan_z_of_a_kept_row_spoils_that_trait_alone(ctx):
    c = _case("mid300")
    base = _run(ctx, c, 3)
    go = c["gene_off"]
    g = list(c["sizes"]).index(64)
    row = int(go[g] + np.flatnonzero(base["kept"][go[g]:go[g + 1]])[2])
    Z = c["Z"][:3].copy()
    Z[1, row] = np.nan
    Z[2, go[g]:go[g + 1]] = np.nan                                                   # no finite z in the gene: top -1
    got = hotpath.gene_sumchi2(c["G"], c["off"], go, Z, c["w"], 1, c["r2"], ctx=ctx)
    assert np.isnan(got["q"][1, g]) and np.isnan(got["pval"][1, g]) and got["top"][2, g] == -1 and np.isnan(got["q"][2, g])
    assert got["q"][0, g] == base["q"][0, g] and got["top"][1, g] == sr.top_row(Z[1, go[g]:go[g + 1]])
    others = np.arange(len(c["sizes"])) != g
    assert np.array_equal(got["q"][:, others], base["q"][:, others]) and np.array_equal(got["lam"], base["lam"], equal_nan=True)


def test_the_bits_do_not_depend_on_the_source_the_queue_the_batch_or_the_trait_count(ctx, monkeypatch):
    c = _case("mid300")
    G, go, w, S = c["G"], c["gene_off"], c["w"], len(c["G"])
    ref = _run(ctx, c, 3)
    rows2, src_off = panel_mod.pack2bit(G, c["off"])
    args = dict(pop_wgt=w, mode=1, prune_r2=c["r2"])

    def sources(cx):
        _same(hotpath.gene_sumchi2_rows(G, np.arange(S), c["off"], go, c["Z"][:3], fmt=_lib.GENO_U8, ctx=cx, **args), ref, "host rows by index")
        for fmt, store_rows, src in ((_lib.GENO_U8, G, None), (_lib.GENO_2BIT, rows2, src_off)):
            store = hotpath.RowStore(np.ascontiguousarray(store_rows), ctx=cx)
            try:
                got = hotpath.gene_sumchi2_rows(store, np.arange(S), c["off"], go, c["Z"][:3], fmt=fmt, pop_src_off=src, ctx=cx, **args)
            finally:
                store.close()
            _same(got, ref, ("resident store", fmt))

    sources(ctx)
    with monkeypatch.context() as m:                       # read when a context is made: one queue
        m.setenv("GAUSS_SIDE_STREAM", "0")
        cx = hotpath.Context(0)
        try:
            _same(hotpath.gene_sumchi2(G, c["off"], go, c["Z"][:3], ctx=cx, **args), ref, "one queue, host bytes")
            sources(cx)
        finally:
            cx.close()
    # a gene alone
    for g in (list(c["sizes"]).index(128), list(c["sizes"]).index(33)):
        r0, r1 = int(go[g]), int(go[g + 1])
        one = hotpath.gene_sumchi2(np.ascontiguousarray(G[r0:r1]), c["off"], [0, r1 - r0], c["Z"][:3, r0:r1], ctx=ctx, **args)
        assert np.array_equal(one["kept"], ref["kept"][r0:r1]) and one["n_kept"][0] == ref["n_kept"][g] and one["sweeps"][0] == ref["sweeps"][g]
        assert np.array_equal(one["lam"][0], ref["lam"][g], equal_nan=True) and np.array_equal(one["q"][:, 0], ref["q"][:, g])
        assert np.array_equal(one["top"][:, 0], ref["top"][:, g]) and np.array_equal(one["pval"][:, 0], ref["pval"][:, g])
    # three traits, three calls
    for t in range(3):
        one = hotpath.gene_sumchi2(G, c["off"], go, c["Z"][t], ctx=ctx, **args)
        assert one["q"].shape == (len(c["sizes"]),) and one["top"].ndim == 1 and one["pval"].ndim == 1
        assert np.array_equal(one["q"], ref["q"][t]) and np.array_equal(one["top"], ref["top"][t]) and np.array_equal(one["pval"], ref["pval"][t], equal_nan=True)
        assert np.array_equal(one["lam"], ref["lam"], equal_nan=True) and np.array_equal(one["kept"], ref["kept"])


def _call(ctx, **change):
    """gauss_gene_sumchi2_rows on 20 SNPs of 200 samples in 3 genes with every argument in order but the changed ones: (rc, message, args)"""
    rng = np.random.default_rng(5)
    G = _rows(rng, 20, 200)
    a = dict(store=G.ctypes.data, ld=G.strides[0], fmt=_lib.GENO_U8, n_snp=20, off=np.array([0, 200], dtype=np.int32), n_pop=1, mode=0,
             gene_off=np.array([0, 7, 7, 20], dtype=np.int32), n_gene=3, z=np.ascontiguousarray(rng.normal(size=(2, 20))), n_trait=2, r2=0.9,
             kept=np.zeros(20, dtype=np.int32), n_kept=np.zeros(3, dtype=np.int32), lam=np.zeros((3, 128)), q=np.zeros((2, 3)), G=G)
    a.update(change)
    rc = ctx.lib.gauss_gene_sumchi2_rows(ctx.handle, a["mode"], a["store"], a["ld"], a["fmt"], None, a["n_snp"], _lib.ptr(a["off"], _ip), None, None,
                                         a["n_pop"], _lib.ptr(a["gene_off"], _ip), a["n_gene"], 0, _lib.ptr(a["z"], _dp), a["n_trait"], a["r2"],
                                         _lib.ptr(a["kept"], _ip), _lib.ptr(a["n_kept"], _ip), _lib.ptr(a["lam"], _dp), _lib.ptr(a["q"], _dp),
                                         None, None, None)
    return rc, ctx.lib.gauss_last_error().decode(), a


def test_every_refusal_is_invalid_with_its_message(ctx):
    rc, msg, a = _call(ctx)
    assert rc == 0, msg                                    # the optional outputs are NULL here: allowed
    want = hotpath.gene_sumchi2(a["G"], a["off"], a["gene_off"], a["z"], None, 0, 0.9, ctx=ctx)
    assert np.array_equal(a["kept"], want["kept"]) and np.array_equal(a["lam"], want["lam"], equal_nan=True) and np.array_equal(a["q"], want["q"])
    who = "gauss_gene_sumchi2_rows: "
    for text, change in ((who + "z is NULL", dict(z=None)), (who + "out_kept is NULL", dict(kept=None)), (who + "out_n_kept is NULL", dict(n_kept=None)),
                         (who + "out_lam is NULL", dict(lam=None)), (who + "out_q is NULL", dict(q=None)),
                         (who + "gene_off is NULL or n_gene < 1", dict(gene_off=None)), (who + "gene_off is NULL or n_gene < 1", dict(n_gene=0)),
                         (who + "n_trait = 0; a call tests 1 .. 64 traits", dict(n_trait=0)), (who + "n_trait = 65; a call tests 1 .. 64 traits", dict(n_trait=65)),
                         (who + "prune_r2 = 0 is outside (0, 1]", dict(r2=0.0)), (who + "prune_r2 = -0.1 is outside (0, 1]", dict(r2=-0.1)),
                         (who + "prune_r2 = 1.5 is outside (0, 1]", dict(r2=1.5)), (who + "prune_r2 = nan is outside (0, 1]", dict(r2=np.nan)),
                         ("gene_off out of range at gene 2", dict(gene_off=np.array([0, 7, 7, 21], dtype=np.int32))),
                         ("gene_off out of range at gene 1", dict(gene_off=np.array([0, 7, 5, 20], dtype=np.int32))),
                         ("bad mode 7", dict(mode=7)), ("n_pop must be in 1..64 (got 0)", dict(n_pop=0)), ("ld (100) < n_samples (200)", dict(ld=100))):
        rc, msg, _ = _call(ctx, **change)
        assert rc == -1 and text in msg, (text, rc, msg)   # GAUSS_E_INVALID
    # one SNP too many in a gene is refused on a store of two rows: no row and no z is read
    tiny = np.array([[0, 1, 2, 1], [2, 1, 0, 1]], dtype=np.uint8)
    rc, msg, _ = _call(ctx, store=tiny.ctypes.data, ld=4, off=np.array([0, 4], dtype=np.int32), n_snp=1026, z=np.zeros(2), n_trait=1,
                       gene_off=np.array([0, 1, 1026], dtype=np.int32), n_gene=2)
    assert rc == -1 and "gene 1 holds 1025 SNPs; a gene holds at most 1024 before pruning" in msg, (rc, msg)
    with pytest.raises(ValueError, match="z has shape"):
        hotpath.gene_sumchi2(a["G"], a["off"], a["gene_off"], np.zeros(19), None, 0, 0.9, ctx=ctx)


def test_the_calls_that_ran_before_give_their_bits_after(ctx):
    c = _case("mid300")
    G = c["G"]
    gm, gu = np.ascontiguousarray(G[::2][:70]), np.ascontiguousarray(G[1::2][:100])
    z1 = np.random.default_rng(1).normal(size=70)

    def before():
        ld = hotpath.gene_ld_batch_rows(G, np.arange(len(G)), c["off"], c["gene_off"], c["w"], 1, 1.0, fmt=_lib.GENO_U8, ctx=ctx)
        imp = hotpath.impute_window(1, gm, gu, c["off"], c["w"], z1, ctx=ctx)
        return ld, imp

    ld0, imp0 = before()
    got = _run(ctx, c, 64)
    ref = _replay(ctx, c, 3)
    for g, want in enumerate(ref):
        assert np.array_equal(got["q"][:3, g], want["q"]) and np.array_equal(got["lam"][g], want["lam"], equal_nan=True), g
    go = c["gene_off"]
    for t in (17, 63):
        assert np.array_equal(got["q"][t], [sr.qstat(c["Z"][t, go[g]:go[g + 1]], ref[g]["kept"]) for g in range(len(ref))])
        assert np.array_equal(got["top"][t], [sr.top_row(c["Z"][t, go[g]:go[g + 1]]) for g in range(len(ref))])
    ld1, imp1 = before()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ld0, ld1))
    for name in ("z", "info"):
        assert np.array_equal(imp0[name], imp1[name]), name
    assert imp0["status"] == imp1["status"]
