"""GPU: the block eigen-solver and the projections of k_hess.hip (gauss_ld_hess_rows) against tests/hess_ref.py.

Every case -- M on both sides of every edge of the solver (blocks of 16 columns, pairs of 32, row chunks of 64), M = 260 and 520,
T in {1, 3, 64}, pooled and weighted, k_max below M, equal to M and above n_pos -- goes through checks 1, 2 and 3:
(1) the returned eigenpairs are eigenpairs of the repaired matrix gauss_ld_rows returns: residual, orthogonality, eigenvalues against
    eigvalsh, each below 8 x the maximum measured on an MI355X for that M (BOUNDS) and never above 1e-10;
(2) proj equals the numpy replay of hess_proj_kernel's sums on the returned vectors bit for bit (the kernel's order is replayable: one
    product and one add per row per lane, then a halving tree);
(3) planted z = R b, k = M: H and C against b^T R b within 1e-8 relative.
Then degenerate inputs, the same bits across sources and launch forms, a trait on its own, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import hess_ref as hr
from gauss_amd import _lib, api, hotpath
from gauss_amd import panel as panel_mod
from test_gpu_clump import _panel

pytestmark = pytest.mark.gpu

_ip, _dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)

# (M, T, mode, n_pop, k_max): b = 16, pair width 32, row chunk 64
CASES = [(1, 1, 0, 1, 1), (2, 3, 1, 2, 7), (15, 64, 0, 1, 7), (16, 1, 1, 3, 16), (17, 3, 0, 2, 8), (31, 64, 1, 1, 31), (32, 1, 0, 3, 16),
         (33, 3, 1, 2, 40), (63, 1, 0, 1, 63), (64, 3, 1, 3, 32), (65, 64, 0, 2, 65), (260, 3, 1, 3, 100), (260, 1, 0, 1, 260),
         (520, 64, 1, 2, 520), (520, 3, 0, 1, 256)]
# Measured on an MI355X (res, orth, dlam: the maxima over the cases of that M, as the first test prints them), and 8 x that as the
# bound.  The factor covers other seeds and rounding; it is no license to be loose.  No bound may exceed 1e-10, the condition the
# statistic needs (the project's 1e-8 on end quantities with two digits to spare).
MEASURED = {1: (0.0, 0.0, 0.0), 2: (1.563e-16, 2.220e-16, 2.210e-16), 15: (4.694e-16, 1.110e-15, 5.773e-16), 16: (4.185e-16, 1.110e-15, 4.754e-16),
            17: (6.382e-16, 6.661e-16, 6.875e-16), 31: (9.042e-16, 1.443e-15, 4.374e-16), 32: (1.409e-15, 1.665e-15, 1.165e-15),
            33: (7.404e-16, 1.665e-15, 8.544e-16), 63: (1.214e-15, 2.887e-15, 1.047e-15), 64: (2.048e-15, 2.776e-15, 7.349e-16),
            65: (1.598e-15, 3.775e-15, 2.026e-15), 260: (4.679e-15, 6.217e-15, 4.626e-15), 520: (8.356e-15, 9.326e-15, 9.923e-15)}
BOUNDS = {M: tuple(8 * x for x in v) for M, v in MEASURED.items()}      # (M = 1 is exact: lam = 1, v = 1)
assert all(b <= 1e-10 for v in BOUNDS.values() for b in v)

_cache = {}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _case(ctx, case):
    """the panel, the matrix gauss_ld_rows returns, the traits and the GPU's answer with its vectors: computed once per case"""
    if case in _cache:
        return _cache[case]
    M, T, mode, n_pop, k_max = case
    k = CASES.index(case)
    p = _panel(M, seed=1200 + k, n_samples=(2000, 2400, 3000)[k % 3], n_pop=n_pop)
    w = p["w"] if mode else None
    z = np.random.default_rng(50 + k).standard_normal((T, M)) * 2.5
    R = hotpath.ld_matrix_rows(p["G"], np.arange(M), p["off"], w, mode, 1.0, fmt=_lib.GENO_U8, ctx=ctx)
    R.setflags(write=False)
    got = hotpath.ld_hess(p["G"], p["off"], z, w, mode, k_max=k_max, eig_min=1e-6, want_vectors=True, ctx=ctx)
    Rp, mono, n_bad = hr.repair(R)                         # (a SNP without variance in one population of a weighted case: repaired alike)
    out = _cache[case] = dict(p=p, w=w, z=z, R=R, Rp=Rp, mono=mono, n_bad=n_bad, got=got)
    return out


_ids = lambda c: "M%d-T%d-%s-P%d-k%d" % (c[0], c[1], "wgt" if c[2] else "pool", c[3], c[4])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_the_eigenpairs_are_eigenpairs(ctx, case):
    M, T, mode, n_pop, k_max = case
    c = _case(ctx, case)
    got, R = c["got"], c["R"]
    assert np.array_equal(R, R.T)
    Rp, mono, n_bad = c["Rp"], c["mono"], c["n_bad"]
    V, lam = got["vectors"], got["lam"]
    assert got["status"] == (2 if n_bad else 0) and got["n_nonfinite"] == n_bad and 1 <= got["sweeps"] <= 30
    assert lam.shape == (M,) and np.all(np.diff(lam) <= 0) and sorted(got["order"]) == list(range(M))
    res = np.linalg.norm(Rp @ V.T - V.T * lam[None, :], axis=0).max() / lam[0]
    orth = np.abs(V @ V.T - np.eye(M)).max()
    dlam = np.abs(lam - np.linalg.eigvalsh(Rp)[::-1]).max() / lam[0]
    print(f"REACHED hess M {M} T {T} mode {mode} P {n_pop}: sweeps {got['sweeps']}, n_pos {got['n_pos']}, res {res:.3e} orth {orth:.3e} "
          f"dlam {dlam:.3e} (bounds {BOUNDS[M][0]:.1e} {BOUNDS[M][1]:.1e} {BOUNDS[M][2]:.1e}), lam {lam[0]:.3f} .. {lam[-1]:.3e}")
    assert got["n_pos"] == hr.n_pos_of(lam, 1e-6) == M - int(mono.sum())          # 2 000 and more samples: full rank
    assert res <= BOUNDS[M][0] and orth <= BOUNDS[M][1] and dlam <= BOUNDS[M][2]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_the_projections_follow_from_the_eigenpairs_bit_for_bit(ctx, case):
    M, T, mode, n_pop, k_max = case
    c = _case(ctx, case)
    got = c["got"]
    kk = min(k_max, got["n_pos"])
    assert got["proj"].shape == (T, k_max) and np.all(np.isnan(got["proj"][:, kk:])) and np.all(np.isfinite(got["proj"][:, :kk]))
    rep = hr.replay_proj(got["vectors"], got["lam"], c["z"], c["mono"], k_max, got["n_pos"])
    assert np.array_equal(_bits(rep), _bits(got["proj"]))
    # and, sign-free, what eigh gives: products of two projections on the same eigenvector, where the eigenvalue stands alone
    ref = hr.rule(c["R"], c["z"], k_max)
    lam = got["lam"]
    gap = np.minimum(np.abs(np.diff(lam, prepend=np.inf)), np.abs(np.diff(lam, append=-np.inf)))[:kk]
    alone = gap > 1e-3 * lam[0]
    a, b = got["proj"][:, :kk][:, alone], ref["proj"][:, :kk][:, alone]
    scale = np.abs(b).max() ** 2 if b.size else 1.0
    assert np.allclose(a[:, None, :] * a[None, :, :], b[:, None, :] * b[None, :, :], rtol=0, atol=1e-8 * scale)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_a_planted_truth_comes_back(ctx, case):
    """z = R b exactly (in fp64, on the GPU's own matrix), k = M: H_t = b_t^T R b_t and C_ab = b_a^T R b_b"""
    M, T, mode, n_pop, _ = case
    c = _case(ctx, case)
    Tp = min(T, 3)
    b = np.random.default_rng(7 + M).standard_normal((Tp, M))
    R = c["Rp"]
    b[:, c["mono"]] = 0.0
    z = b @ R
    K = M - int(c["mono"].sum())
    got = hotpath.ld_hess(c["p"]["G"], c["p"]["off"], z, c["w"], mode, k_max=M, eig_min=0.0, ctx=ctx)
    assert got["n_pos"] == K and got["status"] == (2 if c["n_bad"] else 0)
    est = api.hess_estimates(got["lam"], got["proj"], 1e6, k=K, eig_min=0.0)
    truth = b @ R @ b.T
    ia, ib = est["pairs"]["a"], est["pairs"]["b"]
    worst = max(np.abs(est["H"] / np.diag(truth) - 1).max(), (np.abs(est["pairs"]["C"] - truth[ia, ib]).max() / np.abs(truth).max()) if len(ia) else 0.0)
    print(f"REACHED hess planted M {M}: worst relative error of H and C {worst:.3e}")
    assert est["k"] == K and worst <= 1e-8


def _figures(R, got):
    Rp, mono, n_bad = hr.repair(R)
    V, lam = got["vectors"], got["lam"]
    res = np.linalg.norm(Rp @ V.T - V.T * lam[None, :], axis=0).max() / lam[0]
    orth = np.abs(V @ V.T - np.eye(len(V))).max()
    dlam = np.abs(lam - np.linalg.eigvalsh(Rp)[::-1]).max() / lam[0]
    return res, orth, dlam


def test_the_solve_converges_at_the_limit(ctx):
    """M = GAUSS_HESS_MAX_M = 4 096 of 6 000 samples (full rank): the size at which one MFMA chain over the rows left the Gram entries
    with more rounding noise than the 1e-15 guard lets pass, so that no sweep was free of rotations; the chunks' sums are a tree since.
    Some six seconds: the panel, 27 sweeps of 255 launches, the vectors back and eigvalsh on the host.  Measured on an MI355X: res
    5.301e-14, orth 6.528e-14, dlam 5.374e-14; the bounds are 8 x that"""
    M = _lib.HESS_MAX_M
    p = _panel(M, seed=1200, n_samples=6000, n_pop=1)
    z = np.random.default_rng(M).standard_normal((1, M)) * 2
    R = hotpath.ld_matrix_rows(p["G"], np.arange(M), p["off"], None, 0, 1.0, fmt=_lib.GENO_U8, ctx=ctx)
    got = hotpath.ld_hess(p["G"], p["off"], z, None, 0, k_max=_lib.HESS_MAX_K, want_vectors=True, ctx=ctx)
    res, orth, dlam = _figures(R, got)
    print(f"REACHED hess at the limit: M {M}, sweeps {got['sweeps']}, status {got['status']}, n_pos {got['n_pos']}, res {res:.3e} orth {orth:.3e} dlam {dlam:.3e}")
    assert got["status"] == 0 and got["sweeps"] <= 30 and got["n_pos"] == M
    assert res <= 8 * 5.301e-14 and orth <= 8 * 6.528e-14 and dlam <= 8 * 5.374e-14 and 8 * 6.528e-14 <= 1e-10
    rep = hr.replay_proj(got["vectors"], got["lam"], z, np.zeros(M, dtype=bool), _lib.HESS_MAX_K, got["n_pos"])
    assert np.array_equal(_bits(rep), _bits(got["proj"]))


def test_a_rank_deficient_block_converges_with_a_null_space(ctx):
    """600 SNPs of 300 samples in two populations: half the spectrum is null.  The columns of G = R' V that belong to it are roundings of
    zero whose inner products are noise; the floor M 2^-52 on a column's norm takes them out of the rotations, and the solve ends
    (without it: 30 sweeps and GAUSS_ST_HESS_NOCONV).  Measured on an MI355X: 29 sweeps, n_pos 298, res 1.616e-14, orth 1.421e-14,
    dlam 6.634e-15; the bounds are 8 x that.  Beyond some 1 200 SNPs a rank-deficient block does run its 30 sweeps out"""
    M = 600
    p = _panel(M, seed=1201, n_samples=300, n_pop=2)
    z = np.random.default_rng(M).standard_normal((3, M)) * 2
    R = hotpath.ld_matrix_rows(p["G"], np.arange(M), p["off"], p["w"], 1, 1.0, fmt=_lib.GENO_U8, ctx=ctx)
    got = hotpath.ld_hess(p["G"], p["off"], z, p["w"], 1, k_max=400, want_vectors=True, ctx=ctx)
    res, orth, dlam = _figures(R, got)
    lam = got["lam"]
    print(f"REACHED hess rank-deficient: M {M}, sweeps {got['sweeps']}, status {got['status']}, n_pos {got['n_pos']}, res {res:.3e} orth {orth:.3e} "
          f"dlam {dlam:.3e}, lam[n_pos - 1] {lam[got['n_pos'] - 1]:.3e}, lam[n_pos] {lam[got['n_pos']]:.3e}")
    assert got["status"] == 0 and got["sweeps"] <= 30 and got["n_nonfinite"] == 0
    assert got["n_pos"] == hr.n_pos_of(np.linalg.eigvalsh(hr.repair(R)[0])[::-1], 1e-6) and 250 <= got["n_pos"] < 300
    assert np.abs(lam[300:]).max() <= M * 2.0 ** -52 * 8                              # 300 samples: at least M - 300 null directions, within the floor of 0
    assert res <= 8 * 1.616e-14 and orth <= 8 * 1.421e-14 and dlam <= 8 * 6.634e-15
    assert np.all(np.isnan(got["proj"][:, got["n_pos"]:])) and np.all(np.isfinite(got["proj"][:, :got["n_pos"]]))
    ref = hr.rule(R, z, 400)
    a, b = got["proj"][:, :got["n_pos"]], ref["proj"][:, :got["n_pos"]]
    assert np.allclose(a @ a.T, b @ b.T, rtol=1e-8, atol=1e-8 * np.abs(b @ b.T).max())


def _degenerate(ctx, G, off, z, k_max, mode=0, w=None):
    """n_pos and n_nonfinite as hess_ref gives them; lam within 1e-10 lam_max of eigh's; proj NaN beyond n_pos, the replay of its kernel on
    the returned vectors bit for bit, and -- an eigenvector's sign and the basis of a subspace of equal eigenvalues being free -- equal
    to eigh's through the sign- and basis-free sums p p^T at k = n_pos within 1e-8; the vectors orthonormal within 1e-12"""
    R = hotpath.ld_matrix(G, off, w, mode, 1.0, ctx=ctx)
    got = hotpath.ld_hess(G, off, z, w, mode, k_max=k_max, want_vectors=True, ctx=ctx)
    ref = hr.rule(R, z, k_max)
    lam_max = max(ref["lam"][0], 1.0)
    assert got["n_pos"] == ref["n_pos"] and got["n_nonfinite"] == ref["n_nonfinite"]
    assert np.abs(got["lam"] - ref["lam"]).max() <= 1e-10 * lam_max
    kk = min(k_max, ref["n_pos"])
    assert np.all(np.isnan(got["proj"][:, kk:])) and np.all(np.isfinite(got["proj"][:, :kk]))
    rep = hr.replay_proj(got["vectors"], got["lam"], z, ref["mono"], k_max, got["n_pos"])
    assert np.array_equal(_bits(rep), _bits(got["proj"]))
    # the sign-free end quantities at k = kk against eigh's (a subspace of equal eigenvalues sums to the same H and C)
    if kk:
        a, b = got["proj"][:, :kk], ref["proj"][:, :kk]
        assert np.allclose(a @ a.T, b @ b.T, rtol=1e-8, atol=1e-8 * np.abs(b @ b.T).max())
    V = got["vectors"]
    assert np.abs(V @ V.T - np.eye(len(V))).max() <= 1e-12
    return got, ref, R


def test_a_monomorphic_snp_is_a_zero_row_with_a_zero_eigenvalue(ctx):
    M, d = 70, 33
    p = _panel(M, seed=41, n_samples=2000, n_pop=1)
    G = p["G"].copy()
    G[d, :] = 1                                            # pooled LD of a row without variance is 0 / 0
    z = np.random.default_rng(1).standard_normal((3, M))
    got, ref, R = _degenerate(ctx, G, p["off"], z, k_max=M)
    assert np.all(np.isnan(np.delete(R[d], d))) and ref["mono"][d] and ref["mono"].sum() == 1
    assert got["n_pos"] == M - 1 and got["n_nonfinite"] == 0 and got["status"] == 0 and got["lam"][-1] == 0.0
    assert np.all(got["vectors"][:M - 1, d] == 0.0) and got["vectors"][M - 1, d] == 1.0        # its unit vector, never rotated
    z2 = z.copy()
    z2[:, d] = np.nan                                      # its z is ignored
    again = hotpath.ld_hess(G, p["off"], z2, None, 0, k_max=M, ctx=ctx)
    assert np.array_equal(_bits(again["proj"]), _bits(got["proj"])) and np.array_equal(_bits(again["lam"]), _bits(got["lam"]))


def test_a_duplicated_snp_drops_a_direction(ctx):
    M = 40
    p = _panel(M, seed=43, n_samples=2000, n_pop=2)
    G = p["G"].copy()
    G[21] = G[20]
    z = np.random.default_rng(2).standard_normal((2, M))
    z[:, 21] = z[:, 20]
    got, ref, _ = _degenerate(ctx, G, p["off"], z, k_max=M, mode=1, w=p["w"])
    assert got["n_pos"] == M - 1 and abs(got["lam"][-1]) <= 1e-6 * got["lam"][0] and np.all(np.isnan(got["proj"][:, M - 1]))


def test_one_snp(ctx):
    G = np.array([[0, 2, 1, 1, 0, 2, 1, 0]], dtype=np.uint8)
    got, ref, _ = _degenerate(ctx, G, [0, 8], np.array([[3.0], [-2.0]]), k_max=4)
    assert got["n_pos"] == 1 and got["lam"][0] == 1.0 and np.array_equal(got["proj"][:, 0], [3.0, -2.0]) and got["sweeps"] == 1


def test_a_nan_z_counts_as_zero_for_that_trait(ctx):
    M = 50
    p = _panel(M, seed=44, n_samples=2000, n_pop=1)
    z = np.random.default_rng(3).standard_normal((3, M))
    z[1, 7], z[1, 30], z[2, 0] = np.nan, np.inf, -np.inf
    got, ref, _ = _degenerate(ctx, p["G"], p["off"], z, k_max=20)
    z0 = np.where(np.isfinite(z), z, 0.0)
    again = hotpath.ld_hess(p["G"], p["off"], z0, None, 0, k_max=20, ctx=ctx)
    assert np.array_equal(_bits(again["proj"]), _bits(got["proj"])) and got["status"] == 0


def _same(got, ref, what):
    for name in ("lam", "proj"):
        assert np.array_equal(_bits(got[name]), _bits(ref[name])), (what, name)
    assert (got["sweeps"], got["n_pos"], got["status"], got["n_nonfinite"]) == (ref["sweeps"], ref["n_pos"], ref["status"], ref["n_nonfinite"]), what


def test_the_bits_do_not_depend_on_the_source_or_the_launch_form(ctx, monkeypatch):
    M = 97
    p = _panel(M, seed=77, n_samples=2000, n_pop=3)
    G = p["G"]
    z = np.random.default_rng(4).standard_normal((3, M))
    args = dict(pop_wgt=p["w"], mode=1, k_max=60)
    ref = hotpath.ld_hess(G, p["off"], z, ctx=ctx, **args)
    assert ref["status"] == 0 and ref["n_pos"] == M
    rows2, src_off = panel_mod.pack2bit(G, p["off"])
    perm = np.random.default_rng(5).permutation(M)
    inv = np.argsort(perm).astype(np.int32)                # store row of SNP s when the store holds the rows in `perm` order

    def sources(c):
        _same(hotpath.ld_hess(G, p["off"], z, ctx=c, **args), ref, "host bytes")
        _same(hotpath.ld_hess_rows(G, np.arange(M), p["off"], z, fmt=_lib.GENO_U8, ctx=c, **args), ref, "host rows by index")
        for fmt, store_rows, src in ((_lib.GENO_U8, G, None), (_lib.GENO_2BIT, rows2, src_off)):
            for order, name in ((None, "store order"), (perm, "permuted store")):
                store = hotpath.RowStore(np.ascontiguousarray(store_rows if order is None else store_rows[order]), ctx=c)
                try:
                    got = hotpath.ld_hess_rows(store, np.arange(M) if order is None else inv, p["off"], z, fmt=fmt, pop_src_off=src, ctx=c, **args)
                finally:
                    store.close()
                _same(got, ref, (fmt, name))

    sources(ctx)
    for sw in (dict(GAUSS_GRAM_PACKED="0"), dict(GAUSS_GRAM_PACKED="1"), dict(GAUSS_SIDE_STREAM="0"), dict(GAUSS_CHAIN_MERGED="0")):
        with monkeypatch.context() as m:                   # read when a context is made
            for name, v in sw.items():
                m.setenv(name, v)
            c = hotpath.Context(0)
            try:
                sources(c)
            finally:
                c.close()


def test_a_trait_depends_on_its_own_z_only(ctx):
    case = CASES[5]                                        # M 31, T 64
    c = _case(ctx, case)
    M, T, mode, _, k_max = case
    for t in (0, 17, 63):
        one = hotpath.ld_hess(c["p"]["G"], c["p"]["off"], c["z"][t], c["w"], mode, k_max=k_max, ctx=ctx)
        assert np.array_equal(_bits(one["proj"][0]), _bits(c["got"]["proj"][t])) and np.array_equal(_bits(one["lam"]), _bits(c["got"]["lam"]))


def _call(ctx, **change):
    """gauss_ld_hess_rows on 20 SNPs of 200 samples with every argument in order but the changed ones: (rc, message, arguments)"""
    p = _panel(20, seed=5, n_samples=200, n_pop=1)
    G = p["G"]
    a = dict(store=G.ctypes.data, ld=G.strides[0], fmt=_lib.GENO_U8, n_snp=20, off=p["off"], n_pop=1, z=np.ones((2, 20)), n_trait=2, k_max=5,
             eig_min=1e-6, lam=np.full(20, -7.0), proj=np.full((2, 5), -7.0), mode=0)
    a.update(change)
    rc = ctx.lib.gauss_ld_hess_rows(ctx.handle, a["mode"], a["store"], a["ld"], a["fmt"], None, a["n_snp"], _lib.ptr(a["off"], _ip), None, None,
                                    a["n_pop"], 0, _lib.ptr(a["z"], _dp), a["n_trait"], a["k_max"], a["eig_min"], _lib.ptr(a["lam"], _dp),
                                    _lib.ptr(a["proj"], _dp), None, None, None, None, None, None)
    return rc, ctx.lib.gauss_last_error().decode(), a


def test_every_refusal_is_invalid_with_its_limit_and_launches_nothing(ctx):
    rc, msg, a = _call(ctx)
    assert rc == 0, msg                                    # the optional outputs are NULL here: allowed
    assert np.all(a["lam"] > 0) and np.all(np.isfinite(a["proj"]))
    queued = ctx.counters()                                # runs queued so far: a refusal adds none (the kernels come behind a run)
    for text, change in (("z is NULL", dict(z=None)), ("out_lam is NULL", dict(lam=None)), ("out_proj is NULL", dict(proj=None)),
                         ("n_snp = 0; a block holds 1 .. 4096 SNPs", dict(n_snp=0)),
                         ("n_trait = 0; a call takes 1 .. 64 traits", dict(n_trait=0)), ("n_trait = 65; a call takes 1 .. 64 traits", dict(n_trait=65)),
                         ("k_max = 0; a call projects on 1 .. 1024 eigenvectors", dict(k_max=0)),
                         ("k_max = 1025; a call projects on 1 .. 1024 eigenvectors", dict(k_max=1025)),
                         ("eig_min = -0.1 is outside [0, 1)", dict(eig_min=-0.1)), ("eig_min = 1 is outside [0, 1)", dict(eig_min=1.0)),
                         ("eig_min = nan is outside [0, 1)", dict(eig_min=np.nan)),
                         ("bad mode 7", dict(mode=7)), ("n_pop must be in 1..64 (got 0)", dict(n_pop=0)), ("ld (100) < n_samples (200)", dict(ld=100))):
        lam, proj = np.full(20, -7.0), np.full((2, 5), -7.0)
        rc, msg, _ = _call(ctx, **dict(dict(lam=lam, proj=proj), **change))
        assert rc == -1 and text in msg, (text, rc, msg)   # GAUSS_E_INVALID
        assert np.all(lam == -7.0) and np.all(proj == -7.0) and ctx.counters() == queued, text
    # one SNP too many is refused on a store of two rows: no row is read
    tiny = np.array([[0, 1, 2, 1], [2, 1, 0, 1]], dtype=np.uint8)
    rc, msg, _ = _call(ctx, store=tiny.ctypes.data, ld=4, off=np.array([0, 4], dtype=np.int32), n_snp=4097)
    assert rc == -1 and "n_snp = 4097; a block holds 1 .. 4096 SNPs" in msg, (rc, msg)
