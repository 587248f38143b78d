"""GPU suite: zmix() -- the gauss_zmix_normal_eq kernel against numpy on the pair matrix that gauss_ld_per_pop /
gauss_ld_per_pop_pairs return for the same genotypes, and the whole entry point against the numpy statement of zmix.R built
on the oracle's prep_zmix5 / prep_zmix5_sup (tests/zmix_ref.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from gauss_amd import _lib, api, hotpath, panel, synth

from zmix_ref import finish, kkt, matrix, near_rounding_boundary, normal_eq, reduced_solve

pytestmark = pytest.mark.gpu

POPS = [("AAA", 160, "EUR"), ("BBB", 145, "EUR"), ("CCC", 170, "ASN"), ("DDD", 133, "AFR"), ("EEE", 152, "EUR"),
        ("FFF", 90, "ASN")]
_ip = C.POINTER(C.c_int32)


def _geno(S, P, seed, mono=0):
    """Genotypes of S SNPs in P populations (12-30 samples each, super-populations of three); `mono` SNPs are made
    monomorphic inside some population (their correlations there are NaN: those pairs are dropped)."""
    rng = np.random.default_rng(seed)
    pops = [(f"P{k:02d}", int(rng.integers(12, 31)), f"S{k // 3}") for k in range(P)]
    bp = np.sort(rng.choice(np.arange(1, 50 * S + 100), size=S, replace=False))
    G, _ = synth.synth_genotypes(bp, pops, seed=seed + 1)
    off = np.concatenate([[0], np.cumsum([p[1] for p in pops])]).astype(np.int32)
    for s in rng.choice(S, size=min(mono, S), replace=False):
        k = int(rng.integers(P))
        G[s, off[k]:off[k + 1]] = int(rng.integers(3))
    z = rng.standard_normal(S) * 2.0
    return np.ascontiguousarray(G, dtype=np.uint8), off, z, pops


def _groups(pops):
    names, grp = [], []
    for p in pops:
        if p[2] not in names:
            names.append(p[2])
        grp.append(names.index(p[2]))
    return np.array(grp, dtype=np.int32), len(names)


def _pair_matrix(G, off, z, grp, ctx):
    """[y | r] of every pair i < j in the reference's row order, from the existing kernels."""
    S = G.shape[0]
    iu, ju = np.triu_indices(S, 1)
    y = z[iu] * z[ju]
    if grp is None:
        r = hotpath.ld_per_pop(G, off, ctx=ctx)
    else:
        n_group = int(grp.max()) + 1
        pi, pj = iu.astype(np.int32), ju.astype(np.int32)
        r = np.zeros((n_group, len(pi)))
        lib = ctx.lib
        rc = lib.gauss_ld_per_pop_pairs(ctx.handle, G.ctypes.data, S, G.strides[0], off.ctypes.data_as(_ip), len(off) - 1,
                                        grp.ctypes.data_as(_ip), n_group, pi.ctypes.data_as(_ip), pj.ctypes.data_as(_ip),
                                        len(pi), r.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 0, lib.gauss_last_error()
    return np.column_stack([y, r.T])


def _check_kernel(G, off, z, grp, ctx, tol=1e-12):
    xtx, xty, yty, n_rows = hotpath.zmix_normal_eq(G, off, z, pop_group=grp, ctx=ctx)
    D, d, yy, n = normal_eq(_pair_matrix(G, off, z, grp, ctx))
    assert n_rows == n
    for got, want in ((xtx, D), (xty, d), (np.array([yty]), np.array([yy]))):
        scale = max(1.0, float(np.max(np.abs(want))))
        assert np.max(np.abs(got - want)) <= tol * scale, (np.max(np.abs(got - want)), scale)
    return xtx, xty, yty, n_rows


@pytest.mark.parametrize("S", [2, 100, 300])
@pytest.mark.parametrize("P", [1, 6, 26, 64])
@pytest.mark.parametrize("grouped", [False, True])
def test_normal_eq_kernel(ctx, S, P, grouped):
    G, off, z, pops = _geno(S, P, seed=31 * S + P, mono=S // 10)
    grp = _groups(pops)[0] if grouped else None
    first = _check_kernel(G, off, z, grp, ctx)
    again = hotpath.zmix_normal_eq(G, off, z, pop_group=grp, ctx=ctx)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    assert first[2] == again[2] and first[3] == again[3]
    if S > 2 and P > 1:
        assert first[3] < S * (S - 1) // 2                       # the monomorphic SNPs' pairs were dropped


def test_normal_eq_all_rows_dropped(ctx):
    G, off, z, _ = _geno(40, 3, seed=5)
    G[:, off[1]:off[2]] = 1                                       # population 1 monomorphic everywhere: every row has a NaN
    xtx, xty, yty, n_rows = hotpath.zmix_normal_eq(G, off, z, ctx=ctx)
    assert n_rows == 0 and not xtx.any() and not xty.any() and yty == 0.0


def test_normal_eq_refuses_more_than_64_groups(ctx):
    G, off, z, _ = _geno(10, 65, seed=6)
    with pytest.raises(_lib.GaussHipError, match="1 .. 64"):
        hotpath.zmix_normal_eq(G, off, z, ctx=ctx)


def test_normal_eq_scale(ctx):
    """About 2 * 10^6 pairs at P = 26."""
    G, off, z, _ = _geno(2000, 26, seed=77, mono=20)
    _check_kernel(G, off, z, None, ctx, tol=1e-11)


# ---- the whole entry point ----

@pytest.fixture(scope="module")
def study(tmp_path_factory):
    d = tmp_path_factory.mktemp("zmix_study")
    return panel.make_synthetic_study(str(d), POPS, n_snp=700, bp_lo=1_000_000, bp_hi=2_400_000, frac_measured=0.3, seed=17)


def _files(st):
    p = st["paths"]
    return p["gwas.txt"], p["index.gz"], p["data.gz"], p["desc.txt"]


@pytest.fixture(scope="module")
def packed(study):
    _, idx, dat, desc = _files(study)
    out = os.path.join(os.path.dirname(dat), "panel.gpk")
    assert api.pack_panel(idx, dat, desc, out) > 0
    return out


@pytest.mark.parametrize("level", ["population", "superpopulation"])
@pytest.mark.parametrize("percentile,interval", [(0.5, 2), (0.3, 1), (0.6, 3)])
def test_zmix_end_to_end(ctx, study, packed, level, percentile, interval):
    inp, idx, dat, desc = _files(study)
    df, det = api.zmix(inp, idx, dat, desc, percentile=percentile, interval=interval, level=level, ctx=ctx, detail=True)
    dfp, detp = api.zmix(inp, idx, packed, desc, percentile=percentile, interval=interval, level=level, ctx=ctx, detail=True)
    # text and packed panels: the same bits
    assert df.equals(dfp)
    for k in ("dmat", "dvec", "w_unrounded"):
        assert det[k].tobytes() == detp[k].tobytes(), k
    # the frame of zmix.R
    if level == "population":
        assert list(df.columns) == ["Population", "SuperPopulation", "Weight"]
        assert list(df["Population"]) == [p[0] for p in POPS] and list(df["SuperPopulation"]) == [p[2] for p in POPS]
    else:
        assert list(df.columns) == ["SuperPopulation", "Weight"]
        assert list(df["SuperPopulation"]) == ["EUR", "ASN", "AFR"]
    # the numpy statement on the oracle's matrix
    D, d, yy, n = normal_eq(matrix(inp, idx, dat, desc, percentile=percentile, interval=interval, level=level))
    assert det["n_rows"] == n and det["n_pairs"] == det["n_snp"] * (det["n_snp"] - 1) // 2
    assert np.max(np.abs(det["dmat"] - D)) <= 1e-12 * max(1.0, np.max(np.abs(D)))
    assert np.max(np.abs(det["dvec"] - d)) <= 1e-12 * max(1.0, np.max(np.abs(d)))
    w_unr = det["w_unrounded"]
    assert kkt(D, d, w_unr, tol=1e-8) == []
    want = reduced_solve(D, d, w_unr > 1e-10)
    assert kkt(D, d, want) == []
    assert np.max(np.abs(w_unr - want)) <= 1e-9
    u, fin = finish(want)
    if not near_rounding_boundary(u).any():
        assert np.max(np.abs(df["Weight"].to_numpy() - fin)) <= 1e-15
    assert abs(df["Weight"].sum() - 1.0) <= 1e-14


def test_zmix_feeds_distmix(ctx, study):
    """zmix's frame feeds distmix as pop_wgt_df."""
    inp, idx, dat, desc = _files(study)
    df = api.zmix(inp, idx, dat, desc, percentile=0.5, interval=2, ctx=ctx)
    out = api.distmix(22, 1_500_000, 2_000_000, 300_000, df[["Population", "Weight"]], inp, idx, dat, desc, ctx=ctx)
    assert len(out) > 0 and np.isfinite(out["z"].to_numpy()).all()


def test_zmix_no_valid_rows(ctx, study):
    inp, idx, dat, desc = _files(study)
    with pytest.raises(api.GaussError, match="zmix: no valid rows after filtering."):
        api.zmix(inp, idx, dat, desc, percentile=0.999, interval=50, ctx=ctx)


def test_zmix_missing_desc_column(ctx, study, tmp_path):
    inp, idx, dat, desc = _files(study)
    bad = tmp_path / "desc.txt"
    lines = open(desc).read().splitlines()
    bad.write_text("\n".join([lines[0].replace("Super_Population", "SuperPop")] + lines[1:]) + "\n")
    with pytest.raises(api.GaussError, match="must include Population_Abbreviation and Super_Population"):
        api.zmix(inp, idx, dat, str(bad), percentile=0.5, interval=2, ctx=ctx)


def test_zmix_identical_populations_not_positive_definite(ctx, tmp_path):
    pops = [("AAA", 60, "EUR"), ("BBB", 60, "EUR"), ("CCC", 70, "AFR")]
    rng = np.random.default_rng(3)
    S = 200
    bp = np.sort(rng.choice(np.arange(1_000_000, 1_400_000), size=S, replace=False))
    G, _ = synth.synth_genotypes(bp, pops, seed=4)
    G[:, 60:120] = G[:, 0:60]                                     # BBB's genotypes are AAA's
    keep = G.min(1) != G.max(1)                                   # a SNP monomorphic in the whole panel has norm_var 0 / 0
    G, bp = np.ascontiguousarray(G[keep]), bp[keep]
    S = len(bp)
    af = np.column_stack([G[:, 0:60].mean(1) / 2, G[:, 60:120].mean(1) / 2, G[:, 120:].mean(1) / 2])
    rsid = np.array([f"rs{i}" for i in range(S)])
    chrs = np.full(S, 22)
    a1, a2 = np.full(S, "A"), np.full(S, "G")
    d = str(tmp_path)
    paths = {k: os.path.join(d, k) for k in ("desc.txt", "index.gz", "data.gz", "gwas.txt")}
    panel.write_pop_desc(paths["desc.txt"], pops)
    panel.write_panel(paths["index.gz"], paths["data.gz"], rsid, chrs, bp, a1, a2, G, af, [p[1] for p in pops])
    panel.write_gwas(paths["gwas.txt"], rsid, chrs, bp, a1, a2, rng.standard_normal(S) * 2)
    with pytest.raises(api.GaussError, match="matrix D in quadratic function is not positive definite!"):
        api.zmix(paths["gwas.txt"], paths["index.gz"], paths["data.gz"], paths["desc.txt"], percentile=0.3, interval=1, ctx=ctx)
