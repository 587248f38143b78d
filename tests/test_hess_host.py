"""The host layer of hess.  CPU: the binding and its argument types, the headers and the dynamic symbol tables.
GPU: api.hess, files -> frame, on the text panel, the packed panel and the packed panel through the full SNP map, against
api.computeLD's SNP list and matrix; three study files; a swapped-allele file; a file that lacks a SNP; a planted block."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = ctypes
SNP_COLUMNS = ["rsid", "chr", "bp", "a1", "a2", "af1mix"]
FRAME_COLUMNS = ["trait", "n", "k", "H", "h2", "se", "n_snp", "n_pos", "var_kept"]
REGION = (22, 1_000_000, 2_400_000)


def test_the_binding_and_its_argument_types():
    from gauss_amd import _lib, api, hotpath
    assert "gauss_ld_hess_rows" in _lib.SYMBOLS and "gauss_host_hess" in api.HOST_SYMBOLS
    lib = _lib.load()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rows, hess = lib.gauss_ld_rows.argtypes, lib.gauss_ld_hess_rows.argtypes
    # gauss_ld_rows' row arguments (without diag and out_cor), then z, n_trait, k_max, eig_min, the six outputs and the tests' two
    assert hess[:11] == rows[:11] and hess[11] == rows[12] == C.c_int
    assert hess[12:] == [dp, C.c_int, C.c_int, C.c_double, dp, dp, ip, ip, C.POINTER(C.c_int64), ip, dp, ip]
    h = api.load_host()
    ld = h.gauss_host_computeLD.argtypes
    # computeLD's arguments with a list of study files and their count in place of the one file
    assert h.gauss_host_hess.argtypes == ld[:7] + [C.POINTER(C.c_char_p), C.c_int] + ld[8:-1] + [C.c_int, C.c_double] + [ld[-1]]
    assert callable(api.hess) and callable(api.hess_estimates) and callable(hotpath.ld_hess) and callable(hotpath.ld_hess_rows)


def test_header_export_map_and_symbol_table_agree():
    from gauss_amd import _lib, api
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, path)).read(), flags=re.S)
    assert re.search(r"\bint\s+gauss_ld_hess_rows\s*\(", strip("include/gauss_hip.h"))
    assert re.search(r"\bint\s+gauss_host_hess\s*\(", strip("include/gauss_host.h"))
    hdr = open(os.path.join(ROOT, "include", "gauss_hip.h")).read()
    for name, value in (("M", _lib.HESS_MAX_M), ("TRAITS", _lib.HESS_MAX_TRAITS), ("K", _lib.HESS_MAX_K)):
        assert re.search(r"#define\s+GAUSS_HESS_MAX_%s\s+%d\b" % (name, value), hdr)
    assert re.search(r"#define\s+GAUSS_ST_HESS_NOCONV\s+%d\b" % _lib.ST_HESS_NOCONV, hdr)
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm not available")
    _lib.load(), api.load_host()                           # (built on first use)
    for so, name in (("libgauss_hip.so", "gauss_ld_hess_rows"), ("libgauss_host.so", "gauss_host_hess")):
        syms = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "gauss_amd", "lib", so)], text=True)
        assert re.search(r" T %s$" % name, syms, flags=re.M), (so, name)
        assert not re.search(r" [TW] (?!gauss_)\w*hess", syms), so      # no internal of the feature leaks


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    import cs_ref
    from gauss_amd import api
    d = tmp_path_factory.mktemp("hess_study")
    files = cs_ref.study_files(d)
    packed = os.path.join(os.path.dirname(files[2]), "panel.gpk")
    assert api.pack_panel(files[1], files[2], files[3], packed) > 0
    return dict(files=files, packed=packed, dir=str(d))


def _same_frames(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for c in a.columns:
        assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
    assert a.attrs["snps"].equals(b.attrs["snps"]) and a.attrs["pairs"].equals(b.attrs["pairs"])
    for k in ("lam", "curve", "var_curve", "z"):
        assert np.array_equal(a.attrs[k], b.attrs[k], equal_nan=True), k
    assert all(a.attrs[k] == b.attrs[k] for k in ("n_nonfinite", "sweeps", "status"))


@pytest.mark.gpu
def test_hess_end_to_end_in_both_data_layers(ctx, study, monkeypatch):
    import cs_ref
    import hess_ref as hr
    from gauss_amd import api
    from gauss_amd import panel as pm
    inp, idx, dat, desc = study["files"]
    kw = dict(af1_cutoff=0.02, ctx=ctx)
    ld = api.computeLD(*REGION, cs_ref.WGT, inp, idx, dat, desc, **kw)
    snp, R = ld["snplist"], ld["cormat"]
    M = len(snp)
    one = api.hess(*REGION, cs_ref.WGT, [inp], idx, dat, desc, n=50_000, k_max=128, **kw)
    assert list(one.columns) == FRAME_COLUMNS and len(one) == 1 and len(one.attrs["pairs"]) == 0
    got = one.attrs["snps"]
    assert list(got.columns) == SNP_COLUMNS                # the SNPs are exactly computeLD's
    for c in ("rsid", "chr", "bp", "a1", "a2"):
        assert list(got[c]) == list(snp[c]), c
    assert np.array_equal(got["af1mix"].to_numpy(), snp["af1mix"].to_numpy())
    Rp, mono, n_bad = hr.repair(R)
    lam = one.attrs["lam"]
    assert lam.shape == (M,) and np.abs(lam - np.linalg.eigvalsh(Rp)[::-1]).max() <= 1e-10 * lam[0]
    assert one["n_snp"][0] == M and one["n_pos"][0] == hr.n_pos_of(lam, 1e-6) and one.attrs["n_nonfinite"] == n_bad and one.attrs["status"] == (2 if n_bad else 0)
    assert one.attrs["curve"].shape == (1, 128) and 1 <= one["k"][0] <= min(128, one["n_pos"][0]) and M > 100
    # the estimators are hess_estimates' on the returned pieces, and (sign-free) what eigh gives for the study's z
    ref = hr.rule(R, one.attrs["z"].T, 128)
    est = hr.estimates_loops(ref["lam"], ref["proj"], 50_000, k=int(one["k"][0]))
    print(f"REACHED hess table: {M} SNPs, n_pos {one['n_pos'][0]}, k {one['k'][0]}, H {one['H'][0]:.4f} (eigh {est['H'][0]:.4f}), h2 {one['h2'][0]:.3e}, sweeps {one.attrs['sweeps']}")
    assert abs(one["H"][0] - est["H"][0]) <= 1e-8 * abs(est["H"][0]) and abs(one["h2"][0] - est["h2"][0]) <= 1e-8 * max(abs(est["h2"][0]), 1e-3)
    # text and packed panels, and the packed panel through the full SNP map: bit for bit
    forms = [api.hess(*REGION, cs_ref.WGT, [inp], "(unused)", study["packed"], desc, n=50_000, k_max=128, **kw)]
    monkeypatch.setenv("GAUSS_HOST_FULL_MAP", "1")
    forms.append(api.hess(*REGION, cs_ref.WGT, [inp], "(unused)", study["packed"], desc, n=50_000, k_max=128, **kw))
    forms.append(api.hess(*REGION, cs_ref.WGT, [inp], idx, dat, desc, n=50_000, k_max=128, **kw))
    monkeypatch.delenv("GAUSS_HOST_FULL_MAP")
    for other in forms:
        _same_frames(one, other)

    # three study files: trait 2 and 3 at the SNPs of the first (and nowhere else), 3 pairs
    rng = np.random.default_rng(9)
    z1 = one.attrs["z"][:, 0]
    z2, z3 = 0.5 * z1 + rng.standard_normal(M), rng.standard_normal(M)
    cols = [snp[c].to_numpy() for c in ("rsid", "chr", "bp", "a1", "a2")]
    f2, f3, f2s, f3m = (os.path.join(study["dir"], f) for f in ("t2.txt", "t3.txt", "t2_swapped.txt", "t3_missing.txt"))
    pm.write_gwas(f2, *cols, z2)
    pm.write_gwas(f3, *cols, z3)
    three = api.hess(*REGION, cs_ref.WGT, [inp, f2, f3], idx, dat, desc, n=[50_000, 40_000, 30_000], k=60, k_max=128, overlap=0.1, **kw)
    pairs = three.attrs["pairs"]
    assert len(three) == 3 and list(pairs.columns) == ["a", "b", "C", "cov", "rg", "s"] and len(pairs) == 3
    assert list(zip(pairs["a"], pairs["b"])) == [(1, 2), (1, 3), (2, 3)] and np.all(pairs["s"] == 0.1) and np.all(three["k"] == 60)
    assert np.array_equal(three.attrs["z"], np.stack([z1, z2, z3], axis=1))
    assert three["H"][0] == api.hess(*REGION, cs_ref.WGT, [inp], idx, dat, desc, n=50_000, k=60, k_max=128, **kw)["H"][0]      # a trait on its own
    ref3 = hr.estimates_loops(*(lambda r: (r["lam"], r["proj"]))(hr.rule(R, np.stack([z1, z2, z3]), 128)), [50_000, 40_000, 30_000], k=60, overlap=0.1)
    assert np.allclose(three["H"], ref3["H"], rtol=1e-8) and np.allclose(pairs["C"], ref3["C"][pairs["a"] - 1, pairs["b"] - 1], rtol=1e-8, atol=1e-8)
    assert np.allclose(pairs["cov"], ref3["cov"][pairs["a"] - 1, pairs["b"] - 1], rtol=1e-8, atol=1e-12)
    # swapped alleles in file 2 flip its z: C_12 and C_23 change sign, every H stays
    pm.write_gwas(f2s, cols[0], cols[1], cols[2], cols[4], cols[3], z2)
    swapped = api.hess(*REGION, cs_ref.WGT, [inp, f2s, f3], idx, dat, desc, n=[50_000, 40_000, 30_000], k=60, k_max=128, **kw)
    plain = api.hess(*REGION, cs_ref.WGT, [inp, f2, f3], idx, dat, desc, n=[50_000, 40_000, 30_000], k=60, k_max=128, **kw)
    assert np.array_equal(swapped.attrs["z"][:, 1], -z2) and np.array_equal(swapped["H"].to_numpy(), plain["H"].to_numpy())
    cs, cp = swapped.attrs["pairs"]["C"].to_numpy(), plain.attrs["pairs"]["C"].to_numpy()
    assert np.array_equal(cs, cp * np.array([-1.0, 1.0, -1.0])) and np.all(cp != 0)
    # a file that lacks a SNP is refused, naming the file and the SNP
    keep = np.arange(M) != 7
    pm.write_gwas(f3m, *(c[keep] for c in cols), z3[keep])
    with pytest.raises(Exception, match=r"t3_missing\.txt lacks 1 of the window's %d measured SNPs, the first is %s" % (M, re.escape(str(cols[0][7])))):
        api.hess(*REGION, cs_ref.WGT, [inp, f2, f3m], idx, dat, desc, n=50_000, **kw)


@pytest.mark.gpu
def test_the_parameters_and_the_files_are_refused_with_their_messages(ctx, tmp_path):
    from gauss_amd import api
    missing = str(tmp_path / "nothing.txt")
    args = (22, 1, 2, (["a"], [1.0]), [missing], missing, missing, missing)
    with pytest.raises(Exception, match="nothing.txt"):
        api.hess(*args, n=1000, ctx=ctx)
    for text, kw in (("k_max = 1025; a call projects on 1 .. 1024 eigenvectors", dict(k_max=1025)), ("k_max = 0; it must be at least 1", dict(k_max=0)),
                     ("eig_min = 1 is outside [0, 1)", dict(eig_min=1.0)), ("eig_min = -0.5 is outside [0, 1)", dict(eig_min=-0.5))):
        with pytest.raises(Exception, match=re.escape(text)):
            api.hess(*args, n=1000, ctx=ctx, **kw)
    with pytest.raises(Exception, match=re.escape("65 study files; a call takes 1 .. 64")):
        api.hess(22, 1, 2, (["a"], [1.0]), [missing] * 65, missing, missing, missing, n=1000, ctx=ctx)
    with pytest.raises(ValueError, match="at least one study file"):
        api.hess(22, 1, 2, (["a"], [1.0]), [], missing, missing, missing, n=1000, ctx=ctx)


@pytest.mark.gpu
def test_a_planted_block_through_files(ctx, tmp_path):
    """A synthetic panel of 120 SNPs and 2 400 samples in two populations; z_a = sqrt(n) R beta_a and z_b = sqrt(n) R beta_b with beta_b
    sharing half of beta_a's SNPs, R the LD computeLD returns for the same files: with k = M, H = z^T R^-1 z, so h2 has the closed form
    (z^T R^-1 z - M) / (n - M), here computed by np.linalg.solve; rg has the planted, positive sign"""
    from gauss_amd import api
    from gauss_amd import panel as pm
    from test_gpu_clump import _panel
    n_snp, n = 120, 50_000.0
    p = _panel(n_snp, seed=2026, n_samples=2400, n_pop=1)
    G, bp = p["G"], (1_000_000 + 300 * np.arange(n_snp)).astype(np.int32)
    pops = [("AAA", 1400, "EUR"), ("BBB", 1000, "ASN")]
    af = np.stack([G[:, :1400].sum(axis=1) / 2800.0, G[:, 1400:].sum(axis=1) / 2000.0], axis=1)
    rsid, chrs = np.array([f"rs{i}" for i in range(n_snp)]), np.full(n_snp, 22)
    a1, a2 = np.full(n_snp, "A"), np.full(n_snp, "C")
    q = {k: os.path.join(str(tmp_path), k) for k in ("gwas.txt", "b.txt", "index.gz", "data.gz", "desc.txt")}
    pm.write_pop_desc(q["desc.txt"], pops)
    pm.write_panel_fast(q["index.gz"], q["data.gz"], rsid, chrs, bp, a1, a2, G, af, [1400, 1000], threads=2)
    pm.write_gwas(q["gwas.txt"], rsid, chrs, bp, a1, a2, np.ones(n_snp))
    wgt = (["AAA", "BBB"], [0.6, 0.4])
    args = (22, int(bp[0]), int(bp[-1]), wgt)
    panel = (q["index.gz"], q["data.gz"], q["desc.txt"])
    ld = api.computeLD(*args, q["gwas.txt"], *panel, af1_cutoff=0.01, ctx=ctx)
    R = ld["cormat"]
    assert len(R) == n_snp and np.all(np.isfinite(R)) and np.linalg.eigvalsh(R)[0] > 1e-4
    rng = np.random.default_rng(12)
    beta_a, beta_b = np.zeros(n_snp), np.zeros(n_snp)
    causal = rng.choice(n_snp, size=10, replace=False)
    beta_a[causal] = rng.normal(0, 0.03, size=10)
    beta_b[causal[:5]] = beta_a[causal[:5]]                # b shares half of a's effects, with their signs
    beta_b[rng.choice(np.setdiff1d(np.arange(n_snp), causal), size=5, replace=False)] = rng.normal(0, 0.03, size=5)
    za, zb = np.sqrt(n) * R @ beta_a, np.sqrt(n) * R @ beta_b
    pm.write_gwas(q["gwas.txt"], rsid, chrs, bp, a1, a2, za)
    pm.write_gwas(q["b.txt"], rsid, chrs, bp, a1, a2, zb)
    df = api.hess(*args, [q["gwas.txt"], q["b.txt"]], *panel, n=n, k=n_snp, k_max=n_snp, eig_min=0.0, af1_cutoff=0.01, ctx=ctx)
    assert list(df.attrs["snps"]["rsid"]) == list(rsid) and np.all(df["k"] == n_snp) and np.all(df["n_pos"] == n_snp)
    assert np.array_equal(df.attrs["z"], np.stack([za, zb], axis=1))
    Ha, Hb, Cab = za @ np.linalg.solve(R, za), zb @ np.linalg.solve(R, zb), za @ np.linalg.solve(R, zb)
    h2 = (np.array([Ha, Hb]) - n_snp) / (n - n_snp)
    print(f"REACHED hess planted through files: h2 {df['h2'].to_numpy()} closed form {h2}, C {df.attrs['pairs']['C'][0]:.6f} / {Cab:.6f}, rg {df.attrs['pairs']['rg'][0]}")
    assert np.abs(df["h2"].to_numpy() - h2).max() <= 1e-8 and np.abs(df["H"].to_numpy() / np.array([Ha, Hb]) - 1).max() <= 1e-8
    assert abs(df.attrs["pairs"]["C"][0] - Cab) <= 1e-8 * abs(Cab) and Cab > 0 and df.attrs["pairs"]["cov"][0] > 0
    # z is noise-free, so H = n beta^T R beta exactly; it is above M here (a local h2 of about 1 %), so both h2 are positive and rg is
    # the planted, positive one
    true = n * np.array([beta_a @ R @ beta_a, beta_b @ R @ beta_b, beta_a @ R @ beta_b])
    assert np.allclose([Ha, Hb, Cab], true, rtol=1e-8) and true[0] > 2 * n_snp and true[1] > 2 * n_snp and true[2] / np.sqrt(true[0] * true[1]) > 0.2
    rg = df.attrs["pairs"]["rg"][0]
    assert np.all(df["h2"] > 0) and rg > 0 and abs(rg - (Cab / n) / np.sqrt(h2[0] * h2[1])) <= 1e-8
