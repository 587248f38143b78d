"""The host layer of LD clumping.  CPU: the binding and its argument types, the header / export map / dynamic symbol table,
and clump_keys / clump_output on a hand-made table (a stand-alone program under the address and
undefined-behaviour sanitizers; nothing is loaded into Python).
GPU: api.clump, files -> frame, on the text panel, the packed panel and the packed panel through the full SNP map, against
api.computeLD's SNP list and tests/clump_ref.py on api.computeLD's matrix; and a planted region with two causal blocks."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = ctypes


def test_the_binding_and_its_argument_types():
    from gauss_amd import _lib, api, hotpath
    assert "gauss_ld_clump_rows" in _lib.SYMBOLS and "gauss_host_clump" in api.HOST_SYMBOLS
    lib = _lib.load()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rows, clump = lib.gauss_ld_rows.argtypes, lib.gauss_ld_clump_rows.argtypes
    # gauss_ld_rows' row arguments (without diag and out_cor), then bp, key, n_key, radius, the three thresholds, the four outputs
    assert clump[:11] == rows[:11] and clump[11] == rows[12] == C.c_int
    assert clump[12:] == [ip, dp, C.c_int, C.c_int64, C.c_double, C.c_double, C.c_double, ip, ip, dp, ip]
    h = api.load_host()
    assert h.gauss_host_clump.argtypes == h.gauss_host_computeLD.argtypes[:-1] + [C.c_double] * 4 + [h.gauss_host_computeLD.argtypes[-1]]
    assert callable(api.clump) and callable(hotpath.ld_clump) and callable(hotpath.ld_clump_rows)
    assert hotpath.CLUMP_KEY_INDEX == api.slct_chi2(1e-4) and hotpath.CLUMP_KEY_MEMBER == api.slct_chi2(1e-2)


def test_header_export_map_and_symbol_table_agree():
    from gauss_amd import _lib, api
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, path)).read(), flags=re.S)
    assert re.search(r"\bint\s+gauss_ld_clump_rows\s*\(", strip("include/gauss_hip.h"))
    assert re.search(r"\bint\s+gauss_host_clump\s*\(", strip("include/gauss_host.h"))
    hdr = open(os.path.join(ROOT, "include", "gauss_hip.h")).read()
    assert re.search(r"#define\s+GAUSS_CLUMP_MAX_M\s+%d\b" % _lib.CLUMP_MAX_M, hdr)
    assert re.search(r"#define\s+GAUSS_CLUMP_MAX_KEYS\s+%d\b" % _lib.CLUMP_MAX_KEYS, hdr)
    assert "global: gauss_*;" in open(os.path.join(ROOT, "gauss_amd", "csrc", "exports.map")).read()
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm not available")
    _lib.load(), api.load_host()                           # (built on first use)
    for so, name in (("libgauss_hip.so", "gauss_ld_clump_rows"), ("libgauss_host.so", "gauss_host_clump")):
        syms = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "gauss_amd", "lib", so)], text=True)
        assert re.search(r" T %s$" % name, syms, flags=re.M), (so, name)
        assert not re.search(r" [TW] (?!gauss_)\w*clump", syms), so      # no internal of the feature leaks


@pytest.mark.gpu
def test_the_thresholds_and_the_files_are_refused_with_their_messages(ctx, tmp_path):
    """Through the whole call, on a real context: a threshold out of range, then a file that is not there"""
    from gauss_amd import api
    missing = str(tmp_path / "nothing.txt")
    args = (22, 1, 2, (["a"], [1.0]), missing, missing, missing, missing)
    with pytest.raises(Exception, match="nothing.txt"):
        api.clump(*args, ctx=ctx)
    for text, kw in (("p2 = 0.001 is below p1 = 0.01", dict(p1=1e-2, p2=1e-3)), ("r2 = 1.5 is outside", dict(r2=1.5)),
                     ("r2 = -0.5 is outside", dict(r2=-0.5)), ("kb = -1", dict(kb=-1)), ("kb = inf", dict(kb=np.inf)),
                     ("p1 = 0 is outside (0, 1]", dict(p1=0.0)), ("p1 = -0.01 is outside (0, 1]", dict(p1=-0.01)),
                     ("p2 = 1.5 is outside (0, 1]", dict(p2=1.5))):
        with pytest.raises(Exception, match=re.escape(text)):
            api.clump(*args, ctx=ctx, **kw)


TABLE_MAIN = r'''
#include "host_internal.h"
static void dump(const char* what, const gauss_table& t) {
    std::printf("%s cols", what);
    for (auto& c : t.cols) std::printf(" %s:%d:%zu", c.name.c_str(), c.type, c.type == GAUSS_COL_STR ? c.s.size() : c.type == GAUSS_COL_INT ? c.i.size() : c.d.size());
    std::printf("\n");
    for (auto& c : t.cols) {
        std::printf("%s %s", what, c.name.c_str());
        for (auto& x : c.s) std::printf(" %s", x.c_str());
        for (int x : c.i) std::printf(" %d", x);
        for (double x : c.d) std::printf(" %a", x);
        std::printf("\n");
    }
    for (auto& m : t.named) {
        std::printf("%s named %s %d %d", what, m.name.c_str(), m.nrow, m.ncol);
        for (double x : m.d) std::printf(" %a", x);
        std::printf("\n");
    }
}
static std::unique_ptr<gauss_table> rows6() {
    const char* id[6] = {"s0", "s1", "s2", "s3", "s4", "s5"};
    std::unique_ptr<gauss_table> t(new gauss_table());
    add_ident_columns(*t, 6, [&](size_t i) { return SnpIdent{id[i], 22, 1000 + 10 * (long long)i, "C", "T"}; });
    Column& af = t->add("af1mix", GAUSS_COL_DBL);
    for (int i = 0; i < 6; i++) af.d.push_back(0.25 + 0.0625 * i);
    return t;
}
int main() {
    const std::vector<double> z = {1.0, -5.0, 3.0, 0.5, 4.5, -3.5};
    {   // two clumps: s1 leads s2; s4 leads s5; s0 and s3 are in none
        std::unique_ptr<gauss_table> t = rows6();
        const int32_t owner[6] = {-1, 1, 1, -1, 4, 4}, rank[6] = {0, 1, 0, 0, 2, 0};
        const double r2[6] = {NAN, 1.0, 0.75, NAN, 1.0, 0.5625};
        clump_output(*t, z, owner, rank, r2, 2);
        dump("two", *t);
    }
    {   // nothing clumps: an empty named matrix
        std::unique_ptr<gauss_table> t = rows6();
        const int32_t owner[6] = {-1, -1, -1, -1, -1, -1}, rank[6] = {0, 0, 0, 0, 0, 0};
        const double r2[6] = {NAN, NAN, NAN, NAN, NAN, NAN};
        clump_output(*t, z, owner, rank, r2, 0);
        dump("none", *t);
    }
    ClumpKeys k;
    int rc = clump_keys(NAN, NAN, NAN, NAN, k);
    std::printf("keys default %d %a %a %a %lld\n", rc, k.key_index, k.key_member, k.r2_min, (long long)k.radius);
    std::printf("keys chi2 %a %a\n", slct_chi2_of(1e-4), slct_chi2_of(1e-2));
    rc = clump_keys(5e-8, 5e-8, 0.0, 0.002, k);
    std::printf("keys tight %d %a %a %a %lld\n", rc, k.key_index, k.key_member, k.r2_min, (long long)k.radius);
    std::printf("keys chi2b %a\n", slct_chi2_of(5e-8));
    std::printf("keys bad %d", clump_keys(1e-2, 1e-3, 0.5, 250, k));
    std::printf(" %d", clump_keys(1e-4, 1e-2, 1.0000001, 250, k));
    std::printf(" %d", clump_keys(1e-4, 1e-2, 0.5, -0.001, k));
    std::printf(" %d", clump_keys(1e-4, 1e-2, 0.5, INFINITY, k));
    std::printf(" %d", clump_keys(1e-4, 1e-2, 1.0, 0.0, k));
    std::printf(" %d", clump_keys(0.0, 1e-2, 0.5, 250, k));
    std::printf(" %d", clump_keys(-1e-4, 1e-2, 0.5, 250, k));
    std::printf(" %d", clump_keys(1e-4, 1.5, 0.5, 250, k));
    std::printf(" %d", clump_keys(1e-4, 0.0, 0.5, 250, k));
    std::printf(" %d\n", clump_keys(1.0, 1.0, 0.5, 250, k));
    std::printf("keys why %s\n", gauss_host_last_error());
}
'''


@pytest.fixture(scope="module")
def table_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("clump_table")
    hdir = os.path.join(ROOT, "gauss_amd", "csrc", "host")
    src = tmp / "main.cpp"
    src.write_text(TABLE_MAIN)
    exe = tmp / "table"
    flags = [gxx, "-std=c++17", "-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + hdir]
    srcs = [str(src), os.path.join(hdir, "host_tables.cpp")]
    objs = [str(tmp / f"{k}.o") for k in range(len(srcs))]
    jobs = [subprocess.Popen(flags + ["-c", s, "-o", o]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    subprocess.check_call(flags + objs + ["-o", str(exe), "-Wl,--unresolved-symbols=ignore-all", "-lz", "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.strip().split("\n")


def _table(lines, tag):
    mine = [ln.split()[1:] for ln in lines if ln.startswith(tag + " ")]
    assert mine and mine[0][0] == "cols"
    names = [c.split(":")[0] for c in mine[0][1:]]
    body = {}
    for tok in mine[1:]:
        key, vals = ("named " + tok[1], tok[2:]) if tok[0] == "named" else (tok[0], tok[1:])
        body.setdefault(key, []).extend(vals)
    return names, body


HEX = float.fromhex
COLUMNS = ["rsid", "chr", "bp", "a1", "a2", "af1mix", "z", "pval", "clump", "index_rsid", "r2"]


def test_the_table_has_one_row_per_snp_and_one_matrix_row_per_clump(table_output):
    from math import erfc, sqrt
    names, t = _table(table_output, "two")
    assert names == COLUMNS
    assert t["rsid"] == ["s0", "s1", "s2", "s3", "s4", "s5"] and t["bp"] == ["1000", "1010", "1020", "1030", "1040", "1050"]
    z = [1.0, -5.0, 3.0, 0.5, 4.5, -3.5]
    assert [HEX(x) for x in t["z"]] == z
    for got, zi in zip(t["pval"], z):
        assert abs(HEX(got) - erfc(abs(zi) / sqrt(2.0))) <= 1e-15 * erfc(abs(zi) / sqrt(2.0))
    assert t["clump"] == ["0", "1", "1", "0", "2", "2"] and t["index_rsid"] == [".", "s1", "s1", ".", "s4", "s4"]
    r2 = [HEX(x) for x in t["r2"]]
    assert np.isnan(r2[0]) and np.isnan(r2[3]) and r2[1:3] == [1.0, 0.75] and r2[4:] == [1.0, 0.5625]
    # clumps [2 x 4], column-major: index row, size, first bp, last bp
    assert t["named clumps"][:2] == ["2", "4"]
    assert [HEX(x) for x in t["named clumps"][2:]] == [1.0, 4.0, 2.0, 2.0, 1010.0, 1040.0, 1020.0, 1050.0]
    names, t = _table(table_output, "none")
    assert names == COLUMNS and t["clump"] == ["0"] * 6 and t["index_rsid"] == ["."] * 6 and t["named clumps"] == ["0", "4"]


def test_the_thresholds_come_from_the_p_values(table_output):
    keys = {ln.split()[1]: ln.split()[2:] for ln in table_output if ln.startswith("keys ")}
    chi2 = [HEX(x) for x in keys["chi2"]]
    d = keys["default"]                                    # PLINK's defaults: 1e-4, 1e-2, 0.5, 250 kb
    assert d[0] == "0" and [HEX(x) for x in d[1:4]] == [chi2[0], chi2[1], 0.5] and d[4] == "250000"
    assert 15.13 < chi2[0] < 15.14 and 6.63 < chi2[1] < 6.64
    t = keys["tight"]
    assert t[0] == "0" and HEX(t[1]) == HEX(t[2]) == HEX(keys["chi2b"][0]) and HEX(t[3]) == 0.0 and t[4] == "2"      # 0.002 kb
    # p2 < p1, r2 above 1, kb negative, kb infinite; then r2 = 1 and kb = 0 pass; p outside (0, 1] is refused, never replaced; p = 1 passes
    assert keys["bad"] == ["-1", "-1", "-1", "-1", "0", "-1", "-1", "-1", "-1", "0"]


# ---- files -> frame ------------------------------------------------------------------------------------------------
REGION = (22, 1_000_000, 2_400_000)


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    import cs_ref
    from gauss_amd import api
    files = cs_ref.study_files(tmp_path_factory.mktemp("clump_study"))
    packed = os.path.join(os.path.dirname(files[2]), "panel.gpk")
    assert api.pack_panel(files[1], files[2], files[3], packed) > 0
    return dict(files=files, packed=packed)


def _same_frames(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for c in a.columns:
        if a[c].dtype.kind == "f":
            assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
        else:
            assert list(a[c]) == list(b[c]), c
    assert a.attrs["clumps"].equals(b.attrs["clumps"])


def _check_frame(df, ld, p1, p2, r2, kb):
    """df against clump_ref.replay on computeLD's result for the same arguments"""
    import clump_ref as cr
    from gauss_amd import api
    snp, R = ld["snplist"], ld["cormat"]
    assert list(df.columns) == COLUMNS
    for c in ("rsid", "chr", "bp", "a1", "a2"):
        assert list(df[c]) == list(snp[c]), c
    assert np.array_equal(df["af1mix"].to_numpy(), snp["af1mix"].to_numpy())
    z = df["z"].to_numpy()
    want = cr.replay(R, df["bp"].to_numpy(), z * z, int(round(kb * 1000)), r2, api.slct_chi2(p1), api.slct_chi2(p2))
    own = want["owner"]
    rank_of = np.where(own >= 0, want["rank"][np.maximum(own, 0)], 0)
    assert np.array_equal(df["clump"].to_numpy(), rank_of)
    rs = np.array(list(df["rsid"]))
    assert list(df["index_rsid"]) == [rs[o] if o >= 0 else "." for o in own]
    assert np.array_equal(df["r2"].to_numpy(), want["r2"], equal_nan=True)
    cl = df.attrs["clumps"]
    assert list(cl.columns) == ["index_row", "size", "bp_first", "bp_last"] and len(cl) == want["n_clumps"]
    bp = df["bp"].to_numpy()
    for k in range(len(cl)):
        mem = np.flatnonzero(df["clump"].to_numpy() == k + 1)
        i = int(cl["index_row"][k])
        assert want["rank"][i] == k + 1 and own[i] == i
        assert (int(cl["size"][k]), int(cl["bp_first"][k]), int(cl["bp_last"][k])) == (len(mem), int(bp[mem].min()), int(bp[mem].max()))
    return want


@pytest.mark.gpu
def test_clump_end_to_end_in_both_data_layers(ctx, study, monkeypatch):
    import cs_ref
    from gauss_amd import api
    inp, idx, dat, desc = study["files"]
    kw = dict(af1_cutoff=0.02, ctx=ctx)
    ld = api.computeLD(*REGION, cs_ref.WGT, inp, idx, dat, desc, **kw)
    df = api.clump(*REGION, cs_ref.WGT, inp, idx, dat, desc, **kw)
    want = _check_frame(df, ld, 1e-4, 1e-2, 0.5, 250)
    M = len(df)
    n_members = int((want["owner"] >= 0).sum())
    print(f"REACHED clump table: {M} SNPs, {want['n_clumps']} clumps, {n_members} SNPs in one")
    assert M > 100 and 2 <= want["n_clumps"] <= n_members < M      # (what joins a lead is the planted region's test below)
    forms = [api.clump(*REGION, cs_ref.WGT, inp, "(unused)", study["packed"], desc, **kw)]
    monkeypatch.setenv("GAUSS_HOST_FULL_MAP", "1")
    forms.append(api.clump(*REGION, cs_ref.WGT, inp, "(unused)", study["packed"], desc, **kw))
    forms.append(api.clump(*REGION, cs_ref.WGT, inp, idx, dat, desc, **kw))
    monkeypatch.delenv("GAUSS_HOST_FULL_MAP")
    for other in forms:
        _same_frames(df, other)
    # other thresholds: a short radius and a strict r2 make more, smaller clumps; everything eligible is LD pruning of the region
    tight = api.clump(*REGION, cs_ref.WGT, inp, "(unused)", study["packed"], desc, p1=1e-3, p2=5e-2, r2=0.8, kb=20, **kw)
    _check_frame(tight, ld, 1e-3, 5e-2, 0.8, 20)
    everything = api.clump(*REGION, cs_ref.WGT, inp, "(unused)", study["packed"], desc, p1=1.0, p2=1.0, r2=0.2, kb=1000, **kw)
    w = _check_frame(everything, ld, 1.0, 1.0, 0.2, 1000)
    assert np.all(w["owner"] >= 0)
    with pytest.raises(Exception, match="p2 = 0.001 is below p1 = 0.01"):
        api.clump(*REGION, cs_ref.WGT, inp, idx, dat, desc, p1=1e-2, p2=1e-3, **kw)


@pytest.mark.gpu
def test_two_planted_blocks_give_two_clumps_with_the_planted_leads(ctx, tmp_path):
    """Two causal SNPs 10 kb apart, each with five tags (the causal SNP's genotypes with one in sixteen redrawn: r^2 about 0.8) among
    unlinked SNPs of small z: exactly two clumps, led by the causal SNPs, holding their tags and nothing else"""
    from gauss_amd import api
    from gauss_amd import panel as pm
    rng = np.random.default_rng(2024)
    n_snp, n = 60, 400
    pops = [("AAA", 240, "EUR"), ("BBB", 160, "ASN")]
    G = rng.binomial(2, rng.uniform(0.25, 0.75, size=(n_snp, 1)), size=(n_snp, n)).astype(np.uint8)
    lead_a, lead_b = 20, 40
    tags = {lead_a: [17, 18, 19, 21, 22], lead_b: [37, 38, 39, 41, 42]}
    z = rng.uniform(-1.0, 1.0, size=n_snp)
    for lead, zl in ((lead_a, 8.0), (lead_b, -7.0)):
        z[lead] = zl
        for k, t in enumerate(tags[lead]):
            G[t] = G[lead]
            flip = rng.random(n) < 1 / 16
            G[t, flip] = rng.integers(0, 3, size=int(flip.sum()))
            z[t] = np.sign(zl) * (4.0 + 0.5 * k)
    G[:, [0, 240]], G[:, [1, 241]] = 0, 2
    af = np.stack([G[:, :240].sum(axis=1) / 480.0, G[:, 240:].sum(axis=1) / 320.0], axis=1)
    bp = 1_000_000 + 500 * np.arange(n_snp)                # the leads are 20 SNPs = 10 kb apart
    rsid, chrs = np.array([f"rs{i}" for i in range(n_snp)]), np.full(n_snp, 22)
    a1, a2 = np.full(n_snp, "A"), np.full(n_snp, "C")
    q = {k: os.path.join(str(tmp_path), k) for k in ("gwas.txt", "index.gz", "data.gz", "desc.txt")}
    pm.write_pop_desc(q["desc.txt"], pops)
    pm.write_panel_fast(q["index.gz"], q["data.gz"], rsid, chrs, bp, a1, a2, G, af, [240, 160], threads=2)
    pm.write_gwas(q["gwas.txt"], rsid, chrs, bp, a1, a2, z)
    who = (["AAA", "BBB"], [0.6, 0.4])
    args = (22, int(bp[0]), int(bp[-1]), who, q["gwas.txt"], q["index.gz"], q["data.gz"], q["desc.txt"])
    df = api.clump(*args, af1_cutoff=0.01, ctx=ctx)
    assert list(df["rsid"]) == list(rsid)
    _check_frame(df, api.computeLD(*args, af1_cutoff=0.01, ctx=ctx), 1e-4, 1e-2, 0.5, 250)
    cl = df.attrs["clumps"]
    assert list(cl["index_row"]) == [lead_a, lead_b] and list(cl["size"]) == [6, 6]
    for k, lead in enumerate((lead_a, lead_b)):
        rows = sorted([lead] + tags[lead])
        assert list(np.flatnonzero(df["clump"].to_numpy() == k + 1)) == rows
        assert set(df["index_rsid"][rows]) == {f"rs{lead}"} and np.all(df["r2"].to_numpy()[rows] >= 0.5)
        assert (int(cl["bp_first"][k]), int(cl["bp_last"][k])) == (int(bp[rows[0]]), int(bp[rows[-1]]))
    assert int((df["clump"] == 0).sum()) == n_snp - 12
