"""The host layer of the gene-based sum-of-chi2 test.  CPU: the bindings and their argument types, the header / export map / dynamic
symbol table, and sumchi2_pval / sumchi2_output on hand-made genes (a stand-alone program under the address and undefined-behaviour
sanitizers; nothing is loaded into Python).
GPU: api.sumchi2 / api.sumchi2mix, files -> frame, on the text panel and the packed panel, bit for bit; the genes are api.jepeg's;
num_kept, chisq, pval and the eigenvalues of every gene at the default pruning rebuilt from the files on the CPU (the restated data
layer, each gene's SNPs in position order, the CPU oracle's LD, tests/sumchi2_ref.py), pooled and weighted; and a planted study in
which one gene's SNPs carry a shared effect that none of them shows alone."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sumchi2_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = ctypes


def test_the_bindings_and_their_argument_types():
    from gauss_amd import _lib, api, hotpath
    for name in ("gauss_gene_sumchi2", "gauss_gene_sumchi2_rows"):
        assert name in _lib.SYMBOLS
    for name in ("gauss_host_sumchi2", "gauss_host_sumchi2mix", "gauss_host_sumchi2_pval"):
        assert name in api.HOST_SYMBOLS
    lib = _lib.load()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    tail = [dp, C.c_int, C.c_double, ip, ip, dp, dp, ip, ip, ip]
    # gauss_gene_ld_batch[_rows]' arguments without diag and out_blocks (on_device stays, behind the genes), then z, n_trait, prune_r2, the outputs
    assert lib.gauss_gene_sumchi2.argtypes == lib.gauss_gene_ld_batch.argtypes[:-2] + tail
    assert lib.gauss_gene_sumchi2_rows.argtypes == lib.gauss_gene_ld_batch_rows.argtypes[:-3] + [C.c_int] + tail
    h = api.load_host()
    assert h.gauss_host_sumchi2.argtypes == h.gauss_host_jepeg.argtypes[:-1] + [C.c_double, h.gauss_host_jepeg.argtypes[-1]]
    assert h.gauss_host_sumchi2mix.argtypes == h.gauss_host_jepegmix.argtypes[:-1] + [C.c_double, h.gauss_host_jepegmix.argtypes[-1]]
    assert h.gauss_host_sumchi2_pval.argtypes == [dp, C.c_int, C.c_double, dp, C.POINTER(C.c_int)]
    assert all(callable(f) for f in (api.sumchi2, api.sumchi2mix, api.sumchi2_pval, hotpath.gene_sumchi2, hotpath.gene_sumchi2_rows))
    assert (_lib.SUMCHI2_MAX_N, _lib.SUMCHI2_MAX_KEPT, _lib.SUMCHI2_MAX_TRAITS) == (sr.MAX_N, sr.MAX_KEPT, 64)
    assert (_lib.ST_NOCONV, _lib.ST_SUMCHI2_TOOLARGE, _lib.ST_SUMCHI2_EMPTY) == (sr.ST_NOCONV, sr.ST_TOOLARGE, sr.ST_EMPTY)


def test_header_export_map_and_symbol_table_agree():
    from gauss_amd import _lib, api
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, path)).read(), flags=re.S)
    for name in ("gauss_gene_sumchi2", "gauss_gene_sumchi2_rows"):
        assert re.search(r"\bint\s+%s\s*\(" % name, strip("include/gauss_hip.h")), name
    for name in ("gauss_host_sumchi2", "gauss_host_sumchi2mix", "gauss_host_sumchi2_pval"):
        assert re.search(r"\bint\s+%s\s*\(" % name, strip("include/gauss_host.h")), name
    hdr = open(os.path.join(ROOT, "include", "gauss_hip.h")).read()
    for name, val in (("GAUSS_SUMCHI2_MAX_N", _lib.SUMCHI2_MAX_N), ("GAUSS_SUMCHI2_MAX_KEPT", _lib.SUMCHI2_MAX_KEPT),
                      ("GAUSS_SUMCHI2_MAX_TRAITS", _lib.SUMCHI2_MAX_TRAITS), ("GAUSS_ST_SUMCHI2_TOOLARGE", _lib.ST_SUMCHI2_TOOLARGE),
                      ("GAUSS_ST_SUMCHI2_EMPTY", _lib.ST_SUMCHI2_EMPTY)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    assert "global: gauss_*;" in open(os.path.join(ROOT, "gauss_amd", "csrc", "exports.map")).read()
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm not available")
    _lib.load(), api.load_host()                           # (built on first use)
    for so, names in (("libgauss_hip.so", ("gauss_gene_sumchi2", "gauss_gene_sumchi2_rows")),
                      ("libgauss_host.so", ("gauss_host_sumchi2", "gauss_host_sumchi2mix", "gauss_host_sumchi2_pval"))):
        syms = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "gauss_amd", "lib", so)], text=True)
        for name in names:
            assert re.search(r" T %s$" % name, syms, flags=re.M), (so, name)
        assert not re.search(r" [TW] (?!gauss_)\w*sumchi2", syms), so      # no internal of the feature leaks


def test_the_library_pval_is_the_replay():
    """gauss_host_sumchi2_pval (no GPU) against tests/sumchi2_ref.py's saddle on spectra and tails of every branch"""
    from gauss_amd import api
    rng = np.random.default_rng(4)
    lams = [np.array([2.5]), np.array([1.0, 1.0]), np.linspace(0.02, 3.0, 128), 4.0 * 0.9 ** np.arange(40),
            np.concatenate([rng.uniform(0.1, 2.0, 30), [-1e-12, 0.0, np.nan]])]
    for lam in lams:
        l = lam[lam > 0]
        s1, sd = l.sum(), np.sqrt(2 * (l * l).sum())
        for q in (-1.0, 0.0, 1e-3, s1 - 2 * sd, s1 - 5e-4 * sd, s1, s1 + 5e-4 * sd, s1 + 1.5e-3 * sd, s1 + 3 * sd, s1 + 12 * sd, s1 + 60 * sd, np.nan):
            got, n_pos = api.sumchi2_pval(lam, q, n_pos=True)
            want = sr.saddle(lam, q)
            assert n_pos == len(l)
            assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-10 * want, (len(lam), q, got, want)
    assert np.isnan(api.sumchi2_pval([], 1.0)) and api.sumchi2_pval([np.nan, -1.0], 1.0, n_pos=True)[1] == 0
    assert 0 < api.sumchi2_pval(np.ones(4), 1400.0) < 1e-290


TABLE_MAIN = r'''
#include "host_internal.h"
static void dump(const char* what, const gauss_table& t) {
    std::printf("%s cols", what);
    for (auto& c : t.cols) std::printf(" %s:%d:%zu", c.name.c_str(), c.type, c.type == GAUSS_COL_STR ? c.s.size() : c.type == GAUSS_COL_INT ? c.i.size() : c.d.size());
    std::printf("\n");
    for (auto& c : t.cols) {
        std::printf("%s %s", what, c.name.c_str());
        for (auto& x : c.s) std::printf(" [%s]", x.c_str());
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
int main() {
    {   // four genes: solved, too large, empty, not converged
        const std::vector<std::string> geneid = {"G0", "G1", "G2", "G3"}, rsid = {"s0", "s1", "s2", "s3", "s4", "s5", "s6"};
        const std::vector<int32_t> gene_off = {0, 3, 5, 5, 7};
        const std::vector<double> z = {1.0, -3.0, 2.0, 0.5, NAN, 4.0, -4.5};
        std::vector<double> lam(4 * 128, NAN);
        lam[0] = 1.75; lam[1] = 0.25;
        const int32_t n_kept[4] = {2, 200, 0, 2}, top[4] = {1, 0, -1, 1}, status[4] = {0, GAUSS_ST_SUMCHI2_TOOLARGE, GAUSS_ST_SUMCHI2_EMPTY, GAUSS_ST_NOCONV};
        const double q[4] = {10.0, 0.25, 0.0, 36.25};
        std::unique_ptr<gauss_table> t(sumchi2_output(geneid, gene_off, rsid, z, n_kept, lam.data(), q, top, status));
        dump("four", *t);
    }
    {   // no gene at all
        const std::vector<std::string> none;
        const std::vector<int32_t> gene_off = {0};
        const std::vector<double> z;
        std::unique_ptr<gauss_table> t(sumchi2_output(none, gene_off, none, z, nullptr, nullptr, nullptr, nullptr, nullptr));
        dump("none", *t);
    }
    const double l3[5] = {2.0, 0.5, -1e-9, NAN, 0.25};
    int n_pos = -1;
    double pv = sumchi2_pval(l3, 5, 9.0, &n_pos);
    std::printf("pval three %a %d\n", pv, n_pos);
    std::printf("pval mean %a\n", sumchi2_pval(l3, 5, 2.75, nullptr));
    std::printf("pval below %a\n", sumchi2_pval(l3, 5, 0.4, nullptr));
    std::printf("pval far %a\n", sumchi2_pval(l3, 5, 2500.0, nullptr));
    std::printf("pval one %a\n", sumchi2_pval(l3, 1, 7.0, &n_pos));
    pv = sumchi2_pval(l3 + 2, 2, 7.0, &n_pos);
    std::printf("pval none %a %d\n", pv, n_pos);
    std::printf("pval zero %a %a %a\n", sumchi2_pval(l3, 5, 0.0, nullptr), sumchi2_pval(l3, 5, -2.0, nullptr), sumchi2_pval(l3, 0, 1.0, nullptr));
    std::vector<double> big(128);
    for (int i = 0; i < 128; i++) big[i] = 0.02 + 0.0234 * i;
    std::printf("pval big %a %a\n", sumchi2_pval(big.data(), 128, 300.0, nullptr), sumchi2_pval(big.data(), 128, 60.0, nullptr));
}
'''


@pytest.fixture(scope="module")
def table_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("sumchi2_table")
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


HEX = float.fromhex
COLUMNS = ["geneid", "num_snp", "num_kept", "chisq", "pval", "lam_max", "n_pos", "status", "top_snp", "top_snp_pval", "message"]


def _rows(lines, tag):
    mine = [ln[len(tag) + 1:] for ln in lines if ln.startswith(tag + " ")]
    names = [c.split(":")[0] for c in mine[0].split()[1:]]
    body = {}
    for ln in mine[1:]:
        key, _, rest = ln.partition(" ")
        if key == "named":
            key, _, rest = rest.partition(" ")
            key = "named " + key
        body[key] = re.findall(r"\[(.*?)\]", rest) if "[" in rest else rest.split()
    return names, body


def test_the_table_has_one_row_per_gene_with_its_message(table_output):
    names, b = _rows(table_output, "four")
    assert names == COLUMNS
    assert b["geneid"] == ["G0", "G1", "G2", "G3"] and b["num_snp"] == ["3", "2", "0", "2"] and b["num_kept"] == ["2", "200", "0", "2"]
    assert [HEX(v) for v in b["chisq"]] == [10.0, 0.25, 0.0, 36.25]
    p = [HEX(v) for v in b["pval"]]
    assert abs(p[0] - sr.saddle([1.75, 0.25], 10.0)) <= 1e-10 * p[0] and all(np.isnan(v) for v in p[1:])
    lm = [HEX(v) for v in b["lam_max"]]
    assert lm[0] == 1.75 and all(np.isnan(v) for v in lm[1:])
    assert b["n_pos"] == ["2", "0", "0", "0"] and b["status"] == ["0", "128", "256", "4"]
    assert b["top_snp"] == ["s1", "s3", ".", "s6"]
    tp = [HEX(v) for v in b["top_snp_pval"]]
    assert abs(tp[0] - 2 * sr.pnorm_upper(3.0)) <= 1e-15 and np.isnan(tp[2]) and abs(tp[3] - 2 * sr.pnorm_upper(4.5)) <= 1e-18
    assert b["message"][0] == "" and "200 SNPs survive the pruning" in b["message"][1] and "at most 128" in b["message"][1]
    assert b["message"][2] == "no SNP of the gene is kept" and b["message"][3] == "the eigenvalue solve did not converge"
    lam = b["named lam"]
    assert lam[:2] == ["4", "128"] and len(lam) == 2 + 4 * 128
    m = np.array([HEX(v) for v in lam[2:]]).reshape(128, 4).T          # column-major
    assert m[0, 0] == 1.75 and m[0, 1] == 0.25 and np.all(np.isnan(m[0, 2:])) and np.all(np.isnan(m[1:]))
    names, b = _rows(table_output, "none")
    assert names == COLUMNS and all(b[c] == [] for c in COLUMNS) and b["named lam"] == ["0", "128"]


def test_the_pval_of_the_stand_alone_program_is_the_replay(table_output):
    get = lambda tag: [ln.split()[2:] for ln in table_output if ln.startswith("pval " + tag + " ")][0]
    l3 = [2.0, 0.5, -1e-9, np.nan, 0.25]
    close = lambda got, want: abs(HEX(got) - want) <= 1e-10 * want
    assert close(get("three")[0], sr.saddle(l3, 9.0)) and get("three")[1] == "3"
    assert close(get("mean")[0], sr.saddle(l3, 2.75, branch="edgeworth")) and close(get("below")[0], sr.saddle(l3, 0.4))
    assert close(get("far")[0], sr.saddle(l3, 2500.0)) and 0 < HEX(get("far")[0]) < 1e-200
    assert close(get("one")[0], 2 * sr.pnorm_upper(np.sqrt(3.5)))
    assert np.isnan(HEX(get("none")[0])) and get("none")[1] == "0"
    z = get("zero")
    assert HEX(z[0]) == 1.0 and HEX(z[1]) == 1.0 and np.isnan(HEX(z[2]))
    big = 0.02 + 0.0234 * np.arange(128)
    assert close(get("big")[0], sr.saddle(big, 300.0)) and close(get("big")[1], sr.saddle(big, 60.0))


# ---- GPU: files -> frame ---------------------------------------------------------------------------------------------------------
POPS = [("AAA", 160, "EUR"), ("BBB", 145, "EUR"), ("CCC", 170, "ASN"), ("DDD", 133, "AFR"), ("EEE", 152, "EUR"), ("FFF", 90, "ASN")]
WGT = (["aaa", "CCC", "eee", "FFF", "zzz"], [0.45, 0.2, 0.25, 0.161, 0.3])
PRUNE = 0.9


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    from gauss_amd import api, panel
    d = tmp_path_factory.mktemp("sumchi2_study")
    st = panel.make_synthetic_study(str(d), POPS, n_snp=700, bp_lo=1_000_000, bp_hi=2_400_000, n_genes=40, frac_measured=0.3, seed=17)
    p = st["paths"]
    st["packed"] = os.path.join(str(d), "panel.gpk")
    st["dir"] = str(d)
    assert api.pack_panel(p["index.gz"], p["data.gz"], p["desc.txt"], st["packed"]) > 0
    return st


def _ref_genes(mix, input_file, st, annot=None):
    """The reference statement from the files, on the CPU alone: the restated data layer of jepeg() / jepegmix() (oracle.feeder_py: which
    SNPs a gene holds, their z and genotypes), each gene's SNPs in position order, the CPU oracle's LD of them with diagonal 1.
    Returns [dict(geneid, rsid, z, R)] in gene-id order, the table's."""
    import oracle
    from oracle import feeder_py as fp
    p = st["paths"]
    pops = fp.read_ref_desc(p["desc.txt"])
    flags, w = fp.pop_flags_wgt(pops, *WGT) if mix else (fp.pop_flags(pops, "EUR"), None)
    m = fp.read_input_z(input_file, 0, 0, 0, True)
    fp.read_reference_index(m, p["index.gz"], 0, 0, 0, True)
    fp.read_annotation(m, annot or p["annot.txt"])
    vec = fp.make_snp_vec(m, p["data.gz"], flags, 0.01, w)                 # in (chromosome, position) order
    off = fp._selected_off(pops, flags)
    by_gene = {}
    for s in vec:
        if s.geneid != "." and s.type == 1:
            by_gene.setdefault(s.geneid, []).append(s)
    out = []
    for gid in sorted(by_gene):
        gs = by_gene[gid]
        assert all(a.bp < b.bp for a, b in zip(gs, gs[1:]))
        G = fp._matrix(gs)
        if len(gs) == 1:
            R = np.ones((1, 1))
        else:
            R = oracle.compute_ld(G, off, w) if mix else oracle.ld_pooled(G, off, 1.0)
            np.fill_diagonal(R, 1.0)
        out.append(dict(geneid=gid, rsid=[s.rsid for s in gs], z=np.array([s.z for s in gs]), R=R))
    return out


def _ref_table(genes, z_of=None, r2=PRUNE):
    """[dict(num_snp, num_kept, chisq, pval, lam, top)] of the genes through tests/sumchi2_ref.py; z_of: rsid -> z instead of the file's"""
    rows = []
    for g in genes:
        z = g["z"] if z_of is None else np.array([z_of[r] for r in g["rsid"]])
        r = sr.gene(g["R"], z, r2)
        rows.append(dict(num_snp=len(z), num_kept=r["n_kept"], chisq=float(r["q"][0]), lam=r["lam"], top=int(r["top"][0]), status=r["status"],
                         pval=sr.saddle(r["lam"], float(r["q"][0])) if r["status"] == 0 else np.nan, max_abs_z=float(np.abs(z).max())))
    return rows


def _same_frame(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for c in a.columns:
        if a[c].dtype.kind == "f":
            assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
        else:
            assert list(a[c]) == list(b[c]), c
    assert np.array_equal(a.attrs["lam"], b.attrs["lam"], equal_nan=True)


def _against_reference(df, genes, want, what, r2=PRUNE):
    """num_snp, num_kept, chisq, pval, the eigenvalues and the top SNP of the frame against the reference statement, gene by gene"""
    assert len(df) == len(want), what
    lam = df.attrs["lam"]
    for g, (gene, w) in enumerate(zip(genes, want)):
        tag = (what, g, gene["geneid"])
        # no pair of the gene sits on the pruning threshold under the oracle's LD (the project's LD entries are within 1e-12 of it)
        n = w["num_snp"]
        gap = np.abs(gene["R"] * gene["R"] - r2)[~np.eye(n, dtype=bool)]
        assert gap.size == 0 or float(gap.min()) > 1e-9, tag
        assert df["num_snp"][g] == n and df["num_kept"][g] == w["num_kept"] and df["status"][g] == w["status"] == 0, tag
        assert abs(df["chisq"][g] - w["chisq"]) <= 1e-12 * max(1.0, w["chisq"]), tag
        k = w["num_kept"]
        assert np.abs(lam[g, :k] - w["lam"][:k]).max() <= k * 1e-12 + 8 * k * 2.0 ** -52 * w["lam"][0] and np.all(np.isnan(lam[g, k:])), tag
        assert abs(df["pval"][g] - w["pval"]) <= 1e-8 * w["pval"], (tag, df["pval"][g], w["pval"])
        assert df["top_snp"][g] == gene["rsid"][w["top"]], tag
        assert abs(df["top_snp_pval"][g] - 2 * sr.pnorm_upper(w["max_abs_z"])) <= 1e-12 * df["top_snp_pval"][g], tag


@pytest.mark.gpu
@pytest.mark.parametrize("mix", [False, True])
def test_sumchi2_end_to_end_in_both_data_layers(ctx, study, mix):
    from gauss_amd import api
    p = study["paths"]
    inp, ann, idx, dat, desc = p["gwas.txt"], p["annot.txt"], p["index.gz"], p["data.gz"], p["desc.txt"]
    fn, who, jep = (api.sumchi2mix, WGT, api.jepegmix) if mix else (api.sumchi2, "EUR", api.jepeg)
    df = fn(who, inp, ann, idx, dat, desc, ctx=ctx)
    assert list(df.columns) == COLUMNS and len(df) > 10 and df.attrs["lam"].shape == (len(df), 128)
    _same_frame(df, fn(who, inp, ann, "(unused)", study["packed"], desc, ctx=ctx))
    # the genes are jepeg's (jepeg names a gene only where its own test has a degree of freedom)
    jp = jep(who, inp, ann, idx, dat, desc, ctx=ctx)
    assert len(jp) == len(df) and list(df["num_snp"]) == list(jp["num_snp"])
    named = jp["df"].to_numpy() > 0
    assert named.sum() > 5 and list(df["geneid"][named]) == list(jp["geneid"][named]) and list(df["top_snp"][named]) == list(jp["top_snp"][named])
    assert np.array_equal(df["top_snp_pval"].to_numpy()[named], jp["top_snp_pval"].to_numpy()[named])
    # chisq and pval at the default pruning, rebuilt from the files on the CPU: every gene, its SNPs in position order, the oracle's LD
    genes = _ref_genes(mix, inp, study)
    want = _ref_table(genes)
    assert list(df["geneid"]) == [g["geneid"] for g in genes]
    _against_reference(df, genes, want, "mix" if mix else "pooled")
    assert np.all(df["message"] == "") and np.array_equal(df["lam_max"].to_numpy(), df.attrs["lam"][:, 0])
    # nothing pruned
    full = fn(who, inp, ann, idx, dat, desc, prune_r2=1.0, ctx=ctx)
    assert list(full["num_kept"]) == list(full["num_snp"])
    for g, gene in enumerate(genes):
        q = float(np.sum(gene["z"] ** 2))
        assert abs(full["chisq"][g] - q) <= 1e-12 * max(1.0, q), g


@pytest.mark.gpu
@pytest.mark.parametrize("mix", [False, True])
def test_genes_of_neighbouring_snps_are_pruned_in_position_order(ctx, study, mix):
    """The study's own genes are SNPs scattered over the region: nothing of them is in LD.  Here 14 genes of up to 14 consecutive measured
    SNPs each (largest |r| about 0.85), named so that the sort by gene id moves every gene, pruned at r^2 > 0.3: which SNP survives
    depends on the order inside a gene, and the kept count, chisq and pval must be those of the position order."""
    from gauss_amd import api, panel
    p = study["paths"]
    meas = np.sort(study["measured"])
    rows = []
    for g in range(14):
        for s in meas[g * 14:(g + 1) * 14][::-1]:                            # (the file lists a gene's SNPs from the last to the first)
            rows.append((study["rsid"][s], 22, int(study["bp"][s]), study["a1"][s], study["a2"][s], f"LOC{(g * 5) % 14:02d}", panel.CATEGS[g % 6], 1.0))
    ann = os.path.join(study["dir"], f"dense_annot_{int(mix)}.txt")
    panel.write_annotation(ann, rows)
    fn, who = (api.sumchi2mix, WGT) if mix else (api.sumchi2, "EUR")
    genes = _ref_genes(mix, p["gwas.txt"], study, annot=ann)
    want = _ref_table(genes, r2=0.3)
    pruned = sum(w["num_kept"] < w["num_snp"] for w in want)
    assert len(genes) == 14 and pruned >= 7
    # the order matters: pruning a gene from its last SNP to its first keeps another set somewhere
    assert any(not np.array_equal(sr.prune(g["R"], 0.3)[0], sr.prune(g["R"][::-1, ::-1], 0.3)[0][::-1]) for g in genes)
    for data in (p["data.gz"], study["packed"]):
        df = fn(who, p["gwas.txt"], ann, p["index.gz"], data, p["desc.txt"], prune_r2=0.3, ctx=ctx)
        assert list(df["geneid"]) == [g["geneid"] for g in genes]
        _against_reference(df, genes, want, ("dense", mix), r2=0.3)
    print(f"REACHED dense genes mix {mix}: num_snp {list(df['num_snp'])} num_kept {list(df['num_kept'])}")


@pytest.mark.gpu
def test_a_planted_gene_is_found_and_the_null_genes_are_not(ctx, study):
    """One gene's SNPs carry a shared effect too small for any of them alone: no SNP of it passes 5e-8, the gene's pval is below 2.5e-6
    (the genome-wide gene threshold), every other gene's pval is above 1e-3.  The seed is picked on the CPU so that the reference
    statement alone (the restated data layer, the oracle's LD, tests/sumchi2_ref.py) says so; the frame must then say the same."""
    from gauss_amd import api
    p = study["paths"]
    genes = _ref_genes(True, p["gwas.txt"], study)
    target = max(range(len(genes)), key=lambda g: (len(genes[g]["rsid"]), -g))
    assert len(genes[target]["rsid"]) >= 5
    rows = [ln.split() for ln in open(p["gwas.txt"]).read().splitlines()[1:]]
    in_target = set(genes[target]["rsid"])
    found = None
    for seed in range(200):
        rng = np.random.default_rng(9000 + seed)
        z_of = {r[0]: float(rng.standard_normal()) for r in rows}
        for r in in_target:
            z_of[r] = 3.8 + 0.4 * float(rng.standard_normal())             # |z| = 5.45 is 5e-8
        want = _ref_table(genes, z_of)
        nulls = [w["pval"] for g, w in enumerate(want) if g != target]
        if want[target]["max_abs_z"] < 5.3 and want[target]["pval"] < 2.5e-7 and min(nulls) > 2e-3:
            found = (seed, z_of, want)
            break
    assert found is not None
    seed, z_of, want = found
    planted = os.path.join(study["dir"], "planted_gwas.txt")
    with open(planted, "w") as fh:
        fh.write("rsid chr bp a1 a2 z\n")
        for r in rows:
            fh.write(" ".join(r[:5]) + " " + repr(z_of[r[0]]) + "\n")
    for data in (p["data.gz"], study["packed"]):
        df = api.sumchi2mix(WGT, planted, p["annot.txt"], p["index.gz"], data, p["desc.txt"], ctx=ctx)
        assert list(df["geneid"]) == [g["geneid"] for g in genes]
        _against_reference(df, genes, want, "planted")
        assert df["top_snp_pval"][target] > 5e-8 and df["pval"][target] < 2.5e-6
        others = np.arange(len(df)) != target
        assert df["pval"][others].min() > 1e-3
        print(f"REACHED planted seed {seed}: gene {df['geneid'][target]} of {df['num_snp'][target]} SNPs ({df['num_kept'][target]} kept), top SNP p "
              f"{df['top_snp_pval'][target]:.2e}, gene p {df['pval'][target]:.2e}; smallest null gene p {df['pval'][others].min():.2e}")


@pytest.mark.gpu
def test_prune_r2_is_checked_and_defaults_to_fastbats(ctx, study):
    from gauss_amd import api
    p = study["paths"]
    args = ("EUR", p["gwas.txt"], p["annot.txt"], p["index.gz"], p["data.gz"], p["desc.txt"])
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(api.GaussError, match=re.escape("prune_r2 = %g is outside (0, 1]" % bad)):
            api.sumchi2(*args, prune_r2=bad, ctx=ctx)
    _same_frame(api.sumchi2(*args, prune_r2=None, ctx=ctx), api.sumchi2(*args, prune_r2=0.9, ctx=ctx))
    with pytest.raises(api.GaussError, match="nothing.txt"):
        api.sumchi2("EUR", "nothing.txt", *args[2:], ctx=ctx)
