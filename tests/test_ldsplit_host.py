"""The host layer of LD splitting.  CPU: the binding and its argument types, the header / export map / dynamic symbol table, and
ldsplit_params / ldsplit_output on a hand-made table (a stand-alone program under the address and undefined-behaviour sanitizers;
nothing is loaded into Python).
GPU: api.ldsplit, files -> frame, on the text panel, the packed panel and the packed panel through the full SNP map, against
api.computeLD's SNP list and tests/ldsplit_ref.py on api.computeLD's matrix; api.ldsplit_blocks tiles the region."""
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
    assert "gauss_ld_split_rows" in _lib.SYMBOLS and "gauss_host_ldsplit" in api.HOST_SYMBOLS
    lib = _lib.load()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rows, split = lib.gauss_ld_rows.argtypes, lib.gauss_ld_split_rows.argtypes
    # gauss_ld_rows' row arguments (without diag and out_cor), then bp, radius, thr_r2, the two sizes, max_K, max_r2, the four outputs
    assert split[:11] == rows[:11] and split[11] == rows[12] == C.c_int
    assert split[12:] == [ip, C.c_int64, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, dp, ip, dp, C.POINTER(C.c_int64)]
    h = api.load_host()
    ld = h.gauss_host_computeLD.argtypes
    assert h.gauss_host_ldsplit.argtypes == ld[:-1] + [C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double] + [ld[-1]]
    assert callable(api.ldsplit) and callable(api.ldsplit_blocks) and callable(hotpath.ld_split) and callable(hotpath.ld_split_rows)


def test_header_export_map_and_symbol_table_agree():
    from gauss_amd import _lib, api
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, path)).read(), flags=re.S)
    assert re.search(r"\bint\s+gauss_ld_split_rows\s*\(", strip("include/gauss_hip.h"))
    assert re.search(r"\bint\s+gauss_host_ldsplit\s*\(", strip("include/gauss_host.h"))
    hdr = open(os.path.join(ROOT, "include", "gauss_hip.h")).read()
    for name, value in (("M", _lib.LDSPLIT_MAX_M), ("SIZE", _lib.LDSPLIT_MAX_SIZE), ("K", _lib.LDSPLIT_MAX_K)):
        assert re.search(r"#define\s+GAUSS_LDSPLIT_MAX_%s\s+%d\b" % (name, value), hdr)
    assert (_lib.LDSPLIT_MAX_M, _lib.LDSPLIT_MAX_SIZE, _lib.LDSPLIT_MAX_K) == (8192, 4096, 128)
    assert "global: gauss_*;" in open(os.path.join(ROOT, "gauss_amd", "csrc", "exports.map")).read()
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm not available")
    _lib.load(), api.load_host()                           # (built on first use)
    for so, name in (("libgauss_hip.so", "gauss_ld_split_rows"), ("libgauss_host.so", "gauss_host_ldsplit")):
        syms = subprocess.check_output([nm, "-D", "--defined-only", os.path.join(ROOT, "gauss_amd", "lib", so)], text=True)
        assert re.search(r" T %s$" % name, syms, flags=re.M), (so, name)
        assert not re.search(r" [TW] (?!gauss_)\w*ldsplit", syms), so      # no internal of the feature leaks


def test_the_backtrack_reads_the_boundaries_from_prev():
    from gauss_amd import hotpath
    import ldsplit_ref as lr
    rng = np.random.default_rng(4)
    A = rng.uniform(-1, 1, size=(11, 11))
    R = np.triu(A, 1) + np.triu(A, 1).T + np.eye(11)
    ref = lr.replay(R, np.arange(11, dtype=np.int32), 1 << 32, 0.0, 2, 5, 7, 1.0)
    for K in range(1, 8):
        got = hotpath.ldsplit_backtrack(ref["cost"], ref["prev"], K)
        assert (got is None) == (ref["splits"][K] is None) and (got is None or np.array_equal(got, ref["splits"][K]))
    assert [K for K in range(1, 8) if ref["splits"][K] is not None] == [3, 4, 5]


def test_blocks_tile_by_position_and_a_boundary_between_two_snps_at_one_position_is_refused():
    """api.ldsplit_blocks on a hand-made result: 7 SNPs, rows 2 and 3 at one position"""
    import pandas as pd
    from gauss_amd import api
    bp = np.array([100, 110, 120, 120, 135, 150, 151])
    res = pd.DataFrame(dict(n_block=[2, 3], cost=[0.1, 0.2], perc_kept=[25 / 49, 17 / 49], cost2=[25, 17], max_size_used=[4, 3]))
    res.attrs["snps"] = pd.DataFrame(dict(rsid=[f"rs{i}" for i in range(7)], chr=22, bp=bp, a1="A", a2="C", af1mix=0.5))
    res.attrs["last"] = [np.array([3, 6]), np.array([2, 4, 6])]
    bl = api.ldsplit_blocks(res, 2)
    assert list(bl["first_row"]) == [0, 4] and list(bl["last_row"]) == [3, 6] and list(bl["size"]) == [4, 3]
    assert list(bl["first_rsid"]) == ["rs0", "rs4"] and list(bl["last_rsid"]) == ["rs3", "rs6"]
    assert list(bl["start_bp"]) == [100, 128] and list(bl["end_bp"]) == [127, 151]           # (120 + 135) // 2
    for k in range(2):
        inside = np.flatnonzero((bp >= bl["start_bp"][k]) & (bp <= bl["end_bp"][k]))
        assert inside[0] == bl["first_row"][k] and inside[-1] == bl["last_row"][k]
    with pytest.raises(api.GaussError, match=r"between blocks 1 and 2 of the split into 3 lies between two SNPs at bp 120 \(rs2, rs3\)"):
        api.ldsplit_blocks(res, 3)
    with pytest.raises(api.GaussError, match="no split into 4 blocks"):
        api.ldsplit_blocks(res, 4)
    for kw in (dict(min_size=0), dict(max_size=0), dict(max_K=0)):                           # 0 is "not given" to the C call only
        with pytest.raises(api.GaussError, match="it must be at least 1"):
            api.ldsplit(22, 1, 2, (["a"], [1.0]), "x", "x", "x", "x", **kw)


@pytest.mark.gpu
def test_the_parameters_and_the_files_are_refused_with_their_messages(ctx, tmp_path):
    """Through the whole call, on a real context: a parameter out of range, then a file that is not there"""
    from gauss_amd import api
    missing = str(tmp_path / "nothing.txt")
    args = (22, 1, 2, (["a"], [1.0]), missing, missing, missing, missing)
    with pytest.raises(Exception, match="nothing.txt"):
        api.ldsplit(*args, ctx=ctx)
    for text, kw in (("thr_r2 = 1.5 is outside [0, 1]", dict(thr_r2=1.5)), ("max_r2 = -0.5 is outside [0, 1]", dict(max_r2=-0.5)),
                     ("max_size = 4097; a block holds 1 .. 4096 SNPs", dict(max_size=4097)), ("min_size = 60 is outside 1 .. max_size = 50", dict(min_size=60, max_size=50)),
                     ("min_size = -1; it must be at least 1", dict(min_size=-1)), ("min_size = 0; it must be at least 1", dict(min_size=0)),
                     ("max_size = 0; it must be at least 1", dict(max_size=0)), ("max_K = 0; it must be at least 1", dict(max_K=0)), ("max_K = 129; a call splits into 1 .. 128 blocks", dict(max_K=129)),
                     ("kb = -1", dict(kb=-1)), ("kb = inf", dict(kb=np.inf))):
        with pytest.raises(Exception, match=re.escape(text)):
            api.ldsplit(*args, ctx=ctx, **kw)


TABLE_MAIN = r'''
#include "host_internal.h"
static void dump(const char* what, const gauss_table& t) {
    std::printf("%s cols", what);
    for (auto& c : t.cols) std::printf(" %s:%d:%zu", c.name.c_str(), c.type, c.type == GAUSS_COL_STR ? c.s.size() : c.type == GAUSS_COL_INT ? c.i.size() : c.d.size());
    std::printf("\n");
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
    {   // M = 6, max_K = 4: K = 1 has no split; K = 2: [0, 4) [4, 6); K = 3: [0, 1) [1, 4) [4, 6); K = 4 has none
        std::unique_ptr<gauss_table> t = rows6();
        const double cost[4] = {INFINITY, 0.5, 0.75, INFINITY};
        int32_t prev[4 * 7];
        for (int i = 0; i < 28; i++) prev[i] = -1;
        prev[0 * 7 + 4] = 0; prev[0 * 7 + 1] = 0;           // one block ending at 4 / at 1
        prev[1 * 7 + 6] = 4; prev[1 * 7 + 4] = 1;           // two blocks ending at 6 / at 4
        prev[2 * 7 + 6] = 4;                                // three blocks ending at 6
        const double mx[7] = {0.0, 0.125, 0.25, 0.5, 0.0625, 0.75, 0.0};
        ldsplit_output(*t, 6, 4, cost, prev, mx, 3);
        dump("two", *t);
    }
    {   // nothing feasible: empty matrices
        std::unique_ptr<gauss_table> t = rows6();
        const double cost[2] = {INFINITY, INFINITY};
        int32_t prev[14];
        for (int i = 0; i < 14; i++) prev[i] = -1;
        const double mx[7] = {0, 0, 0, 0, 0, 0, 0};
        ldsplit_output(*t, 6, 2, cost, prev, mx, 0);
        dump("none", *t);
    }
    LdSplitParams k;
    int rc = ldsplit_params(NAN, 0, 0, 0, NAN, NAN, k);
    std::printf("par default %d %a %d %d %d %a %lld\n", rc, k.thr_r2, k.min_size, k.max_size, k.max_K, k.max_r2, (long long)k.radius);
    rc = ldsplit_params(0.0, 1, 4096, 1, 1.0, 0.002, k);
    std::printf("par edge %d %a %d %d %d %a %lld\n", rc, k.thr_r2, k.min_size, k.max_size, k.max_K, k.max_r2, (long long)k.radius);
    std::printf("par bad %d", ldsplit_params(1.5, 1, 10, 1, 1.0, NAN, k));
    std::printf(" %d", ldsplit_params(0.1, 1, 10, 1, -0.1, NAN, k));
    std::printf(" %d", ldsplit_params(0.1, 11, 10, 1, 1.0, NAN, k));
    std::printf(" %d", ldsplit_params(0.1, -1, 10, 1, 1.0, NAN, k));
    std::printf(" %d", ldsplit_params(0.1, 1, 4097, 1, 1.0, NAN, k));
    std::printf(" %d", ldsplit_params(0.1, 1, 10, 129, 1.0, NAN, k));
    std::printf(" %d", ldsplit_params(0.1, 1, 10, -1, 1.0, NAN, k));
    std::printf(" %d", ldsplit_params(0.1, 1, 10, 1, 1.0, -0.001, k));
    std::printf(" %d", ldsplit_params(0.1, 1, 10, 1, 1.0, INFINITY, k));
    std::printf(" %d\n", ldsplit_params(0.1, 10, 10, 128, 0.0, 0.0, k));
    std::printf("par why %s\n", gauss_host_last_error());
}
'''


@pytest.fixture(scope="module")
def table_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("ldsplit_table")
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
SNP_COLUMNS = ["rsid", "chr", "bp", "a1", "a2", "af1mix"]


def _named(lines, tag):
    cols = [ln.split()[2:] for ln in lines if ln.startswith(tag + " cols")][0]
    out = {}
    for ln in lines:
        tok = ln.split()
        if tok[0] == tag and tok[1] == "named":
            nr, nc = int(tok[3]), int(tok[4])
            out[tok[2]] = np.array([HEX(x) for x in tok[5:]]).reshape(nc, nr).T
    return [c.split(":")[0] for c in cols], out


def test_the_table_keeps_the_snps_and_holds_one_row_per_feasible_K(table_output):
    names, m = _named(table_output, "two")
    assert names == SNP_COLUMNS and list(m) == ["splits", "last", "max_r2_at", "n_nonfinite"]
    # n_block, cost, perc_kept, cost2, max_size_used: sizes 4 + 2, then 1 + 3 + 2
    assert m["splits"].tolist() == [[2.0, 0.5, 20 / 36, 20.0, 4.0], [3.0, 0.75, 14 / 36, 14.0, 3.0]]
    assert m["last"].tolist() == [[3.0, 5.0, -1.0], [0.0, 3.0, 5.0]]
    assert m["max_r2_at"].reshape(-1).tolist() == [0.0, 0.125, 0.25, 0.5, 0.0625, 0.75, 0.0] and m["n_nonfinite"].tolist() == [[3.0]]
    names, m = _named(table_output, "none")
    assert names == SNP_COLUMNS and m["splits"].shape == (0, 5) and m["last"].size == 0 and m["max_r2_at"].shape == (7, 1)


def test_the_defaults_and_the_limits_of_the_parameters(table_output):
    par = {ln.split()[1]: ln.split()[2:] for ln in table_output if ln.startswith("par ")}
    d = par["default"]
    assert d[0] == "0" and HEX(d[1]) == 0.02 and d[2:5] == ["50", "1000", "128"] and HEX(d[5]) == 0.3 and d[6] == str(1 << 32)
    e = par["edge"]
    assert e[0] == "0" and HEX(e[1]) == 0.0 and e[2:5] == ["1", "4096", "1"] and HEX(e[5]) == 1.0 and e[6] == "2"
    assert par["bad"] == ["-1"] * 9 + ["0"]


# ---- files -> frame ------------------------------------------------------------------------------------------------
REGION = (22, 1_000_000, 2_400_000)
SPLIT = dict(thr_r2=0.02, min_size=10, max_size=60, max_K=20, max_r2=0.9)


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    import cs_ref
    from gauss_amd import api
    files = cs_ref.study_files(tmp_path_factory.mktemp("ldsplit_study"))
    packed = os.path.join(os.path.dirname(files[2]), "panel.gpk")
    assert api.pack_panel(files[1], files[2], files[3], packed) > 0
    return dict(files=files, packed=packed)


def _same_frames(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for c in a.columns:
        assert np.array_equal(a[c].to_numpy(), b[c].to_numpy()), c
    assert a.attrs["snps"].equals(b.attrs["snps"]) and a.attrs["n_nonfinite"] == b.attrs["n_nonfinite"]
    assert np.array_equal(a.attrs["max_r2_at"], b.attrs["max_r2_at"])
    assert len(a.attrs["last"]) == len(b.attrs["last"]) and all(np.array_equal(x, y) for x, y in zip(a.attrs["last"], b.attrs["last"]))


def _check_frame(df, ld, kb, thr_r2, min_size, max_size, max_K, max_r2):
    """df against ldsplit_ref.replay on computeLD's result for the same arguments"""
    import ldsplit_ref as lr
    snp, R = ld["snplist"], ld["cormat"]
    M = len(snp)
    assert list(df.columns) == ["n_block", "cost", "perc_kept", "cost2", "max_size_used"]
    got = df.attrs["snps"]
    assert list(got.columns) == SNP_COLUMNS
    for c in ("rsid", "chr", "bp", "a1", "a2"):
        assert list(got[c]) == list(snp[c]), c
    assert np.array_equal(got["af1mix"].to_numpy(), snp["af1mix"].to_numpy())
    radius = (1 << 32) if kb is None else int(round(kb * 1000))
    want = lr.replay(R, snp["bp"].to_numpy(), radius, thr_r2, min_size, max_size, max_K, max_r2)
    ks = [K for K in range(1, max_K + 1) if want["splits"][K] is not None]
    assert list(df["n_block"]) == ks
    assert np.array_equal(df["cost"].to_numpy(), want["cost"][np.array(ks, dtype=int) - 1])
    assert np.array_equal(df.attrs["max_r2_at"], want["max_r2"]) and df.attrs["n_nonfinite"] == want["n_nonfinite"]
    for r, K in enumerate(ks):
        last = df.attrs["last"][r]
        assert np.array_equal(last, want["splits"][K] - 1)
        sizes = np.diff(np.concatenate([[-1], last]))
        assert len(sizes) == K and sizes.sum() == M and sizes.min() >= min_size and sizes.max() <= max_size
        assert df["cost2"][r] == int((sizes ** 2).sum()) and df["max_size_used"][r] == sizes.max()
        assert df["perc_kept"][r] == float((sizes ** 2).sum()) / (float(M) * float(M))
    return want, ks


def _check_blocks(df, K):
    from gauss_amd import api
    snps = df.attrs["snps"]
    bp = snps["bp"].to_numpy().astype(np.int64)
    bl = api.ldsplit_blocks(df, K)
    assert list(bl.columns) == ["block", "first_row", "last_row", "size", "first_rsid", "last_rsid", "start_bp", "end_bp"]
    assert len(bl) == K and list(bl["block"]) == list(range(1, K + 1))
    r = list(df["n_block"]).index(K)
    assert np.array_equal(bl["last_row"].to_numpy(), df.attrs["last"][r])
    # rows: no gap, no overlap, the whole region
    assert bl["first_row"][0] == 0 and bl["last_row"][K - 1] == len(snps) - 1
    assert np.array_equal(bl["first_row"].to_numpy()[1:], bl["last_row"].to_numpy()[:-1] + 1)
    assert np.array_equal(bl["size"].to_numpy(), bl["last_row"].to_numpy() - bl["first_row"].to_numpy() + 1)
    assert list(bl["first_rsid"]) == list(snps["rsid"][bl["first_row"]]) and list(bl["last_rsid"]) == list(snps["rsid"][bl["last_row"]])
    # positions: no gap, no overlap, every SNP of a block inside its range and in no other
    assert bl["start_bp"][0] == bp[0] and bl["end_bp"][K - 1] == bp[-1]
    assert np.array_equal(bl["start_bp"].to_numpy()[1:], bl["end_bp"].to_numpy()[:-1] + 1)
    for k in range(K):
        inside = np.flatnonzero((bp >= bl["start_bp"][k]) & (bp <= bl["end_bp"][k]))
        assert inside[0] == bl["first_row"][k] and inside[-1] == bl["last_row"][k]
    return bl


@pytest.mark.gpu
def test_ldsplit_end_to_end_in_both_data_layers(ctx, study, monkeypatch):
    import cs_ref
    from gauss_amd import api
    inp, idx, dat, desc = study["files"]
    kw = dict(af1_cutoff=0.02, ctx=ctx)
    ld = api.computeLD(*REGION, cs_ref.WGT, inp, idx, dat, desc, **kw)
    df = api.ldsplit(*REGION, cs_ref.WGT, inp, idx, dat, desc, **SPLIT, **kw)
    want, ks = _check_frame(df, ld, None, **SPLIT)
    M = len(ld["snplist"])
    print(f"REACHED ldsplit table: {M} SNPs, K = {ks[0]} .. {ks[-1]} feasible, cost {df['cost'].min():.4f} .. {df['cost'].max():.4f}")
    assert M > 100 and len(ks) >= 3 and len(ks) < SPLIT["max_K"]
    forms = [api.ldsplit(*REGION, cs_ref.WGT, inp, "(unused)", study["packed"], desc, **SPLIT, **kw)]
    monkeypatch.setenv("GAUSS_HOST_FULL_MAP", "1")
    forms.append(api.ldsplit(*REGION, cs_ref.WGT, inp, "(unused)", study["packed"], desc, **SPLIT, **kw))
    forms.append(api.ldsplit(*REGION, cs_ref.WGT, inp, idx, dat, desc, **SPLIT, **kw))
    monkeypatch.delenv("GAUSS_HOST_FULL_MAP")
    for other in forms:
        _same_frames(df, other)
    for K in ks:
        _check_blocks(df, K)
    with pytest.raises(Exception, match="no split into 99 blocks"):
        api.ldsplit_blocks(df, 99)
    # other parameters: a distance limit and a strict max_r2; then the defaults, under which a region of M < 2 * 50 ... SNPs is one block
    near = api.ldsplit(*REGION, cs_ref.WGT, inp, "(unused)", study["packed"], desc, thr_r2=0.05, min_size=5, max_size=40, max_K=40, max_r2=0.5, kb=100, **kw)
    _check_frame(near, ld, 100, 0.05, 5, 40, 40, 0.5)
    plain = api.ldsplit(*REGION, cs_ref.WGT, inp, idx, dat, desc, **kw)
    _check_frame(plain, ld, None, 0.02, 50, 1000, 128, 0.3)
    with pytest.raises(Exception, match="min_size = 60 is outside 1 .. max_size = 50"):
        api.ldsplit(*REGION, cs_ref.WGT, inp, idx, dat, desc, min_size=60, max_size=50, **kw)


@pytest.mark.gpu
def test_three_planted_groups_through_files_give_the_planted_blocks(ctx, tmp_path):
    """tests/test_gpu_ldsplit.py's planted region (three groups of 20, 25 and 15 SNPs; on the CPU oracle's LD the planted split is the best
    3-block split by 9.8, asserted there) written out with the synthetic panel helpers: files -> frame -> blocks"""
    from gauss_amd import api
    from gauss_amd import panel as pm
    from test_gpu_ldsplit import _planted
    G, bp, ends = _planted()
    n_snp = len(G)
    pops = [("AAA", 240, "EUR"), ("BBB", 160, "ASN")]
    af = np.stack([G[:, :240].sum(axis=1) / 480.0, G[:, 240:].sum(axis=1) / 320.0], axis=1)
    rsid, chrs = np.array([f"rs{i}" for i in range(n_snp)]), np.full(n_snp, 22)
    a1, a2 = np.full(n_snp, "A"), np.full(n_snp, "C")
    q = {k: os.path.join(str(tmp_path), k) for k in ("gwas.txt", "index.gz", "data.gz", "desc.txt")}
    pm.write_pop_desc(q["desc.txt"], pops)
    pm.write_panel_fast(q["index.gz"], q["data.gz"], rsid, chrs, bp, a1, a2, G, af, [240, 160], threads=2)
    pm.write_gwas(q["gwas.txt"], rsid, chrs, bp, a1, a2, np.random.default_rng(1).normal(size=n_snp))
    args = (22, int(bp[0]), int(bp[-1]), (["AAA", "BBB"], [0.6, 0.4]), q["gwas.txt"], q["index.gz"], q["data.gz"], q["desc.txt"])
    kw = dict(thr_r2=0.02, min_size=5, max_size=40, max_K=6, max_r2=1.0)
    df = api.ldsplit(*args, af1_cutoff=0.01, ctx=ctx, **kw)
    assert list(df.attrs["snps"]["rsid"]) == list(rsid)
    _check_frame(df, api.computeLD(*args, af1_cutoff=0.01, ctx=ctx), None, **kw)
    bl = _check_blocks(df, 3)
    assert list(bl["last_row"]) == list(ends - 1) and list(bl["size"]) == [20, 25, 15]
    assert list(bl["first_rsid"]) == ["rs0", "rs20", "rs45"] and list(bl["last_rsid"]) == ["rs19", "rs44", "rs59"]
