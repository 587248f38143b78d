"""The host layer of the LD scores.  CPU: what a GPU-less machine can check -- the window descriptor and its ctypes mirror, the host
entry points and their binding, the hotpath's key, the refusals that come before any GPU work (a missing file, a window with no target,
a window of more targets or rows than one call takes), and ldscore_output / kish_n_eff on
hand-made rows (a stand-alone program under the address and undefined-behaviour sanitizers; nothing is loaded into Python).
GPU: dist_ldscore / distmix_ldscore, files -> table, on the text panel, the packed panel and the packed panel through the full SNP map,
against the window oracle/feeder_py.py builds from the same files and tests/ldscore_ref.py on the oracle's LD of its rows."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import desc_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_FIELDS = ["lds_on", "lds_n_annot", "lds_radius", "lds_bp_m", "lds_bp_u", "lds_n", "lds_annot", "out_lds_raw", "out_lds_l2", "out_lds_mass"]


def test_window_descriptor_mirror_has_the_size_and_the_fields_of_the_header():
    from gauss_amd import _lib
    names = [f[0] for f in _lib.WindowDesc._fields_]
    at = names.index("lds_on")
    assert names[at: at + 10] == LDS_FIELDS and names[at - 1] == "out_status" and names[at + 10] == "out_b11"      # in front of the matrices
    assert [n for n in names if "lds_" in n] == LDS_FIELDS and names[-3:] == ["out_loo_z", "out_loo_info", "out_loo_t"]
    fields = ["out_status"] + LDS_FIELDS + ["out_b11"]
    size, offs, _ = desc_layout(fields)
    assert ctypes.sizeof(_lib.WindowDesc) == size
    assert [getattr(_lib.WindowDesc, n).offset for n in fields] == offs
    # lds_on and lds_n_annot share a word: 1 + 1 + 8 words from out_status to out_b11
    assert offs == sorted(offs) and offs[2] - offs[1] == 4 and offs[-1] - offs[0] == 8 * (1 + 1 + 8)
    hdr = open(os.path.join(ROOT, "include", "gauss_hip.h")).read()
    assert re.search(r"#define\s+GAUSS_LDS_MAX_ANNOT\s+%d\b" % _lib.LDS_MAX_ANNOT, hdr) and _lib.LDS_MAX_ANNOT == 32
    assert re.search(r"#define\s+GAUSS_LDS_CHUNK\s+%d\b" % _lib.LDS_CHUNK, hdr)
    import ldscore_ref
    assert ldscore_ref.CHUNK == _lib.LDS_CHUNK


def test_zero_initialised_descriptor_asks_for_nothing():
    from gauss_amd import _lib
    d = _lib.WindowDesc()
    assert d.lds_on == 0 and d.lds_n_annot == 0 and d.lds_radius == 0 and d.lds_n == 0.0
    assert not any(getattr(d, n) for n in LDS_FIELDS if n.startswith("out_") or n in ("lds_bp_m", "lds_bp_u", "lds_annot"))


def test_host_header_declares_and_api_binds_the_calls():
    from gauss_amd import api
    src = open(os.path.join(ROOT, "include", "gauss_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gauss_host_dist_ldscore", "gauss_host_distmix_ldscore"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in api.HOST_SYMBOLS
    assert re.search(r"#define\s+GAUSS_KIND_LDSCORE\s+11\b", src) and re.search(r"#define\s+GAUSS_KIND_LDSCOREMIX\s+12\b", src)
    assert callable(api.dist_ldscore) and callable(api.distmix_ldscore)
    h = api.load_host()                                   # builds on a GPU-less machine too; the symbols must be exported
    for fn, plain in ((h.gauss_host_dist_ldscore, h.gauss_host_dist), (h.gauss_host_distmix_ldscore, h.gauss_host_distmix)):
        assert fn.argtypes[:-1] == plain.argtypes[:-1] + [ctypes.c_double] and fn.argtypes[-1] == plain.argtypes[-1]


def test_hotpath_sets_the_fields():
    from gauss_amd import _lib, hotpath
    gm, gu = np.zeros((5, 8), dtype=np.uint8), np.zeros((3, 8), dtype=np.uint8)
    mk = lambda q, **kw: (lambda d: (d, hotpath._Win(d, dict(mode=0, geno_m=gm, geno_u=gu, pop_off=[0, 8], z1=np.zeros(5), lam=0.0, ldscore=q, **kw))))(_lib.WindowDesc())
    bm, bu = [1, 2, 3, 5, 8], [2, 4, 9]
    d, w = mk(dict(radius=3, bp_m=bm, bp_u=bu, n=100))
    assert (d.kind, d.u_codings, d.lds_on, d.lds_n_annot, d.lds_radius, d.lds_n) == (_lib.WIN_LD, 1, 1, 0, 3, 100.0)
    assert [d.lds_bp_m[k] for k in range(5)] == bm and [d.lds_bp_u[k] for k in range(3)] == bu and not d.lds_annot
    assert d.out_lds_raw and d.out_lds_l2 and d.out_lds_mass and d.out_b11 and d.out_b21 and not d.prs_n_s
    r = w.result()
    assert all(r[k].shape == (1, 5) for k in ("lds_raw", "lds_l2", "lds_mass")) and r["b11"].shape == (5, 5) and r["b21"].shape == (3, 5)
    annot = np.arange(16.0).reshape(2, 8)
    d, w = mk(dict(radius=2 ** 40, bp_m=bm, bp_u=bu, n=50.5, annot=annot), want_matrices=False)
    assert (d.lds_n_annot, d.lds_radius, d.lds_n) == (2, 2 ** 40, 50.5) and [d.lds_annot[k] for k in range(16)] == list(range(16))
    assert not d.out_b11 and not d.out_b21
    r = w.result()
    assert r["b11"] is None and r["b21"] is None and r["lds_raw"].shape == (3, 5)
    d, w = mk(None)
    assert d.lds_on == 0 and not d.out_lds_raw and "lds_raw" not in w.result() and d.kind == _lib.WIN_IMPUTE


def test_no_matrices_is_for_a_window_that_asks():
    """want_matrices=False without ldscore= would run an LD window that returns nothing: the Python layer refuses it"""
    from gauss_amd import _lib, hotpath
    gm, gu = np.zeros((5, 8), dtype=np.uint8), np.zeros((3, 8), dtype=np.uint8)
    with pytest.raises(ValueError, match="want_matrices=False is for an LD window that asks"):
        hotpath._Win(_lib.WindowDesc(), dict(mode=0, geno_m=gm, geno_u=gu, pop_off=[0, 8], z1=np.zeros(5), lam=0.0, ld_codings=1, want_matrices=False), True)
    with pytest.raises(ValueError, match="want_matrices=False is for an LD window that asks"):
        hotpath.ld_window(0, gm, gu, [0, 8], None, ctx=object(), want_matrices=False)


def test_refusals_that_need_no_gpu(tmp_path):
    """A missing file is named before anything else happens, as by the other one-window calls."""
    import types
    from gauss_amd import api
    missing = str(tmp_path / "nothing.txt")
    fake = types.SimpleNamespace(handle=ctypes.c_void_p(1))      # never dereferenced: the files are looked at first
    with pytest.raises(Exception, match="nothing.txt"):
        api.dist_ldscore(22, 1, 2, 1, "EUR", missing, missing, missing, missing, ctx=fake)
    with pytest.raises(Exception, match="nothing.txt"):
        api.distmix_ldscore(22, 1, 2, 1, (["a"], [1.0]), missing, missing, missing, missing, n=500, ctx=fake)


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
    for (auto& m : t.messages) std::printf("%s message %s\n", what, m.c_str());
}
int main() {
    const char* id[3] = {"t0", "t1", "t2"};
    std::vector<LdsRow> rows;
    for (int i = 0; i < 3; i++) rows.push_back(LdsRow{SnpIdent{id[i], 22, 1000 + 10 * i, "C", "T"}, 0.25 + 0.125 * i});
    const double l2[3] = {1.5, 2.25, 3.0}, raw[3] = {1.75, 2.5, 3.125}, mass[3] = {4.0, 5.0, 5.0};
    gauss_table* t = ldscore_output(true, rows, l2, raw, mass, 321.5, 9, 7, 300000);
    dump("mix", *t);
    gauss_table_free(t);
    const double bad[3] = {1.75, NAN, 3.125};
    t = ldscore_output(false, rows, bad, bad, mass, 100.0, 9, 7, 0);
    dump("pop", *t);
    gauss_table_free(t);
    const double w[4] = {0.5, 0.0, 0.25, 0.311};
    const int32_t off[5] = {0, 100, 150, 350, 390};
    std::printf("kish %a %a\n", kish_n_eff(w, off, 4), kish_n_eff(w, off, 1));
}
'''


@pytest.fixture(scope="module")
def table_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("ldscore_table")
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


def test_the_table_has_one_row_per_target_and_the_four_numbers(table_output):
    names, t = _table(table_output, "mix")
    assert names == ["rsid", "chr", "bp", "a1", "a2", "af1mix", "l2", "l2_raw", "n_band"]
    assert t["rsid"] == ["t0", "t1", "t2"] and t["bp"] == ["1000", "1010", "1020"] and t["n_band"] == ["4", "5", "5"]
    assert [HEX(x) for x in t["l2"]] == [1.5, 2.25, 3.0] and [HEX(x) for x in t["l2_raw"]] == [1.75, 2.5, 3.125]
    assert [HEX(x) for x in t["af1mix"]] == [0.25, 0.375, 0.5]
    assert t["named ldscore"][:2] == ["1", "4"] and [HEX(x) for x in t["named ldscore"][2:]] == [321.5, 9.0, 7.0, 300000.0]
    assert "message" not in t
    names, t = _table(table_output, "pop")
    assert names[5] == "af1ref" and np.isnan(HEX(t["l2_raw"][1])) and "no variance" in " ".join(t["message"])


def test_kish_effective_size(table_output):
    """(sum w)^2 / sum (w^2 / n) over the populations of non-zero weight, the weights as passed; one population: its own size"""
    got = [HEX(x) for x in [ln for ln in table_output if ln.startswith("kish")][0].split()[1:]]
    w, n = np.array([0.5, 0.25, 0.311]), np.array([100.0, 200.0, 40.0])
    assert abs(got[0] - w.sum() ** 2 / np.sum(w * w / n)) <= 1e-12 * got[0] and abs(got[1] - 100.0) <= 1e-10


# ---- files -> table ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def study(tmp_path_factory):
    import cs_ref
    from gauss_amd import api
    files = cs_ref.study_files(tmp_path_factory.mktemp("ldscore_study"))
    packed = os.path.join(os.path.dirname(files[2]), "panel.gpk")
    assert api.pack_panel(files[1], files[2], files[3], packed) > 0
    return dict(files=files, packed=packed)


@pytest.mark.parametrize("mix", [False, True])
def test_a_window_without_a_target_is_refused_before_any_gpu_work(study, mix, monkeypatch):
    """Both data layers build the window on the host: one that holds panel SNPs and none of the study's is refused with a message"""
    import types
    import cs_ref
    from gauss_amd import api
    fake = types.SimpleNamespace(handle=ctypes.c_void_p(1))      # never dereferenced: the window is refused first
    inp, idx, dat, desc = study["files"]
    empty = os.path.join(os.path.dirname(inp), "empty_study.txt")
    with open(inp) as f, open(empty, "w") as g:
        g.write(f.readline())
        g.write("rs_nowhere 22 999 A C 1.0\n")
    fn, who = (api.distmix_ldscore, cs_ref.WGT) if mix else (api.dist_ldscore, "EUR")
    for full_map in ("0", "1"):
        monkeypatch.setenv("GAUSS_HOST_FULL_MAP", full_map)
        with pytest.raises(Exception, match="no SNP to score"):
            fn(*cs_ref.STUDY_WINDOW, who, empty, "(unused)", study["packed"], desc, ctx=fake)


def _flat_study(d, n_snp, n_study, prefix):
    """A panel of n_snp SNPs 100 bp apart from 1 000 000 on, 16 samples in two populations, every SNP polymorphic in both, and a study
    file that lists the first n_study of them: (gwas, index, data, description, packed)"""
    from gauss_amd import api
    from gauss_amd import panel as pm
    rng = np.random.default_rng(n_snp)
    pops = [("AAA", 10, "EUR"), ("BBB", 6, "ASN")]
    G = rng.integers(0, 3, size=(n_snp, 16), dtype=np.uint8)
    G[:, [0, 10]], G[:, [1, 11]] = 0, 2
    af = np.stack([G[:, :10].sum(axis=1) / 20.0, G[:, 10:].sum(axis=1) / 12.0], axis=1)
    rsid, chrs, bp = np.array([f"rs{i}" for i in range(n_snp)]), np.full(n_snp, 22), 1_000_000 + 100 * np.arange(n_snp)
    a1, a2 = np.full(n_snp, "A"), np.full(n_snp, "C")
    q = {k: os.path.join(str(d), f"{prefix}_{k}") for k in ("gwas.txt", "index.gz", "data.gz", "desc.txt", "panel.gpk")}
    pm.write_pop_desc(q["desc.txt"], pops)
    pm.write_panel_fast(q["index.gz"], q["data.gz"], rsid, chrs, bp, a1, a2, G, af, [10, 6], threads=2)
    k = n_study
    pm.write_gwas(q["gwas.txt"], rsid[:k], chrs[:k], bp[:k], a1[:k], a2[:k], np.zeros(k))
    assert api.pack_panel(q["index.gz"], q["data.gz"], q["desc.txt"], q["panel.gpk"]) == n_snp
    return tuple(q.values())


@pytest.mark.parametrize("n_snp,n_study,start_bp,what", [(8200, 8200, 1_000_000, "8200 SNPs to score and 8200 panel SNPs"),
                                                         (131_100, 3, 1_000_000, "3 SNPs to score and 131100 panel SNPs")],
                         ids=["targets", "rows"])
def test_a_window_beyond_what_one_job_admits_is_refused_before_any_gpu_work(tmp_path, n_snp, n_study, start_bp, what, monkeypatch):
    """More than GAUSS_HOST_LDSCORE_MAX_TARGETS (8 192) SNPs to score, or more than GAUSS_HOST_LDSCORE_MAX_ROWS (131 072) panel SNPs in
    the extended window: dist and distmix, the text panel and the packed panel in both data layers, say to shorten the window"""
    import types
    from gauss_amd import api
    hdr = open(os.path.join(ROOT, "include", "gauss_host.h")).read()
    assert re.search(r"#define\s+GAUSS_HOST_LDSCORE_MAX_TARGETS\s+8192\b", hdr) and re.search(r"#define\s+GAUSS_HOST_LDSCORE_MAX_ROWS\s+131072\b", hdr)
    fake = types.SimpleNamespace(handle=ctypes.c_void_p(1))      # never dereferenced: the window is refused first
    gwas, idx, dat, desc, packed = _flat_study(tmp_path, n_snp, n_study, "flat")
    win = (22, start_bp, start_bp + 100 * n_study - 1, 100 * n_snp)
    text = "the window has " + what + " in all; one call takes at most 8192 and 131072: shorten the window"
    for fn, who in ((api.dist_ldscore, "EUR"), (api.distmix_ldscore, (["AAA", "BBB"], [0.6, 0.4]))):
        for full_map, files in (("0", ("(unused)", packed)), ("1", ("(unused)", packed)), ("0", (idx, dat))):
            monkeypatch.setenv("GAUSS_HOST_FULL_MAP", full_map)
            with pytest.raises(Exception) as e:
                fn(*win, who, gwas, *files, desc, af1_cutoff=0.01, ctx=fake)
            assert text in str(e.value), (fn.__name__, full_map, files, str(e.value))


def _window(mix, files):
    """The window as the host layer must build it, from oracle/feeder_py.py's reading of the files: the targets are the study's SNPs
    that the panel has inside [start_bp, end_bp]; every other SNP of the extended window's vector is a reference row"""
    import cs_ref
    from oracle import feeder_py as fp
    chr_, start_bp, end_bp, wing = cs_ref.STUDY_WINDOW
    who, cutoff = (cs_ref.WGT, 0.02) if mix else ("EUR", 0.01)
    inp, index, data, desc = files
    pops = fp.read_ref_desc(desc)
    flags, w = fp.pop_flags_wgt(pops, *who) if mix else (fp.pop_flags(pops, who), None)
    lo, hi = start_bp - wing, end_bp + wing
    m = fp.read_input_z(inp, chr_, lo, hi, False)
    fp.read_reference_index(m, index, chr_, lo, hi, False)
    vec = [s for s in fp.make_snp_vec(m, data, flags, cutoff, w) if s.type in (0, 1)]
    tgt = [s for s in vec if s.type == 1 and start_bp <= s.bp <= end_bp]
    ref = [s for s in vec if not (s.type == 1 and start_bp <= s.bp <= end_bp)]
    sizes = [p[1] for p, f in zip(pops, flags) if f]
    return dict(tgt=tgt, ref=ref, gm=fp._matrix(tgt), gu=fp._matrix(ref), off=fp._selected_off(pops, flags), sizes=sizes,
                w=None if w is None else np.asarray(w, dtype=np.float64), who=who, cutoff=cutoff)


@pytest.mark.gpu
@pytest.mark.parametrize("mix", [False, True])
def test_dist_ldscore_and_distmix_ldscore_end_to_end(ctx, study, mix, monkeypatch):
    import cs_ref
    import ldscore_ref as lr
    import oracle
    from gauss_amd import api
    win = cs_ref.STUDY_WINDOW
    chr_, start_bp, end_bp, wing = win
    fw = _window(mix, study["files"])
    tgt, ref = fw["tgt"], fw["ref"]
    fn = api.distmix_ldscore if mix else api.dist_ldscore
    inp, idx, dat, desc = study["files"]
    kw = dict(af1_cutoff=fw["cutoff"], ctx=ctx)
    df = fn(*win, fw["who"], inp, idx, dat, desc, **kw)
    afcol = "af1mix" if mix else "af1ref"
    assert list(df.columns) == ["rsid", "chr", "bp", "a1", "a2", afcol, "l2", "l2_raw", "n_band"]
    # the targets are exactly the study's SNPs that the panel has inside [start_bp, end_bp] ...
    assert list(df["rsid"]) == [s.rsid for s in tgt] and list(df["bp"]) == [s.bp for s in tgt] and len(tgt) > 20
    assert list(df["a1"]) == [s.a1 for s in tgt] and np.all((df["bp"] >= start_bp) & (df["bp"] <= end_bp))
    assert np.allclose(df[afcol].to_numpy(), np.array([s.af1mix if mix else s.af1ref for s in tgt]), rtol=1e-12, atol=0)
    # ... and a wing's SNP that the study measured is a reference row
    wing_measured = [s for s in ref if s.type == 1]
    assert wing_measured and all(s.bp < start_bp or s.bp > end_bp for s in wing_measured) and any(s.type == 0 for s in ref)
    bm, bu = np.array([s.bp for s in tgt]), np.array([s.bp for s in ref])
    # n_eff: the selected samples, or Kish's size of the weights as passed
    if mix:
        w, n = fw["w"], np.asarray(fw["sizes"], dtype=np.float64)
        keep = w != 0
        n_eff = w[keep].sum() ** 2 / np.sum(w[keep] ** 2 / n[keep])
        assert abs(df.attrs["n_eff"] - n_eff) <= 1e-12 * n_eff
    else:
        n_eff = float(sum(fw["sizes"]))
        assert df.attrs["n_eff"] == n_eff
    af_all = np.array([s.af1mix if mix else s.af1ref for s in tgt + ref])
    assert df.attrs["M"] == len(tgt) + len(ref) and df.attrs["M_5_50"] == int(np.sum(np.minimum(af_all, 1 - af_all) > 0.05))
    assert df.attrs["radius"] == wing and df.attrs["M_5_50"] < df.attrs["M"]
    # l2_raw against the numpy statement on the oracle's LD of the same rows
    cpu = oracle.ld_blocks(1 if mix else 0, fw["gm"], fw["gu"], fw["off"], fw["w"], 1.0, (0,))
    want = lr.plain(cpu["b11"], cpu["b21"], bm, bu, wing, df.attrs["n_eff"])
    cnt = lr.count(bm, bu, wing)
    gap = np.abs(df["l2_raw"].to_numpy() - want["raw"][0])
    print(f"REACHED ldscore table mix={mix}: targets {len(tgt)} rows {len(tgt) + len(ref)} n_eff {df.attrs['n_eff']:.3f}  "
          f"l2_raw against the oracle's LD {float(gap.max()):.2e} (bound {4e-12 * float(cnt.max()):.2e})")
    assert np.all(gap <= 4e-12 * cnt) and np.array_equal(df["n_band"].to_numpy(), cnt.astype(np.int64))
    nm2 = df.attrs["n_eff"] - 2.0
    raw, band = df["l2_raw"].to_numpy(), df["n_band"].to_numpy().astype(np.float64)
    assert np.array_equal(df["l2"].to_numpy(), raw * (1.0 + 1.0 / nm2) - band / nm2)
    assert 1 < cnt.min() and cnt.max() < len(tgt) + len(ref)               # the band cuts: no target sees the whole window
    # n= overrides the sample size, and only that
    other = fn(*win, fw["who"], inp, idx, dat, desc, n=1234.5, **kw)
    assert other.attrs["n_eff"] == 1234.5 and np.array_equal(other["l2_raw"].to_numpy(), raw)
    assert np.array_equal(other["l2"].to_numpy(), raw * (1.0 + 1.0 / 1232.5) - band / 1232.5)
    # both data layers, text and packed: the same table bit for bit
    forms = [fn(*win, fw["who"], inp, "(unused)", study["packed"], desc, **kw)]
    monkeypatch.setenv("GAUSS_HOST_FULL_MAP", "1")
    forms.append(fn(*win, fw["who"], inp, "(unused)", study["packed"], desc, **kw))
    forms.append(fn(*win, fw["who"], inp, idx, dat, desc, **kw))
    for other in forms:
        assert list(other.columns) == list(df.columns) and len(other) == len(df) and other.attrs == df.attrs
        for c in df.columns:
            if df[c].dtype.kind == "f":
                assert np.array_equal(df[c].to_numpy(), other[c].to_numpy(), equal_nan=True), c
            else:
                assert list(df[c]) == list(other[c]), c
    monkeypatch.delenv("GAUSS_HOST_FULL_MAP")
    # a sample size the window refuses
    with pytest.raises(Exception, match="lds_n = "):
        fn(*win, fw["who"], inp, idx, dat, desc, n=1.5, **kw)
