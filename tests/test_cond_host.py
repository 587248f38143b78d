"""CPU: the definition of the imputed SNPs conditioned on the selected signals -- three routes with no shared arithmetic
(tests/cond_ref.py) -- and the plumbing a GPU-less machine can check: the C ABI's window descriptor and its ctypes mirror, the host
entry points, the table builder.

The routes agree to 1e-10 as |d| / max(1, |want|), the bound tests/test_traits_miss_host.py holds a closed form to against the
oracle; where cond_z is NaN is compared only after every route's margin says that no imputed SNP sits within 1e-9 of its guard."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cond_ref import cond_by_augmented, cond_by_definition, cond_by_residual, window_mats
from helpers import desc_layout, small_panel, split_window
from slct_ref import min_var_frac, planted_z, slct_by_definition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
MARGIN = 1e-9
CHI2_GWS = 29.716785                       # 5e-8, two-sided


def _err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), "NaNs in different places"
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok])))) if ok.any() else 0.0


def agree(B, B21, z, S, mvf_u=0.1, what="", impute=None):
    a = cond_by_definition(B, B21, z, S, mvf_u)
    b = cond_by_residual(B, B21, z, S, mvf_u, impute=impute)
    c = cond_by_augmented(B, B21, z, S, mvf_u)
    assert min(a["margin"], b["margin"], c["margin"]) > MARGIN, (what, a["margin"], b["margin"], c["margin"])
    e = dict(res_z=_err(b["z"], a["z"]), res_var=_err(b["var"], a["var"]), aug_z=_err(c["z"], a["z"]), aug_var=_err(c["var"], a["var"]))
    print(f"cond {what}: n {len(S)}  U {len(a['z'])}  NaN {int(np.isnan(a['z']).sum())}  margin {a['margin']:.3e}  "
          + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= TOL, (what, e)
    return a


def _window(M, mode, U=40, lam=0.1):
    p = small_panel(n_snp=M + U + 20, scale=0.02, seed=11 + M)
    gm, gu, z1 = split_window(dict(G=p["G"][: M + U]), M)
    B, B21 = window_mats(mode, gm, gu, p["off"], p["w"] if mode else None, lam)
    return p, gm, gu, z1, B, B21


@pytest.mark.parametrize("M", [2, 65, 300])
@pytest.mark.parametrize("mode", [0, 1])
def test_three_routes_agree(M, mode):
    """Pooled and weighted LD; the set the selection finds at the genome-wide threshold on planted signals, the 32 SNPs of a run
    that never stops, one SNP, and nothing selected."""
    p, gm, gu, z1, B, B21 = _window(M, mode)
    z = planted_z(B, (M // 7, M // 2, M - 1), (10.0, -9.0, 9.5), seed=M + mode) if M > 2 else np.array([7.0, 3.0])
    mvf = min_var_frac(0.9, 0.1)
    sel = slct_by_definition(B, z, 32, CHI2_GWS, mvf)
    assert sel["n"] >= 1
    a = agree(B, B21, z, sel["idx"], what=f"M={M} mode={mode} selected")
    assert a["var"].min() >= -1e-12 and a["var"].max() <= 1 + 1e-12
    if M > 2:
        assert np.isfinite(a["z"]).any()
        many = slct_by_definition(B, z, 32, 0.0, mvf)
        assert many["n"] == 32
        agree(B, B21, z, many["idx"], what=f"M={M} mode={mode} 32 selected")
    agree(B, B21, z, sel["idx"][:1], what=f"M={M} mode={mode} one")
    none = agree(B, B21, z, [], what=f"M={M} mode={mode} none")
    assert np.array_equal(none["var"], np.ones(B21.shape[0]))


def test_three_routes_agree_on_a_repaired_matrix():
    """Duplicated measured rows at lambda = 0: MakePosDef rebuilds B11; the identities hold on the repaired matrix as long as the
    same B is used throughout."""
    from oracle import oracle_np
    p = small_panel(n_snp=70, scale=0.02, n_pops=6, seed=21)
    gm, gu, _ = split_window(p, 30)
    gm = np.ascontiguousarray(np.vstack([gm, gm[:3]]))
    B0, B21 = window_mats(0, gm, gu, p["off"], None, 0.0)
    B, acted = oracle_np.make_pos_def(B0, 1e-5)
    assert acted
    z = planted_z(B, (4, 15, 24), (8.0, -7.0, 7.5), seed=2)
    sel = slct_by_definition(B, z, 32, 4.0, min_var_frac(0.9, 0.0))
    assert sel["n"] >= 2 and sel["min_margin"] > MARGIN
    agree(B, B21, z, sel["idx"], what="repaired matrix")


def test_the_oracle_as_the_imputer_of_the_residual():
    """cond_by_residual with run_dist itself imputing the residual: the route the GPU test takes."""
    import oracle
    p, gm, gu, z1, B, B21 = _window(65, 0)
    z = planted_z(B, (9, 32, 64), (10.0, -9.0, 9.5), seed=5)
    sel = slct_by_definition(B, z, 32, CHI2_GWS, min_var_frac(0.9, 0.1))

    def impute(r):
        q = oracle.run_impute(0, gm, gu, p["off"], None, r)
        return q["z"] * np.sqrt(q["info"]), q["info"]

    agree(B, B21, z, sel["idx"], what="oracle imputes the residual", impute=impute)


def test_unmeasured_twin_of_an_isolated_selected_snp_has_nothing_left():
    """The ridge does not cap the explained share of an imputed SNP: the duplicate of the only measured SNP has info = 1 / (1 + lambda)
    and the selected SNP explains all of it -- while the measured twin of a selected SNP keeps 1 - 1 / (1 + lambda)^2."""
    lam = 0.1
    B, B21 = np.array([[1 + lam]]), np.array([[1.0], [0.4]])
    a = cond_by_definition(B, B21, np.array([6.0]), [0], 1 - 0.9)
    assert abs(a["var"][0]) < 1e-15 and np.isnan(a["z"][0])
    assert abs(a["var"][1]) < 1e-15                        # one measured SNP explains all an imputed SNP has: info = b^2 / (1 + lambda)


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
COND_FIELDS = ["cond_min_var_frac", "out_cond_z", "out_cond_var"]


def test_window_descriptor_mirror_has_the_size_and_the_fields_of_the_header():
    from gauss_amd import _lib
    names = [f[0] for f in _lib.WindowDesc._fields_]
    at = names.index("out_slct_var")
    assert names[at + 1: at + 4] == COND_FIELDS and names[at + 4] == "miss_more"
    assert [n for n in names if "cond" in n] == COND_FIELDS and not any("slct" in n for n in COND_FIELDS)
    fields = ["out_slct_var"] + COND_FIELDS + ["miss_more"]
    size, offs, _ = desc_layout(fields)
    assert ctypes.sizeof(_lib.WindowDesc) == size
    assert [getattr(_lib.WindowDesc, n).offset for n in fields] == offs
    assert offs == sorted(offs) and offs[4] - offs[1] == 24          # three 8-byte fields, nothing between them and miss_more


def test_zero_initialised_descriptor_asks_for_nothing():
    from gauss_amd import _lib
    d = _lib.WindowDesc()
    assert d.cond_min_var_frac == 0.0 and not d.out_cond_z and not d.out_cond_var


def test_host_header_declares_and_api_binds_the_calls():
    from gauss_amd import api
    src = open(os.path.join(ROOT, "include", "gauss_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gauss_host_dist_cond", "gauss_host_distmix_cond"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in api.HOST_SYMBOLS
    assert callable(api.dist_cond) and callable(api.distmix_cond)
    h = api.load_host()                                   # builds on a GPU-less machine too; the symbols must be exported
    assert h.gauss_host_dist_cond.argtypes == h.gauss_host_dist_slct.argtypes
    assert h.gauss_host_distmix_cond.argtypes == h.gauss_host_distmix_slct.argtypes


def test_integration_snippet_compiles_against_the_header():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    subprocess.check_call([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi", "cond_snippet.cpp")])


def test_hotpath_sets_the_fields_and_the_guard_without_the_ridge_correction():
    from gauss_amd import _lib, hotpath
    gm, gu = np.zeros((5, 8), dtype=np.uint8), np.zeros((3, 8), dtype=np.uint8)
    mk = lambda slct: (lambda d: (d, hotpath._Win(d, dict(mode=0, geno_m=gm, geno_u=gu, pop_off=[0, 8], z1=np.zeros(5), lam=0.1, slct=slct))))(_lib.WindowDesc())
    d, w = mk(dict(max=4, chi2_stop=3.0, unmeasured=True))
    assert d.slct_max == 4 and d.out_cond_z and d.out_cond_var and abs(d.cond_min_var_frac - 0.1) < 1e-15
    assert abs(d.slct_min_var_frac - (1 - 0.9 / 1.21)) < 1e-15
    r = w.result()
    assert r["cond_z"].shape == (3,) and r["cond_var"].shape == (3,)
    d, w = mk(dict(max=4, chi2_stop=3.0, collin=0.8, unmeasured=True, min_var_frac_u=0.25))
    assert d.cond_min_var_frac == 0.25
    d, w = mk(dict(max=4, chi2_stop=3.0))
    assert not d.out_cond_z and not d.out_cond_var and "cond_z" not in w.result()


def test_refusals_that_need_no_gpu(tmp_path):
    """A missing file is named before anything else happens, as by the *_slct calls."""
    import types
    from gauss_amd import api
    missing = str(tmp_path / "nothing.txt")
    fake = types.SimpleNamespace(handle=ctypes.c_void_p(1))      # never dereferenced: the files are looked at first
    with pytest.raises(Exception, match="nothing.txt"):
        api.dist_cond(22, 1, 2, 1, "EUR", missing, missing, missing, missing, ctx=fake)
    with pytest.raises(Exception, match="nothing.txt"):
        api.distmix_cond(22, 1, 2, 1, (["a"], [1.0]), missing, missing, missing, missing, ctx=fake)


TABLE_MAIN = r'''
#include "host_internal.h"
// a made-up window: 6 table rows of the prediction window (measured 1, 3, 4 -> rows 0, 2, 5; unmeasured 0, 1, 2 -> rows 1, 3, 4), and two
// measured SNPs in the wings (measured 0 and 2), which the builder appends
int main() {
    gauss_table* t = new gauss_table();
    std::vector<SlctRow> win;
    const char* ids[6] = {"m1", "u0", "m3", "u1", "u2", "m4"};
    add_ident_columns(*t, 6, [&](size_t i) { return SnpIdent{ids[i], 22, 2000 + (long long)i, "A", "G"}; });
    Column &af = t->add("af1ref", GAUSS_COL_DBL), &z = t->add("z", GAUSS_COL_DBL), &pv = t->add("pval", GAUSS_COL_DBL);
    Column &info = t->add("info", GAUSS_COL_DBL), &type = t->add("type", GAUSS_COL_INT);
    for (int i = 0; i < 6; i++) { af.d.push_back(0.1 * i); z.d.push_back(1.0 + i); pv.d.push_back(0.5); info.d.push_back(0.9); type.i.push_back(ids[i][0] == 'm'); }
    std::vector<SlctRow> rows;
    const char* mid[5] = {"m0", "m1", "m2", "m3", "m4"};
    const int wing[5] = {1, 0, 1, 0, 0};
    for (int i = 0; i < 5; i++) rows.push_back(SlctRow{SnpIdent{mid[i], 22, 1000 + i, "C", "T"}, 0.25 + i, 0.5 * i, wing[i]});
    const std::vector<int32_t> row_m = {-1, 0, -1, 2, 5}, row_u = {1, 3, 4};
    const int n = 2;
    const int32_t idx[32] = {2, 3};                       // a wing SNP first, then measured 3
    std::vector<double> zin(32, NAN), joint(32, NAN), zc = {0.5, 0.25, NAN, NAN, 2.0}, var = {0.75, 0.5, 0.0, 0.0, 0.875};
    zin[0] = 7.5; zin[1] = -6.5; joint[0] = 7.25; joint[1] = -6.25;
    const std::vector<double> cz = {1.5, NAN, -2.5}, cv = {0.625, 0.05, 0.375};
    cond_output(*t, rows, row_m, row_u, n, idx, zin.data(), joint.data(), zc.data(), var.data(), cz.data(), cv.data());
    for (auto& c : t->cols) std::printf("%s:%zu ", c.name.c_str(), c.type == GAUSS_COL_STR ? c.s.size() : c.type == GAUSS_COL_INT ? c.i.size() : c.d.size());
    std::printf("\n");
    for (int r = 0; r < 8; r++)
        std::printf("%s %d %g %g %g %d %d %d %.17g %.17g %g\n", t->cols[0].s[r].c_str(), t->cols[2].i[r], t->cols[6].d[r], t->cols[8].d[r], t->cols[5].d[r],
                    t->cols[9].i[r], t->cols[10].i[r], t->cols[11].i[r], t->cols[12].d[r], t->cols[13].d[r], t->cols[14].d[r]);
    const NamedMat& s = t->named[0];
    std::printf("%s %d %d", s.name.c_str(), s.nrow, s.ncol);
    for (double v : s.d) std::printf(" %g", v);
    std::printf("\n");
    delete t;
    // a table with a column the builder has no value for in a wing row: refused with a message, the table left as it came
    gauss_table* t2 = new gauss_table();
    add_ident_columns(*t2, 1, [&](size_t) { return SnpIdent{"m1", 22, 2000, "A", "G"}; });
    t2->add("z", GAUSS_COL_DBL).d.push_back(1.0);
    t2->add("extra", GAUSS_COL_DBL).d.push_back(2.0);
    const std::vector<int32_t> rm2 = {-1, 0, -1, -1, -1}, ru2 = {-1, -1, -1};
    const int rc = cond_output(*t2, rows, rm2, ru2, n, idx, zin.data(), joint.data(), zc.data(), var.data(), cz.data(), cv.data());
    std::printf("refused %d %zu %d %zu %s\n", rc, t2->cols.size(), t2->nrow(), t2->named.size(), gauss_host_last_error());
    // and one column more than the reserved room is refused instead of moving the columns under the references add() gave out
    bool caught = false;
    try { for (int k = 0; k < 10; k++) t2->add("more", GAUSS_COL_INT); } catch (const std::length_error&) { caught = true; }
    std::printf("full %d %zu\n", (int)caught, t2->cols.size());
    delete t2;
}
'''


def test_table_builder_under_the_address_sanitizer(tmp_path):
    """cond_output alone, as a stand-alone program built with -fsanitize=address: dist()'s rows stay as they are, the wings'
    measured SNPs follow in matrix order, the five columns are appended (15 in all: within the room gauss_table reserves), imputed
    rows carry the conditional statistics, and `signals` lists the selected SNPs with their table rows.  A table with a column the
    builder does not know is refused and left as it came; a 17th column is refused by gauss_table::add."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    hdir = os.path.join(ROOT, "gauss_amd", "csrc", "host")
    src = tmp_path / "main.cpp"
    src.write_text(TABLE_MAIN)
    exe = tmp_path / "tab"
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address", "-I" + hdir, str(src), os.path.join(hdir, "host_tables.cpp"),
                           "-o", str(exe), "-Wl,--unresolved-symbols=ignore-all", "-lz", "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    want = ["rsid", "chr", "bp", "a1", "a2", "af1ref", "z", "pval", "info", "type", "wing", "order", "z_cond", "pval_cond", "var_left"]
    assert lines[0].split() == [f"{c}:8" for c in want]
    rows = [ln.split() for ln in lines[1:9]]
    assert [r[0] for r in rows] == ["m1", "u0", "m3", "u1", "u2", "m4", "m0", "m2"]          # dist()'s rows, then the wings in matrix order
    assert [int(r[1]) for r in rows] == [2000, 2001, 2002, 2003, 2004, 2005, 1000, 1002]
    assert [float(r[2]) for r in rows[:6]] == [1, 2, 3, 4, 5, 6] and [float(r[2]) for r in rows[6:]] == [0.0, 1.0]      # z: untouched / the study's
    assert [float(r[3]) for r in rows[6:]] == [1.0, 1.0] and [float(r[4]) for r in rows[6:]] == [0.25, 2.25]          # info 1, af
    assert [int(r[5]) for r in rows] == [1, 0, 1, 0, 0, 1, 1, 1]                                # type: the wings' SNPs are measured
    assert [int(r[6]) for r in rows] == [0, 0, 0, 0, 0, 0, 1, 1]                                # wing
    assert [int(r[7]) for r in rows] == [0, 0, 2, 0, 0, 0, 0, 1]                                # order
    zc = [float(r[8]) for r in rows]
    assert zc[0] == 0.25 and zc[1] == 1.5 and math.isnan(zc[2]) and math.isnan(zc[3]) and zc[4] == -2.5 and zc[5] == 2.0 and zc[6] == 0.5 and math.isnan(zc[7])
    pv = [float(r[9]) for r in rows]
    for a, b in zip(zc, pv):
        assert (math.isnan(a) and math.isnan(b)) or abs(b - math.erfc(abs(a) / 1.4142135623730951)) <= 1e-15
    assert [float(r[10]) for r in rows] == [0.5, 0.625, 0.0, 0.05, 0.375, 0.875, 0.75, 0.0]     # var_left
    assert lines[9].split() == ["signals", "2", "3", "7", "2", "7.5", "-6.5", "7.25", "-6.25"]
    assert lines[10].split()[:5] == ["refused", "-1", "7", "1", "0"] and "'extra'" in lines[10]
    assert lines[11].split() == ["full", "1", "16"]
