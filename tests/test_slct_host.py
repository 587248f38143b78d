"""CPU: the definition of the stepwise conditional signal selection -- the partial Cholesky recurrence the GPU kernel evaluates
against step-by-step conditioning with np.linalg.solve -- and the plumbing a GPU-less machine can check: the C ABI's window
descriptor and its ctypes mirror, the host entry points, the chi^2 threshold.

The two routes must select the same SNPs in the same order (asserted only after the reference's margin says no decision is within
1e-9 of a tie) and agree on every value to 1e-8 as |d| / max(1, |want|), the project's bar for solve outputs."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import desc_layout, small_panel, split_window
from loo_ref import window_b11
from slct_ref import min_var_frac, planted_z, slct_by_definition, slct_recurrence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-8
MARGIN = 1e-9
G = np.load(os.path.join(ROOT, "tests", "golden", "window_small.npz"))
CHI2_GWS = 29.716785                       # 5e-8, two-sided


def _err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), "NaNs in different places"
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok])))) if ok.any() else 0.0


def agree(B, z, K, stop, mvf, forced=(), what=""):
    a = slct_recurrence(B, z, K, stop, mvf, forced)
    b = slct_by_definition(B, z, K, stop, mvf, forced)
    e = {k: _err(a[k], b[k]) for k in ("zin", "joint", "zc", "var")} if a["n"] == b["n"] else {}
    print(f"slct {what}: n {a['n']} / {b['n']}  idx {b['idx'].tolist()}  margin {b['min_margin']:.3e}  " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert b["min_margin"] > MARGIN and a["min_margin"] > MARGIN, (what, a["min_margin"], b["min_margin"])
    assert a["n"] == b["n"] and np.array_equal(a["idx"], b["idx"]) and a["skipped"] == b["skipped"], what
    assert max(e.values()) <= TOL, (what, e)
    return b


@pytest.mark.parametrize("mode", [0, 1])
def test_recurrence_equals_definition_on_the_golden_window(mode):
    """tests/golden/window_small.npz, pooled and weighted LD: its own Z-scores at a low threshold (several SNPs enter), and with three
    planted signals at the genome-wide one."""
    B = window_b11(mode, G["gm"], G["off"], G["w"] if mode else None, 0.1)
    mvf = min_var_frac(0.9, 0.1)
    r = agree(B, G["zin"], 32, 2.0, mvf, what=f"golden mode {mode}, own z, stop 2")
    assert 1 <= r["n"] < 32
    z = planted_z(B, (5, 20, 33), (7.0, -6.5, 8.0), seed=1)
    r = agree(B, z, 32, CHI2_GWS, mvf, what=f"golden mode {mode}, planted")
    assert r["n"] >= 3 and np.all(np.isnan(r["zc"][r["idx"]])) and np.all(np.abs(r["var"][r["idx"]]) < 1e-12)


@pytest.mark.parametrize("M", [65, 300])
def test_recurrence_equals_definition_with_planted_signals(M):
    p = small_panel(n_snp=M + 40, scale=0.02, seed=11 + M)
    gm, _, _ = split_window(dict(G=p["G"][: M + 30]), M)
    for mode in (0, 1):
        B = window_b11(mode, gm, p["off"], p["w"] if mode else None, 0.1)
        z = planted_z(B, (M // 7, M // 2, M - 9), (10.0, -9.0, 9.5), seed=M + mode)
        r = agree(B, z, 32, CHI2_GWS, min_var_frac(0.9, 0.1), what=f"M={M} mode={mode} planted")
        assert 2 <= r["n"] < 32                 # (how many of the three survive conditioning is the data's business)


def test_forced_lists():
    """Forced SNPs enter first, in the caller's order, whatever their chi^2; slct_max == n_forced is a pure conditional analysis."""
    B = window_b11(0, G["gm"], G["off"], None, 0.1)
    z = planted_z(B, (5, 20, 33), (7.0, -6.5, 8.0), seed=1)
    mvf = min_var_frac(0.9, 0.1)
    r = agree(B, z, 3, CHI2_GWS, mvf, forced=(11, 2, 40), what="forced only")
    assert list(r["idx"]) == [11, 2, 40] and r["skipped"] == 0
    assert abs(r["zin"][0] - z[11] / math.sqrt(1.1)) <= 1e-12
    r = agree(B, z, 32, CHI2_GWS, mvf, forced=(11, 2), what="forced then free")
    assert list(r["idx"][:2]) == [11, 2] and r["n"] > 2
    free = agree(B, z, 32, CHI2_GWS, mvf, what="free")
    r = agree(B, z, 32, CHI2_GWS, mvf, forced=tuple(free["idx"][::-1]), what="the free choice forced in reverse order")
    assert _err(np.sort(r["joint"]), np.sort(free["joint"])) <= TOL          # the joint z does not depend on the order of entry
    assert _err(r["zc"], free["zc"]) <= TOL


def test_guard_excludes_the_twin_of_a_selected_snp_only_with_the_ridge_correction():
    """Duplicated measured rows: B_ij = 1, B_ii = 1 + lambda, so the selected twin explains 1 / (1 + lambda)^2 = 0.826 of the other.
    The guard the host passes, 1 - collin / (1 + lambda)^2, excludes it; a plain 1 - collin would not."""
    lam = 0.1
    p = small_panel(n_snp=90, scale=0.02, seed=31)
    gm, _, _ = split_window(dict(G=p["G"][:80]), 50)
    gm = np.ascontiguousarray(np.vstack([gm, gm[[7, 23]]]))                 # rows 50, 51 are twins of 7, 23
    B = window_b11(0, gm, p["off"], None, lam)
    assert B[50, 7] == 1.0 and B[51, 23] == 1.0
    z = planted_z(B, (7, 23, 40), (9.0, -8.0, 7.0), seed=3, noise=0.3)
    z[50], z[51] = z[7] - 0.01, z[23] + 0.01                               # the originals win their ties by a clear margin
    r = agree(B, z, 32, CHI2_GWS, min_var_frac(0.9, lam), what="twins, corrected guard")
    assert 7 in r["idx"] and 23 in r["idx"] and 50 not in r["idx"] and 51 not in r["idx"]
    assert np.isnan(r["zc"][50]) and np.isnan(r["zc"][51])                 # excluded, not selected
    assert abs(r["var"][50] - (1 - 1 / (1 + lam) ** 2)) < 0.05
    naive = agree(B, z, 32, CHI2_GWS, 1.0 - 0.9, what="twins, plain 1 - collin")
    assert not np.isnan(naive["zc"][50]) or 50 in naive["idx"]             # the plain test never fires on a twin
    assert naive["var"][50] > 0.1 or 50 in naive["idx"]
    # a forced twin fails the guard and is left out
    f = agree(B, z, 4, CHI2_GWS, min_var_frac(0.9, lam), forced=(7, 50, 23), what="forced twin")
    assert f["skipped"] == 1 and list(f["idx"][:2]) == [7, 23] and 50 not in f["idx"]


def test_one_and_two_snps():
    lam = 0.1
    mvf = min_var_frac(0.9, lam)
    for z0, enters in ((6.0, True), (5.0, False)):                          # 36 / 1.1 = 32.7 >= 29.7 > 25 / 1.1
        r = agree(np.array([[1 + lam]]), np.array([z0]), 32, CHI2_GWS, mvf, what=f"M=1 z={z0}")
        assert r["n"] == (1 if enters else 0)
        if enters:
            assert abs(r["zin"][0] - z0 / math.sqrt(1 + lam)) <= 1e-15 and abs(r["joint"][0] - r["zin"][0]) <= 1e-15
        else:
            assert abs(r["zc"][0] - z0 / math.sqrt(1 + lam)) <= 1e-15 and r["var"][0] == 1.0
    B = np.array([[1 + lam, 0.4], [0.4, 1 + lam]])
    r = agree(B, np.array([7.0, -6.5]), 32, CHI2_GWS, mvf, what="M=2 both")
    assert list(r["idx"]) == [0, 1]
    r = agree(B, np.array([7.0, 3.0]), 32, CHI2_GWS, mvf, what="M=2 one")
    assert list(r["idx"]) == [0] and np.isnan(r["zc"][0]) and not np.isnan(r["zc"][1])


def test_k_reached_and_nothing_selected():
    p = small_panel(n_snp=160, scale=0.02, seed=19)
    gm, _, z1 = split_window(dict(G=p["G"][:150]), 120)
    B = window_b11(1, gm, p["off"], p["w"], 0.1)
    mvf = min_var_frac(0.9, 0.1)
    r = agree(B, z1, 32, 0.05, mvf, what="K = 32 reached")
    assert r["n"] == 32
    r = agree(B, z1, 1, 0.05, mvf, what="K = 1")
    assert r["n"] == 1 and r["idx"][0] == int(np.argmax(z1 * z1 / np.diag(B)))
    r = agree(B, z1, 32, 1e3, mvf, what="nothing selected")
    assert r["n"] == 0 and r["joint"].shape == (0,) and np.array_equal(r["var"], np.ones(120))
    assert _err(r["zc"], z1 / np.sqrt(np.diag(B))) <= 1e-15


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
def _pval(chi2):
    return 2 * (0.5 * math.erfc(math.sqrt(chi2) / 1.4142135623730951))      # the library's normal tail (host_tables.cpp), same libm


@pytest.mark.parametrize("p", [5e-8, 1e-5, 0.05])
def test_chi2_threshold_round_trips_to_the_bit(p):
    """gauss_host_slct_chi2 is the smallest chi2 whose two-sided p-value is below p: the double just under it is not."""
    from gauss_amd import api
    import oracle
    c = api.slct_chi2(p)
    assert _pval(c) < p and not _pval(math.nextafter(c, 0.0)) < p
    assert abs(2 * oracle.pnorm_upper(math.sqrt(c)) - p) <= 1e-9 * p        # and the oracle's tail agrees on what that means
    assert api.slct_chi2(p) > api.slct_chi2(p * 2)                          # monotone
    if p == 5e-8:
        assert abs(c - CHI2_GWS) < 1e-5


def test_chi2_threshold_refuses_what_is_no_p_value():
    from gauss_amd import api
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(Exception, match="positive"):
            api.slct_chi2(bad)
    assert api.slct_chi2(1.5) == 0.0


def test_host_header_declares_and_api_binds_the_calls():
    from gauss_amd import api
    src = open(os.path.join(ROOT, "include", "gauss_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gauss_host_dist_slct", "gauss_host_distmix_slct", "gauss_host_slct_chi2"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in api.HOST_SYMBOLS
    assert callable(api.dist_slct) and callable(api.distmix_slct) and callable(api.slct_chi2)
    h = api.load_host()                                   # builds on a GPU-less machine too; the symbols must be exported
    assert h.gauss_host_dist_slct.argtypes[:-6] == h.gauss_host_dist.argtypes[:-1]
    assert h.gauss_host_distmix_slct.argtypes[:-6] == h.gauss_host_distmix.argtypes[:-1]


SLCT_FIELDS = ["slct_max", "slct_chi2_stop", "slct_min_var_frac", "slct_forced", "n_slct_forced", "out_slct_n", "out_slct_idx",
               "out_slct_zin", "out_slct_joint", "out_slct_zc", "out_slct_var"]


def test_window_descriptor_mirror_has_the_size_and_the_fields_of_the_header():
    from gauss_amd import _lib
    names = [f[0] for f in _lib.WindowDesc._fields_]
    assert [n for n in names if "slct" in n] == SLCT_FIELDS
    assert _lib.SLCT_MAX == 32 and _lib.ST_SLCT_SKIPPED == 8
    size, offs, (kmax, bit) = desc_layout(SLCT_FIELDS, ["GAUSS_SLCT_MAX", "GAUSS_ST_SLCT_SKIPPED"])
    assert ctypes.sizeof(_lib.WindowDesc) == size and kmax == _lib.SLCT_MAX and bit == _lib.ST_SLCT_SKIPPED
    assert [getattr(_lib.WindowDesc, n).offset for n in SLCT_FIELDS] == offs


def test_zero_initialised_descriptor_asks_for_nothing():
    from gauss_amd import _lib
    d = _lib.WindowDesc()
    assert d.slct_max == 0 and d.n_slct_forced == 0 and not d.slct_forced and not d.out_slct_n and not d.out_slct_zc


TABLE_MAIN = r'''
#include "host_internal.h"
int main() {
    const int M = 153, n = 32;
    std::vector<SlctRow> rows;
    for (int i = 0; i < M; i++) rows.push_back(SlctRow{SnpIdent{"rs1", 22, 1000 + i, "A", "G"}, 0.25, 0.5 * i, i % 2});
    std::vector<int32_t> idx(32, -1);
    for (int a = 0; a < n; a++) idx[a] = 4 * a;
    std::vector<double> zin(32, 1.5), joint(32, 2.5), zc(M, 0.5), var(M, 0.75);
    zc[8] = NAN;
    gauss_table* t = slct_output(true, rows, n, idx.data(), zin.data(), joint.data(), zc.data(), var.data());
    for (auto& c : t->cols) std::printf("%s:%zu ", c.name.c_str(), c.type == GAUSS_COL_STR ? c.s.size() : c.type == GAUSS_COL_INT ? c.i.size() : c.d.size());
    const Column &order = t->cols[8], &ze = t->cols[9], &pv = t->cols[12];
    std::printf("\n%d %d %d %g %d %d %.17g\n", order.i[0], order.i[4], order.i[1], ze.d[4], (int)std::isnan(ze.d[1]), (int)std::isnan(pv.d[8]), pv.d[0]);
    delete t;
}
'''


def test_table_builder_fills_all_fourteen_columns_under_the_address_sanitizer(tmp_path):
    """slct_output alone, as a stand-alone program built with -fsanitize=address: the widest table of the host library (14 columns)
    must fit the room gauss_table reserves for the references add() hands out."""
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
    cols, vals = out.stdout.strip().split("\n")
    want = ["rsid", "chr", "bp", "a1", "a2", "af1mix", "z", "wing", "order", "z_entry", "z_joint", "z_cond", "pval_cond", "var_left"]
    assert cols.split() == [f"{c}:153" for c in want]
    o0, o4, o1, ze4, ze1_nan, pv8_nan, pv0 = vals.split()
    assert (o0, o4, o1, ze4, ze1_nan, pv8_nan) == ("1", "2", "0", "1.5", "1", "1")
    assert abs(float(pv0) - math.erfc(0.5 / 1.4142135623730951)) <= 1e-15
