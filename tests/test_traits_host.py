"""CPU: further traits on one window's LD -- what a GPU-less machine can check.  The C ABI's window descriptor and its ctypes mirror,
the two host entry points, the study matcher and the table writer as a stand-alone program under the address / undefined-behaviour
sanitizers, and the identity the kernels evaluate (G = B^-1 Z, B21 G / sqrt(info)) against one oracle run per trait at 1e-10."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from helpers import desc_layout, small_panel, split_window
from traits_ref import traits_by_oracle, traits_closed_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAITS_FIELDS = ["n_traits_more", "z_more", "out_z_more"]


def test_window_descriptor_mirror_has_the_size_and_the_fields_of_the_header():
    from gauss_amd import _lib
    names = [f[0] for f in _lib.WindowDesc._fields_]
    at = names.index("n_traits_more")
    assert names[at:at + 3] == TRAITS_FIELDS and names[at + 3:] == ["out_loo_z", "out_loo_info", "out_loo_t"]
    assert not any("slct" in n for n in TRAITS_FIELDS)
    assert _lib.TRAITS_MORE_MAX == 63
    size, offs, (tmax,) = desc_layout(TRAITS_FIELDS, ["GAUSS_TRAITS_MORE_MAX"])
    assert ctypes.sizeof(_lib.WindowDesc) == size and tmax == _lib.TRAITS_MORE_MAX
    assert [getattr(_lib.WindowDesc, n).offset for n in TRAITS_FIELDS] == offs


def test_zero_initialised_descriptor_asks_for_nothing():
    from gauss_amd import _lib
    d = _lib.WindowDesc()
    assert d.n_traits_more == 0 and not d.z_more and not d.out_z_more


def test_host_header_declares_and_api_binds_the_calls():
    from gauss_amd import api
    src = open(os.path.join(ROOT, "include", "gauss_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gauss_host_dist_traits", "gauss_host_distmix_traits"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in api.HOST_SYMBOLS
    assert callable(api.dist_traits) and callable(api.distmix_traits)
    h = api.load_host()                                   # builds on a GPU-less machine too; the symbols must be exported
    tail = [ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    assert h.gauss_host_dist_traits.argtypes[:-3] == h.gauss_host_dist.argtypes[:-1]
    assert h.gauss_host_distmix_traits.argtypes[:-3] == h.gauss_host_distmix.argtypes[:-1]
    for f, plain in ((h.gauss_host_dist_traits, h.gauss_host_dist), (h.gauss_host_distmix_traits, h.gauss_host_distmix)):
        assert f.argtypes[-3:-1] == tail and f.argtypes[-1] == plain.argtypes[-1]


HOST_MAIN = r'''
#include "host_internal.h"
extern "C" const char* gauss_host_last_error();
static GwasCache study(const std::vector<GwasRow>& rows)
{
    GwasCache c;
    c.rows = rows;
    c.by_pos.resize(rows.size());
    for (size_t i = 0; i < rows.size(); i++) c.by_pos[i] = (uint32_t)i;
    std::stable_sort(c.by_pos.begin(), c.by_pos.end(), [&](uint32_t x, uint32_t y) {
        const GwasRow &a = c.rows[x], &b = c.rows[y];
        return a.chr < b.chr || (a.chr == b.chr && a.bp < b.bp);
    });
    return c;
}
int main() {
    // the window's measured SNPs, panel orientation
    const SnpIdent win[4] = {{"rs1", 22, 100, "A", "G"}, {"rs2", 22, 200, "C", "T"}, {"rs3", 22, 300, "G", "A"}, {"rs4", 22, 300, "G", "T"}};
    auto at = [&](size_t i) { return win[i]; };
    // file order is not position order; rs2 swapped; rs3 listed twice (the later row wins, here the swapped one); rows of other SNPs
    // (another position, another chromosome, other alleles at a window position) are ignored
    GwasCache ok = study({{"rs3", "G", "A", 22, 300, 1.5}, {"x9", "A", "C", 22, 150, 9.0}, {"rs2", "T", "C", 22, 200, 2.0}, {"rs1", "A", "G", 22, 100, -0.5},
                          {"rs3", "A", "G", 22, 300, 4.0}, {"x8", "A", "G", 21, 100, 8.0}, {"rs4", "G", "T", 22, 300, 0.25}, {"x7", "C", "G", 22, 100, 7.0}});
    double z[4] = {0, 0, 0, 0};
    int rc = traits_match(ok, "ok.txt", 4, at, z);
    std::printf("%d %g %g %g %g\n", rc, z[0], z[1], z[2], z[3]);
    GwasCache lacks = study({{"rs1", "A", "G", 22, 100, -0.5}, {"rs3", "G", "C", 22, 300, 1.0}, {"rs2", "C", "T", 21, 200, 1.0}});
    rc = traits_match(lacks, "lacks.txt", 4, at, z);
    std::printf("%d|%s\n", rc, gauss_host_last_error());
    GwasCache nan = study({{"rs1", "A", "G", 22, 100, -0.5}, {"rs2", "T", "C", 22, 200, NAN}, {"rs3", "G", "A", 22, 300, 1.0}, {"rs4", "G", "T", 22, 300, INFINITY}});
    rc = traits_match(nan, "nan.txt", 4, at, z);
    std::printf("%d|%s\n", rc, gauss_host_last_error());

    // 64 traits x 153 rows: trait 1's table as dist_output lays it out, 63 further traits; measured and unmeasured SNPs alternate, three
    // measured and two unmeasured SNPs sit in the wings (no row)
    const int nrow = 153, n_more = 63;
    gauss_table t;
    add_ident_columns(t, (size_t)nrow, [&](size_t i) { return SnpIdent{"rs", 22, (long long)(1000 + i), "A", "G"}; });
    Column &af = t.add("af1ref", GAUSS_COL_DBL), &zc = t.add("z", GAUSS_COL_DBL), &pv = t.add("pval", GAUSS_COL_DBL);
    Column &info = t.add("info", GAUSS_COL_DBL), &type = t.add("type", GAUSS_COL_INT);
    std::vector<int32_t> row_m = {-1, -1}, row_u = {-1};
    for (int r = 0; r < nrow; r++) {
        af.d.push_back(0.25); zc.d.push_back(0.01 * r - 0.7); pv.d.push_back(2 * pnorm_upper(fabs(zc.d.back()))); info.d.push_back(0.5); type.i.push_back(r % 2);
        (r % 2 ? row_m : row_u).push_back(r);
    }
    row_m.push_back(-1); row_u.push_back(-1);
    const size_t M = row_m.size(), U = row_u.size();
    std::vector<double> zm((size_t)n_more * M), zo((size_t)n_more * U);
    for (int k = 0; k < n_more; k++) {
        for (size_t i = 0; i < M; i++) zm[(size_t)k * M + i] = 1000.0 * (k + 1) + (double)i;
        for (size_t i = 0; i < U; i++) zo[(size_t)k * U + i] = -(1000.0 * (k + 1) + (double)i);
    }
    traits_output(t, n_more, row_m, row_u, zm.data(), zo.data());
    std::printf("%zu %zu", t.cols.size(), t.named.size());
    for (const NamedMat& nm : t.named) std::printf(" %s %d %d %zu", nm.name.c_str(), nm.nrow, nm.ncol, nm.d.size());
    const NamedMat &Z = t.named[0], &P = t.named[1];
    int bad = 0;
    for (int r = 0; r < nrow; r++) {
        if (Z.d[(size_t)r] != zc.d[(size_t)r] || P.d[(size_t)r] != pv.d[(size_t)r]) bad++;
        for (int k = 0; k < n_more; k++) {
            // row r is measured SNP 2 + r / 2 (odd rows) or unmeasured SNP 1 + r / 2 (even rows)
            const double want = r % 2 ? 1000.0 * (k + 1) + (2 + r / 2) : -(1000.0 * (k + 1) + (1 + r / 2));
            const size_t o = (size_t)(1 + k) * nrow + (size_t)r;
            if (Z.d[o] != want || P.d[o] != 2 * pnorm_upper(fabs(want))) bad++;
        }
    }
    std::printf(" %d %.17g\n", bad, P.d[0]);
}
'''


def test_matcher_and_table_writer_under_the_sanitizers(tmp_path):
    """traits_match and traits_output alone, as a stand-alone program built with -fsanitize=address,undefined: swapped alleles flip
    the sign, the later duplicate wins, rows of other SNPs are ignored, a missing SNP and a non-finite z are refused with the file,
    the rsid and the count; 64 traits x 153 rows fill z_traits / pval_traits, column 0 the frame's own columns."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    hdir = os.path.join(ROOT, "gauss_amd", "csrc", "host")
    src = tmp_path / "main.cpp"
    src.write_text(HOST_MAIN)
    exe = tmp_path / "traits"
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + hdir, str(src),
                           os.path.join(hdir, "host_tables.cpp"), "-o", str(exe), "-Wl,--unresolved-symbols=ignore-all", "-lz", "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    ok, lacks, nan, tab = out.stdout.strip().split("\n")
    assert ok.split() == ["0", "-0.5", "-2", "-4", "0.25"]
    rc, msg = lacks.split("|", 1)
    assert int(rc) != 0 and "lacks.txt" in msg and "rs2" in msg and "3 of the window's 4" in msg, msg
    rc, msg = nan.split("|", 1)
    assert int(rc) != 0 and "nan.txt" in msg and "rs2" in msg and "not finite" in msg, msg
    f = tab.split()
    assert f[:2] == ["10", "2"] and f[2:6] == ["z_traits", "153", "64", str(153 * 64)] and f[6:10] == ["pval_traits", "153", "64", str(153 * 64)]
    assert f[10] == "0"
    assert abs(float(f[11]) - math.erfc(0.7 / math.sqrt(2))) <= 1e-15


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M", [40, 300])
def test_closed_form_equals_one_oracle_run_per_trait(mode, M):
    """The identity the kernels evaluate, in LAPACK on the oracle's own b11 / b21, against oracle.run_impute called once per trait
    with z1 = z_t (pooled and weighted LD): 1e-10 as |d| / max(1, |want|)."""
    p = small_panel(n_snp=M + 90, scale=0.02, seed=11 + M)
    gm, gu, z1 = split_window(dict(G=p["G"][: M + 60]), M)
    w = p["w"] if mode else None
    T = 5 if M > 100 else 17
    Z = np.random.default_rng(M).standard_normal((T, M)) * 2.0
    Z[0] = z1
    mats = oracle.run_impute(mode, gm, gu, p["off"], w, z1, want_mats=True)
    want = traits_by_oracle(mode, gm, gu, p["off"], w, Z)
    assert mats["mpd"] == 0 and want["mpd"] == 0
    got = traits_closed_form(mats["b11"], mats["b21"], Z)
    e = float(np.max(np.abs(got["z"] - want["z"]) / np.maximum(1.0, np.abs(want["z"]))))
    ei = float(np.max(np.abs(got["info"] - want["info"]) / want["info"]))
    print(f"closed form against the oracle, M={M} mode={mode}: z {e:.3e}  info rel {ei:.3e}")
    assert e <= 1e-10 and ei <= 1e-10
    assert np.array_equal(want["z"][0], mats["z"])
