"""CPU: further traits that lack some measured SNPs -- what a GPU-less machine can check.  The rank-|D| downdate the kernels evaluate
(tests/traits_miss_ref.py) against one oracle run per trait at 1e-10, and the C ABI's new descriptor block against its ctypes mirror."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from helpers import desc_layout, small_panel, split_window
from traits_miss_ref import miss_by_oracle, miss_closed_form, random_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS_FIELDS = ["miss_more", "out_info_more", "out_z_miss", "out_info_miss"]

# (M, U, k): around the 64-row blocks of L^-1, k up to the limit of 32
SHAPES = [(12, 20, 1), (63, 65, 5), (65, 63, 32), (129, 130, 17), (300, 130, 32), (129, 65, 31)]


def _err(got, want):
    at = ~np.isnan(want)
    assert np.array_equal(at, ~np.isnan(got))
    return float(np.max(np.abs(got[at] - want[at]) / np.maximum(1.0, np.abs(want[at])))) if at.any() else 0.0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M,U,k", SHAPES)
def test_closed_form_equals_one_oracle_run_per_trait(mode, M, U, k):
    """The downdate in LAPACK on the oracle's b11 / b21 of the FULL measured set against oracle.run_impute on the measured set
    without D, the SNPs of D unmeasured: 1e-10 as |d| / max(1, |want|) for z and info of the unmeasured and of the missing SNPs.
    MakePosDef acts in no run (full set or subset), so the identity is exact."""
    p = small_panel(n_snp=M + U + 60, scale=0.02, seed=11 + M)
    gm, gu, z1 = split_window(dict(G=p["G"][: M + U]), M)
    w = p["w"] if mode else None
    Z = np.random.default_rng(M + k).standard_normal((3, M)) * 2.0
    mask = random_mask(3, M, [k, 0, max(1, k // 2)], seed=M)
    mats = oracle.run_impute(mode, gm, gu, p["off"], w, z1, want_mats=True)
    want = miss_by_oracle(mode, gm, gu, p["off"], w, Z, mask)
    assert mats["mpd"] == 0 and want["mpd"] == 0
    got = miss_closed_form(mats["b11"], mats["b21"], Z, mask)
    errs = {key: _err(got[key], want[key]) for key in ("z", "info", "z_miss", "info_miss")}
    print(f"downdate against the oracle, M={M} U={U} k={k} mode={mode}: " + "  ".join(f"{a} {b:.3e}" for a, b in errs.items()))
    assert max(errs.values()) <= 1e-10, errs
    assert _err(got["info"][1], mats["info"]) <= 1e-12                 # the trait that lacks nothing: the window's own info


def test_window_descriptor_mirror_has_the_size_and_the_fields_of_the_header():
    from gauss_amd import _lib
    names = [f[0] for f in _lib.WindowDesc._fields_]
    at = names.index("miss_more")
    assert names[at:at + 4] == MISS_FIELDS and names[at + 4] == "n_traits_more"       # the block sits in front of the traits block
    assert not any("slct" in n for n in MISS_FIELDS)
    assert _lib.TRAITS_MISS_MAX == 32 and _lib.TRAITS_MISS_UNION_MAX == 128
    size, offs, (kmax, emax) = desc_layout(MISS_FIELDS + ["n_traits_more"], ["GAUSS_TRAITS_MISS_MAX", "GAUSS_TRAITS_MISS_UNION_MAX"])
    assert ctypes.sizeof(_lib.WindowDesc) == size and (kmax, emax) == (_lib.TRAITS_MISS_MAX, _lib.TRAITS_MISS_UNION_MAX)
    assert [getattr(_lib.WindowDesc, n).offset for n in MISS_FIELDS + ["n_traits_more"]] == offs


def test_zero_initialised_descriptor_asks_for_nothing():
    from gauss_amd import _lib
    d = _lib.WindowDesc()
    assert not d.miss_more and not d.out_info_more and not d.out_z_miss and not d.out_info_miss and d.n_traits_more == 0


def test_host_header_declares_and_api_binds_the_calls():
    import re
    from gauss_amd import api
    src = open(os.path.join(ROOT, "include", "gauss_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gauss_host_dist_traits_miss", "gauss_host_distmix_traits_miss"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in api.HOST_SYMBOLS
    h = api.load_host()                                   # builds on a GPU-less machine too; the symbols must be exported
    assert h.gauss_host_dist_traits_miss.argtypes == h.gauss_host_dist_traits.argtypes
    assert h.gauss_host_distmix_traits_miss.argtypes == h.gauss_host_distmix_traits.argtypes
    import inspect
    for fn in (api.dist_traits, api.distmix_traits):
        assert inspect.signature(fn).parameters["missing"].default == "refuse"
        with pytest.raises(ValueError, match="'refuse' or 'impute'"):
            fn(22, 1, 2, 0, "EUR", ["a.txt"], "i", "d", "p", missing="drop")


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
    // rs2 swapped; rs3 listed twice (the later row wins, here the swapped one); rs4 absent (other alleles at its position do not count)
    GwasCache some = study({{"rs3", "G", "A", 22, 300, 1.5}, {"x9", "A", "C", 22, 150, 9.0}, {"rs2", "T", "C", 22, 200, 2.0}, {"rs1", "A", "G", 22, 100, -0.5},
                            {"rs3", "A", "G", 22, 300, 4.0}, {"x8", "A", "G", 21, 100, 8.0}, {"rs4", "G", "C", 22, 300, 0.25}});
    double z[4] = {7, 7, 7, 7};
    uint8_t m[4] = {9, 9, 9, 9};
    size_t lacks = 99;
    int rc = traits_match(some, "some.txt", 4, at, z, m, &lacks);
    std::printf("%d %g %g %g %g %d%d%d%d %zu\n", rc, z[0], z[1], z[2], z[3], m[0], m[1], m[2], m[3], lacks);
    GwasCache lacks3 = study({{"rs1", "A", "G", 22, 100, -0.5}, {"rs3", "G", "C", 22, 300, 1.0}, {"rs2", "C", "T", 21, 200, 1.0}});
    rc = traits_match(lacks3, "lacks.txt", 4, at, z, m, &lacks);
    std::printf("%d %g %d%d%d%d %zu\n", rc, z[0], m[0], m[1], m[2], m[3], lacks);
    rc = traits_match(lacks3, "lacks.txt", 4, at, z);                       // without a mask: refused as before
    std::printf("%d|%s\n", rc, gauss_host_last_error());
    GwasCache nan = study({{"rs1", "A", "G", 22, 100, -0.5}, {"rs2", "T", "C", 22, 200, NAN}, {"rs3", "G", "A", 22, 300, 1.0}});
    rc = traits_match(nan, "nan.txt", 4, at, z, m, &lacks);
    std::printf("%d|%s\n", rc, gauss_host_last_error());

    // the three limits: 200 measured SNPs, three files
    const size_t M = 200;
    const char* paths[3] = {"f1.txt", "f2.txt", "f3.txt"};
    std::vector<uint8_t> mask(3 * M, 0);
    for (size_t i = 0; i < 32; i++) { mask[i] = 1; mask[M + 32 + i] = 1; mask[2 * M + 64 + i] = 1; }
    std::printf("%d\n", traits_miss_limits(paths, 3, M, mask.data(), 10));      // 32 each, 96 distinct: fine
    mask[M + 150] = 1;
    rc = traits_miss_limits(paths, 3, M, mask.data(), 10);
    std::printf("%d|%s\n", rc, gauss_host_last_error());                         // f2.txt lacks 33
    mask[M + 150] = 0;
    std::vector<uint8_t> wide(5 * M, 0);
    for (int k = 0; k < 5; k++) for (size_t i = 0; i < 26; i++) wide[(size_t)k * M + 26 * k + i] = 1;      // 130 distinct, 26 each
    const char* paths5[5] = {"g1.txt", "g2.txt", "g3.txt", "g4.txt", "g5.txt"};
    rc = traits_miss_limits(paths5, 5, M, wide.data(), 10);
    std::printf("%d|%s\n", rc, gauss_host_last_error());
    std::vector<uint8_t> few(2 * 40, 0);
    for (size_t i = 0; i < 30; i++) few[40 + i] = 1;                             // the second file keeps 10 of 40
    rc = traits_miss_limits(paths, 2, 40, few.data(), 10);
    std::printf("%d|%s\n", rc, gauss_host_last_error());
    few[40] = 0;                                                                 // 11 of 40: fine
    std::printf("%d\n", traits_miss_limits(paths, 2, 40, few.data(), 10));

    // 64 traits x 153 rows: trait 1's table as dist_output lays it out; measured and unmeasured SNPs alternate, three measured and two
    // unmeasured SNPs sit in the wings (no row).  Further trait k lacks measured SNP 2 + k (a row) and, for even k, measured SNP 0 (a wing)
    const int nrow = 153, n_more = 63;
    gauss_table t;
    add_ident_columns(t, (size_t)nrow, [&](size_t i) { return SnpIdent{"rs", 22, (long long)(1000 + i), "A", "G"}; });
    Column &af = t.add("af1ref", GAUSS_COL_DBL), &zc = t.add("z", GAUSS_COL_DBL), &pv = t.add("pval", GAUSS_COL_DBL);
    Column &info = t.add("info", GAUSS_COL_DBL), &type = t.add("type", GAUSS_COL_INT);
    std::vector<int32_t> row_m = {-1, -1}, row_u = {-1};
    for (int r = 0; r < nrow; r++) {
        af.d.push_back(0.25); zc.d.push_back(0.01 * r - 0.7); pv.d.push_back(2 * pnorm_upper(fabs(zc.d.back())));
        info.d.push_back(r % 2 ? 1.0 : 0.5 + 0.001 * r); type.i.push_back(r % 2);
        (r % 2 ? row_m : row_u).push_back(r);
    }
    row_m.push_back(-1); row_u.push_back(-1);
    const size_t Mt = row_m.size(), U = row_u.size();
    std::vector<double> zm((size_t)n_more * Mt), zo((size_t)n_more * U), io((size_t)n_more * U), zmiss, imiss;
    std::vector<uint8_t> tm((size_t)n_more * Mt, 0);
    for (int k = 0; k < n_more; k++) {
        for (size_t i = 0; i < Mt; i++) zm[(size_t)k * Mt + i] = 1000.0 * (k + 1) + (double)i;
        for (size_t i = 0; i < U; i++) { zo[(size_t)k * U + i] = -(1000.0 * (k + 1) + (double)i); io[(size_t)k * U + i] = 0.25 + 0.001 * k + 1e-6 * i; }
        if (k % 2 == 0) { tm[(size_t)k * Mt] = 1; zmiss.push_back(-5.0); imiss.push_back(0.05); }
        tm[(size_t)k * Mt + 2 + k] = 1; zmiss.push_back(77.0 + k); imiss.push_back(0.125 + 0.001 * k);
    }
    const TraitsMiss miss = {tm.data(), io.data(), zmiss.data(), imiss.data()};
    traits_output(t, n_more, row_m, row_u, zm.data(), zo.data(), &miss);
    std::printf("%zu %zu", t.cols.size(), t.named.size());
    for (const NamedMat& nm : t.named) std::printf(" %s %d %d %zu", nm.name.c_str(), nm.nrow, nm.ncol, nm.d.size());
    const NamedMat &Z = t.named[0], &P = t.named[1], &I = t.named[2], &Ty = t.named[3], &N = t.named[4];
    int bad = 0;
    for (int r = 0; r < nrow; r++) {
        if (Z.d[(size_t)r] != zc.d[(size_t)r] || P.d[(size_t)r] != pv.d[(size_t)r] || I.d[(size_t)r] != info.d[(size_t)r] || Ty.d[(size_t)r] != type.i[(size_t)r]) bad++;
        for (int k = 0; k < n_more; k++) {
            // row r is measured SNP 2 + r / 2 (odd rows) or unmeasured SNP 1 + r / 2 (even rows)
            const bool lacks_it = r % 2 && 2 + r / 2 == 2 + k;
            const double want = lacks_it ? 77.0 + k : r % 2 ? 1000.0 * (k + 1) + (2 + r / 2) : -(1000.0 * (k + 1) + (1 + r / 2));
            const double want_i = lacks_it ? 0.125 + 0.001 * k : r % 2 ? 1.0 : 0.25 + 0.001 * k + 1e-6 * (1 + r / 2);
            const double want_t = lacks_it ? 0.0 : (double)(r % 2);
            const size_t o = (size_t)(1 + k) * nrow + (size_t)r;
            if (Z.d[o] != want || P.d[o] != 2 * pnorm_upper(fabs(want)) || I.d[o] != want_i || Ty.d[o] != want_t) bad++;
        }
    }
    if (N.d[0] != 0.0) bad++;
    for (int k = 0; k < n_more; k++) if (N.d[(size_t)(1 + k)] != (k % 2 == 0 ? 2.0 : 1.0)) bad++;
    std::printf(" %d\n", bad);
}
'''


def test_matcher_limits_and_table_writer_under_the_sanitizers(tmp_path):
    """traits_match with a mask, traits_miss_limits and traits_output with the missing SNPs' section, as a stand-alone program built with
    -fsanitize=address,undefined: missing SNPs become mask bits (swapped alleles and the later duplicate as before, a non-finite z that
    is present still refused, no mask: the old refusal); each of the three limits names file, count and limit; info_traits /
    type_traits / n_missing are filled for 64 traits x 153 rows with measured, unmeasured and wing SNPs."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    hdir = os.path.join(ROOT, "gauss_amd", "csrc", "host")
    src = tmp_path / "main.cpp"
    src.write_text(HOST_MAIN)
    exe = tmp_path / "traits_miss"
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + hdir, str(src),
                           os.path.join(hdir, "host_tables.cpp"), "-o", str(exe), "-Wl,--unresolved-symbols=ignore-all", "-lz", "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    some, lacks, old, nan, fine, over, wide, few, fine2, tab = out.stdout.strip().split("\n")
    assert some.split() == ["0", "-0.5", "-2", "-4", "0", "0001", "1"]
    assert lacks.split() == ["0", "-0.5", "0111", "3"]
    rc, msg = old.split("|", 1)
    assert int(rc) != 0 and "lacks.txt" in msg and "3 of the window's 4" in msg and "every trait must be measured at the SNPs of the first" in msg
    rc, msg = nan.split("|", 1)
    assert int(rc) != 0 and "nan.txt" in msg and "rs2" in msg and "not finite" in msg, msg
    assert fine == "0" and fine2 == "0"
    rc, msg = over.split("|", 1)
    assert int(rc) != 0 and "f2.txt lacks 33 of the window's 200" in msg and "at most 32" in msg, msg
    rc, msg = wide.split("|", 1)
    assert int(rc) != 0 and "130 distinct" in msg and "g5.txt" in msg and "at most 128" in msg, msg
    rc, msg = few.split("|", 1)
    assert int(rc) != 0 and "f2.txt has 10 of the window's 40" in msg and "more than 10" in msg, msg
    f = tab.split()
    assert f[:2] == ["10", "5"]
    for a, name in enumerate(("z_traits", "pval_traits", "info_traits", "type_traits")):
        assert f[2 + 4 * a: 6 + 4 * a] == [name, "153", "64", str(153 * 64)]
    assert f[18:22] == ["n_missing", "64", "1", "64"] and f[22] == "0"
