"""CPU: the plumbing of the credible sets that a GPU-less machine can check -- the C ABI's window descriptor and its ctypes mirror,
the host entry points, the hotpath's key, and CsRider's ask() / table() on a hand-made WindowView against the table builders
(a stand-alone program under the address and undefined-behaviour sanitizers; nothing is loaded into Python)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import desc_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS_FIELDS = ["cs_coverage", "cs_prior_var", "out_cs_pip", "out_cs_set", "out_cs_set_pip", "out_cs_size", "out_cs_mass", "out_cs_lse"]


def test_window_descriptor_mirror_has_the_size_and_the_fields_of_the_header():
    from gauss_amd import _lib
    names = [f[0] for f in _lib.WindowDesc._fields_]
    at = names.index("cs_coverage")
    assert names[at: at + 8] == CS_FIELDS and names[at + 8] == "slct_max" and names[at - 1] == "pop_src_off"
    assert [n for n in names if "cs_" in n] == CS_FIELDS and names[-3:] == ["out_loo_z", "out_loo_info", "out_loo_t"]
    fields = ["pop_src_off"] + CS_FIELDS + ["slct_max"]
    size, offs, _ = desc_layout(fields)
    assert ctypes.sizeof(_lib.WindowDesc) == size
    assert [getattr(_lib.WindowDesc, n).offset for n in fields] == offs
    assert offs == sorted(offs) and offs[-1] - offs[1] == 64          # eight 8-byte fields, nothing between them and slct_max


def test_zero_initialised_descriptor_asks_for_nothing():
    from gauss_amd import _lib
    d = _lib.WindowDesc()
    assert d.cs_coverage == 0.0 and d.cs_prior_var == 0.0
    assert not any((d.out_cs_pip, d.out_cs_set, d.out_cs_set_pip, d.out_cs_size, d.out_cs_mass, d.out_cs_lse))


def test_host_header_declares_and_api_binds_the_calls():
    from gauss_amd import api
    src = open(os.path.join(ROOT, "include", "gauss_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gauss_host_dist_cs", "gauss_host_distmix_cs"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in api.HOST_SYMBOLS
    assert callable(api.dist_cs) and callable(api.distmix_cs)
    h = api.load_host()                                   # builds on a GPU-less machine too; the symbols must be exported
    for cs, cond in ((h.gauss_host_dist_cs, h.gauss_host_dist_cond), (h.gauss_host_distmix_cs, h.gauss_host_distmix_cond)):
        assert cs.argtypes[:-1] == cond.argtypes[:-1] + [ctypes.c_double, ctypes.c_double] and cs.argtypes[-1] == cond.argtypes[-1]


def test_integration_snippet_compiles_against_the_header():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    subprocess.check_call([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi", "cs_snippet.cpp")])


def test_hotpath_sets_the_fields_and_both_guards():
    from gauss_amd import _lib, hotpath
    gm, gu = np.zeros((5, 8), dtype=np.uint8), np.zeros((3, 8), dtype=np.uint8)
    mk = lambda slct: (lambda d: (d, hotpath._Win(d, dict(mode=0, geno_m=gm, geno_u=gu, pop_off=[0, 8], z1=np.zeros(5), lam=0.1, slct=slct))))(_lib.WindowDesc())
    d, w = mk(dict(max=4, chi2_stop=3.0, cs=dict()))
    assert d.slct_max == 4 and d.cs_coverage == 0.95 and d.cs_prior_var == 25.0
    assert all((d.out_cs_pip, d.out_cs_set, d.out_cs_set_pip, d.out_cs_size, d.out_cs_mass, d.out_cs_lse))
    assert not d.out_cond_z and not d.out_cond_var and abs(d.cond_min_var_frac - 0.1) < 1e-15          # the guard is read, the columns are not asked
    assert abs(d.slct_min_var_frac - (1 - 0.9 / 1.21)) < 1e-15
    r = w.result()
    assert r["cs_pip"].shape == (8,) and r["cs_set"].shape == (8,) and r["cs_set"].dtype == np.int32 and r["cs_set_pip"].shape == (8,)
    assert r["cs_size"].shape == (0,) and r["cs_raw"]["size"].shape == (4,) and "cond_z" not in r
    d, w = mk(dict(max=4, chi2_stop=3.0, collin=0.8, unmeasured=True, min_var_frac_u=0.25, cs=dict(coverage=0.5, prior_var=9.0)))
    assert d.cond_min_var_frac == 0.25 and d.cs_coverage == 0.5 and d.cs_prior_var == 9.0 and d.out_cond_z
    d, w = mk(dict(max=4, chi2_stop=3.0, unmeasured=True))
    assert not d.out_cs_pip and d.cs_coverage == 0.0 and "cs_pip" not in w.result()


def test_refusals_that_need_no_gpu(tmp_path):
    """A missing file is named before anything else happens, as by the *_cond calls."""
    import types
    from gauss_amd import api
    missing = str(tmp_path / "nothing.txt")
    fake = types.SimpleNamespace(handle=ctypes.c_void_p(1))      # never dereferenced: the files are looked at first
    with pytest.raises(Exception, match="nothing.txt"):
        api.dist_cs(22, 1, 2, 1, "EUR", missing, missing, missing, missing, ctx=fake)
    with pytest.raises(Exception, match="nothing.txt"):
        api.distmix_cs(22, 1, 2, 1, (["a"], [1.0]), missing, missing, missing, missing, coverage=0.9, prior_var=4.0, ctx=fake)


RIDER_MAIN = r'''
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
// the call's own table of the made-up window: 6 rows of the prediction window (measured 1, 3, 4 -> rows 0, 2, 5; unmeasured 0, 1, 2 ->
// rows 1, 3, 4); measured 0 and 2 lie in the wings and are not listed
static int plain(gauss_table** out) {
    gauss_table* t = new gauss_table();
    const char* ids[6] = {"m1", "u0", "m3", "u1", "u2", "m4"};
    add_ident_columns(*t, 6, [&](size_t i) { return SnpIdent{ids[i], 22, 2000 + (long long)i, "A", "G"}; });
    Column &af = t->add("af1mix", GAUSS_COL_DBL), &z = t->add("z", GAUSS_COL_DBL), &pv = t->add("pval", GAUSS_COL_DBL);
    Column &info = t->add("info", GAUSS_COL_DBL), &type = t->add("type", GAUSS_COL_INT);
    for (int i = 0; i < 6; i++) { af.d.push_back(0.1 * i); z.d.push_back(1.0 + i); pv.d.push_back(0.5 / (1 + i)); info.d.push_back(0.9 - 0.1 * i); type.i.push_back(ids[i][0] == 'm'); }
    *out = t;
    return 0;
}
int main() {
    const char* mid[5] = {"m0", "m1", "m2", "m3", "m4"};
    const int wing[5] = {1, 0, 1, 0, 0};
    WindowView v;
    v.mix = true;
    std::vector<SlctRow> rows;
    for (int i = 0; i < 5; i++) {
        const SnpIdent id{mid[i], 22, 1000 + i, "C", "T"};
        v.measured.push_back(ViewSnp{id, 0.25 + i, 0.5 * i - 1, wing[i]});
        rows.push_back(SlctRow{id, 0.25 + i, 0.5 * i - 1, wing[i]});
    }
    v.row_m = {-1, 0, -1, 2, 5}; v.row_u = {1, 3, 4};
    v.plain = plain;
    const int32_t idx[4] = {2, 3, -1, -1};                  // a wing SNP first, then measured 3
    const std::vector<double> zin = {7.5, -6.5, NAN, NAN}, joint = {7.25, -6.25, NAN, NAN};
    const std::vector<double> zc = {0.5, 0.25, NAN, NAN, 2.0}, var = {0.75, 0.5, 0.0, 0.0, 0.875};
    const std::vector<double> cz = {1.5, NAN, -2.5}, cv = {0.625, 0.05, 0.375};
    // candidates: measured 0 .. 4, then unmeasured 0 .. 2.  Set 0 (lead: measured 2, a wing SNP) holds measured 2 and unmeasured 0;
    // set 1 (lead: measured 3) holds unmeasured 2 and measured 3 and 4
    const std::vector<double> pip = {0.0, 0.015625, 0.75, 0.25, 0.125, 0.25, 0.0, 0.5};
    const std::vector<int32_t> set = {-1, -1, 0, 1, 1, 0, -1, 1};
    const std::vector<double> set_pip = {0.0, 0.0, 0.75, 0.25, 0.125, 0.25, 0.0, 0.5};
    const std::vector<int32_t> size = {2, 3, 0, 0};
    const std::vector<double> mass = {1.0, 0.875, NAN, NAN}, lse = {40.5, 31.25, NAN, NAN};
    for (int pass = 0; pass < 2; pass++) {
        const char* cond[2] = {"m3", "m0"};
        CsRider r(0.0, 0.0, 4, cond, 2, pass ? 0.5 : 0.0, pass ? 4.0 : NAN);
        gauss_window_desc d;
        memset(&d, 0, sizeof(d));
        d.n_measured = 5; d.n_unmeasured = 3; d.lambda = 0.1;
        const int rc = r.check() || r.ask(d, v);
        std::printf("cs%d ask %d %d %d %zu %zu %zu %zu %d %d %d %a %a %a %a\n", pass, rc, d.slct_max, d.n_slct_forced, r.pip.size(), r.set.size(), r.size.size(),
                    r.cond_z.size(), d.out_cs_pip == r.pip.data() && d.out_cs_set == r.set.data() && d.out_cs_set_pip == r.set_pip.data(),
                    d.out_cs_size == r.size.data() && d.out_cs_mass == r.mass.data() && d.out_cs_lse == r.lse.data(),
                    d.out_cond_z == r.cond_z.data() && d.out_slct_n == &r.n, d.cs_coverage, d.cs_prior_var, d.slct_min_var_frac, d.cond_min_var_frac);
        if (pass) continue;
        r.n = 2; r.idx.assign(idx, idx + 4); r.zin = zin; r.joint = joint; r.zc = zc; r.var = var; r.cond_z = cz; r.cond_var = cv;
        r.pip = pip; r.set = set; r.set_pip = set_pip; r.size = size; r.mass = mass; r.lse = lse;
        gauss_table *got = nullptr, *want = nullptr;
        if (r.table(v, &got)) return 1;
        plain(&want);
        if (cond_output(*want, rows, v.row_m, v.row_u, 2, idx, zin.data(), joint.data(), zc.data(), var.data(), cz.data(), cv.data())) return 1;
        if (cs_output(*want, rows, v.row_m, v.row_u, 2, idx, pip.data(), set.data(), set_pip.data(), size.data(), mass.data(), lse.data())) return 1;
        dump("cs.got", *got); dump("cs.want", *want);
        gauss_table_free(got); gauss_table_free(want);
    }
    // a table that is not the conditional one of the window is refused and left as it came
    gauss_table* t2 = nullptr;
    plain(&t2);
    const int rc = cs_output(*t2, rows, v.row_m, v.row_u, 2, idx, pip.data(), set.data(), set_pip.data(), size.data(), mass.data(), lse.data());
    std::printf("refused %d %zu %zu %s\n", rc, t2->cols.size(), t2->named.size(), gauss_host_last_error());
    gauss_table_free(t2);
    {   // the selection's refusals are the rider's
        const char* twice[2] = {"m1", "m1"};
        gauss_window_desc d;
        memset(&d, 0, sizeof(d));
        d.n_measured = 5; d.n_unmeasured = 3;
        CsRider a(0.0, 0.0, 4, twice, 2, 0.0, 0.0);
        std::printf("refused %d", a.ask(d, v)); std::printf(" %s %d\n", gauss_host_last_error(), d.out_cs_pip == nullptr);
    }
}
'''


@pytest.fixture(scope="module")
def rider_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("cs_rider")
    hdir = os.path.join(ROOT, "gauss_amd", "csrc", "host")
    src = tmp / "main.cpp"
    src.write_text(RIDER_MAIN)
    exe = tmp / "rider"
    flags = [gxx, "-std=c++17", "-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + hdir]
    srcs = [str(src), os.path.join(hdir, "host_riders.cpp"), os.path.join(hdir, "host_tables.cpp")]
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
        assert key not in body
        body[key] = vals
    return names, body, mine


HEX = float.fromhex


def test_the_rider_builds_the_table_its_builders_give_for_the_same_rows(rider_output):
    """CsRider::table() on fixed result arrays against cond_output + cs_output called on rows written out by hand: the same columns,
    rows and named matrices to the bit -- and what they are: dist_cond's 15 columns and rows, then pip cs cs_pip (18 columns, beyond
    the 16 a table reserves by default: the builder asks for its room), cs in the numbering of `order`, `sets` beside `signals`."""
    got, want = _table(rider_output, "cs.got"), _table(rider_output, "cs.want")
    assert got[2] == want[2]
    names, t, _ = got
    assert names == ["rsid", "chr", "bp", "a1", "a2", "af1mix", "z", "pval", "info", "type", "wing", "order", "z_cond", "pval_cond", "var_left",
                     "pip", "cs", "cs_pip"]
    assert t["rsid"] == ["m1", "u0", "m3", "u1", "u2", "m4", "m0", "m2"]                      # the call's rows, then the wings in matrix order
    assert t["order"] == ["0", "0", "2", "0", "0", "0", "0", "1"]
    assert t["cs"] == ["0", "1", "2", "0", "2", "2", "0", "1"]                                # a set carries its lead's `order`
    assert [HEX(x) for x in t["pip"]] == [0.015625, 0.25, 0.25, 0.0, 0.5, 0.125, 0.0, 0.75]
    assert [HEX(x) for x in t["cs_pip"]] == [0.0, 0.25, 0.25, 0.0, 0.5, 0.125, 0.0, 0.75]
    assert [HEX(x) for x in t["var_left"]] == [0.5, 0.625, 0.0, 0.05, 0.375, 0.875, 0.75, 0.0]          # dist_cond's columns are untouched
    assert t["named signals"][:2] == ["2", "3"] and [HEX(x) for x in t["named signals"][2:4]] == [7.0, 2.0]
    # sets [2 x 4], column-major: table row of the lead (the wing SNP m2 sits in row 7), size, mass, lse
    assert t["named sets"][:2] == ["2", "4"] and [HEX(x) for x in t["named sets"][2:]] == [7.0, 2.0, 2.0, 3.0, 1.0, 0.875, 40.5, 31.25]


def test_ask_sets_the_descriptor_and_the_defaults(rider_output):
    tok = [ln for ln in rider_output if ln.startswith("cs0 ask")][0].split()[2:]
    # rc, slct_max, forced, buffer sizes (pip / set: M + U; size: slct_max; cond_z: U), the pointers are the rider's, the defaults
    assert tok[:10] == ["0", "4", "2", "8", "8", "4", "3", "1", "1", "1"]
    assert HEX(tok[10]) == 0.95 and HEX(tok[11]) == 25.0                  # coverage 0 and prior_var NaN: the defaults
    assert HEX(tok[12]) == 1.0 - 0.9 / ((1.0 + 0.1) * (1.0 + 0.1)) and HEX(tok[13]) == 1.0 - 0.9
    tok = [ln for ln in rider_output if ln.startswith("cs1 ask")][0].split()[2:]
    assert tok[0] == "0" and HEX(tok[10]) == 0.5 and HEX(tok[11]) == 4.0
    refused = [ln for ln in rider_output if ln.startswith("refused")]
    assert refused[0].split()[1:4] == ["-1", "10", "0"] and "not the conditional one" in refused[0]
    assert refused[1].split()[1] == "-1" and "cond_rsids: m1 is listed twice" in refused[1] and refused[1].split()[-1] == "1"
