"""CPU: the plumbing of the joint fine-mapping across studies that a GPU-less machine can check -- the C ABI's window descriptor and its
ctypes mirror, the host entry points, the hotpath's keys and maps, and the map builder and the table builder on hand-made arrays (a
stand-alone program under the address and undefined-behaviour sanitizers; nothing is loaded into Python)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import desc_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XS_FIELDS = ["xs_group", "xs_from_lead", "out_xs_V", "out_xs_purity", "out_xs_mu", "out_xs_n"]


def test_window_descriptor_mirror_has_the_size_and_the_fields_of_the_header():
    from gauss_amd import _lib
    names = [f[0] for f in _lib.WindowDesc._fields_]
    at = names.index("xs_group")
    assert names[at: at + 6] == XS_FIELDS and names[at - 1] == "out_b21" and names[at + 6] == "kind"      # in front of the QCAT block
    assert [n for n in names if "xs_" in n] == XS_FIELDS
    fields = ["out_b21"] + XS_FIELDS + ["kind"]
    size, offs, _ = desc_layout(fields)
    assert ctypes.sizeof(_lib.WindowDesc) == size
    assert [getattr(_lib.WindowDesc, n).offset for n in fields] == offs
    # xs_group has a word of its own (padded), then five 8-byte fields, then kind
    assert offs == sorted(offs) and offs[1] - offs[0] == 8 and offs[-1] - offs[1] == 8 + 5 * 8


def test_zero_initialised_descriptor_asks_for_nothing():
    from gauss_amd import _lib
    d = _lib.WindowDesc()
    assert d.xs_group == 0 and not any(getattr(d, n) for n in XS_FIELDS[1:])


def test_host_header_declares_and_api_binds_the_calls():
    from gauss_amd import api
    src = open(os.path.join(ROOT, "include", "gauss_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gauss_host_dist_xsusie", "gauss_host_distmix_xsusie"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in api.HOST_SYMBOLS
    assert callable(api.dist_xsusie) and callable(api.distmix_xsusie)
    h = api.load_host()                                   # builds on a GPU-less machine too; the symbols must be exported
    assert h.gauss_host_dist_xsusie.argtypes[-9:] == h.gauss_host_dist_susie.argtypes[-9:]
    assert h.gauss_host_distmix_xsusie.argtypes[-9:] == h.gauss_host_distmix_susie.argtypes[-9:]
    hdr = open(os.path.join(ROOT, "include", "gauss_hip.h")).read()
    assert re.search(r"#define\s+GAUSS_XS_MAX\s+4\b", hdr)


def test_integration_snippet_compiles_against_the_header():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    subprocess.check_call([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi", "xsusie_snippet.cpp")])


def test_hotpath_sets_the_fields_and_builds_the_maps():
    from gauss_amd import _lib, hotpath
    gm, gu = np.zeros((5, 8), dtype=np.uint8), np.zeros((3, 8), dtype=np.uint8)
    mk = lambda susie, xs=None: (lambda d: (d, hotpath._Win(d, dict(mode=0, geno_m=gm, geno_u=gu, pop_off=[0, 8], z1=np.zeros(5), lam=0.1, susie=susie), xs=xs)))(_lib.WindowDesc())
    d, w = mk(dict(L=3, group=2, want_mu=True), xs=("leader", 3))
    assert d.xs_group == 2 and d.susie_L == 3 and d.out_susie_pip and d.out_xs_V and d.out_xs_purity and d.out_xs_mu and d.out_xs_n and not d.xs_from_lead
    r = w.result()
    assert r["xs_V"].shape == (3, 3) and r["xs_mu"].shape == (3, 3, 8) and r["xs_n"] == 0 and "susie_pip" in r
    d, w = mk(dict(L=3, group=2, from_lead=[0, 1, -1, 7, 2, 3, 4, 5], tol=0.0, max_sweeps=9, measured_only=True), xs=("peer", 3))
    assert d.xs_group == 2 and d.susie_L == 3 and d.susie_max_sweeps == 9 and d.susie_tol == 0.0 and d.susie_measured_only == 1
    assert d.xs_from_lead and [d.xs_from_lead[j] for j in range(8)] == [0, 1, -1, 7, 2, 3, 4, 5]
    assert not d.out_susie_pip and not d.out_xs_V and "susie_pip" not in w.result() and "xs_V" not in w.result()
    d, w = mk(dict(L=3))
    assert d.xs_group == 0 and "xs_V" not in w.result()
    m = hotpath.xs_maps([10, 11, 12, 13, 99], [13, 7, 10, 12])
    assert m.dtype == np.int32 and m.tolist() == [2, -1, 3, 0, -1]
    with pytest.raises(ValueError, match="twice"):
        hotpath.xs_maps([1, 2], [3, 3])
    with pytest.raises(ValueError, match="2 .. 4 studies"):
        hotpath.fine_map_studies([dict()])


def test_refusals_that_need_no_gpu(tmp_path):
    """A missing file is named before anything else happens, as by the other one-window calls; so is a group of one"""
    import types
    from gauss_amd import api
    missing = str(tmp_path / "nothing.txt")
    fake = types.SimpleNamespace(handle=ctypes.c_void_p(1))      # never dereferenced: the files are looked at first
    with pytest.raises(Exception, match="nothing.txt"):
        api.dist_xsusie(22, 1, 2, 1, ["EUR", "ASN"], [missing, missing], missing, missing, missing, ctx=fake)
    with pytest.raises(Exception, match="nothing.txt"):
        api.distmix_xsusie(22, 1, 2, 1, [(["a"], [1.0]), (["a"], [0.5])], [missing, missing], missing, missing, missing, L=3, ctx=fake)
    with pytest.raises(Exception, match="n_studies = 1: the joint fit takes 2 .. 4 studies"):
        api.dist_xsusie(22, 1, 2, 1, ["EUR"], [missing], missing, missing, missing, ctx=fake)
    with pytest.raises(ValueError, match="same populations"):
        api.distmix_xsusie(22, 1, 2, 1, [(["a"], [1.0]), (["b"], [0.5])], [missing, missing], missing, missing, missing, ctx=fake)


XS_MAIN = r'''
#include "host_internal.h"
static void dump(const char* what, const gauss_table& t) {
    std::printf("%s cols", what);
    for (auto& c : t.cols) std::printf(" %s", c.name.c_str());
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
// the made-up window of tests/test_susie_host.py: 6 rows of the prediction window (measured 1, 3, 4 -> rows 0, 2, 5; unmeasured 0, 1, 2 ->
// rows 1, 3, 4); measured 0 and 2 lie in the wings
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
    // the map builder: the leader's eight candidates against a peer of six in another order that lacks two of them and has one of its own
    const int64_t lead[8] = {100, 101, 102, 103, 104, 200, 201, 202}, peer[6] = {201, 103, 100, 777, 104, 202};
    int32_t from[8];
    const int n = xs_build_map(lead, 8, peer, 6, from);
    std::printf("map %d", n);
    for (int j = 0; j < 8; j++) std::printf(" %d", from[j]);
    std::printf("\n");
    std::printf("empty %d\n", xs_build_map(lead, 0, peer, 0, from));
    const int64_t twice[3] = {5, 6, 5};
    std::printf("peer-twice %d", xs_build_map(lead, 8, twice, 3, from)); std::printf(" %s\n", gauss_host_last_error());
    std::printf("lead-twice %d", xs_build_map(twice, 3, peer, 6, from)); std::printf(" %s\n", gauss_host_last_error());
    // the table builder on SusieRider's table of fixed result arrays
    const char* mid[5] = {"m0", "m1", "m2", "m3", "m4"};
    const int wing[5] = {1, 0, 1, 0, 0};
    WindowView v;
    v.mix = true;
    for (int i = 0; i < 5; i++) v.measured.push_back(ViewSnp{SnpIdent{mid[i], 22, 1000 + i, "C", "T"}, 0.25 + i, 0.5 * i - 1, wing[i]});
    v.row_m = {-1, 0, -1, 2, 5}; v.row_u = {1, 3, 4};
    v.plain = plain;
    for (int pass = 0; pass < 2; pass++) {
        SusieRider r(2, 0.5, 4.0, 0.25, 7, 0.25, 0, 0);
        gauss_window_desc d;
        memset(&d, 0, sizeof(d));
        d.n_measured = 5; d.n_unmeasured = 3; d.lambda = 0.1;
        if (r.check() || r.ask(d, v)) return 1;
        std::vector<double> xs_V(6, NAN), xs_purity(6, NAN);
        int32_t status[3] = {GAUSS_ST_SUSIE_NOFIT, GAUSS_ST_CLAMPED | GAUSS_ST_SUSIE_NOFIT, GAUSS_ST_SUSIE_NOFIT};
        if (pass == 0) {
            r.pip = {0.0, 0.015625, 0.75, 0.25, 0.125, 0.25, 0.0, 0.5};
            r.set = {-1, -1, 0, -1, -1, 0, -1, -1};
            r.set_pip = {0.0, 0.0, 0.75, 0.0, 0.0, 0.25, 0.0, 0.0};
            r.alpha = {0.0, 0.0, 0.75, 0.0, 0.0, 0.25, 0.0, 0.0,   0.0, 0.015625, 0.0, 0.25, 0.125, 0.0, 0.0, 0.5};
            r.V = {30.5, 0.0}; r.lse = {40.5, -0.25}; r.mass = {1.0, 0.875}; r.purity = {0.625, 0.125}; r.size = {2, 3}; r.kept = {1, 0};
            r.sweeps = {3.0, 0.125};
            xs_V = {30.5, 0.0, 11.0, 0.0, 7.5, 0.0};                   // [K = 3][L = 2]
            xs_purity = {0.5, 0.125, 0.625, 0.0625, 0.25, 0.03125};
            status[0] = status[1] = status[2] = 0;
        }
        const uint8_t joint[8] = {1, 1, 0, 1, 1, 1, 0, 1};             // by leader candidate: measured 2 (a wing SNP) and unmeasured 1 are not joint
        gauss_table* got = nullptr;
        if (r.table(v, &got)) return 1;
        if (xsusie_output(*got, v.row_m, v.row_u, joint, 3, 2, xs_V.data(), xs_purity.data(), status)) return 1;
        dump(pass == 0 ? "fit" : "nofit", *got);
        gauss_table_free(got);
    }
    gauss_table other;
    const uint8_t j1[1] = {1};
    std::printf("refused %d", xsusie_output(other, {0}, {}, j1, 2, 2, nullptr, nullptr, nullptr)); std::printf(" %s\n", gauss_host_last_error());
}
'''


@pytest.fixture(scope="module")
def xs_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("xsusie_host")
    hdir = os.path.join(ROOT, "gauss_amd", "csrc", "host")
    src = tmp / "main.cpp"
    src.write_text(XS_MAIN)
    exe = tmp / "xs"
    flags = [gxx, "-std=c++17", "-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + hdir]
    srcs = [str(src), os.path.join(hdir, "host_riders.cpp"), os.path.join(hdir, "host_tables.cpp")]
    objs = [str(tmp / f"{k}.o") for k in range(len(srcs))]
    jobs = [subprocess.Popen(flags + ["-c", s, "-o", o]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    subprocess.check_call(flags + objs + ["-o", str(exe), "-Wl,--unresolved-symbols=ignore-all", "-lz", "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.strip().split("\n")


HEX = float.fromhex


def _table(lines, tag):
    mine = [ln.split()[1:] for ln in lines if ln.startswith(tag + " ")]
    assert mine and mine[0][0] == "cols"
    body = {}
    for tok in mine[1:]:
        key, vals = ("named " + tok[1], tok[2:]) if tok[0] == "named" else (tok[0], tok[1:])
        body.setdefault(key, []).extend(vals)
    return mine[0][1:], body


def test_the_map_builder(xs_output):
    line = lambda tag: [ln for ln in xs_output if ln.startswith(tag + " ")][0].split()[1:]
    assert line("map") == ["5", "2", "-1", "-1", "1", "4", "-1", "0", "5"]          # shared, then from_lead
    assert line("empty") == ["0"]
    assert line("peer-twice")[0] == "-1" and "candidates 0 and 2 of a study are the same panel SNP" in " ".join(line("peer-twice"))
    assert line("lead-twice")[0] == "-1" and "of the first study" in " ".join(line("lead-twice"))


def test_the_table_builder(xs_output):
    """xsusie_output() on SusieRider's table: the column joint by table row, `effects` with every study's V and purity, the messages"""
    names, t = _table(xs_output, "fit")
    assert names == ["rsid", "chr", "bp", "a1", "a2", "af1mix", "z", "pval", "info", "type", "wing", "pip", "cs", "cs_pip", "joint"]
    assert t["rsid"] == ["m1", "u0", "m3", "u1", "u2", "m4", "m0", "m2"]
    # candidates m0 m1 m2 m3 m4 u0 u1 u2 = 1 1 0 1 1 1 0 1
    assert t["joint"] == ["1", "1", "1", "0", "1", "1", "1", "0"]
    assert [HEX(x) for x in t["pip"]] == [0.015625, 0.25, 0.25, 0.0, 0.5, 0.125, 0.0, 0.75]
    # effects [2 x 11], column-major: row, V_1 V_2 V_3, purity_1 purity_2 purity_3, lse, size, mass, kept
    assert t["named effects"][:2] == ["2", "11"]
    assert [HEX(x) for x in t["named effects"][2:]] == [7.0, 4.0, 30.5, 0.0, 11.0, 0.0, 7.5, 0.0, 0.5, 0.125, 0.625, 0.0625, 0.25, 0.03125,
                                                        40.5, -0.25, 2.0, 3.0, 1.0, 0.875, 1.0, 0.0]
    assert t["named fit"][:2] == ["1", "3"] and [HEX(x) for x in t["named fit"][2:]] == [3.0, 0.125, 1.0]
    assert "message" not in t
    names, t = _table(xs_output, "nofit")
    msg = " ".join(t["message"])
    assert np.all(np.isnan([HEX(x) for x in t["pip"]])) and "was not fitted" in msg
    assert "the group was not fitted: the B11 of study 2 was repaired by MakePosDef" in msg and "study 1 " not in msg and "study 3" not in msg
    assert t["joint"] == ["1", "1", "1", "0", "1", "1", "1", "0"] and np.all(np.isnan([HEX(x) for x in t["named effects"][4:16]]))
    refused = [ln for ln in xs_output if ln.startswith("refused")][0]
    assert refused.split()[1] == "-1" and "not susie_output's" in refused
