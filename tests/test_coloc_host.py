"""CPU: the plumbing of the multi-trait fit and its colocalisation that a GPU-less machine can check -- the C ABI's window descriptor
and its ctypes mirror, the integration snippet, the hotpath's keys, the reference's layout of the pairs, the host entry points, and
ColocRider's ask() / table() on a hand-made WindowView (a stand-alone program under the address and undefined-behaviour sanitizers;
nothing is loaded into Python)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import desc_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORE = ["pip", "set", "set_pip", "V", "lse", "mass", "purity", "size", "kept", "alpha", "mu", "lbf", "sweeps", "status"]
COLOC_FIELDS = ["coloc_traits_more", "coloc_p1", "coloc_p2", "coloc_p12", "out_coloc_lbf"] + ["out_coloc_more_" + k for k in MORE] + \
               ["out_coloc_pp", "out_coloc_hit", "out_coloc_hit_pp", "out_coloc_n"]


def test_window_descriptor_mirror_has_the_size_and_the_fields_of_the_header():
    from gauss_amd import _lib
    names = [f[0] for f in _lib.WindowDesc._fields_]
    at = names.index("coloc_traits_more")
    assert names[at: at + len(COLOC_FIELDS)] == COLOC_FIELDS and names[at + len(COLOC_FIELDS)] == "u_codings" and names[at - 1] == "out_num_eig"
    assert [n for n in names if "coloc_" in n] == COLOC_FIELDS
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is needed to check the descriptor against the header"
    fields = ["out_num_eig"] + COLOC_FIELDS + ["u_codings", "susie_L"]
    size, offs, (cap,) = desc_layout(fields, ["GAUSS_SUSIE_TRAITS_MORE_MAX"])
    assert ctypes.sizeof(_lib.WindowDesc) == size and cap == _lib.SUSIE_TRAITS_MORE_MAX == 7
    assert [getattr(_lib.WindowDesc, n).offset for n in fields] == offs
    # an int with its padding, then 3 + 1 + 14 + 4 eight-byte fields, then u_codings and susie_L in one word
    assert offs == sorted(offs) and offs[1] - offs[0] == 8 and offs[-2] - offs[1] == 8 + 22 * 8 and offs[-1] - offs[-2] == 4


def test_zero_initialised_descriptor_asks_for_nothing():
    from gauss_amd import _lib
    d = _lib.WindowDesc()
    assert d.coloc_traits_more == 0 and d.coloc_p1 == d.coloc_p2 == d.coloc_p12 == 0.0
    assert not any(getattr(d, n) for n in COLOC_FIELDS if n.startswith("out_"))


def test_integration_snippet_compiles_against_the_header():
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is needed to check the descriptor against the header"
    subprocess.check_call([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi", "coloc_snippet.cpp")])
    hdr = open(os.path.join(ROOT, "include", "gauss_hip.h")).read()
    assert re.search(r"#define\s+GAUSS_SUSIE_TRAITS_MORE_MAX\s+7\b", hdr)


def test_hotpath_sets_the_fields():
    from gauss_amd import _lib, hotpath
    gm, gu = np.zeros((5, 8), dtype=np.uint8), np.zeros((3, 8), dtype=np.uint8)
    mk = lambda susie, z_more=None: (lambda d: (d, hotpath._Win(d, dict(mode=0, geno_m=gm, geno_u=gu, pop_off=[0, 8], z1=np.zeros(5), lam=0.1, z_more=z_more,
                                                                    susie=susie))))(_lib.WindowDesc())
    d, w = mk(dict())                                  # the fit of trait 1 alone asks for nothing new
    assert d.coloc_traits_more == 0 and d.coloc_p12 == 0.0 and not any(getattr(d, n) for n in COLOC_FIELDS if n.startswith("out_"))
    assert "susie_more_pip" not in w.result() and "coloc_pp" not in w.result() and "susie_lbf" not in w.result()
    d, w = mk(dict(L=4, traits=2, coloc={}, want_lbf=True, want_alpha=True), np.zeros((3, 5)))
    assert (d.coloc_traits_more, d.coloc_p1, d.coloc_p2, d.coloc_p12) == (2, 1e-4, 1e-4, 1e-5) and d.n_traits_more == 3
    assert all(getattr(d, n) for n in COLOC_FIELDS if n.startswith("out_"))
    r = w.result()
    assert r["susie_lbf"].shape == (4, 8) and r["susie_more_pip"].shape == (2, 8) and r["susie_more_alpha"].shape == (2, 4, 8)
    assert r["susie_more_lbf"].shape == (2, 4, 8) and r["susie_more_kept"].shape == (2, 4) and r["susie_more_status"].shape == (2,)
    assert r["susie_more_sweeps"].shape == (2,) and r["susie_more_delta"].shape == (2,)
    assert r["coloc_pp"].shape == (3, 4, 4, 5) and r["coloc_hit"].shape == r["coloc_hit_pp"].shape == (3, 4, 4) and r["coloc_n"].shape == (3,)
    assert np.all(r["coloc_hit"] == -1) and np.all(np.isnan(r["coloc_pp"]))
    d, w = mk(dict(traits=1, coloc=dict(p1=1e-3, p2=2e-3, p12=5e-4)), np.zeros((1, 5)))
    assert (d.coloc_p1, d.coloc_p2, d.coloc_p12) == (1e-3, 2e-3, 5e-4) and not d.out_coloc_lbf and not d.out_coloc_more_alpha
    d, w = mk(dict(traits=9), np.zeros((9, 5)))        # the library refuses; the buffers stay at the cap
    assert d.coloc_traits_more == 9 and w.result()["susie_more_pip"].shape == (_lib.SUSIE_TRAITS_MORE_MAX, 8)


def test_the_reference_s_pairs_are_in_the_documented_order():
    import coloc_ref as cr
    assert cr.pair_list(1) == [(0, 1)] and cr.pair_list(3) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] and len(cr.pair_list(7)) == 28


def test_host_header_declares_and_api_binds_the_calls(tmp_path):
    import types
    from gauss_amd import api
    src = open(os.path.join(ROOT, "include", "gauss_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gauss_host_dist_coloc", "gauss_host_distmix_coloc"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in api.HOST_SYMBOLS
    h = api.load_host()                                   # builds on a GPU-less machine too; the symbols must be exported
    dbl = ctypes.c_double
    for fn, traits, susie in ((h.gauss_host_dist_coloc, h.gauss_host_dist_traits, h.gauss_host_dist_susie),
                              (h.gauss_host_distmix_coloc, h.gauss_host_distmix_traits, h.gauss_host_distmix_susie)):
        n = len(traits.argtypes) - 1                      # the *_traits arguments, those *_susie adds to the plain call, p1, p2, p12, out
        assert fn.argtypes == traits.argtypes[:-1] + susie.argtypes[n - 2:-1] + [dbl, dbl, dbl] + traits.argtypes[-1:]
    missing = str(tmp_path / "nothing.txt")
    fake = types.SimpleNamespace(handle=ctypes.c_void_p(1))      # never dereferenced: the files are looked at first
    with pytest.raises(Exception, match="nothing.txt"):
        api.dist_coloc(22, 1, 2, 1, "EUR", [missing, missing], missing, missing, missing, ctx=fake)
    with pytest.raises(Exception, match="nothing.txt"):
        api.distmix_coloc(22, 1, 2, 1, (["a"], [1.0]), [missing, missing, missing], missing, missing, missing, L=3, p12=1e-6, ctx=fake)


RIDER_MAIN = r'''
#include "host_internal.h"
// the two further study files of the made-up window, in memory: the stand-alone program has no data layer.  File "b" lists the
// measured SNPs with swapped alleles (the sign flips); file "lacks" has no row for m3
int files_ok(std::initializer_list<const char*> names) { for (const char* n : names) if (!n) return herr("file name is NULL"); return 0; }
std::shared_ptr<const GwasCache> load_gwas_cached(const std::string& path, std::string& err)
{
    if (path != "a" && path != "b" && path != "lacks") { err = "cannot open " + path; return nullptr; }
    auto gw = std::make_shared<GwasCache>();
    const char* mid[5] = {"m0", "m1", "m2", "m3", "m4"};
    for (int i = 0; i < 5; i++) {
        if (path == "lacks" && i == 3) continue;
        const bool swap = path == "b";
        gw->rows.push_back(GwasRow{mid[i], swap ? "T" : "C", swap ? "C" : "T", 22, 1000 + i, (path == "a" ? 10.0 : 20.0) + i});
        gw->by_pos.push_back((uint32_t)gw->rows.size() - 1);
    }
    return gw;
}
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
// the call's own table of the made-up window (tests/test_susie_host.py's): 6 rows of the prediction window (measured 1, 3, 4 -> rows
// 0, 2, 5; unmeasured 0, 1, 2 -> rows 1, 3, 4); measured 0 and 2 lie in the wings and are not listed
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
    for (int i = 0; i < 5; i++) {
        const SnpIdent id{mid[i], 22, 1000 + i, "C", "T"};
        v.measured.push_back(ViewSnp{id, 0.25 + i, 0.5 * i - 1, wing[i]});
    }
    v.row_m = {-1, 0, -1, 2, 5}; v.row_u = {1, 3, 4};
    v.plain = plain;
    const char* files[2] = {"a", "b"};
    for (int pass = 0; pass < 3; pass++) {
        ColocRider r(files, 2, SusieRider(pass ? 2 : 0, 0.0, 0.0, 0.0, 0, pass ? 0.25 : 0.0, -1, 0), pass ? 1e-3 : 0.0, pass ? 2e-3 : NAN, pass ? 5e-4 : -1.0);
        gauss_window_desc d;
        memset(&d, 0, sizeof(d));
        d.n_measured = 5; d.n_unmeasured = 3; d.lambda = 0.1;
        const int rc = r.check() || r.ask(d, v);
        std::printf("coloc%d ask %d %d %d %d %zu %zu %zu %zu %zu %zu %d %d %d %a %a %a %a %a\n", pass, rc, d.coloc_traits_more, d.n_traits_more, d.susie_L,
                    r.pip.size(), r.alpha.size(), r.V.size(), r.sweeps.size(), r.pp.size(), r.n.size(),
                    d.out_coloc_more_pip == r.pip.data() && d.out_coloc_more_set == r.set.data() && d.out_coloc_more_set_pip == r.set_pip.data() &&
                    d.out_coloc_more_alpha == r.alpha.data() && d.out_coloc_more_V == r.V.data() && d.out_coloc_more_lse == r.lse.data() &&
                    d.out_coloc_more_mass == r.mass.data() && d.out_coloc_more_purity == r.purity.data() && d.out_coloc_more_size == r.size.data() &&
                    d.out_coloc_more_kept == r.kept.data() && d.out_coloc_more_sweeps == r.sweeps.data(),
                    d.out_coloc_pp == r.pp.data() && d.out_coloc_hit == r.hit.data() && d.out_coloc_hit_pp == r.hit_pp.data() && d.out_coloc_n == r.n.data(),
                    d.out_susie_pip == r.susie.pip.data() && d.z_more == r.traits.z.data() && d.out_z_more == r.traits.out_z.data() && !d.miss_more && !d.slct_max,
                    d.coloc_p1, d.coloc_p2, d.coloc_p12, r.traits.z[1], r.traits.z[5 + 3]);
        if (pass == 0) continue;
        if (pass == 1) {
            // candidates: measured 0 .. 4, then unmeasured 0 .. 2; L = 2.  Trait 1: effect 0 (lead: measured 2, a wing SNP) is kept.  Trait 2:
            // effect 1 (lead: unmeasured 0) is kept.  Trait 3: nothing kept, its sweeps ran out.  One pair of kept effects: traits (1, 2),
            // effects (1, 2), hit = candidate 5 (unmeasured 0, table row 1)
            SusieRider& s = r.susie;
            s.pip = {0.0, 0.015625, 0.75, 0.25, 0.125, 0.25, 0.0, 0.5};
            s.set = {-1, -1, 0, -1, -1, 0, -1, -1};
            s.set_pip = {0.0, 0.0, 0.75, 0.0, 0.0, 0.25, 0.0, 0.0};
            s.alpha = {0.0, 0.0, 0.75, 0.0, 0.0, 0.25, 0.0, 0.0,   0.0, 0.015625, 0.0, 0.25, 0.125, 0.0, 0.0, 0.5};
            s.V = {30.5, 0.0}; s.lse = {40.5, -0.25}; s.mass = {1.0, 0.875}; s.purity = {0.625, 0.125}; s.size = {2, 3}; s.kept = {1, 0};
            s.sweeps = {7.0, 0.125};
            for (int c = 0; c < 8; c++) { r.pip[c] = 0.0625 * c; r.pip[8 + c] = 0.03125 * c; r.set_pip[c] = 0.0; r.set_pip[8 + c] = 0.0; }
            r.set[5] = 1; r.set_pip[5] = 0.875;
            for (size_t e = 0; e < r.alpha.size(); e++) r.alpha[e] = 0.0;
            r.alpha[0 * 16 + 0 * 8 + 3] = 1.0; r.alpha[0 * 16 + 1 * 8 + 5] = 0.875; r.alpha[1 * 16 + 0 * 8 + 7] = 0.5; r.alpha[1 * 16 + 1 * 8 + 1] = 0.5;
            r.V = {0.0, 20.0, 1.0, 2.0}; r.lse = {0.0, 30.0, 0.5, 0.25}; r.mass = {0.5, 0.875, 0.5, 0.5}; r.purity = {1.0, 1.0, 0.25, 0.125};
            r.size = {4, 1, 5, 6}; r.kept = {0, 1, 0, 0};
            r.sweeps = {5.0, 0.0625, 100.0, 0.5};              // trait 3: delta 0.5 against tol 0.25
            r.n = {8, 8, 7};
            const size_t e = (0 * 2 + 0) * 2 + 1;              // pair (0, 1), la = 0, lb = 1
            r.hit[e] = 5; r.hit_pp[e] = 0.75;
            const double pp[5] = {0.0, 0.0625, 0.0625, 0.125, 0.75};
            for (int h = 0; h < 5; h++) r.pp[5 * e + h] = pp[h];
        }                                                      // pass 2: the buffers as ask() left them -- a window that was not fitted
        gauss_table* got = nullptr;
        if (r.table(v, &got)) return 1;
        dump(pass == 1 ? "fit" : "nofit", *got);
        gauss_table_free(got);
    }
    const char* one[8] = {"a", "a", "a", "a", "a", "a", "a", "a"};
    ColocRider none(one, 0, SusieRider(0, 0, 0, 0, 0, 0, -1, 0), 0, 0, 0), many(one, 8, SusieRider(0, 0, 0, 0, 0, 0, -1, 0), 0, 0, 0);
    ColocRider big(one, 1, SusieRider(33, 0, 0, 0, 0, 0, -1, 0), 0, 0, 0);
    std::printf("refused none %d", none.check()); std::printf(" %s\n", gauss_host_last_error());
    std::printf("refused many %d", many.check()); std::printf(" %s\n", gauss_host_last_error());
    std::printf("refused big %d", big.check()); std::printf(" %s\n", gauss_host_last_error());
    const char* bad[2] = {"a", "lacks"};
    ColocRider lacks(bad, 2, SusieRider(0, 0, 0, 0, 0, 0, -1, 0), 0, 0, 0);
    gauss_window_desc d;
    memset(&d, 0, sizeof(d));
    d.n_measured = 5; d.n_unmeasured = 3; d.lambda = 0.1;
    std::printf("refused lacks %d", lacks.check() || lacks.ask(d, v)); std::printf(" %s\n", gauss_host_last_error());
}
'''


@pytest.fixture(scope="module")
def rider_output(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is needed to build the stand-alone rider program"
    tmp = tmp_path_factory.mktemp("coloc_rider")
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
        body.setdefault(key, []).extend(vals)
    return names, body


HEX = float.fromhex


def test_ask_sets_the_descriptor_and_the_defaults(rider_output):
    """ColocRider::ask() on a hand-made view, as a stand-alone program under the address and undefined-behaviour sanitizers: the further
    files matched (swapped alleles flip the sign), every further trait fitted, the buffers sized and handed over, coloc's defaults."""
    tok = [ln for ln in rider_output if ln.startswith("coloc0 ask")][0].split()[2:]
    # rc, k, n_traits_more, L; sizes: pip k T, alpha k L T, V k L, sweeps 2 k, pp 5 pairs L L, n pairs; the pointers are the rider's
    assert tok[:13] == ["0", "2", "2", "10", "16", "160", "20", "4", "1500", "3", "1", "1", "1"]
    assert [HEX(x) for x in tok[13:16]] == [1e-4, 1e-4, 1e-5]
    assert [HEX(x) for x in tok[16:18]] == [11.0, -23.0]          # file a: 10 + i at m1; file b (alleles swapped): -(20 + i) at m3
    tok = [ln for ln in rider_output if ln.startswith("coloc1 ask")][0].split()[2:]
    assert tok[:10] == ["0", "2", "2", "2", "16", "32", "4", "4", "60", "3"] and [HEX(x) for x in tok[13:16]] == [1e-3, 2e-3, 5e-4]
    refused = {ln.split()[1]: ln for ln in rider_output if ln.startswith("refused")}
    assert refused["none"].split()[2] == "-1" and "at least two study files" in refused["none"]
    assert refused["many"].split()[2] == "-1" and "at most 8 traits" in refused["many"]
    assert refused["big"].split()[2] == "-1" and "at most 32 effects" in refused["big"]
    assert refused["lacks"].split()[2] != "0" and "lacks" in refused["lacks"] and "m3" in refused["lacks"]


def test_the_rider_builds_the_table(rider_output):
    """ColocRider::table() on fixed result arrays: *_susie's rows and its columns for trait 1, pip_t cs_t cs_pip_t per further trait,
    the *_traits matrices on every row, effects_t / fit_t per trait, one `coloc` row per pair of kept effects, a message per trait."""
    names, t = _table(rider_output, "fit")
    assert names == ["rsid", "chr", "bp", "a1", "a2", "af1mix", "z", "pval", "info", "type", "wing", "pip", "cs", "cs_pip",
                     "pip_2", "cs_2", "cs_pip_2", "pip_3", "cs_3", "cs_pip_3"]
    assert t["rsid"] == ["m1", "u0", "m3", "u1", "u2", "m4", "m0", "m2"] and t["wing"] == ["0"] * 6 + ["1", "1"]
    # trait 1: the bits tests/test_susie_host.py expects of SusieRider on the same arrays
    assert [HEX(x) for x in t["pip"]] == [0.015625, 0.25, 0.25, 0.0, 0.5, 0.125, 0.0, 0.75] and t["cs"] == ["0", "1", "0", "0", "0", "0", "0", "1"]
    assert [HEX(x) for x in t["cs_pip"]] == [0.0, 0.25, 0.0, 0.0, 0.0, 0.0, 0.0, 0.75]
    # candidates 0 .. 7 sit in rows 6, 0, 7, 2, 5, 1, 3, 4
    rows = [6, 0, 7, 2, 5, 1, 3, 4]
    for k, step in ((2, 0.0625), (3, 0.03125)):
        want = [0.0] * 8
        for c, r in enumerate(rows):
            want[r] = step * c
        assert [HEX(x) for x in t[f"pip_{k}"]] == want
    assert t["cs_2"] == ["0", "2", "0", "0", "0", "0", "0", "0"] and t["cs_3"] == ["0"] * 8
    assert [HEX(x) for x in t["cs_pip_2"]] == [0.0, 0.875, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert t["named effects_1"][:2] == ["2", "7"]
    assert [HEX(x) for x in t["named effects_1"][2:]] == [7.0, 4.0, 30.5, 0.0, 40.5, -0.25, 2.0, 3.0, 1.0, 0.875, 0.625, 0.125, 1.0, 0.0]
    assert [HEX(x) for x in t["named effects_2"][2:]] == [2.0, 1.0, 0.0, 20.0, 0.0, 30.0, 4.0, 1.0, 0.5, 0.875, 1.0, 1.0, 0.0, 1.0]
    assert [HEX(x) for x in t["named effects_3"][2:4]] == [4.0, 0.0]
    assert [[HEX(x) for x in t[f"named fit_{k}"][2:]] for k in (1, 2, 3)] == [[7.0, 0.125, 1.0], [5.0, 0.0625, 1.0], [100.0, 0.5, 0.0]]
    assert "named effects" not in t and "named fit" not in t
    # z_traits [8 x 3] on every row, the wings' measured SNPs included: column 0 the table's z, then file a (10 + i), file b (-(20 + i))
    z = [HEX(x) for x in t["named z_traits"][2:]]
    assert t["named z_traits"][:2] == ["8", "3"] and z[:8] == [HEX(x) for x in t["z"]]
    assert [z[8 + r] for r in (0, 2, 5, 6, 7)] == [11.0, 13.0, 14.0, 10.0, 12.0] and [z[16 + r] for r in (0, 2, 5, 6, 7)] == [-21.0, -23.0, -24.0, -20.0, -22.0]
    # coloc [1 x 12]: trait_a trait_b cs_a cs_b n H0 .. H4 hit_row hit_pp
    assert t["named coloc"][:2] == ["1", "12"]
    assert [HEX(x) for x in t["named coloc"][2:]] == [1.0, 2.0, 1.0, 2.0, 8.0, 0.0, 0.0625, 0.0625, 0.125, 0.75, 1.0, 0.75]
    msg = " ".join(t["message"])
    assert "trait 3: the sweeps ran out" in msg and "trait 1" not in msg and "trait 2" not in msg
    names, t = _table(rider_output, "nofit")
    assert np.all(np.isnan([HEX(x) for x in t["pip"] + t["pip_2"] + t["pip_3"]])) and t["cs"] == t["cs_2"] == t["cs_3"] == ["0"] * 8
    assert t["named coloc"][:2] == ["0", "12"] and len(t["named coloc"]) == 2
    assert all(f"trait {k}: the window was not fitted" in " ".join(t["message"]) for k in (1, 2, 3))
