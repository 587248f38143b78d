"""CPU: the plumbing of the multi-causal fine-mapping that a GPU-less machine can check -- the C ABI's window descriptor and its ctypes
mirror, the host entry points, the hotpath's key, and SusieRider's ask() / table() on a hand-made WindowView (a stand-alone program
under the address and undefined-behaviour sanitizers; nothing is loaded into Python)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import desc_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUSIE_FIELDS = ["susie_L", "susie_coverage", "susie_prior_var", "susie_tol", "susie_min_abs_corr", "out_susie_pip", "out_susie_set",
                "out_susie_set_pip", "out_susie_V", "out_susie_lse", "out_susie_mass", "out_susie_purity", "out_susie_size", "out_susie_kept",
                "out_susie_alpha", "out_susie_mu", "out_susie_sweeps", "susie_max_sweeps", "susie_estimate_var", "susie_measured_only"]


def test_window_descriptor_mirror_has_the_size_and_the_fields_of_the_header():
    from gauss_amd import _lib
    names = [f[0] for f in _lib.WindowDesc._fields_]
    at = names.index("susie_L")
    assert names[at: at + 20] == SUSIE_FIELDS and names[at + 20] == "geno_format" and names[at - 1] == "u_codings"
    assert [n for n in names if "susie_" in n] == SUSIE_FIELDS and names[-3:] == ["out_loo_z", "out_loo_info", "out_loo_t"]
    fields = ["u_codings"] + SUSIE_FIELDS + ["geno_format", "rows_m"]
    size, offs, _ = desc_layout(fields)
    assert ctypes.sizeof(_lib.WindowDesc) == size
    assert [getattr(_lib.WindowDesc, n).offset for n in fields] == offs
    # u_codings and susie_L share a word, sixteen 8-byte fields, max_sweeps / estimate_var and measured_only / geno_format share two
    assert offs == sorted(offs) and offs[1] - offs[0] == 4 and offs[-1] - offs[0] == 8 + 16 * 8 + 16


def test_zero_initialised_descriptor_asks_for_nothing():
    from gauss_amd import _lib
    d = _lib.WindowDesc()
    assert d.susie_L == 0 and d.susie_max_sweeps == 0 and d.susie_coverage == 0.0
    assert not any(getattr(d, n) for n in SUSIE_FIELDS if n.startswith("out_"))


def test_host_header_declares_and_api_binds_the_calls():
    from gauss_amd import api
    src = open(os.path.join(ROOT, "include", "gauss_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gauss_host_dist_susie", "gauss_host_distmix_susie"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in api.HOST_SYMBOLS
    assert callable(api.dist_susie) and callable(api.distmix_susie)
    h = api.load_host()                                   # builds on a GPU-less machine too; the symbols must be exported
    tail = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int]
    for fn, plain in ((h.gauss_host_dist_susie, h.gauss_host_dist), (h.gauss_host_distmix_susie, h.gauss_host_distmix)):
        assert fn.argtypes[:-1] == plain.argtypes[:-1] + tail and fn.argtypes[-1] == plain.argtypes[-1]
    hdr = open(os.path.join(ROOT, "include", "gauss_hip.h")).read()
    assert re.search(r"#define\s+GAUSS_ST_SUSIE_NOCONV\s+16\b", hdr) and re.search(r"#define\s+GAUSS_ST_SUSIE_NOFIT\s+32\b", hdr)
    assert re.search(r"#define\s+GAUSS_SUSIE_MAX_L\s+32\b", hdr)


def test_integration_snippet_compiles_against_the_header():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    subprocess.check_call([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi", "susie_snippet.cpp")])


def test_hotpath_sets_the_fields():
    from gauss_amd import _lib, hotpath
    gm, gu = np.zeros((5, 8), dtype=np.uint8), np.zeros((3, 8), dtype=np.uint8)
    mk = lambda susie: (lambda d: (d, hotpath._Win(d, dict(mode=0, geno_m=gm, geno_u=gu, pop_off=[0, 8], z1=np.zeros(5), lam=0.1, susie=susie))))(_lib.WindowDesc())
    d, w = mk(dict())
    assert (d.susie_L, d.susie_max_sweeps, d.susie_estimate_var, d.susie_measured_only) == (10, 100, 1, 0)
    assert (d.susie_coverage, d.susie_prior_var, d.susie_tol, d.susie_min_abs_corr) == (0.95, 25.0, 1e-4, 0.5)
    assert all(getattr(d, n) for n in SUSIE_FIELDS if n.startswith("out_") and n not in ("out_susie_alpha", "out_susie_mu"))
    assert not d.out_susie_alpha and not d.out_susie_mu and not d.slct_max
    r = w.result()
    assert r["susie_pip"].shape == (8,) and r["susie_set"].dtype == np.int32 and r["susie_V"].shape == (10,) and "susie_alpha" not in r
    d, w = mk(dict(L=3, coverage=0.5, prior_var=4.0, tol=0.0, max_sweeps=7, min_abs_corr=0.25, estimate_var=False, measured_only=True, want_alpha=True))
    assert (d.susie_L, d.susie_max_sweeps, d.susie_estimate_var, d.susie_measured_only) == (3, 7, 0, 1)
    assert (d.susie_coverage, d.susie_prior_var, d.susie_tol, d.susie_min_abs_corr) == (0.5, 4.0, 0.0, 0.25)
    assert d.out_susie_alpha and w.result()["susie_alpha"].shape == (3, 8)
    d, w = mk(None)
    assert d.susie_L == 0 and not d.out_susie_pip and "susie_pip" not in w.result()


def test_refusals_that_need_no_gpu(tmp_path):
    """A missing file is named before anything else happens, as by the other one-window calls."""
    import types
    from gauss_amd import api
    missing = str(tmp_path / "nothing.txt")
    fake = types.SimpleNamespace(handle=ctypes.c_void_p(1))      # never dereferenced: the files are looked at first
    with pytest.raises(Exception, match="nothing.txt"):
        api.dist_susie(22, 1, 2, 1, "EUR", missing, missing, missing, missing, ctx=fake)
    with pytest.raises(Exception, match="nothing.txt"):
        api.distmix_susie(22, 1, 2, 1, (["a"], [1.0]), missing, missing, missing, missing, L=3, coverage=0.9, ctx=fake)


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
    for (auto& m : t.messages) std::printf("%s message %s\n", what, m.c_str());
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
    for (int i = 0; i < 5; i++) {
        const SnpIdent id{mid[i], 22, 1000 + i, "C", "T"};
        v.measured.push_back(ViewSnp{id, 0.25 + i, 0.5 * i - 1, wing[i]});
    }
    v.row_m = {-1, 0, -1, 2, 5}; v.row_u = {1, 3, 4};
    v.plain = plain;
    for (int pass = 0; pass < 3; pass++) {
        SusieRider r(pass ? 2 : 0, pass ? 0.5 : 0.0, pass ? 4.0 : NAN, pass ? 0.25 : 0.0, pass ? 7 : 0, pass == 1 ? 0.25 : pass ? -1.0 : 0.0, pass ? 0 : -1, pass ? 1 : 0);
        gauss_window_desc d;
        memset(&d, 0, sizeof(d));
        d.n_measured = 5; d.n_unmeasured = 3; d.lambda = 0.1;
        const int rc = r.check() || r.ask(d, v);
        std::printf("susie%d ask %d %d %d %d %d %zu %zu %zu %zu %d %d %a %a %a %a\n", pass, rc, d.susie_L, d.susie_max_sweeps, d.susie_estimate_var,
                    d.susie_measured_only, r.pip.size(), r.set.size(), r.alpha.size(), r.V.size(),
                    d.out_susie_pip == r.pip.data() && d.out_susie_set == r.set.data() && d.out_susie_set_pip == r.set_pip.data() && d.out_susie_alpha == r.alpha.data(),
                    d.out_susie_V == r.V.data() && d.out_susie_lse == r.lse.data() && d.out_susie_mass == r.mass.data() && d.out_susie_purity == r.purity.data() &&
                    d.out_susie_size == r.size.data() && d.out_susie_kept == r.kept.data() && d.out_susie_sweeps == r.sweeps.data() && !d.slct_max,
                    d.susie_coverage, d.susie_prior_var, d.susie_tol, d.susie_min_abs_corr);
        if (pass == 0) continue;
        // candidates: measured 0 .. 4, then unmeasured 0 .. 2.  Effect 0 (lead: measured 2, a wing SNP) is kept and holds measured 2 and
        // unmeasured 0; effect 1 (lead: unmeasured 2) is not kept
        if (pass == 1) {
            r.pip = {0.0, 0.015625, 0.75, 0.25, 0.125, 0.25, 0.0, 0.5};
            r.set = {-1, -1, 0, -1, -1, 0, -1, -1};
            r.set_pip = {0.0, 0.0, 0.75, 0.0, 0.0, 0.25, 0.0, 0.0};
            r.alpha = {0.0, 0.0, 0.75, 0.0, 0.0, 0.25, 0.0, 0.0,   0.0, 0.015625, 0.0, 0.25, 0.125, 0.0, 0.0, 0.5};
            r.V = {30.5, 0.0}; r.lse = {40.5, -0.25}; r.mass = {1.0, 0.875}; r.purity = {0.625, 0.125}; r.size = {2, 3}; r.kept = {1, 0};
            r.sweeps = {7.0, 0.5};                             // delta 0.5 against tol 0.25: the sweeps ran out
        }                                                      // pass 2: the buffers as ask() left them -- a window that was not fitted
        gauss_table* got = nullptr;
        if (r.table(v, &got)) return 1;
        dump(pass == 1 ? "fit" : "nofit", *got);
        gauss_table_free(got);
        if (pass == 1) {                                       // the same buffers behind a negative tol: running the sweeps out was asked for
            SusieRider q(2, 0.5, 4.0, 0.25, 7, -1.0, 0, 1);
            gauss_window_desc e;
            memset(&e, 0, sizeof(e));
            e.n_measured = 5; e.n_unmeasured = 3; e.lambda = 0.1;
            if (q.ask(e, v)) return 1;
            std::printf("negtolask %a\n", e.susie_tol);
            q.pip = r.pip; q.set = r.set; q.set_pip = r.set_pip; q.alpha = r.alpha; q.V = r.V; q.lse = r.lse; q.mass = r.mass; q.purity = r.purity;
            q.size = r.size; q.kept = r.kept; q.sweeps = r.sweeps;
            if (q.table(v, &got)) return 1;
            dump("negtol", *got);
            gauss_table_free(got);
        }
    }
    SusieRider big(33, 0, 0, 0, 0, 0, -1, 0);
    std::printf("refused %d", big.check()); std::printf(" %s\n", gauss_host_last_error());
}
'''


@pytest.fixture(scope="module")
def rider_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("susie_rider")
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


def test_the_rider_builds_the_table(rider_output):
    """SusieRider::table() on fixed result arrays: the call's own rows, then the wings' measured SNPs in matrix order; wing, pip, cs,
    cs_pip; `effects` and `fit`; the message when the sweeps ran out."""
    names, t = _table(rider_output, "fit")
    assert names == ["rsid", "chr", "bp", "a1", "a2", "af1mix", "z", "pval", "info", "type", "wing", "pip", "cs", "cs_pip"]
    assert t["rsid"] == ["m1", "u0", "m3", "u1", "u2", "m4", "m0", "m2"]
    assert t["wing"] == ["0", "0", "0", "0", "0", "0", "1", "1"] and t["type"] == ["1", "0", "1", "0", "0", "1", "1", "1"]
    assert [HEX(x) for x in t["pip"]] == [0.015625, 0.25, 0.25, 0.0, 0.5, 0.125, 0.0, 0.75]
    assert t["cs"] == ["0", "1", "0", "0", "0", "0", "0", "1"]
    assert [HEX(x) for x in t["cs_pip"]] == [0.0, 0.25, 0.0, 0.0, 0.0, 0.0, 0.0, 0.75]
    assert [HEX(x) for x in t["z"][6:]] == [-1.0, 0.0]                      # the wings' rows carry the study's z
    # effects [2 x 7], column-major: table row of the lead (the wing SNP m2 sits in row 7, u2 in row 4), V, lse, size, mass, purity, kept
    assert t["named effects"][:2] == ["2", "7"]
    assert [HEX(x) for x in t["named effects"][2:]] == [7.0, 4.0, 30.5, 0.0, 40.5, -0.25, 2.0, 3.0, 1.0, 0.875, 0.625, 0.125, 1.0, 0.0]
    assert t["named fit"][:2] == ["1", "3"] and [HEX(x) for x in t["named fit"][2:]] == [7.0, 0.5, 0.0]
    assert "the sweeps ran out" in " ".join(t["message"])
    names, t = _table(rider_output, "negtol")               # a negative tol: exactly max_sweeps sweeps, converged = 0, no message
    assert "message" not in t and [HEX(x) for x in t["named fit"][2:]] == [7.0, 0.5, 0.0]
    assert HEX([ln for ln in rider_output if ln.startswith("negtolask")][0].split()[1]) == 0.0
    names, t = _table(rider_output, "nofit")
    assert np.all(np.isnan([HEX(x) for x in t["pip"]])) and t["cs"] == ["0"] * 8 and "was not fitted" in " ".join(t["message"])
    assert [HEX(x) for x in t["named effects"][2:4]] == [-1.0, -1.0] and [HEX(x) for x in t["named fit"][2:]][::2] == [0.0, 0.0]


def test_ask_sets_the_descriptor_and_the_defaults(rider_output):
    tok = [ln for ln in rider_output if ln.startswith("susie0 ask")][0].split()[2:]
    # rc, L, max_sweeps, estimate_var, measured_only, buffer sizes (pip / set: M + U; alpha: L (M + U); V: L), the pointers are the rider's
    assert tok[:11] == ["0", "10", "100", "1", "0", "8", "8", "80", "10", "1", "1"]
    assert [HEX(x) for x in tok[11:15]] == [0.95, 25.0, 1e-4, 0.5]
    tok = [ln for ln in rider_output if ln.startswith("susie1 ask")][0].split()[2:]
    assert tok[:9] == ["0", "2", "7", "0", "1", "8", "8", "16", "2"] and [HEX(x) for x in tok[11:15]] == [0.5, 4.0, 0.25, 0.25]
    refused = [ln for ln in rider_output if ln.startswith("refused")]
    assert refused[0].split()[1] == "-1" and "at most 32 effects" in refused[0]
