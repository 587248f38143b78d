"""CPU: the riders of a one-window call (host_internal.h: Rider, host_riders.cpp) build their tables from the WindowView of the call
exactly as the table builders do from rows written out by hand -- a stand-alone program under the address and undefined-behaviour
sanitizers, no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RIDERS_MAIN = r'''
#include "host_internal.h"
// every column and every named matrix of a table, values to the bit
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
static int plain_calls = 0;
static int plain(gauss_table** out) {
    plain_calls++;
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
    for (int i = 0; i < 5; i++) v.measured.push_back(ViewSnp{SnpIdent{mid[i], 22, 1000 + i, "C", "T"}, 0.25 + i, 0.5 * i - 1, wing[i]});
    v.row_m = {-1, 0, -1, 2, 5}; v.row_u = {1, 3, 4};
    v.plain = plain;
    // the same rows written out by hand, as the builders take them
    std::vector<LooRow> loo_rows;
    std::vector<SlctRow> slct_rows;
    for (int i = 0; i < 5; i++) {
        const SnpIdent id{mid[i], 22, 1000 + i, "C", "T"};
        if (!wing[i]) loo_rows.push_back(LooRow{id, 0.25 + i, 0.5 * i - 1, i});
        slct_rows.push_back(SlctRow{id, 0.25 + i, 0.5 * i - 1, wing[i]});
    }
    gauss_table* got = nullptr;
    gauss_table* want = nullptr;

    {   // loo: ask() sizes the three arrays and hands them to the descriptor; table() lists the prediction window's measured SNPs
        LooRider r;
        gauss_window_desc d;
        memset(&d, 0, sizeof(d));
        d.n_measured = 5; d.n_unmeasured = 3;
        const int rc = r.check() || r.ask(d, v);
        std::printf("loo ask %d %zu %d\n", rc, r.z.size(), d.out_loo_z == r.z.data() && d.out_loo_info == r.info.data() && d.out_loo_t == r.t.data());
        r.z = {0.125, -1.5, 2.25, NAN, 4.5}; r.info = {0.5, 0.625, 0.75, 0.0, 0.875}; r.t = {-0.25, 1.75, -2.5, 3.25, -4.0};
        if (r.table(v, &got)) return 1;
        want = loo_output(true, loo_rows, r.z.data(), r.info.data(), r.t.data());
        dump("loo.got", *got); dump("loo.want", *want);
        gauss_table_free(got); gauss_table_free(want);
    }
    const int32_t idx[4] = {2, 3, -1, -1};                  // a wing SNP first, then measured 3
    const std::vector<double> zin = {7.5, -6.5, NAN, NAN}, joint = {7.25, -6.25, NAN, NAN};
    const std::vector<double> zc = {0.5, 0.25, NAN, NAN, 2.0}, var = {0.75, 0.5, 0.0, 0.0, 0.875};
    const std::vector<double> cz = {1.5, NAN, -2.5}, cv = {0.625, 0.05, 0.375};
    for (int unmeasured = 0; unmeasured < 2; unmeasured++) {
        // slct / cond: ask() finds the conditioning SNPs among the view's measured SNPs, in the caller's order
        const char* cond[2] = {"m3", "m0"};
        SlctRider r(0.0, 0.0, 4, cond, 2, unmeasured != 0);
        gauss_window_desc d;
        memset(&d, 0, sizeof(d));
        d.n_measured = 5; d.n_unmeasured = 3; d.lambda = 0.1;
        const int rc = r.check() || r.ask(d, v);
        std::printf("slct%d ask %d %d %d %d %d %zu %zu %zu %d %d %a %a\n", unmeasured, rc, d.slct_max, d.n_slct_forced, d.slct_forced[0], d.slct_forced[1],
                    r.idx.size(), r.zc.size(), r.cond_z.size(), d.out_slct_n == &r.n && d.out_slct_idx == r.idx.data() && d.out_slct_zc == r.zc.data(),
                    unmeasured ? d.out_cond_z == r.cond_z.data() && d.out_cond_var == r.cond_var.data() : !d.out_cond_z && !d.out_cond_var,
                    d.slct_min_var_frac, d.cond_min_var_frac);
        r.n = 2; r.idx.assign(idx, idx + 4); r.zin = zin; r.joint = joint; r.zc = zc; r.var = var;
        if (unmeasured) { r.cond_z = cz; r.cond_var = cv; }
        if (r.table(v, &got)) return 1;
        if (!unmeasured) want = slct_output(true, slct_rows, 2, idx, zin.data(), joint.data(), zc.data(), var.data());
        else {
            plain(&want);
            if (cond_output(*want, slct_rows, v.row_m, v.row_u, 2, idx, zin.data(), joint.data(), zc.data(), var.data(), cz.data(), cv.data())) return 1;
        }
        dump(unmeasured ? "cond.got" : "slct.got", *got); dump(unmeasured ? "cond.want" : "slct.want", *want);
        gauss_table_free(got); gauss_table_free(want);
    }
    {   // the refusals of ask() that the window decides
        const char* twice[2] = {"m1", "m1"};
        const char* stranger[1] = {"u0"};
        gauss_window_desc d;
        memset(&d, 0, sizeof(d));
        d.n_measured = 5; d.n_unmeasured = 3;
        SlctRider a(0.0, 0.0, 4, twice, 2, false), b(0.0, 0.0, 4, stranger, 1, true), c(0.0, 0.0, 33, nullptr, 0, false);
        std::printf("refused %d", a.ask(d, v)); std::printf(" %s\n", gauss_host_last_error());
        std::printf("refused %d", b.ask(d, v)); std::printf(" %s\n", gauss_host_last_error());
        std::printf("refused %d", c.ask(d, v)); std::printf(" %s\n", gauss_host_last_error());
    }
    // traits: 2 further traits; trait 2 lacks measured 1 (in the window) and measured 2 (in a wing), trait 3 lacks measured 4
    const std::vector<double> tz = {0.5, 0.0, 0.0, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 0.0}, toz = {1.25, 2.25, 3.25, -1.25, -2.25, -3.25};
    const std::vector<uint8_t> mask = {0, 1, 1, 0, 0, 0, 0, 0, 0, 1};
    const std::vector<double> info_more = {0.5, 0.375, 0.25, 0.75, 0.625, 0.125}, z_miss = {6.5, 7.5, -8.5}, info_miss = {0.0625, 0.1875, 0.3125};
    for (int miss = 0; miss < 2; miss++) {
        TraitsRider r(nullptr, 2, miss != 0);
        r.z = tz; r.out_z = toz;
        if (miss) { r.mask = mask; r.info = info_more; r.z_miss = z_miss; r.info_miss = info_miss; }
        if (r.table(v, &got)) return 1;
        plain(&want);
        const TraitsMiss tm = {mask.data(), info_more.data(), z_miss.data(), info_miss.data()};
        traits_output(*want, 2, v.row_m, v.row_u, tz.data(), toz.data(), miss ? &tm : nullptr);
        dump(miss ? "miss.got" : "traits.got", *got); dump(miss ? "miss.want" : "traits.want", *want);
        gauss_table_free(got); gauss_table_free(want);
    }
    {   // check(): the refusals that need no window
        const char* none[1] = {nullptr};
        TraitsRider a(nullptr, 1, false), b(none, 1, true), c(none, GAUSS_TRAITS_MORE_MAX + 1, false);
        std::printf("refused %d", a.check()); std::printf(" %s\n", gauss_host_last_error());
        std::printf("refused %d", c.check()); std::printf(" %s\n", gauss_host_last_error());
        (void)b;
    }
    std::printf("plain %d\n", plain_calls);
}
'''


@pytest.fixture(scope="module")
def riders_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("riders")
    hdir = os.path.join(ROOT, "gauss_amd", "csrc", "host")
    src = tmp / "main.cpp"
    src.write_text(RIDERS_MAIN)
    exe = tmp / "riders"
    # the three translation units side by side, unoptimised: the instrumented build is most of this test's time
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
    """{column or 'named <name>': tokens} of one dumped table, and its column names in order."""
    mine = [ln.split()[1:] for ln in lines if ln.startswith(tag + " ")]
    assert mine and mine[0][0] == "cols"
    names = [c.split(":")[0] for c in mine[0][1:]]
    body = {}
    for tok in mine[1:]:
        key, vals = ("named " + tok[1], tok[2:]) if tok[0] == "named" else (tok[0], tok[1:])
        assert key not in body
        body[key] = vals
    return names, body, mine


IDENT = ["rsid", "chr", "bp", "a1", "a2"]
PLAIN = IDENT + ["af1mix", "z", "pval", "info", "type"]
HEX = float.fromhex


@pytest.mark.parametrize("tag", ["loo", "slct", "cond", "traits", "miss"])
def test_a_rider_builds_the_table_its_builder_gives_for_the_same_rows(riders_output, tag):
    """Five measured SNPs, two of them in the wings, three unmeasured ones, a 6-row table of the call's own: each rider's table(), on
    fixed result arrays, against loo_output / slct_output / cond_output / traits_output called on rows written out by hand -- the
    same column names and types, the same rows in the same order, every value and every named matrix to the bit."""
    got, want = _table(riders_output, tag + ".got")[2], _table(riders_output, tag + ".want")[2]
    assert got == want


def test_the_tables_are_the_ones_the_calls_document(riders_output):
    """... and what those tables are: names, row order and the values that show which SNP went where."""
    names, t, _ = _table(riders_output, "loo.got")
    assert names == IDENT + ["af1mix", "z", "z_loo", "info_loo", "t", "pval"]
    assert t["rsid"] == ["m1", "m3", "m4"] and t["bp"] == ["1001", "1003", "1004"]            # the wings' SNPs are not listed
    assert [HEX(x) for x in t["z_loo"][:1] + t["z_loo"][2:]] == [-1.5, 4.5] and t["z_loo"][1] == "nan"      # index = matrix row, not table row
    assert [HEX(x) for x in t["af1mix"]] == [1.25, 3.25, 4.25] and [HEX(x) for x in t["z"]] == [-0.5, 0.5, 1.0]
    names, t, _ = _table(riders_output, "slct.got")
    assert names == IDENT + ["af1mix", "z", "wing", "order", "z_entry", "z_joint", "z_cond", "pval_cond", "var_left"]
    assert t["rsid"] == ["m0", "m1", "m2", "m3", "m4"] and t["wing"] == ["1", "0", "1", "0", "0"] and t["order"] == ["0", "0", "1", "2", "0"]
    names, t, _ = _table(riders_output, "cond.got")
    assert names == PLAIN + ["wing", "order", "z_cond", "pval_cond", "var_left"]
    assert t["rsid"] == ["m1", "u0", "m3", "u1", "u2", "m4", "m0", "m2"]                      # the call's rows, then the wings in matrix order
    assert t["order"] == ["0", "0", "2", "0", "0", "0", "0", "1"] and t["named signals"][:2] == ["2", "3"]
    assert [HEX(x) for x in t["var_left"]] == [0.5, 0.625, 0.0, 0.05, 0.375, 0.875, 0.75, 0.0]
    for tag in ("traits", "miss"):
        names, t, _ = _table(riders_output, tag + ".got")
        assert names == PLAIN and t["rsid"] == ["m1", "u0", "m3", "u1", "u2", "m4"]
        z = [HEX(x) for x in t["named z_traits"][2:]]
        assert t["named z_traits"][:2] == ["6", "3"] and z[:6] == [1, 2, 3, 4, 5, 6]
        assert z[6:12] == [6.5 if tag == "miss" else 0.0, 1.25, 2.5, 2.25, 3.25, 3.5]
        assert z[12:] == [-1.5, -1.25, -3.5, -2.25, -3.25, -8.5 if tag == "miss" else 0.0]
    assert "named info_traits" not in _table(riders_output, "traits.got")[1]
    t = _table(riders_output, "miss.got")[1]
    assert [HEX(x) for x in t["named n_missing"][2:]] == [0, 2, 1]                            # the wing's SNP counts, and has no row
    assert [HEX(x) for x in t["named type_traits"][2:]][6:] == [0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 0]


def test_ask_sets_the_descriptor_and_refuses_what_the_window_shows(riders_output):
    lines = riders_output
    assert [ln for ln in lines if ln.startswith("loo ask")] == ["loo ask 0 5 1"]
    for u in (0, 1):
        tok = [ln for ln in lines if ln.startswith(f"slct{u} ask")][0].split()[2:]
        # rc, slct_max, forced: measured 3 then measured 0 (the caller's order), buffer sizes (cond: max(U, 1)), the pointers are the rider's
        assert tok[:9] == ["0", "4", "2", "3", "0", "4", "5", "3" if u else "0", "1"] and tok[9] == "1"
        assert HEX(tok[10]) == 1.0 - 0.9 / ((1.0 + 0.1) * (1.0 + 0.1)) and HEX(tok[11]) == ((1.0 - 0.9) if u else 0.0)
    refused = [ln for ln in lines if ln.startswith("refused")]
    assert all(ln.split()[1] == "-1" for ln in refused)
    assert "cond_rsids: m1 is listed twice" in refused[0]
    assert "cond_rsids: u0 is not a measured SNP of the extended window" in refused[1]
    assert "max_signals = 33: at most 32 signals are selected" in refused[2]
    assert "bad more_input_files" in refused[3]
    assert "further traits: a call takes at most" in refused[4]
    assert lines[-1] == "plain 6"            # cond, traits and miss asked the view for the call's own table once each, and so did the test


def test_one_window_calls_refuse_first_failure_first_on_every_panel_form(tmp_path, monkeypatch):
    """Up to its descriptor a one-window call needs no GPU.  A description file that is not there, an unknown
    population, a study file that is not there and a window with too few SNPs are refused in that order -- each call below has every
    later fault too -- with the same text on the text panel, on the packed panel (a lean window) and on the packed panel under
    GAUSS_HOST_FULL_MAP=1 (the literal data layer): by the plain call, a call with a rider, the joint fit, the LD scores and computeLD."""
    import ctypes
    import types
    from gauss_amd import api, panel
    pops = [("P00", 60, "EUR"), ("P01", 45, "ASN"), ("P02", 52, "EUR")]
    p = panel.make_synthetic_study(str(tmp_path), pops, n_snp=300, bp_lo=1_000_000, bp_hi=2_000_000, frac_measured=0.4, seed=5)["paths"]
    inp, idx, dat, desc = p["gwas.txt"], p["index.gz"], p["data.gz"], p["desc.txt"]
    gpk = str(tmp_path / "p.gpk")
    assert api.pack_panel(idx, dat, desc, gpk) > 0
    fake = types.SimpleNamespace(handle=ctypes.c_void_p(1))      # never dereferenced: every call is refused before the GPU is asked
    nofile, nodesc = str(tmp_path / "nothing.txt"), str(tmp_path / "nodesc.txt")
    wgt, bad_wgt = (["P00", "P01"], [0.5, 0.5]), (["P00", "XYZ"], [0.5, 0.5])
    empty = (22, 1_000_000, 1_000_001)                            # a window that holds no SNP
    calls = {                                                     # (who, input, desc) -> the call on (index, data)
        "dist": lambda who, f, d: lambda i, g: api.dist(*empty, 0, who[0], f, i, g, d, ctx=fake),
        "dist_susie": lambda who, f, d: lambda i, g: api.dist_susie(*empty, 0, who[0], f, i, g, d, ctx=fake),
        "distmix_traits": lambda who, f, d: lambda i, g: api.distmix_traits(*empty, 0, who[1], [f, f], i, g, d, ctx=fake),
        "dist_xsusie": lambda who, f, d: lambda i, g: api.dist_xsusie(*empty, 0, [who[0], "ASN"], [f, f], i, g, d, ctx=fake),
        "distmix_ldscore": lambda who, f, d: lambda i, g: api.distmix_ldscore(*empty, 0, who[1], f, i, g, d, ctx=fake),
        "computeLD": lambda who, f, d: lambda i, g: api.computeLD(*empty, who[1], f, i, g, d, ctx=fake),
    }
    few = {"distmix_ldscore": "LD scores: no SNP of .* the window has no SNP to score", "computeLD": "computeLD not performed \\(measured 0\\)",
           "distmix_traits": "Not enough number of SNPs loaded - DISTMIX not performed"}
    stages = [("no description file", (("XYZ", bad_wgt)), nofile, nodesc, lambda name: "nodesc.txt"),
              ("an unknown population", ("XYZ", bad_wgt), nofile, desc, lambda name: "XYZ"),
              ("no study file", ("EUR", wgt), nofile, desc, lambda name: "nothing.txt"),
              ("too few SNPs", ("EUR", wgt), inp, desc, lambda name: few.get(name, "Not enough number of SNPs loaded - DIST not performed"))]
    for name, make in calls.items():
        for what, who, f, d, want in stages:
            if what == "an unknown population" and name in ("distmix_traits", "distmix_ldscore", "computeLD"):
                continue                                          # (a weight under a name the panel lacks is ignored, not refused)
            call = make(who, f, d)
            said = []
            for index, data, full in ((idx, dat, "0"), ("(unused)", gpk, "0"), ("(unused)", gpk, "1")):
                monkeypatch.setenv("GAUSS_HOST_FULL_MAP", full)
                with pytest.raises(Exception, match=want(name)) as e:
                    call(index, data)
                said.append(str(e.value))
            assert said[0] == said[1] == said[2], (name, what, said)
