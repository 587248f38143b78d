"""CPU: the plumbing of the polygenic score weights that a GPU-less machine can check -- the C ABI's window descriptor and its ctypes
mirror, the host entry points, the hotpath's key, and PrsRider's ask() / table() on a hand-made WindowView (a stand-alone program under
the address and undefined-behaviour sanitizers; nothing is loaded into Python)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import desc_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRS_FIELDS = ["prs_n_s", "prs_n_lam", "prs_s", "prs_lam", "prs_n", "prs_tol", "prs_max_sweeps", "out_prs_beta", "out_prs_nnz",
              "out_prs_sweeps", "out_prs_delta", "out_prs_br", "out_prs_bg", "out_prs_kkt"]


def test_window_descriptor_mirror_has_the_size_and_the_fields_of_the_header():
    from gauss_amd import _lib
    names = [f[0] for f in _lib.WindowDesc._fields_]
    at = names.index("prs_n_s")
    assert names[at: at + 14] == PRS_FIELDS and names[at + 14] == "out_z" and names[at - 1] == "min_abs_eig"      # between the window's inputs and its outputs
    assert [n for n in names if "prs_" in n] == PRS_FIELDS and names[-3:] == ["out_loo_z", "out_loo_info", "out_loo_t"]
    fields = ["min_abs_eig"] + PRS_FIELDS + ["out_z"]
    size, offs, _ = desc_layout(fields)
    assert ctypes.sizeof(_lib.WindowDesc) == size
    assert [getattr(_lib.WindowDesc, n).offset for n in fields] == offs
    # n_s and n_lam share a word; max_sweeps has one of its own: 1 + 1 + 4 + 1 + 7 words from min_abs_eig to out_z
    assert offs == sorted(offs) and offs[2] - offs[1] == 4 and offs[-1] - offs[0] == 8 * (1 + 1 + 4 + 1 + 7)
    hdr = open(os.path.join(ROOT, "include", "gauss_hip.h")).read()
    assert re.search(r"#define\s+GAUSS_ST_PRS_NOCONV\s+64\b", hdr) and _lib.ST_PRS_NOCONV == 64
    for name, v in (("S", _lib.PRS_MAX_S), ("LAM", _lib.PRS_MAX_LAM), ("SWEEPS", _lib.PRS_MAX_SWEEPS), ("M", _lib.PRS_MAX_M)):
        assert re.search(r"#define\s+GAUSS_PRS_MAX_%s\s+%d\b" % (name, v), hdr), name


def test_zero_initialised_descriptor_asks_for_nothing():
    from gauss_amd import _lib
    d = _lib.WindowDesc()
    assert d.prs_n_s == 0 and d.prs_n_lam == 0 and d.prs_max_sweeps == 0 and d.prs_n == 0.0
    assert not any(getattr(d, n) for n in PRS_FIELDS if n.startswith("out_") or n in ("prs_s", "prs_lam"))


def test_host_header_declares_and_api_binds_the_calls():
    from gauss_amd import api
    src = open(os.path.join(ROOT, "include", "gauss_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gauss_host_dist_prs", "gauss_host_distmix_prs"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in api.HOST_SYMBOLS
    assert callable(api.dist_prs) and callable(api.distmix_prs)
    h = api.load_host()                                   # builds on a GPU-less machine too; the symbols must be exported
    dp = ctypes.POINTER(ctypes.c_double)
    tail = [ctypes.c_double, dp, ctypes.c_int, dp, ctypes.c_int, ctypes.c_double, ctypes.c_int]
    for fn, plain in ((h.gauss_host_dist_prs, h.gauss_host_dist), (h.gauss_host_distmix_prs, h.gauss_host_distmix)):
        assert fn.argtypes[:-1] == plain.argtypes[:-1] + tail and fn.argtypes[-1] == plain.argtypes[-1]


def test_integration_snippet_compiles_against_the_header():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    subprocess.check_call([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi", "prs_snippet.cpp")])


def test_hotpath_sets_the_fields():
    from gauss_amd import _lib, hotpath
    gm, gu = np.zeros((5, 8), dtype=np.uint8), np.zeros((3, 8), dtype=np.uint8)
    mk = lambda prs: (lambda d: (d, hotpath._Win(d, dict(mode=0, geno_m=gm, geno_u=gu, pop_off=[0, 8], z1=np.zeros(5), lam=0.1, prs=prs))))(_lib.WindowDesc())
    d, w = mk(dict(n=1000))
    assert (d.prs_n_s, d.prs_n_lam, d.prs_max_sweeps, d.prs_n, d.prs_tol) == (4, 20, 100, 1000.0, 1e-4)
    assert [d.prs_s[k] for k in range(4)] == [0.2, 0.5, 0.9, 1.0]
    lam = [d.prs_lam[k] for k in range(20)]
    assert abs(lam[0] - 0.1) < 1e-15 and abs(lam[-1] - 0.001) < 1e-15 and np.allclose(np.diff(np.log(lam)), np.log(0.01) / 19)
    assert all(getattr(d, n) for n in PRS_FIELDS if n.startswith("out_")) and not d.slct_max and not d.susie_L
    r = w.result()
    assert r["prs_beta"].shape == (4, 20, 5) and r["prs_nnz"].dtype == np.int32 and r["prs_sweeps"].shape == (4, 20)
    assert all(r["prs_" + k].shape == (4, 20) for k in ("delta", "br", "bg", "kkt"))
    d, w = mk(dict(n=77.5, s=[1.0, 0.25], lam=[0.0], tol=0.0, max_sweeps=7))
    assert (d.prs_n_s, d.prs_n_lam, d.prs_max_sweeps, d.prs_n, d.prs_tol) == (2, 1, 7, 77.5, 0.0)
    assert [d.prs_s[0], d.prs_s[1], d.prs_lam[0]] == [1.0, 0.25, 0.0] and w.result()["prs_beta"].shape == (2, 1, 5)
    d, w = mk(None)
    assert d.prs_n_s == 0 and not d.out_prs_beta and "prs_beta" not in w.result()
    with pytest.raises(ValueError, match="prs_n_s = 0"):
        mk(dict(n=1000, s=[]))


def test_refusals_that_need_no_gpu(tmp_path):
    """A missing file is named before anything else happens, as by the other one-window calls."""
    import types
    from gauss_amd import api
    missing = str(tmp_path / "nothing.txt")
    fake = types.SimpleNamespace(handle=ctypes.c_void_p(1))      # never dereferenced: the files are looked at first
    with pytest.raises(Exception, match="nothing.txt"):
        api.dist_prs(22, 1, 2, 1, "EUR", missing, missing, missing, missing, 1000, ctx=fake)
    with pytest.raises(Exception, match="nothing.txt"):
        api.distmix_prs(22, 1, 2, 1, (["a"], [1.0]), missing, missing, missing, missing, 1000, s=[0.5], lam=[0.1, 0.01], ctx=fake)
    with pytest.raises(Exception, match="at most 8"):
        api.dist_prs(22, 1, 2, 1, "EUR", missing, missing, missing, missing, 1000, s=[0.5] * 9, ctx=fake)
    with pytest.raises(ValueError):
        api.dist_prs(22, 1, 2, 1, "EUR", missing, missing, missing, missing, 1000, lam=[], ctx=fake)


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
int main() {
    const char* mid[3] = {"m0", "m1", "m2"};
    const int wing[3] = {1, 0, 0};
    const double z[3] = {3.0, NAN, -4.0};
    WindowView v;
    v.mix = true;
    for (int i = 0; i < 3; i++) {
        const SnpIdent id{mid[i], 22, 1000 + i, "C", "T"};
        v.measured.push_back(ViewSnp{id, 0.25 + 0.125 * i, z[i], wing[i]});
    }
    v.row_m = {-1, 0, 1}; v.row_u = {};
    const double s[2] = {0.5, 1.0}, lam[3] = {0.25, 0.125, 0.0};
    for (int pass = 0; pass < 3; pass++) {
        PrsRider r(pass ? 27.0 : 1000.0, pass ? s : nullptr, pass ? 2 : 0, pass ? lam : nullptr, pass ? 3 : 0, pass ? 0.5 : NAN, pass ? 7 : 0);
        gauss_window_desc d;
        memset(&d, 0, sizeof(d));
        d.n_measured = 3; d.n_unmeasured = 2; d.lambda = 0.1;
        const int rc = r.check() || r.ask(d, v);
        std::printf("prs%d ask %d %d %d %d %zu %zu %zu %d %d %a %a %a %a %a %a\n", pass, rc, d.prs_n_s, d.prs_n_lam, d.prs_max_sweeps, r.beta.size(), r.nnz.size(),
                    r.kkt.size(), d.prs_s == r.s.data() && d.prs_lam == r.lam.data() && !d.slct_max && !d.susie_L,
                    d.out_prs_beta == r.beta.data() && d.out_prs_nnz == r.nnz.data() && d.out_prs_sweeps == r.sweeps.data() && d.out_prs_delta == r.delta.data() &&
                    d.out_prs_br == r.br.data() && d.out_prs_bg == r.bg.data() && d.out_prs_kkt == r.kkt.data(),
                    d.prs_n, d.prs_tol, d.prs_s[0], d.prs_s[d.prs_n_s - 1], d.prs_lam[0], d.prs_lam[d.prs_n_lam - 1]);
        if (pass == 0) continue;
        // n = 27: r = 3 / sqrt(25 + 9), 0 (frozen), -4 / sqrt(25 + 16); r_max = 4 / sqrt(41) = 0.6247; tol r_max = 0.3123
        if (pass == 1) {
            for (int c = 0; c < 6; c++) {
                for (int i = 0; i < 3; i++) r.beta[c * 3 + i] = i == 1 ? 0.0 : 0.5 * c + 0.125 * i;
                r.nnz[c] = c ? 2 : 1; r.sweeps[c] = c == 4 ? 7 : 2 + c; r.delta[c] = c == 4 ? 0.375 : 0.25;      // cell 4: above tol r_max, its sweeps ran out
                r.br[c] = 0.0625 * c; r.bg[c] = 0.03125 * c; r.kkt[c] = 0.015625 * c;
            }
        }                                                      // pass 2: the buffers as ask() left them -- a window that was not fitted
        gauss_table* got = nullptr;
        if (r.table(v, &got)) return 1;
        dump(pass == 1 ? "fit" : "nofit", *got);
        gauss_table_free(got);
    }
    const std::vector<double> many(33, 0.5);
    PrsRider big(1000.0, many.data(), 9, lam, 3, 0, 0), wide(1000.0, s, 2, many.data(), 33, 0, 0);
    std::printf("refused %d", big.check()); std::printf(" %s\n", gauss_host_last_error());
    std::printf("refused %d", wide.check()); std::printf(" %s\n", gauss_host_last_error());
}
'''


@pytest.fixture(scope="module")
def rider_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("prs_rider")
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
    """PrsRider::table() on fixed result arrays: one row per measured SNP of the extended window in matrix order, r from z and n (0 for
    the frozen SNP), `beta` and `grid` column-major, converged by the kernel's rule, the message when a cell ran its sweeps out."""
    names, t = _table(rider_output, "fit")
    assert names == ["rsid", "chr", "bp", "a1", "a2", "af1mix", "z", "r", "wing"]
    assert t["rsid"] == ["m0", "m1", "m2"] and t["wing"] == ["1", "0", "0"]
    r = [HEX(x) for x in t["r"]]
    assert r == [3.0 / np.sqrt(27.0 - 2.0 + 9.0), 0.0, -4.0 / np.sqrt(27.0 - 2.0 + 16.0)] and np.isnan(HEX(t["z"][1]))
    assert t["named beta"][:2] == ["6", "3"]
    beta = np.array([HEX(x) for x in t["named beta"][2:]]).reshape(3, 6).T      # column-major [6 x 3]
    assert np.array_equal(beta, np.array([[0.0 if i == 1 else 0.5 * c + 0.125 * i for i in range(3)] for c in range(6)]))
    assert t["named grid"][:2] == ["6", "9"]
    g = np.array([HEX(x) for x in t["named grid"][2:]]).reshape(9, 6).T
    assert np.array_equal(g[:, 0], [0.5] * 3 + [1.0] * 3) and np.array_equal(g[:, 1], [0.25, 0.125, 0.0] * 2)
    assert np.array_equal(g[:, 2], [1, 2, 2, 2, 2, 2]) and np.array_equal(g[:, 3], [2, 3, 4, 5, 7, 7])
    assert np.array_equal(g[:, 4], [0.25] * 4 + [0.375, 0.25]) and np.array_equal(g[:, 5], 0.0625 * np.arange(6))
    assert np.array_equal(g[:, 6], 0.03125 * np.arange(6)) and np.array_equal(g[:, 7], 0.015625 * np.arange(6))
    assert np.array_equal(g[:, 8], [1, 1, 1, 1, 0, 1]) and "ran its sweeps out" in " ".join(t["message"])
    names, t = _table(rider_output, "nofit")
    assert np.all(np.isnan([HEX(x) for x in t["named beta"][2:]])) and "was not fitted" in " ".join(t["message"])
    g = np.array([HEX(x) for x in t["named grid"][2:]]).reshape(9, 6).T
    assert np.all(g[:, 2:4] == 0) and np.all(g[:, 8] == 0) and np.all(np.isnan(g[:, 4:8]))


def test_ask_sets_the_descriptor_and_the_defaults(rider_output):
    tok = [ln for ln in rider_output if ln.startswith("prs0 ask")][0].split()[2:]
    # rc, n_s, n_lam, max_sweeps, buffer sizes (beta: cells x M; nnz, kkt: cells), the pointers are the rider's
    assert tok[:9] == ["0", "4", "20", "100", "240", "80", "80", "1", "1"]
    vals = [HEX(x) for x in tok[9:15]]
    assert vals[:4] == [1000.0, 1e-4, 0.2, 1.0] and abs(vals[4] - 0.1) < 1e-15 and abs(vals[5] - 0.001) < 1e-15
    tok = [ln for ln in rider_output if ln.startswith("prs1 ask")][0].split()[2:]
    assert tok[:9] == ["0", "2", "3", "7", "18", "6", "6", "1", "1"] and [HEX(x) for x in tok[9:15]] == [27.0, 0.5, 0.5, 1.0, 0.25, 0.0]
    refused = [ln for ln in rider_output if ln.startswith("refused")]
    assert refused[0].split()[1] == "-1" and "at most 8" in refused[0] and refused[1].split()[1] == "-1" and "at most 32" in refused[1]
