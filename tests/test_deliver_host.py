"""CPU: the delivery of a window's result sections (gauss_amd/csrc/gauss_deliver.h) as a stand-alone program under the sanitizers.
One window with every section present is delivered from a block with res[u] = u, so every output shows which doubles of the block it
took; the expected indices are written out here from the order documented above ResLayout and the sub-layouts (gauss_internal.h), not
taken from the library.  Then the two fills (not finite; multi-causal fit not made), a peer of a group and a window with the selection
alone."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gauss_amd", "csrc")

ST_CLAMPED, ST_NONFINITE, ST_SLCT_SKIPPED, ST_SUSIE_NOCONV, ST_SUSIE_NOFIT, ST_PRS_NOCONV = 1, 2, 8, 16, 32, 64

DBL = ("loo_z loo_info loo_t slct_zin slct_joint slct_zc slct_var cond_z cond_var cs_pip cs_set_pip cs_mass cs_lse susie_pip susie_set_pip susie_V "
       "susie_lse susie_mass susie_purity susie_alpha susie_mu susie_sweeps susie_lbf more_pip more_set_pip more_V more_lse more_mass more_purity "
       "more_alpha more_mu more_lbf more_sweeps coloc_pp coloc_hit_pp xs_V xs_purity xs_mu prs_beta prs_delta prs_br prs_bg prs_kkt z_more info_more "
       "z_miss info_miss").split()
INT = "slct_n slct_idx cs_set cs_size susie_set susie_size susie_kept more_set more_size more_kept more_status coloc_hit coloc_n xs_n prs_nnz prs_sweeps".split()

MAIN = r'''
#include "gauss_deliver.h"
#include <cstdio>
constexpr int CAP = 64;
constexpr double UNTOUCHED = -7777.0;
#define DBL_OUTS(X) ''' + " ".join(f"X({n})" for n in DBL) + r'''
#define INT_OUTS(X) ''' + " ".join(f"X({n})" for n in INT) + r'''
static void run(const char* label, Riders rd, int M, int U, int bits, bool repaired)
{
    std::vector<std::vector<double>> db;
    std::vector<std::vector<int32_t>> ib;
#define X(n) db.emplace_back(CAP, UNTOUCHED); rd.out.n = db.back().data();
    DBL_OUTS(X)
#undef X
#define X(n) ib.emplace_back(CAP, (int32_t)UNTOUCHED); rd.out.n = ib.back().data();
    INT_OUTS(X)
#undef X
    const ResLayout lay = rd.layout(U, M, U);
    std::vector<double> res(lay.count), z(CAP, UNTOUCHED), info(CAP, UNTOUCHED);
    for (size_t u = 0; u < res.size(); u++) res[u] = (double)u;
    const int got = deliver_window(res.data(), M, U, rd, z.data(), info.data(), bits, repaired);
    std::printf("case %s\nbits %d\ncount %zu\n", label, got, lay.count);
    auto line = [](const char* name, const double* v) { std::printf("%s", name); for (int e = 0; e < CAP && v[e] != UNTOUCHED; e++) std::printf(" %g", v[e]); std::printf("\n"); };
    auto iline = [](const char* name, const int32_t* v) { std::printf("%s", name); for (int e = 0; e < CAP && v[e] != (int32_t)UNTOUCHED; e++) std::printf(" %d", v[e]); std::printf("\n"); };
    line("z", z.data()); line("info", info.data());
#define X(n) line(#n, rd.out.n);
    DBL_OUTS(X)
#undef X
#define X(n) iline(#n, rd.out.n);
    INT_OUTS(X)
#undef X
    std::printf("res"); for (double v : res) std::printf(" %g", v); std::printf("\n");
}
int main()
{
    Riders all;
    all.loo = true;
    all.traits_T = 2; all.miss = true; all.miss_n = 3;
    all.slct_K = 2; all.cond = all.cs = true;
    all.susie_L = 2; all.susie_am = all.susie_lbf = true; all.susie_k = 1; all.coloc = true;
    all.xs_group = 1; all.xs_K = 2; all.xs_pos = 0; all.xs_mu = true;
    all.prs_n_s = 2; all.prs_n_lam = 2;
    run("all", all, 3, 2, 0, false);
    run("nonfinite", all, 3, 2, GAUSS_ST_NONFINITE, true);
    run("nofit", all, 3, 2, GAUSS_ST_CLAMPED, true);
    Riders peer;
    peer.susie_L = 2; peer.xs_group = 1; peer.xs_K = 2; peer.xs_pos = 1;
    run("peer", peer, 3, 2, 0, true);
    Riders slct;
    slct.slct_K = 2;
    run("slct", slct, 3, 2, 0, false);
}
'''

M, U, T, K, L, NT, NMISS, NS, NLAM, XK = 3, 2, 5, 2, 2, 2, 3, 2, 2, 2


def _expected():
    """name -> the block's indices it takes, for the window with every section; and the words no output takes."""
    want, at = {}, 0

    def take(name, n, stride=1, start=None):
        nonlocal at
        first = at if start is None else start
        want[name] = [first + stride * e for e in range(n)]
        if start is None:
            at += n

    take("z", U); take("info", U)
    take("loo_z", M); take("loo_info", M); take("loo_t", M)
    take("z_more", NT * U)
    take("info_more", NT * U); take("z_miss", NMISS); take("info_miss", NMISS)
    take("slct_n", 1); take("slct:skipped", 1); take("slct_idx", K); take("slct_zin", K); take("slct_joint", K); take("slct_zc", M); take("slct_var", M)
    take("cond_z", U); take("cond_var", U)
    take("cs_size", K); take("cs_mass", K); take("cs_lse", K); take("cs_pip", T); take("cs_set", T); take("cs_set_pip", T)

    def fit(pre):          # V, lse, size, mass, purity, kept [L]; fit [4]; pip, set, set_pip [T]; alpha, mu [L][T]
        for f in ("V", "lse", "size", "mass", "purity", "kept"):
            take(pre + f, L)
        take(pre + "sweeps", 2); take(pre + ":noconv", 1); take(pre + ":unused", 1)
        for f in ("pip", "set", "set_pip"):
            take(pre + f, T)
        take(pre + "alpha", L * T); take(pre + "mu", L * T)

    fit("susie_")
    take("susie_lbf", L * T)           # susie_more: trait 1's lbf, the further trait's block with its lbf behind it, then the one pair
    fit("more_")
    take("more_lbf", L * T)
    take("coloc_pp", 5 * L * L); take("coloc_hit", L * L); take("coloc_hit_pp", L * L); take("coloc_n", 1)
    take("xs_V", XK * L); take("xs_purity", XK * L); take("xs_n", 1); take("xs_mu", XK * L * T)
    nc = NS * NLAM         # cell [nc][8] = nnz, sweeps, delta, br, bg, kkt, noconv, unused; then beta [nc][M]
    for w, f in enumerate(("prs_nnz", "prs_sweeps", "prs_delta", "prs_br", "prs_bg", "prs_kkt", "prs:noconv", "prs:unused")):
        take(f, nc, stride=8, start=at + w)
    at += 8 * nc
    take("prs_beta", nc * M)
    return want, at


def _cases(text):
    cases, cur = {}, None
    for ln in text.strip().split("\n"):
        name, *vals = ln.split()
        if name == "case":
            cur = cases.setdefault(vals[0], {})
        elif name in ("bits", "count"):
            cur[name] = int(vals[0])
        else:
            cur[name] = [float(v) for v in vals]
    return cases


@pytest.fixture(scope="module")
def delivered(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("deliver")
    src = tmp / "main.cpp"
    src.write_text(MAIN)
    exe = tmp / "deliver"
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DGAUSS_LAYOUTS_ONLY",
                           "-I" + CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return _cases(out.stdout)


def test_every_output_takes_its_documented_doubles_and_the_block_is_covered_once(delivered):
    got = delivered["all"]
    want, count = _expected()
    assert count == 290 and got["count"] == count
    outs = {k: v for k, v in want.items() if ":" not in k}
    assert set(outs) == set(DBL + INT + ["z", "info"]) - {"more_status"}
    for name, idx in outs.items():
        assert got[name] == idx, name
    # res[u] = u makes every flag word non-zero: each raises its bit, the further trait's in its own status word
    assert got["bits"] == ST_SLCT_SKIPPED | ST_SUSIE_NOCONV | ST_PRS_NOCONV
    assert got["more_status"] == [ST_SUSIE_NOCONV]
    # every double of the block behind z and info is taken by exactly one output, but for the flag words that the status bits take
    # (the selection's skipped, each fit's word 2, each cell's word 6) and the two documented unused words (fit word 3, cell word 7)
    taken = sorted(i for name in outs if name not in ("z", "info") for i in got[name])
    rest = sorted(i for name, idx in want.items() if ":" in name for i in idx)
    assert len(rest) == 1 + 2 * 2 + 2 * NS * NLAM
    assert sorted(taken + rest) == list(range(2 * U, count))
    assert got["res"] == list(range(count))                   # a fitted, finite window's block is left as it is


def _same(got, want):
    return len(got) == len(want) and all((math.isnan(a) and math.isnan(b)) or a == b for a, b in zip(got, want))


def test_a_window_that_is_not_finite_is_nan_but_for_the_documented_sentinels(delivered):
    got, (want, count) = delivered["nonfinite"], _expected()
    assert got["bits"] == ST_NONFINITE and got["more_status"] == [ST_NONFINITE]
    nan = float("nan")
    sentinel = {"slct_n": 0, "slct_idx": -1, "cs_size": 0, "cs_set": -1, "prs_nnz": 0, "prs_sweeps": 0,
                "susie_size": 0, "susie_kept": 0, "susie_set": -1, "more_size": 0, "more_kept": 0, "more_set": -1,
                "coloc_hit": -1, "coloc_n": 0, "xs_n": 0}
    for name, idx in want.items():
        if ":" in name:
            continue
        if name in ("susie_sweeps", "more_sweeps"):
            assert _same(got[name], [0.0, nan]), name              # fit word 0 (sweeps run) = 0, the last delta NaN
        else:
            assert _same(got[name], [sentinel.get(name, nan)] * len(idx)), name
    res = got["res"]
    for name in ("slct:skipped", "susie_:noconv", "more_:noconv", "prs:noconv"):
        assert all(res[i] == 0.0 for i in want[name]), name
    assert all(math.isnan(res[i]) for name in ("susie_:unused", "more_:unused", "prs:unused") for i in want[name])


def test_a_repaired_window_keeps_its_sections_but_the_fit_is_not_made(delivered):
    got, (want, count) = delivered["nofit"], _expected()
    # the flag words outside the fit still hold res[u] = u; the fit's are 0
    assert got["bits"] == ST_CLAMPED | ST_SUSIE_NOFIT | ST_SLCT_SKIPPED | ST_PRS_NOCONV
    assert got["more_status"] == [ST_SUSIE_NOFIT]
    nan = float("nan")
    sentinel = {"size": 0, "kept": 0, "set": -1, "coloc_hit": -1, "coloc_n": 0, "xs_n": 0}
    for name, idx in want.items():
        if ":" in name:
            continue
        fit = name.startswith(("susie_", "more_", "coloc_", "xs_"))
        if not fit:
            assert got[name] == idx, name
        elif name.endswith("_sweeps"):
            assert _same(got[name], [0.0, nan]), name              # fit words 0 and 2 = 0
        else:
            key = name if name in sentinel else name.split("_", 1)[1]
            assert _same(got[name], [sentinel.get(key, nan)] * len(idx)), name
    res = got["res"]
    assert all(res[i] == 0.0 for name in ("susie_:noconv", "more_:noconv") for i in want[name])
    lo, hi = want["susie_V"][0], want["xs_mu"][-1] + 1
    assert res[:lo] == list(range(lo)) and res[hi:] == list(range(hi, count))      # nothing outside the fit's sections is touched


def test_absent_sections_take_nothing(delivered):
    peer = delivered["peer"]                     # a peer of a group returns nothing of the fit: z and info are its whole block
    assert peer["count"] == 2 * U and peer["bits"] == ST_SUSIE_NOFIT          # (a member of its group was repaired)
    assert peer["z"] == [0, 1] and peer["info"] == [2, 3]
    assert all(peer[name] == [] for name in DBL + INT)
    slct = delivered["slct"]
    assert slct["count"] == 2 * U + 2 + 3 * K + 2 * M and slct["bits"] == ST_SLCT_SKIPPED
    want = {"slct_n": [4], "slct_idx": [6, 7], "slct_zin": [8, 9], "slct_joint": [10, 11], "slct_zc": [12, 13, 14], "slct_var": [15, 16, 17]}
    for name in DBL + INT:
        assert slct[name] == want.get(name, []), name
