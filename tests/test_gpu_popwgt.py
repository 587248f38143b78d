"""GPU suite: afmix() / cpw2() -- the gauss_pop_weights kernel against a numpy restatement (eigh, the clamp rule, inv), the
whole entry points against the restated pipeline, recovery of a known mixture, and the afmix vignette's printed weights where
the 33KG panel is available."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

from gauss_amd import _lib, api, hotpath, panel

from popwgt_ref import ST_CLAMPED, ST_NONFINITE, finish, interval_weights, make_panel, pops_table

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _matrix(P, sizes, seed, dup=None, nan=None):
    """Interval-major AF-like rows: the study column a noisy mixture of the population columns.  dup: interval whose last
    population column repeats its first (exactly singular Cxx); nan: interval with one NaN row."""
    rng = np.random.default_rng(seed)
    blocks = []
    for i, n in enumerate(sizes):
        af = rng.uniform(0.05, 0.95, (n, P))
        if dup == i and P > 1:
            af[:, -1] = af[:, 0]
        w = rng.dirichlet(np.ones(P))
        study = np.clip(af @ w + rng.normal(0, 0.02, n), 0, 1)
        b = np.column_stack([study, af])
        if nan == i:
            b[n // 2, 1 + (P // 2)] = np.nan
        blocks.append(b)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.ascontiguousarray(np.vstack(blocks)), off


def _check(x, off, ctx):
    got, st = hotpath.pop_weights(x, off, ctx=ctx)
    want, wst, lmin = interval_weights(x, off)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want).any(1)
    assert np.all((st[~fin] & ST_NONFINITE) != 0) and np.all((st[fin] & ST_NONFINITE) == 0)
    for i in np.nonzero(fin)[0]:
        scale = max(1.0, float(np.max(np.abs(want[i]))))
        assert np.max(np.abs(got[i] - want[i])) <= 1e-8 * scale, (i, np.max(np.abs(got[i] - want[i])), scale)
    clear = fin & ((lmin < 0.5e-5) | (lmin > 2e-5))            # numpy's lambda_min clear of 1e-5
    assert np.array_equal(st[clear] & ST_CLAMPED, wst[clear] & ST_CLAMPED)
    return got, st, wst


@pytest.mark.parametrize("P", [1, 2, 26, 29, 64])
def test_kernel_against_numpy(P, ctx):
    small = max(2, P // 2)                                       # n_i < P: always clamped (for P > 2)
    sizes = [small, 2, 1, 40, 300, 1000, 700, 600]
    x, off = _matrix(P, sizes, seed=100 + P, dup=6, nan=7)
    got, st, wst = _check(x, off, ctx)
    assert np.isnan(got[2]).all() and np.isnan(got[7]).all()       # one row: 0 / 0; a NaN row
    if P > 2:
        assert st[0] & ST_CLAMPED and st[6] & ST_CLAMPED          # n_i < P; a duplicated population column
    assert not np.isnan(got[1]).any()                            # n_i = 2 is finite (rank one, clamped)


def test_kernel_split_reduction_of_a_long_interval(ctx):
    x, off = _matrix(29, [100_000, 3, 1000], seed=7)
    got, st, _ = _check(x, off, ctx)
    again, st2 = hotpath.pop_weights(x, off, ctx=ctx)
    assert got.tobytes() == again.tobytes() and np.array_equal(st, st2)


def test_kernel_refuses_more_than_64_populations(ctx):
    x, off = _matrix(65, [100], seed=1)
    lib = _lib.load()
    w = np.zeros(65)
    rc = lib.gauss_pop_weights(ctx.handle, x.ctypes.data_as(C.POINTER(C.c_double)), off.ctypes.data_as(C.POINTER(C.c_int64)), 1, 65,
                               1e-5, w.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert rc == -1
    assert b"64" in lib.gauss_last_error()


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def study(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("popwgt_gpu"))
    P = 5
    pn = make_panel(d, 3000, pops_table(P), seed=21)
    packed = os.path.join(d, "pw_packed.bin")
    api.pack_panel(pn["paths"]["index.gz"], pn["paths"]["data.gz"], pn["paths"]["desc.txt"], packed)
    rng = np.random.default_rng(4)
    w = np.array([0.4, 0.3, 0.2, 0.1, 0.0])
    idx = np.sort(rng.choice(3000, 2600, replace=False))
    rows = []
    for i in rng.permutation(idx):
        rsid, c, bp, a1, a2 = pn["snps"][i]
        af = float(np.clip(pn["af"][i] @ w + rng.normal(0, 0.03), 0.001, 0.999))
        if rng.random() < 0.15:
            a1, a2, af = a2, a1, 1 - af
        rows.append((rsid, c, bp, a1, a2, af))
    path = os.path.join(d, "study_af.txt")
    panel.write_study_af(path, *[[r[k] for r in rows] for k in range(6)])
    return dict(pn=pn, packed=packed, input=path, S=len(rows))


def _files(s, packed):
    p = s["pn"]["paths"]
    return (s["input"], p["index.gz"], s["packed"] if packed else p["data.gz"], p["desc.txt"])


@pytest.mark.parametrize("kind", ["afmix", "cpw2"])
def test_entry_points_against_the_restated_pipeline(study, kind, ctx, monkeypatch):
    monkeypatch.setenv("GAUSS_AUTO_PACK", "0")
    fn = getattr(api, kind)
    k = api.KIND_AFMIX if kind == "afmix" else api.KIND_CPW2
    res = {}
    for packed in (False, True):
        res[packed] = fn(*_files(study, packed), interval=10, ctx=ctx, detail=True)
    (df, det), (dfp, detp) = res[False], res[True]
    assert det["w_raw"].tobytes() == detp["w_raw"].tobytes() and det["w_interval"].tobytes() == detp["w_interval"].tobytes()
    assert df.equals(dfp)
    assert list(df.columns) == (["sup.pop", "pop", "wgt"] if kind == "afmix" else ["pop", "wgt"])
    _, x, off = api.popwgt_inputs(k, *_files(study, True), interval=10)
    w_int, _, _ = interval_weights(x, off)
    raw, rounded = finish(w_int)
    assert np.max(np.abs(det["w_raw"] - raw)) <= 1e-8
    pops = [p[0] for p in study["pn"]["pops"]]
    got = dict(zip(df["pop"], df["wgt"]))
    for p, r, wr in zip(pops, rounded, raw):
        near_mid = abs((wr * 1000) % 1 - 0.5) * 1e-3 <= 1e-8
        if near_mid:
            continue
        assert got.get(p, 0.0) == (r if r > 0 else 0.0), (p, got.get(p), r)
    if kind == "afmix":
        assert abs(got["P00"] - 0.4) < 0.05 and abs(got["P03"] - 0.1) < 0.05


def test_default_interval_is_1000(study, ctx, monkeypatch):
    monkeypatch.setenv("GAUSS_AUTO_PACK", "0")
    assert study["S"] >= 2000
    a, da = api.afmix(*_files(study, True), ctx=ctx, detail=True)
    b, db = api.afmix(*_files(study, True), interval=1000, ctx=ctx, detail=True)
    assert da["w_interval"].shape == (1000, 5)
    assert da["w_raw"].tobytes() == db["w_raw"].tobytes() and a.equals(b)


def test_intervals_of_one_snp_give_an_empty_frame(study, ctx, monkeypatch):
    monkeypatch.setenv("GAUSS_AUTO_PACK", "0")
    S = study["S"]
    for interval in (S - 3, S):
        df, det = api.afmix(*_files(study, True), interval=interval, ctx=ctx, detail=True)
        assert len(df) == 0 and np.isnan(det["w_raw"]).all()
        assert det["messages"] and f"{S} measured SNPs and interval = {interval}" in det["messages"][0]
        assert np.count_nonzero(det["status"] & ST_NONFINITE) == 2 * interval - S
    with pytest.raises(api.GaussError, match=rf"{S} measured SNPs and interval = {S + 1}"):
        api.cpw2(*_files(study, True), interval=S + 1, ctx=ctx)


def test_recovers_an_exact_mixture_and_feeds_distmix(tmp_path, ctx, monkeypatch):
    monkeypatch.setenv("GAUSS_AUTO_PACK", "0")
    d = str(tmp_path)
    P, n = 4, 5000
    pops = [(f"Q{k}", 20, ["AFR", "EUR", "EAS", "AMR"][k]) for k in range(P)]
    pn = make_panel(d, n, pops, seed=33, prefix="mix")
    w = np.array([0.55, 0.25, 0.15, 0.05])
    mix = pn["af"] @ w
    rs, cs, bps, a1s, a2s = zip(*pn["snps"])
    study = os.path.join(d, "mix_af.txt")
    panel.write_study_af(study, rs, cs, bps, a1s, a2s, mix)
    files = (study, pn["paths"]["index.gz"], pn["paths"]["data.gz"], pn["paths"]["desc.txt"])
    df = api.afmix(*files, interval=10, ctx=ctx)
    got = dict(zip(df["pop"], df["wgt"]))
    for k in range(P):
        assert abs(got.get(f"Q{k}", 0.0) - w[k]) <= 0.01, (k, got)
    # the weights as distmix's pop_wgt_df (first two columns: pop, wgt)
    rng = np.random.default_rng(2)
    meas = np.sort(rng.choice(np.arange(1000, 2000), 400, replace=False))
    gwas = os.path.join(d, "mix_z.txt")
    panel.write_gwas(gwas, [rs[i] for i in meas], [cs[i] for i in meas], [bps[i] for i in meas], [a1s[i] for i in meas],
                     [a2s[i] for i in meas], rng.standard_normal(len(meas)))
    lo, hi = bps[1200], bps[1700]
    out = api.distmix(7, lo, hi, 5000, df[["pop", "wgt"]], gwas, pn["paths"]["index.gz"], pn["paths"]["data.gz"],
                      pn["paths"]["desc.txt"], ctx=ctx)
    assert len(out) > 100 and np.isfinite(np.asarray(out["z"], dtype=float)).all()


KG = os.environ.get("GAUSS_33KG_DIR")


@pytest.mark.skipif(not KG, reason="set GAUSS_33KG_DIR to the 33KG panel (33kg_index.gz, 33kg_geno.gz, 33kg_pop_desc.txt) "
                                   "to replay the afmix vignette")
def test_afmix_vignette_known_answers(ctx, tmp_path):
    ka = json.load(open(os.path.join(HERE, "golden", "afmix_known_answers.json")))
    study = tmp_path / "PGC2_Chr22_ilmn1M_AF1.txt"                # the study file ships gzip-compressed; afmix reads plain text
    with gzip.open(os.path.join(HERE, "golden", ka["input_file"])) as f:
        study.write_bytes(f.read())
    df = api.afmix(str(study), os.path.join(KG, "33kg_index.gz"),
                   os.path.join(KG, "33kg_geno.gz"), os.path.join(KG, "33kg_pop_desc.txt"), ctx=ctx)
    got = [(a, b, float(c)) for a, b, c in zip(df["sup.pop"], df["pop"], df["wgt"])]
    assert got == [(r["sup.pop"], r["pop"], r["wgt"]) for r in ka["afmix"]]
