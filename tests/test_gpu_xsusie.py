"""GPU: the joint fine-mapping across the studies of a group (k_xsusie.hip) against its definition (tests/xsusie_ref.py) evaluated on the
B11 / B21 the GPU returns for every study.  alpha, mu, pip, set_pip, mass, lse, V, purity and every study's V, purity and mu are held
to max(10 e_ref, 2 K max(1, r_max^2) 1e-8) absolute (xsusie_ref.value_tol); sizes, set, kept, the sweeps and the count of joint
candidates are exact, and no decision of a case may be borderline.  Every case prints a REACHED line."""
import numpy as np
import pytest

import cs_ref
import susie_ref as sr
import xsusie_ref as xr
from gauss_amd import hotpath

pytestmark = pytest.mark.gpu

ST_CLAMPED, ST_NONFINITE, ST_NOCONV, ST_NOFIT = 1, 2, 16, 32
VALUE = (("susie_alpha", "alpha"), ("susie_mu", "mu"), ("susie_pip", "pip"), ("susie_set_pip", "set_pip"), ("susie_mass", "mass"),
         ("susie_lse", "lse"), ("susie_V", "V"), ("susie_purity", "purity"), ("xs_V", "xs_V"), ("xs_purity", "xs_purity"), ("xs_mu", "xs_mu"))
LEAD_KEYS = ("susie_pip", "susie_set", "susie_set_pip", "susie_V", "susie_lse", "susie_mass", "susie_purity", "susie_size", "susie_kept",
             "susie_sweeps", "susie_delta", "susie_alpha", "susie_mu", "xs_V", "xs_purity", "xs_mu", "xs_n")


def _wins(studies, maps, kw, group=1):
    out = []
    for k, st in enumerate(studies):
        q = dict(kw, group=group, want_alpha=True, want_mu=True)
        if maps[k] is not None:
            q["from_lead"] = maps[k]
        out.append(dict(st, susie=q))
    return out


def _job(ctx, wins, runs=1, want_mats=True):
    job = hotpath.Job(wins, ctx=ctx, want_mats=want_mats)
    for _ in range(runs):
        job.run()
    out = [job.fetch() for _ in range(runs)]
    out = [[{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()} for r in run] for run in out]
    job.close()
    return out if runs > 1 else out[0]


def _check(res, studies, maps, kw, what):
    """res: the group's results with b11 / b21.  The reference on the GPU's matrices, vetted again there."""
    mats = [(r["b11"], r["b21"], st["z1"]) for r, st in zip(res, studies)]
    tb, want = xr.fit_textbook(mats, maps, **kw), xr.fit_w(mats, maps, **kw)
    e_ref = xr.gap(tb, want)
    tol = xr.value_tol(want, e_ref)
    bl = xr.borderline(want, kw, tol)
    assert bl == [], (what, bl)
    got = res[0]
    e = {}
    for g, w in VALUE:
        p, q = np.asarray(got[g], dtype=np.float64), np.asarray(want[w], dtype=np.float64)
        assert p.shape == q.shape and np.array_equal(np.isnan(p), np.isnan(q)), (what, g)
        e[w] = float(np.nanmax(np.abs(p - q), initial=0.0))
    print(f"REACHED xsusie {what}: K {want['K']}  T {len(want['pip'])}  joint {want['xs_n']}  L {len(want['V'])}  sweeps {want['sweeps']}  "
          f"kept {int(want['kept'].sum())}  r_max {want['rmax']:.2f}  e_ref {e_ref:.2e}  " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"  (bound {tol:.2e})")
    assert max(e.values()) <= tol, (what, e, tol)
    assert np.array_equal(got["susie_size"], want["size"]), (what, got["susie_size"], want["size"])
    assert np.array_equal(got["susie_set"], want["set"]), what
    assert np.array_equal(got["susie_kept"] != 0, want["kept"]), (what, got["susie_kept"], want["kept"])
    assert got["susie_sweeps"] == want["sweeps"], (what, got["susie_sweeps"], want["sweeps"])
    assert got["xs_n"] == want["xs_n"], (what, got["xs_n"], want["xs_n"])
    assert abs(got["susie_delta"] - want["delta"]) <= tol
    conv = want["delta"] < sr.args_of(**kw)["tol"]
    for r in res:
        assert bool(r["status"] & ST_NOCONV) == (not conv and r is got), (what, r["status"])
        assert r["status"] & ~ST_NOCONV == 0
    for r in res[1:]:
        assert "susie_pip" not in r and "xs_V" not in r
    return want


@pytest.mark.parametrize("group", xr.SMALL_GROUPS, ids=lambda g: g[0])
def test_small_groups(ctx, group):
    name, build, kw = group
    studies, maps = build()
    _check(_job(ctx, _wins(studies, maps, kw)), studies, maps, kw, name)


def test_the_largest_window_of_chr22_in_two_studies(ctx):
    studies, maps, kw = xr.large_group()
    _check(_job(ctx, _wins(studies, maps, kw)), studies, maps, kw, "M=1213 U=2512 K=2, 5 sweeps")


def test_the_planted_window(ctx):
    """The acceptance case: each study alone reports {causal, its ancestry's tag}; the group reports {causal} with alpha > 0.99"""
    studies, (causal, tagA, tagB) = xr.planted_window()
    kw = dict(L=5)
    for st, tag in zip(studies, (tagA, tagB)):
        one = hotpath.impute_window(st["mode"], st["geno_m"], st["geno_u"], st["pop_off"], st["pop_wgt"], st["z1"], ctx=ctx,
                                    susie=dict(kw, want_alpha=True))
        kept = np.flatnonzero(one["susie_kept"])
        assert one["status"] == 0 and len(kept) == 1
        assert sorted(np.flatnonzero(one["susie_set"] == kept[0]).tolist()) == sorted((causal, tag))
        print(f"REACHED xsusie planted, study alone: set {sorted((causal, tag))}  alpha {one['susie_alpha'][kept[0]][[causal, tag]]}")
    res = _job(ctx, _wins(studies, [None, None], kw))
    _check(res, studies, [None, None], kw, "planted window")
    got = res[0]
    kept = np.flatnonzero(got["susie_kept"])
    assert len(kept) == 1 and np.flatnonzero(got["susie_set"] == kept[0]).tolist() == [causal]
    assert got["susie_alpha"][kept[0]][causal] > 0.99 and got["susie_size"][kept[0]] == 1
    print(f"REACHED xsusie planted, joint: set [{causal}]  alpha {got['susie_alpha'][kept[0]][causal]:.6f}  sweeps {got['susie_sweeps']}")


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_a_group_beside_other_windows_and_two_runs(ctx):
    """In a job that holds a group, a plain susie window and a plain window, the two windows outside the group return the bits they
    return in a job without the group; every member's z / info are those of the window alone; two runs give the same bits."""
    studies, maps = xr.subset_group(xr.permute_drop_ids(), 31)
    kw = dict(L=5, tol=0.0, max_sweeps=5)
    p, gm, gu, z1 = sr.small_window(63, 40, 12)
    fit = dict(mode=1, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=p["w"], z1=z1, susie=dict(L=4, max_sweeps=20, want_alpha=True))
    plain = dict(fit, susie=None)
    g = _wins(studies, maps, kw, group=7)
    runs = _job(ctx, [g[0], fit, g[1], plain], runs=2, want_mats=False)
    without = _job(ctx, [fit, plain], want_mats=False)
    for run in runs:
        _same(run[1], without[0], ("z", "info", "status", "susie_pip", "susie_set", "susie_set_pip", "susie_V", "susie_lse", "susie_mass", "susie_purity",
                                   "susie_size", "susie_kept", "susie_sweeps", "susie_delta", "susie_alpha", "susie_mu"))
        _same(run[3], without[1], ("z", "info", "status"))
        for k, st in zip((0, 2), studies):
            alone = hotpath.impute_window(st["mode"], st["geno_m"], st["geno_u"], st["pop_off"], st["pop_wgt"], st["z1"], ctx=ctx)
            _same(run[k], alone, ("z", "info"))
    _same(runs[0][0], runs[1][0], LEAD_KEYS)
    only = _job(ctx, g, want_mats=False)                          # ... and the group returns the same bits wherever it stands in a job
    _same(runs[0][0], only[0], LEAD_KEYS)


def test_permuting_a_peer_moves_nothing_beyond_the_bound(ctx):
    """The peer's rows in another order, with its map: the joint sums still run in leader order, so the leader's values move by no
    more than the bound (the peer's own solve sums in another order), and every exact output stays"""
    studies, maps = xr.subset_group(xr.permute_drop_ids(), 31)
    kw = dict(L=5, tol=0.0, max_sweeps=5)
    a = _job(ctx, _wins(studies, maps, kw))
    want = _check(a, studies, maps, kw, "before the permutation")
    rng = np.random.default_rng(8)
    st = studies[1]
    M, U = st["geno_m"].shape[0], st["geno_u"].shape[0]
    pm, pu = rng.permutation(M), rng.permutation(U)
    moved = dict(st, geno_m=np.ascontiguousarray(st["geno_m"][pm]), geno_u=np.ascontiguousarray(st["geno_u"][pu]), z1=st["z1"][pm])
    new_at = np.empty(M + U, dtype=np.int64)                      # old candidate -> new candidate
    new_at[pm] = np.arange(M)
    new_at[M + pu] = M + np.arange(U)
    m2 = np.where(maps[1] >= 0, new_at[np.maximum(maps[1], 0)], -1).astype(np.int32)
    b = _job(ctx, _wins([studies[0], moved], [None, m2], kw))
    tol = xr.value_tol(want, 0.0)
    for g, _ in VALUE:
        assert float(np.nanmax(np.abs(np.asarray(a[0][g]) - np.asarray(b[0][g])), initial=0.0)) <= tol, g
    _same(a[0], b[0], ("susie_size", "susie_set", "susie_kept", "susie_sweeps", "xs_n"))


def test_every_launch_form_returns_the_same_bits(ctx, monkeypatch):
    """The switches tests/test_gpu_susie.py cycles through, on a job of a group and a window outside it"""
    studies, maps = xr.subset_group(xr.permute_drop_ids(), 31)
    kw = dict(L=5, max_sweeps=20)
    p, gm, gu, z1 = sr.small_window(63, 40, 12)
    wins = _wins(studies, maps, kw) + [dict(mode=1, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=p["w"], z1=z1, susie=dict(L=4, want_alpha=True))]
    ref = _job(ctx, wins, want_mats=False)
    assert ref[0]["susie_kept"].any()
    switches = [dict(GAUSS_CHAIN_ASIDE="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2"),
                dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="0"), dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2", GAUSS_EPI_EARLY="0"),
                dict(GAUSS_SHARE_MEASURED="0"), dict(GAUSS_SHARE_MEASURED="2"), dict(GAUSS_NO_SHIFT_CERT="1"),
                dict(GAUSS_FUSED_SOLVE="0", GAUSS_CHAIN_ASIDE="0")]
    for sw in switches:
        with monkeypatch.context() as m:
            for k, v in sw.items():
                m.setenv(k, v)
            got = _job(ctx, wins, want_mats=False)
            _same(got[0], ref[0], LEAD_KEYS + ("z", "info", "status"))
            _same(got[1], ref[1], ("z", "info", "status"))
            _same(got[2], ref[2], ("z", "info", "status", "susie_pip", "susie_alpha"))


def test_a_clamped_member_leaves_the_whole_group_unfitted(ctx):
    """MakePosDef repairs the peer: NOFIT on every member, the leader's sections NaN / 0 / -1, every member's z / info and the rest of
    the job untouched"""
    p, gm, gu, z1 = cs_ref.clamped_window()
    M, U = gm.shape[0], gu.shape[0]
    bad = dict(mode=0, geno_m=gm, geno_u=gu, pop_off=p["off"], pop_wgt=None, z1=z1, lam=0.0)
    rng = np.random.default_rng(2)
    good = dict(bad, lam=0.1, z1=z1 + rng.standard_normal(M))
    other = dict(good, susie=dict(L=3, want_alpha=True))
    kw = dict(L=3)
    for order, at_bad in (((good, bad), 1), ((bad, good), 0)):
        res = _job(ctx, _wins(list(order), [None, None], kw) + [other], want_mats=False)
        alone = [hotpath.impute_window(0, gm, gu, p["off"], None, w["z1"], lam=w["lam"], ctx=ctx) for w in order]
        assert alone[at_bad]["status"] == ST_CLAMPED and alone[1 - at_bad]["status"] == 0
        for r, a in zip(res, alone):
            assert r["status"] == a["status"] | ST_NOFIT
            _same(r, a, ("z", "info"))
        lead = res[0]
        for k in ("susie_pip", "susie_set_pip", "susie_V", "susie_lse", "susie_mass", "susie_purity", "susie_alpha", "susie_mu", "xs_V", "xs_purity",
                  "xs_mu"):
            assert np.all(np.isnan(lead[k])), k
        assert np.all(lead["susie_size"] == 0) and np.all(lead["susie_kept"] == 0) and np.all(lead["susie_set"] == -1)
        assert lead["susie_sweeps"] == 0 and lead["xs_n"] == 0
        fit = hotpath.impute_window(0, gm, gu, p["off"], None, other["z1"], ctx=ctx, susie=other["susie"])
        _same(res[2], fit, ("z", "info", "status", "susie_pip", "susie_set", "susie_alpha", "susie_sweeps"))


def test_refusals(ctx):
    studies, maps = xr.subset_group(xr.permute_drop_ids(), 31)
    kw = dict(L=3)
    a, b = _wins(studies, maps, kw)
    job = lambda ws: hotpath.Job(ws, ctx=ctx)
    with pytest.raises(Exception, match="xs_group = 1 has 1 window"):
        job([a])
    five = [a] + [dict(b) for _ in range(4)]
    with pytest.raises(Exception, match="xs_group = 1 has 5 windows"):
        job(five)
    for key, bad, name in (("L", 4, "susie_L"), ("coverage", 0.9, "susie_coverage"), ("prior_var", 9.0, "susie_prior_var"), ("tol", 1e-3, "susie_tol"),
                           ("min_abs_corr", 0.4, "susie_min_abs_corr"), ("max_sweeps", 7, "susie_max_sweeps"), ("estimate_var", False, "susie_estimate_var"),
                           ("measured_only", True, "susie_measured_only")):
        with pytest.raises(Exception, match=f"window 1: {name} differs from the leader's"):
            job([a, dict(b, susie=dict(b["susie"], **{key: bad}))])
    # a peer with outputs of the fit: the descriptor is filled by hand, hotpath gives a peer none
    for field, pat in (("out_susie_pip", "out_susie_\\* on a peer"), ("out_xs_V", "out_xs_\\* on a peer")):
        buf = np.zeros(4096)
        with pytest.raises(Exception, match=pat):
            _raw_job(ctx, [a, b], lambda descs: setattr(descs[1], field, buf.ctypes.data_as(hotpath._dp)))
    with pytest.raises(Exception, match="coloc_traits_more = 1 in a group"):
        job([dict(a, z_more=np.zeros((1, 12)), susie=dict(a["susie"], traits=1)), b])
    T1 = 29
    for bad, pat in ((np.full(23, T1), "xs_from_lead\\[0\\] = 29 is neither -1 nor a candidate"), (np.full(23, -2), "xs_from_lead\\[0\\] = -2"),
                     (np.r_[3, 3, np.full(21, -1)], "xs_from_lead\\[0\\] = xs_from_lead\\[1\\] = 3")):
        with pytest.raises(Exception, match=pat):
            job([a, dict(b, susie=dict(b["susie"], from_lead=bad.astype(np.int32)))])
    with pytest.raises(Exception, match="xs_from_lead is NULL .* but n_measured / n_unmeasured = 9 / 20 differ from the leader's 12 / 11"):
        job([a, dict(b, susie={k: v for k, v in b["susie"].items() if k != "from_lead"})])
    with pytest.raises(Exception, match="xs_from_lead on the leader"):
        job([dict(a, susie=dict(a["susie"], from_lead=np.arange(23, dtype=np.int32))), b])
    with pytest.raises(Exception, match="xs_group = 1 .*needs susie_L > 0"):
        _raw_job(ctx, [a, b], lambda descs: setattr(descs[0], "susie_L", 0))
    with pytest.raises(Exception, match="xs_group = -1"):
        _raw_job(ctx, [a, b], lambda descs: setattr(descs[0], "xs_group", -1))
    with pytest.raises(Exception, match="xs_from_lead maps a group leader's candidates: it needs xs_group > 0"):
        _raw_job(ctx, [a, b], lambda descs: setattr(descs[1], "xs_group", 0))
    st = studies[0]
    with pytest.raises(Exception, match="a group .* is two or more windows of one job"):
        hotpath.impute_window(st["mode"], st["geno_m"], st["geno_u"], st["pop_off"], st["pop_wgt"], st["z1"], ctx=ctx, susie=dict(L=3, group=1))


def _raw_job(ctx, wins, poke):
    """A job whose descriptors `poke` alters before the library sees them: what hotpath itself never builds"""
    import ctypes as C
    real = ctx.lib.gauss_job_create

    class Lib:
        def __getattr__(self, name):
            return getattr(ctx.lib, name)

        def gauss_job_create(self, handle, descs, n, on_device, out):
            poke(descs)
            return real(handle, descs, n, on_device, out)

    class Ctx:
        lib, handle = Lib(), ctx.handle

    job = hotpath.Job(wins, ctx=Ctx())
    job.close()


def test_fine_map_studies_builds_the_maps(ctx):
    """hotpath.fine_map_studies from SNP ids: the result of the job its maps describe"""
    ids = xr.permute_drop_ids()
    studies, maps = xr.subset_group(ids, 31)
    kw = dict(L=5, tol=0.0, max_sweeps=5)
    got = hotpath.fine_map_studies([dict(st, ids_m=im, ids_u=iu) for st, (im, iu) in zip(studies, ids)], susie=dict(kw, want_alpha=True, want_mu=True),
                                   ctx=ctx)
    want = _job(ctx, _wins(studies, maps, kw), want_mats=False)[0]
    _same(got, want, LEAD_KEYS)
    assert np.array_equal(got["ids"], np.concatenate(ids[0])) and np.array_equal(got["joint"], maps[1] >= 0) and got["xs_n"] == 15
    assert np.array_equal(hotpath.xs_maps(np.concatenate(ids[0]), np.concatenate(ids[1])), maps[1])


# ---- the host entry points, files -> table -----------------------------------------------------------------------
WGT_B = (["aaa", "CCC", "eee", "FFF", "zzz"], [0.05, 0.5, 0.1, 0.4, 0.3])      # study B's mix of cs_ref.WGT's populations


@pytest.fixture(scope="module")
def two_studies(tmp_path_factory):
    """cs_ref's synthetic study and a second GWAS of the same trait on the same panel: a fifth of the first one's SNPs are not
    measured in it, the scores are related but its own"""
    import os
    from gauss_amd import api
    d = tmp_path_factory.mktemp("xsusie_study")
    files = cs_ref.study_files(d)
    lines = open(files[0]).read().split("\n")
    rng = np.random.default_rng(41)
    second = os.path.join(os.path.dirname(files[0]), "gwas_b.txt")
    with open(second, "w") as f:
        f.write(lines[0] + "\n")
        for k, ln in enumerate(x for x in lines[1:] if x.strip()):
            if k % 5 == 2:
                continue
            tok = ln.split()
            tok[5] = repr(0.8 * float(tok[5]) + 0.6 * float(rng.standard_normal()))
            f.write(" ".join(tok) + "\n")
    packed = os.path.join(os.path.dirname(files[2]), "panel.gpk")
    assert api.pack_panel(files[1], files[2], files[3], packed) > 0
    return dict(files=files, second=second, packed=packed)


def _feeder(inp, index, data, desc, who, cutoff, mix):
    """cs_ref.feeder_window for any study file and population argument"""
    from oracle import feeder_py as fp
    chr_, start_bp, end_bp, wing = cs_ref.STUDY_WINDOW
    pops = fp.read_ref_desc(desc)
    flags, w = fp.pop_flags_wgt(pops, *who) if mix else (fp.pop_flags(pops, who), None)
    lo, hi = start_bp - wing, end_bp + wing
    m = fp.read_input_z(inp, chr_, lo, hi, False)
    fp.read_reference_index(m, index, chr_, lo, hi, False)
    vec = fp.make_snp_vec(m, data, flags, cutoff, w)
    meas = [s for s in vec if s.type == 1]
    unme = [s for s in vec if s.type == 0 and start_bp <= s.bp <= end_bp]
    return dict(meas=meas, unme=unme, mode=1 if mix else 0, geno_m=fp._matrix(meas), geno_u=fp._matrix(unme), pop_off=fp._selected_off(pops, flags),
                pop_wgt=None if w is None else np.asarray(w, dtype=np.float64), z1=np.array([s.z for s in meas]))


@pytest.mark.parametrize("mix", [False, True])
def test_dist_xsusie_and_distmix_xsusie_end_to_end(ctx, two_studies, mix):
    """Two study files and two population arguments on a text and on a packed panel: the same table.  Its shared columns are study
    1's dist() / distmix() bit for bit; pip, cs, cs_pip, joint and `effects` are hotpath.fine_map_studies' result for the windows
    the oracle's data layer builds for the two studies, by rsid."""
    from gauss_amd import api
    win = cs_ref.STUDY_WINDOW
    inp, idx, dat, desc = two_studies["files"]
    inputs = [inp, two_studies["second"]]
    who = [cs_ref.WGT, WGT_B] if mix else ["EUR", "ASN"]
    cutoff = 0.02 if mix else 0.01
    fn, fn_plain = (api.distmix_xsusie, api.distmix) if mix else (api.dist_xsusie, api.dist)
    args = dict(L=6, coverage=0.9, max_sweeps=40)
    df = fn(*win, who, inputs, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx, **args)
    plain = fn_plain(*win, who[0], inp, idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)
    assert list(df.columns) == list(plain.columns) + ["wing", "pip", "cs", "cs_pip", "joint"]
    own = df.iloc[: len(plain)].reset_index(drop=True)
    for c in plain.columns:
        a, b = own[c], plain[c]
        assert np.array_equal(a.to_numpy(), b.to_numpy(), equal_nan=True) if a.dtype.kind == "f" else list(a) == list(b), c
    fw = [_feeder(f, idx, dat, desc, w, cutoff, mix) for f, w in zip(inputs, who)]
    number = {}
    ids = [(np.array([number.setdefault(s.rsid, len(number)) for s in q["meas"]]), np.array([number.setdefault(s.rsid, len(number)) for s in q["unme"]]))
           for q in fw]
    studies = [dict({k: q[k] for k in ("mode", "geno_m", "geno_u", "pop_off", "pop_wgt", "z1")}, ids_m=i[0], ids_u=i[1]) for q, i in zip(fw, ids)]
    hp = hotpath.fine_map_studies(studies, susie=dict(args, want_alpha=True), ctx=ctx, want_mats=True)
    maps = [None, hotpath.xs_maps(np.concatenate(ids[0]), np.concatenate(ids[1]))]
    crossed = int(np.sum((maps[1][: len(ids[0][0])] >= len(ids[1][0]))))
    assert crossed > 0 and 0 < hp["xs_n"] < len(hp["ids"])      # SNPs measured in study 1 and imputed in study 2; SNPs study 2 lacks
    by = {r: k for k, r in enumerate(df["rsid"])}
    rows = np.array([by[s.rsid] for s in fw[0]["meas"]] + [by[s.rsid] for s in fw[0]["unme"]])
    assert len(set(rows.tolist())) == len(rows) == len(df)
    assert np.array_equal(df["pip"].to_numpy()[rows], hp["susie_pip"]) and np.array_equal(df["cs_pip"].to_numpy()[rows], hp["susie_set_pip"])
    assert np.array_equal(df["cs"].to_numpy()[rows], hp["susie_set"] + 1)
    assert np.array_equal(df["joint"].to_numpy()[rows] != 0, hp["joint"])
    eff, fit = df.attrs["effects"], df.attrs["fit"]
    assert eff["V"].shape == (2, 6) and np.array_equal(eff["V"], hp["xs_V"], equal_nan=True) and np.array_equal(eff["purity"], hp["xs_purity"], equal_nan=True)
    assert np.array_equal(eff["size"], hp["susie_size"]) and np.array_equal(eff["kept"], hp["susie_kept"] != 0)
    assert np.array_equal(eff["row"], rows[np.argmax(hp["susie_alpha"], axis=1)])
    for k in ("lse", "mass"):
        assert np.array_equal(eff[k], hp["susie_" + k], equal_nan=True), k
    assert fit["sweeps"] == hp["susie_sweeps"] and fit["converged"] == (not hp["status"] & ST_NOCONV) and fit["delta"] == hp["susie_delta"]
    assert eff["kept"].any()
    print(f"REACHED xsusie table mix={mix}: T {len(hp['ids'])}  joint {hp['xs_n']}  measured-here-imputed-there {crossed}  kept {int(eff['kept'].sum())}  "
          f"sweeps {fit['sweeps']}")
    other = fn(*win, who, inputs, "(unused)", two_studies["packed"], desc, af1_cutoff=cutoff, ctx=ctx, **args)
    assert list(other.columns) == list(df.columns) and len(other) == len(df)
    for c in df.columns:
        a, b = df[c], other[c]
        assert np.array_equal(a.to_numpy(), b.to_numpy(), equal_nan=True) if a.dtype.kind == "f" else list(a) == list(b), c
    assert all(np.array_equal(other.attrs["effects"][k], eff[k], equal_nan=True) for k in eff) and other.attrs["fit"] == fit
    with pytest.raises(Exception, match="2 .. 4 studies"):
        fn(*win, who[:1], inputs[:1], idx, dat, desc, af1_cutoff=cutoff, ctx=ctx)


def test_the_whole_snp_map_on_a_packed_panel_gives_the_lean_windows_table(ctx, two_studies, monkeypatch):
    """GAUSS_HOST_FULL_MAP=1 on the packed panel (every study's window built by the literal data layer, rows from the packed store)
    against the same call without it (lean windows): the same frame, bit for bit, for dist_xsusie and distmix_xsusie"""
    from gauss_amd import api
    inp, _, _, desc = two_studies["files"]
    inputs = [inp, two_studies["second"]]
    for mix in (False, True):
        fn = api.distmix_xsusie if mix else api.dist_xsusie
        who = [cs_ref.WGT, WGT_B] if mix else ["EUR", "ASN"]
        call = lambda: fn(*cs_ref.STUDY_WINDOW, who, inputs, "(unused)", two_studies["packed"], desc, af1_cutoff=0.02 if mix else 0.01, ctx=ctx,
                          L=6, coverage=0.9, max_sweeps=40)
        lean = call()
        with monkeypatch.context() as m:
            m.setenv("GAUSS_HOST_FULL_MAP", "1")
            full = call()
        assert list(full.columns) == list(lean.columns) and len(full) == len(lean) > 0
        for c in lean.columns:
            a, b = lean[c], full[c]
            assert np.array_equal(a.to_numpy(), b.to_numpy(), equal_nan=True) if a.dtype.kind == "f" else list(a) == list(b), (mix, c)
        assert all(np.array_equal(full.attrs["effects"][k], v, equal_nan=True) for k, v in lean.attrs["effects"].items()), mix
        assert full.attrs["fit"] == lean.attrs["fit"]
