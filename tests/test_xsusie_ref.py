"""CPU: the definition of the joint fine-mapping across studies (tests/xsusie_ref.py) -- the statement with every R_k formed explicitly
against the W form the kernels evaluate, an independent plain loop for measured_only, a group of identical studies against the
single-study fit it must sharpen, the planted window the feature rests on, and every group of tests/test_gpu_xsusie.py: the two
statements agree (their gap is the case's e_ref) and no decision is borderline, so that the GPU test may compare sizes, sets, kept
flags, sweeps and the joint candidate count exactly."""
import numpy as np
import pytest

import susie_ref as sr
import xsusie_ref as xr

E_REF_MAX = 1e-10         # as tests/test_susie_ref.py: what separates the statements is rounding carried through the sweeps


def vet(studies, maps, what, **kw):
    """Both statements on the CPU's matrices of the studies; returns the W-form result.  Exact outputs agree, nothing is borderline."""
    mats = [xr.mats_of(s) + (s["z1"],) for s in studies]
    a, b = xr.fit_textbook(mats, maps, **kw), xr.fit_w(mats, maps, **kw)
    e_ref = xr.gap(a, b)
    tol = xr.value_tol(b, e_ref)
    print(f"xsusie {what}: K {b['K']}  T {b['alpha'].shape[1]}  joint {b['xs_n']}  sweeps {b['sweeps']}  kept {int(b['kept'].sum())}  "
          f"sizes {b['size'].tolist()}  e_ref {e_ref:.2e}  tol {tol:.2e}  r_max {b['rmax']:.2f}")
    assert e_ref <= E_REF_MAX, (what, e_ref)
    for k in xr.EXACT_KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)
    assert np.array_equal(a["member"], b["member"]), what
    assert xr.borderline(b, kw, tol) == [], (what, xr.borderline(b, kw, tol))
    return b


@pytest.mark.parametrize("group", xr.SMALL_GROUPS, ids=lambda g: g[0])
def test_small_groups_are_committable(group):
    name, build, kw = group
    studies, maps = build()
    res = vet(studies, maps, name, **kw)
    if kw.get("tol", 1.0) == 0.0:
        assert res["sweeps"] == kw["max_sweeps"]
    else:
        assert 1 < res["sweeps"] < sr.DEFAULTS["max_sweeps"]
    if name == "permute-drop":
        assert res["xs_n"] == 15 and res["alpha"].shape[1] == 23
    if name == "T257-T255":
        assert res["xs_n"] == 255 and np.all(res["alpha"][:, -2:] == 0)
    if name == "peer-U1025":
        assert res["xs_n"] == 100 and maps[1].max() > 40 + 1024 - 1     # the peer's own order crosses SUSIE_CH = 1024 unmeasured SNPs
    if name == "measured-only":
        assert res["xs_n"] == 12 and np.all(res["alpha"][:, 12:] == 0)


def test_the_large_group_is_committable():
    studies, maps, kw = xr.large_group()
    vet(studies, maps, "chr22's largest shape, two studies", **kw)


def test_measured_only_is_the_plain_loop():
    for name, K, ev in (("two studies", 2, True), ("three studies, fixed V", 3, False)):
        studies, maps = xr.identity_group(12, 11, K, 14)
        kw = dict(L=3, tol=0.0, max_sweeps=4, estimate_var=ev, measured_only=True)
        res = vet(studies, maps, f"measured_only {name}", **kw)
        mats = [xr.mats_of(s) for s in studies]
        want = xr.plain_measured([s["z1"] for s in studies], [m[0] for m in mats], maps, 3, 25.0, 4, 0.0, ev)
        err = float(np.max(np.abs(res["alpha"][:, :12] - want)))
        print(f"xsusie measured_only {name}: |alpha - plain loop| {err:.2e}")
        assert err <= 1e-10
    # ... and through maps: the peer measures eight of the leader's twelve SNPs, in another order
    ids = [(np.arange(12), np.arange(12, 23)), (np.array([3, 1, 7, 0, 30, 9, 4, 11, 5, 31]), np.array([2, 6, 8, 10, 14, 20]))]
    studies, maps = xr.subset_group(ids, 31)
    kw = dict(L=2, tol=0.0, max_sweeps=4, measured_only=True)
    res = vet(studies, maps, "measured_only through a map", **kw)
    mats = [xr.mats_of(s) for s in studies]
    want = xr.plain_measured([s["z1"] for s in studies], [m[0] for m in mats], maps, 2, 25.0, 4, 0.0, True)
    assert res["xs_n"] == 8 and float(np.max(np.abs(res["alpha"][:, :12] - want))) <= 1e-10


def test_one_study_twice_is_not_one_study():
    """Two copies of one study: the same candidates and LD, twice the evidence -- the joint alpha is sharper than the single fit's,
    and every per-study quantity is the same in both copies"""
    studies, maps = xr.identity_group(12, 11, 1, 14)
    st = studies[0]
    B, C = xr.mats_of(st)
    res = vet([st, dict(st)], [None, None], "one study twice", L=3, tol=0.0, max_sweeps=5)
    one = sr.fit_w(B, C, st["z1"], L=3, tol=0.0, max_sweeps=5)
    assert np.array_equal(res["xs_V"][0], res["xs_V"][1]) and np.array_equal(res["xs_mu"][0], res["xs_mu"][1])
    assert res["alpha"][0].max() >= one["alpha"][0].max()


def test_a_nan_in_one_study():
    """A non-finite score in study 2: its unmeasured SNPs and that SNP are inadmissible there, and so jointly"""
    studies, maps = xr.identity_group(12, 11, 2, 14)
    studies[1]["z1"] = studies[1]["z1"].copy()
    studies[1]["z1"][5] = np.nan
    res = vet(studies, maps, "NaN in study 2", L=3, tol=0.0, max_sweeps=3)
    assert res["xs_n"] == 11 and not res["adm"][5] and not res["adm"][12:].any()
    assert np.all(res["alpha"][:, 5] == 0) and np.all(np.isfinite(res["pip"]))


def test_the_planted_window():
    """The acceptance case: each study alone cannot tell the causal SNP from its own ancestry's tag; the joint fit can"""
    studies, (causal, tagA, tagB) = xr.planted_window()
    kw = dict(L=5)
    alone = []
    for st, tag in zip(studies, (tagA, tagB)):
        B, C = xr.mats_of(st)
        r = B[causal, tag] / np.sqrt((B[causal, causal] - 0.1) * (B[tag, tag] - 0.1))      # (without the ridge lambda = 0.1)
        assert r > 0.97, r
        one = sr.fit_w(B, C, st["z1"], **kw)
        kept = np.flatnonzero(one["kept"])
        assert len(kept) == 1 and set(np.flatnonzero(one["member"][kept[0]])) == {causal, tag}, (kept, np.flatnonzero(one["member"][kept[0]]))
        alone.append(one["alpha"][kept[0]][[causal, tag]])
    rA = xr.mats_of(studies[1])[0]
    assert abs(rA[causal, tagA]) / np.sqrt(rA[causal, causal] * rA[tagA, tagA]) < 0.1      # tagA is loose in study B's ancestry
    res = vet(studies, [None, None], "planted window", **kw)
    kept = np.flatnonzero(res["kept"])
    print(f"xsusie planted window: alone {alone[0]} / {alone[1]}; joint alpha {res['alpha'][kept[0]][causal]:.6f} in {res['sweeps']} sweeps")
    assert len(kept) == 1 and list(np.flatnonzero(res["member"][kept[0]])) == [causal]
    assert res["alpha"][kept[0]][causal] > 0.99
