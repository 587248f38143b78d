"""CPU side of the per-population correlation tests (tests/test_gpu_percor_segments.py holds the kernels): the exact reference
agrees with the loop-literal oracle and with numpy's normal equations at derived levels, and every input of the GPU tests is what
it is meant to be -- populations on the planner's cuts, SNP pairs in every kind of tile, rows dropped but not most of them."""
import math

import numpy as np
import pytest

import oracle
import percor_ref as pr
from gauss_amd import synth
from zmix_ref import normal_eq

REL = 2.0 ** -50


def _small(seed, sizes, S=40, mono=6):
    rng = np.random.default_rng(seed)
    pops = [(f"P{k}", m, f"S{k // 2}") for k, m in enumerate(sizes)]
    bp = np.sort(rng.choice(np.arange(1, 3000 * S), size=S, replace=False))
    G, _ = synth.synth_genotypes(bp, pops, seed=seed + 1)
    off = synth.pop_offsets(sizes)
    for s in rng.choice(S, size=mono, replace=False):
        k = int(rng.integers(len(sizes)))
        G[s, off[k]:off[k + 1]] = int(rng.integers(3))
    return np.ascontiguousarray(G, dtype=np.uint8), off, rng.standard_normal(S) * 2.0


def _agree(got, want, rel):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.all(np.isfinite(got[~np.isnan(got)])) and np.all(np.isfinite(want[~np.isnan(want)]))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    assert np.all(err <= rel * np.abs(want[ok])), float(np.max(err / np.maximum(np.abs(want[ok]), 1e-300)))
    return float(np.max(err / np.maximum(np.abs(want[ok]), 1e-300))) if ok.any() else 0.0


def test_reference_agrees_with_oracle_ungrouped():
    G, off, z = _small(11, [23, 40, 17, 64, 31])
    rows = pr.pair_rows(G, off, z)
    want = oracle.ld_per_pop(G, off)
    assert np.isnan(want).any() and not np.isnan(want).all(axis=1).any()
    print("ungrouped: max rel", _agree(rows[:, 1:].T, want, REL), "bound", REL)
    iu, ju = np.triu_indices(G.shape[0], 1)
    assert np.array_equal(rows[:, 0], z[iu] * z[ju])


def test_reference_agrees_with_oracle_grouped():
    """A group pooled = one population of the group's columns: Pearson's r does not depend on the order of the samples."""
    sizes, grp = [23, 40, 17, 64, 31, 12], [0, 1, 0, 2, 1, 0]
    G, off, z = _small(12, sizes)
    G[5, :] = 1                                                    # monomorphic in every group
    for p in (0, 2, 5):
        G[7, off[p]:off[p + 1]] = 2                                # one value over group 0: NaN there, finite elsewhere
    G[9, off[0]:off[1]], G[9, off[2]:off[3]] = 0, 2                # monomorphic in two populations of group 0, not in the group
    rows = pr.pair_rows(G, off, z, grp)
    cols = [np.concatenate([np.arange(off[p], off[p + 1]) for p in range(len(sizes)) if grp[p] == g]) for g in range(3)]
    pooled = np.ascontiguousarray(np.concatenate([G[:, c] for c in cols], axis=1))
    want = oracle.ld_per_pop(pooled, synth.pop_offsets([len(c) for c in cols]))
    print("grouped: max rel", _agree(rows[:, 1:].T, want, REL), "bound", REL)
    iu, ju = np.triu_indices(G.shape[0], 1)
    r = rows[:, 1:]
    assert np.isnan(r[(iu == 5) | (ju == 5)]).all()
    on7 = (iu == 7) | (ju == 7)
    assert np.isnan(r[on7, 0]).all() and np.isfinite(r[on7 & (iu != 5) & (ju != 5), 1:]).any()
    assert np.isfinite(r[(iu == 9) | (ju == 9), 0]).any()


def test_isqrt_and_decimal_statements_agree():
    G, off, _ = _small(13, [23, 40, 300])
    sums = pr.group_sums(G, off, [0, 1, 0])
    rng = np.random.default_rng(2)
    for _ in range(400):
        g, i, j = int(rng.integers(2)), int(rng.integers(40)), int(rng.integers(40))
        a = (sums["n"][g], sums["Sx"][g][i], sums["Sx"][g][j], sums["Sxx"][g][i], sums["Sxx"][g][j], sums["Sxy"][g][i, j])
        assert all(isinstance(v, int) for v in a)
        x, y = pr.exact_r(*a), pr.exact_r_decimal(*a)
        assert (math.isnan(x) and math.isnan(y)) or x == y, (a, x, y)
    assert pr.exact_r(10, 5, 5, 5, 5, 5) == 1.0 and pr.exact_r(4, 2, 2, 2, 2, 0) == -1.0
    assert math.isnan(pr.exact_r(4, 4, 2, 4, 2, 2))


@pytest.mark.parametrize("grp", [None, [0, 1, 0, 2, 1]])
def test_normal_eq_exact_agrees_with_numpy(grp):
    G, off, z = _small(14, [23, 40, 17, 64, 31], S=60)
    rows = pr.pair_rows(G, off, z, grp)
    ex = pr.normal_eq_exact(rows)
    D, d, yy, n = normal_eq(rows)
    assert ex["n_rows"] == n and 0 < n < len(rows)
    A = ex["A"]
    bound = pr.normal_eq_bound(n, A)
    for got, want, b in ((D, ex["xtx"], bound[1:, 1:]), (d, ex["xty"], bound[0, 1:]), (np.array(yy), np.array(ex["yty"]), bound[0, 0])):
        assert np.all(np.abs(got - want) <= b), float(np.max(np.abs(got - want) / b))
    assert np.all(A >= np.abs(np.block([[np.array([[ex["yty"]]]), ex["xty"][None, :]], [ex["xty"][:, None], ex["xtx"]]])))


def test_planner_rule_puts_the_tables_on_the_cuts():
    sc = pr.segment_chunks
    assert sc(384, 384) == [6] and sc(385, 384) == [4, 3] and sc(1000, 384) == [6, 6, 4]
    assert [sc(m, 384) for m in (17, 64, 130)] == [[1], [1], [3]]
    assert sc(2048, 2048) == [32] and sc(2049, 2048) == [17, 16] and sc(4200, 2048) == [22, 22, 22]
    assert [len(sc(m, 384)) for m in (2048, 2049, 4200)] == [6, 6, 11]
    assert pr.segment_ranges(385, 384) == [(0, 256), (256, 385)] and pr.segment_ranges(1000, 384) == [(0, 384), (384, 768), (768, 1000)]
    first, mid, last, two_multi, mixed = set(), set(), set(), 0, 0
    for table, (sizes, grp, seg_max) in pr.TABLES.items():
        assert sum(sizes) <= 10_000 and len(sizes) == len(grp) and sorted(set(grp)) == list(range(max(grp) + 1))
        for S in pr.SNP_COUNTS:
            assert S <= 300 and pr.seg_max_every_pair(S, sizes) == 384
        want = {384, 385, 1000, 17, 64, 130} if seg_max == 384 else {2048, 2049, 4200}
        assert want <= set(sizes)
        multi = [len(sc(m, seg_max)) > 1 for m in sizes]
        assert [m for m, f in zip(sizes, multi) if f] == [m for m in sizes if m in (385, 1000, 2049, 4200)]
        if multi[0]:
            first.add(seg_max)
        if multi[-1]:
            last.add(seg_max)
        if any(multi[1:-1]):
            mid.add(seg_max)
        per_group = [[f for f, g in zip(multi, grp) if g == k] for k in range(max(grp) + 1)]
        assert any(any(fs) and not all(fs) for fs in per_group), table          # a multi-segment population beside single ones
        two_multi += any(sum(fs) >= 2 for fs in per_group)
    assert first == mid == last == {384, 2048} and two_multi >= 2


@pytest.mark.parametrize("name", list(pr.CASES))
def test_case_is_what_it_is_meant_to_be(name):
    c = pr.case(name)
    G, off, grp, S = c["G"], c["off"], c["grp"], c["S"]
    assert G.shape == (S, sum(c["sizes"])) and G.dtype == np.uint8 and G.max() <= 2
    assert [int(off[p + 1] - off[p]) for p in range(len(c["sizes"]))] == c["sizes"]
    assert c["multis"] and c["singles"] and len(c["seg_mono"]) >= 1
    var = lambda v: int(v.min()) != int(v.max())
    for s, p, a, b in c["seg_mono"]:                                # one value inside the segment, polymorphic in the population
        assert p in c["multis"] and (a, b) in pr.segment_ranges(c["sizes"][p], c["seg_max"])
        assert not var(G[s, off[p] + a:off[p] + b]) and var(G[s, off[p]:off[p + 1]])
    for s, p in c["pop_mono"]:
        assert not var(G[s, off[p]:off[p + 1]])
    for s, g in c["grp_mono"]:
        assert not var(np.concatenate([G[s, off[p]:off[p + 1]] for p in range(len(grp)) if grp[p] == g]))
    iu, ju = np.triu_indices(S, 1)
    pi, pj = pr.pair_list(S)
    assert np.all(pi < pj) and pj.max() < S and len(set(zip(pi.tolist(), pj.tolist()))) == len(pi)
    listed = pr.pair_row_index(S, pi, pj)
    assert np.array_equal(iu[listed], pi) and np.array_equal(ju[listed], pj)
    for grouped in (False, True):
        rows = pr.case_rows(name, grouped)
        r = rows[:, 1:]
        assert np.all(np.isfinite(r) | np.isnan(r)) and np.all(np.abs(r[np.isfinite(r)]) <= 1.0)
        keep = np.isfinite(rows).all(axis=1)
        ne = pr.case_normal_eq(name, grouped)
        assert ne["n_rows"] == int(keep.sum())
        on = lambda s: (iu == s) | (ju == s)
        gcol = lambda p: int(grp[p]) if grouped else p
        for s, p, _, _ in c["seg_mono"]:                            # finite wherever the partner is
            assert np.isfinite(r[on(s), gcol(p)]).any()
        for s, g in c["grp_mono"]:
            cols = [g] if grouped else [p for p in range(len(grp)) if grp[p] == g]
            assert np.isnan(r[on(s)][:, cols]).all()
        if not grouped:
            for s, p in c["pop_mono"]:
                assert np.isnan(r[on(s), p]).all()
        if S == 2:                                                  # one pair: it cannot be both kept and dropped
            mono = bool(c["pop_mono"])
            assert mono == (c["name"].split("-")[0] in pr.S2_POP_MONO)
            assert keep.all() if (grouped or not mono) else (not keep.any() and np.isnan(r).sum() == 1)
            continue
        dropped = len(rows) - int(keep.sum())
        assert 1 <= dropped <= len(rows) // 2, (dropped, len(rows))
        # kept rows in a diagonal tile, an off-diagonal tile and the last (ragged) tile: among all pairs and among the listed ones
        for sel in (np.arange(len(rows)), listed):
            ti, tj, k = iu[sel] // pr.TILE, ju[sel] // pr.TILE, keep[sel]
            last = (S - 1) // pr.TILE
            assert (k & (ti == tj)).any() and (k & (ti != tj)).any() and (k & (tj == last)).any()
            assert (~k).any() or sel is listed
        tiles = set(zip((pi // pr.TILE).tolist(), (pj // pr.TILE).tolist()))
        if S == 300:
            assert tiles == {(0, 0), (0, 1), (0, 2), (1, 1), (2, 2)}      # (1, 2) is left out: only some tile pairs
            assert {(127, 128), (0, 299), (128, 129)} <= set(zip(pi.tolist(), pj.tolist()))
        else:
            assert tiles == {(0, 0), (0, 1)} and {(127, 128), (0, 128)} <= set(zip(pi.tolist(), pj.tolist()))
        assert (S % pr.TILE) != 0
