"""CPU: the two numpy statements of the LD-splitting rule (tests/ldsplit_ref.py) against each other, and the rule's corners.

replay() is the literal rule (scans and a dynamic programme), the one the kernels are held to bit for bit; cross_cost() / exhaustive()
sum the cross-block band pairs of a given split with math.fsum and try every composition.  1e-12 relative: a cost is a sum of at
most 66 values in [0, 1] in two different orders, each within 66 * 2^-53 = 7.3e-15 relative of the exact sum."""
import numpy as np
import pytest

import ldsplit_ref as lr

BIG = 1 << 40


def _sym(M, seed):
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1.0, 1.0, size=(M, M))
    R = np.triu(A, 1) + np.triu(A, 1).T + np.eye(M)
    bp = np.cumsum(rng.integers(0, 50, size=M)).astype(np.int32)
    return R, bp


def _close(a, b):
    return abs(a - b) <= 1e-12 * max(abs(b), 1.0)


@pytest.mark.parametrize("M", range(1, 13))
def test_the_dynamic_programme_finds_the_exhaustive_minimum(M):
    R, bp = _sym(M, 100 + M)
    for min_size, max_size, radius, thr, max_r2 in ((1, M + 3, BIG, 0.0, 1.0), (2, 5, BIG, 0.02, 1.0), (1, 4, 120, 0.1, 0.8), (3, 3, BIG, 0.0, 1.0)):
        got = lr.replay(R, bp, radius, thr, min_size, max_size, M + 1, max_r2)
        assert got["n_nonfinite"] == 0 and got["cost"].shape == (M + 1,)
        for K in range(1, M + 2):
            best, ties = lr.exhaustive(R, bp, K, radius, thr, min_size, max_size, max_r2)
            split = got["splits"][K]
            if not ties:
                assert np.isinf(got["cost"][K - 1]) and split is None, (M, K)
                continue
            assert _close(got["cost"][K - 1], best), (M, K, got["cost"][K - 1], best)
            assert tuple(int(e) for e in split) in ties, (M, K, split, ties)
            sizes = np.diff(np.concatenate([[0], split]))
            assert sizes.min() >= min_size and sizes.max() <= max_size and split[-1] == M


def test_exact_ties_go_to_the_smaller_a():
    # block-diagonal, zeros between the blocks: every boundary that does not cut a block costs exactly 0
    R = np.eye(8)
    R[0, 1] = R[1, 0] = R[4, 5] = R[5, 4] = 0.5
    bp = np.arange(8, dtype=np.int32)
    got = lr.replay(R, bp, BIG, 0.0, 1, 8, 3, 1.0)
    assert list(got["cost"]) == [0.0, 0.0, 0.0]
    # K = 2: the last block starts at the smallest free a: [0, 2) [2, 8); K = 3: a = 3 for the last block, then a = 2 is the only start
    # of a second block that costs nothing: [0, 2) [2, 3) [3, 8)
    assert list(got["splits"][2]) == [2, 8] and got["prev"][1, 8] == 2
    assert list(got["splits"][3]) == [2, 3, 8] and got["prev"][2, 8] == 3 and got["prev"][1, 3] == 2
    # among the splits of exactly equal cost the programme's is the one whose last block starts first, then the one before it, ...
    for K in range(2, 6):
        best, ties = lr.exhaustive(R, bp, K, BIG, 0.0, 1, 8, 1.0)
        assert best == 0.0 and len(ties) > 1
        full = lr.replay(R, bp, BIG, 0.0, 1, 8, K, 1.0)["splits"][K]
        assert tuple(int(e) for e in full) == min(ties, key=lambda ends: ends[::-1])
    # duplicated SNPs (rows 2 and 3 are one SNP at one position): cuts of equal cost up to rounding
    rng = np.random.default_rng(3)
    g = rng.normal(size=(5, 40))
    g = g[[0, 1, 2, 2, 3, 4]]
    R = np.corrcoef(g)
    bp = np.array([1, 2, 3, 3, 4, 5], dtype=np.int32)
    got = lr.replay(R, bp, BIG, 0.0, 1, 6, 6, 1.0)
    for K in range(1, 7):
        best, ties = lr.exhaustive(R, bp, K, BIG, 0.0, 1, 6, 1.0)
        assert _close(got["cost"][K - 1], best) and tuple(int(e) for e in got["splits"][K]) in ties


def test_infeasible_K_gives_inf_and_none():
    R, bp = _sym(10, 7)
    got = lr.replay(R, bp, BIG, 0.0, 3, 4, 6, 1.0)
    # 10 = 3 + 3 + 4 in three blocks; two blocks hold at most 8, four at least 12
    assert [np.isfinite(c) for c in got["cost"]] == [False, False, True, False, False, False]
    assert got["splits"][3] is not None and all(got["splits"][K] is None for K in (1, 2, 4, 5, 6))
    assert np.all(got["prev"][[0, 1, 3, 4, 5], 10] == -1)


def test_max_r2_forbids_a_boundary():
    R = np.eye(6)
    R[2, 3] = R[3, 2] = 0.9            # e = 0.81 spans boundary 3 only
    R[0, 1] = R[1, 0] = 0.1            # and the free split would cut at 3 were it not for the cheaper cuts: make every other cut dearer
    for i in range(5):
        if i != 2:
            R[i, i + 1] = R[i + 1, i] = 0.95
    bp = np.arange(6, dtype=np.int32)
    free = lr.replay(R, bp, BIG, 0.0, 1, 6, 2, 1.0)
    assert list(free["splits"][2]) == [3, 6] and free["max_r2"][3] == 0.9 * 0.9
    shut = lr.replay(R, bp, BIG, 0.0, 1, 6, 2, 0.5)
    assert np.isinf(shut["cost"][1]) and shut["splits"][2] is None           # every boundary spans a pair above 0.5
    R[0, 1] = R[1, 0] = 0.6            # boundary 1 now spans 0.36 only
    shut = lr.replay(R, bp, BIG, 0.0, 1, 6, 2, 0.5)
    assert list(shut["splits"][2]) == [1, 6] and shut["cost"][1] == 0.6 * 0.6
    assert np.all(shut["prev"][:, 3] == -1)


def test_threshold_radius_and_band_each_exclude_a_pair():
    """M = 5 in blocks of 2 .. 3: the two splits cut at 2 (cost e02 + e12 + e13) or at 3 (cost e13 + e23 + e24)"""
    R = np.eye(5)

    def put(i, j, e):
        R[i, j] = R[j, i] = np.sqrt(e)

    put(1, 2, 0.04), put(0, 2, 0.03), put(2, 3, 0.05), put(1, 3, 0.01), put(0, 1, 0.9), put(3, 4, 0.9)
    bp = np.array([0, 10, 20, 30, 40], dtype=np.int32)
    base = lr.replay(R, bp, BIG, 0.0, 2, 3, 2, 1.0)                      # 0.08 at 2 against 0.06 at 3
    assert list(base["splits"][2]) == [3, 5]
    for ends in ((2, 5), (3, 5)):
        assert _close(lr.cross_cost(R, bp, ends, BIG, 0.0, 3)[0], 0.08 if ends[0] == 2 else 0.06)
    thr = lr.replay(R, bp, BIG, 0.045, 2, 3, 2, 1.0)                     # only e23 is left: cutting at 2 is free
    assert list(thr["splits"][2]) == [2, 5] and thr["cost"][1] == 0.0
    near = lr.replay(R, bp, 10, 0.0, 2, 3, 2, 1.0)                       # neighbours only: e12 = 0.04 against e23 = 0.05
    assert list(near["splits"][2]) == [2, 5] and near["cost"][1] == R[1, 2] * R[1, 2]
    # j - i = 3 = max_size is outside the band: such a pair is cut by every admissible split, so it could only shift every cost by the
    # same constant and never change the optimum; it is not read at all -- not even a NaN there is counted
    for e in (0.5, np.nan):
        Q = R.copy()
        Q[0, 3] = Q[3, 0] = Q[1, 4] = Q[4, 1] = np.sqrt(e)
        got = lr.replay(Q, bp, BIG, 0.0, 2, 3, 2, 1.0)
        assert got["n_nonfinite"] == 0
        for name in ("cost", "prev", "max_r2"):
            assert np.array_equal(got[name], base[name]), name
    Q[0, 3] = Q[3, 0] = Q[1, 4] = Q[4, 1] = np.sqrt(0.5)
    wide = lr.replay(Q, bp, BIG, 0.0, 2, 4, 2, 1.0)                      # max_size = 4 takes them in: (0, 3) spans 1 .. 3, (1, 4) 2 .. 4
    assert list(wide["splits"][2]) == [3, 5] and _close(wide["cost"][1], base["cost"][1] + 1.0)
    assert wide["max_r2"][2] == Q[0, 3] * Q[0, 3]


def test_a_nan_row_is_counted_and_ignored():
    R, bp = _sym(9, 11)
    R[4, :] = R[:, 4] = np.nan
    R[4, 4] = 1.0
    got = lr.replay(R, bp, BIG, 0.0, 1, 4, 9, 1.0)
    # row 4's band pairs: (4, 5..7) and (1..3, 4)
    assert got["n_nonfinite"] == 6 and np.all(np.isfinite(got["max_r2"]))
    Z = np.where(np.isnan(R), 0.0, R)
    want = lr.replay(Z, bp, BIG, 0.0, 1, 4, 9, 1.0)
    for name in ("cost", "prev", "max_r2"):
        assert np.array_equal(got[name], want[name]), name
    for K in range(3, 10):
        best, ties = lr.exhaustive(R, bp, K, BIG, 0.0, 1, 4, 1.0)
        assert _close(got["cost"][K - 1], best) and tuple(int(e) for e in got["splits"][K]) in ties
