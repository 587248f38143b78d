"""CPU: the two numpy statements of the LD scores (tests/ldscore_ref.py) against each other and against closed forms.  The replayed
order and the masked np.sum differ by the rounding of a sum of at most M + U non-negative terms: 1e-12 relative holds them apart from
any real disagreement."""
import numpy as np
import pytest

import ldscore_ref as lr


def _random_case(M, U, seed, C=0, n_samples=300):
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 3, size=(M + U, n_samples)).astype(np.float64)
    G[:, 0], G[:, 1] = 0, 2                              # no monomorphic row
    R = np.atleast_2d(np.corrcoef(G))
    pick = np.sort(rng.permutation(M + U)[:M])
    rest = np.setdiff1d(np.arange(M + U), pick)
    bp = np.sort(rng.integers(1, 200_000, size=M + U))
    annot = None
    if C:
        annot = np.vstack([rng.integers(0, 2, size=M + U).astype(np.float64) if c % 2 == 0 else rng.normal(size=M + U) for c in range(C)])
        annot = np.hstack([annot[:, pick], annot[:, rest]])
    return R[np.ix_(pick, pick)], R[np.ix_(rest, pick)], bp[pick], bp[rest], annot


@pytest.mark.parametrize("M,U,radius,C", [(1, 0, 0, 0), (5, 3, 10_000, 2), (65, 130, 30_000, 3), (130, 63, 10 ** 9, 1), (64, 64, 0, 0),
                                           (70, 700, 20_000, 0)])
def test_the_two_statements_agree(M, U, radius, C):
    b11, b21, bm, bu, annot = _random_case(M, U, seed=M * 1000 + U, C=C)
    a = lr.replay(b11, b21, bm, bu, radius, 400.0, annot)
    b = lr.plain(b11, b21, bm, bu, radius, 400.0, annot)
    assert a["raw"].shape == (1 + C, M)
    for key in ("raw", "l2", "mass"):
        scale = np.maximum(np.abs(b[key]), 1.0) if key != "raw" else np.maximum(np.abs(b[key]), 1e-300)
        if C:       # a real-valued weight makes a sum of mixed signs: held against the sum of the absolute terms
            absw = lr.plain(b11, b21, bm, bu, radius, 400.0, np.abs(annot))
            scale = np.maximum(scale, np.abs(absw[key]))
        assert np.all(np.abs(a[key] - b[key]) <= 1e-12 * scale), key
    assert np.array_equal(a["mass"][0], lr.count(bm, bu, radius))
    assert np.array_equal(b["mass"][0], lr.count(bm, bu, radius))


def test_identical_rows_in_independent_blocks_score_their_block_size():
    """Blocks of b identical SNPs, the blocks uncorrelated: r^2 = 1 inside a block and 0 across, so raw = b whatever the split into
    measured and other rows"""
    sizes = [1, 3, 7, 70]
    blk = np.repeat(np.arange(len(sizes)), sizes)
    R = (blk[:, None] == blk[None, :]).astype(np.float64)
    S = len(blk)
    rng = np.random.default_rng(5)
    pick = np.sort(rng.permutation(S)[:40])
    rest = np.setdiff1d(np.arange(S), pick)
    bp = np.arange(S) * 10
    for f in (lr.replay, lr.plain):
        got = f(R[np.ix_(pick, pick)], R[np.ix_(rest, pick)], bp[pick], bp[rest], 10 ** 6, 100.0)
        assert np.array_equal(got["raw"][0], np.asarray(sizes, dtype=np.float64)[blk[pick]])
        assert np.array_equal(got["mass"][0], np.full(len(pick), float(S)))


def test_radius_zero_counts_both_snps_at_one_position():
    R = np.array([[1.0, 0.5, 0.25], [0.5, 1.0, 0.125], [0.25, 0.125, 1.0]])
    for f in (lr.replay, lr.plain):
        got = f(R[:2, :2], R[2:, :2], [100, 100], [101], 0, 50.0)
        assert np.array_equal(got["mass"][0], [2.0, 2.0])
        assert np.array_equal(got["raw"][0], [1.25, 1.25])
        got = f(R[:2, :2], R[2:, :2], [100, 100], [100], 0, 50.0)
        assert np.array_equal(got["mass"][0], [3.0, 3.0])
        assert np.array_equal(got["raw"][0], [1.0 + 0.25 + 0.0625, 0.25 + 1.0 + 0.015625])


def test_one_snp_alone_has_l2_exactly_one():
    for n in (3.0, 10.0, 503.0, 1e6):
        for f in (lr.replay, lr.plain):
            got = f(np.ones((1, 1)), None, [7], None, 0, n)
            assert got["raw"][0, 0] == 1.0 and got["mass"][0, 0] == 1.0
            assert got["l2"][0, 0] == 1.0, n


def test_a_row_outside_the_band_is_not_read_and_one_inside_is():
    """NaN in the LD of a far row reaches no target whose band misses it; inside the band it gives NaN, under a zero weight too"""
    b11 = np.eye(3)
    b21 = np.array([[np.nan, np.nan, np.nan]])
    annot = np.zeros((1, 4))
    for f in (lr.replay, lr.plain):
        got = f(b11, b21, [0, 50, 1000], [1010], 20, 100.0, annot)
        assert np.array_equal(np.isnan(got["raw"][0]), [False, False, True])
        assert np.array_equal(np.isnan(got["raw"][1]), [False, False, True])
        assert np.array_equal(got["raw"][0][:2], [1.0, 1.0]) and np.array_equal(got["mass"][0], [1.0, 1.0, 2.0])
        assert np.isnan(got["l2"][0, 2]) and np.all(np.isfinite(got["l2"][0, :2]))


def test_the_chunks_never_hold_rows_of_both_matrices():
    assert lr.chunks(65, 70, 64) == [(0, 64), (64, 65), (65, 129), (129, 135)]
    assert lr.chunks(1, 0, 64) == [(0, 1)]
    assert lr.chunks(64, 64, 64) == [(0, 64), (64, 128)]
