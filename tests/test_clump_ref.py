"""CPU: the two numpy statements of LD clumping (tests/clump_ref.py) against each other and against closed forms.  The outputs are
integers and copied products: every comparison is exact.  The definition they restate is the library's (include/gauss_hip.h); the
first test holds the two to the limits that header and binding state."""
import os

import numpy as np
import pytest

import clump_ref as cr

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "gauss_hip.h")


def test_the_header_states_the_definition_and_the_binding_its_limits():
    from gauss_amd import _lib, hotpath
    text = open(HEADER).read()
    for line in ("int gauss_ld_clump_rows(", "#define GAUSS_CLUMP_MAX_M    8192", "#define GAUSS_CLUMP_MAX_KEYS 64",
                 "if t2 >= r2_min: owner[j] = i;  r2[j] = t2", "it is LD pruning"):
        assert line in text, line
    assert (_lib.CLUMP_MAX_M, _lib.CLUMP_MAX_KEYS) == (8192, 64)
    assert callable(hotpath.ld_clump) and callable(hotpath.ld_clump_rows)


@pytest.mark.parametrize("block", range(6))
def test_the_two_statements_agree(block):
    """300 seeded cases: ties in key and position, NaN keys, a NaN row of R, r2_min on an entry's own square, 1 .. 3 traits"""
    for seed in range(block * 50, block * 50 + 50):
        c = cr.random_case(seed)
        a, b = cr.replay(**c), cr.plain(**c)
        assert cr.same(a, b), seed
        own = np.asarray(a["owner"])
        assert np.array_equal(own == -1, np.isnan(a["r2"])), seed
        assert np.array_equal(np.asarray(a["rank"]) > 0, own == np.arange(own.shape[-1])), seed


def _blocks(sizes):
    """block-diagonal LD of identical rows: r = 1 inside a block, 0 across"""
    M = sum(sizes)
    R, lab = np.zeros((M, M)), np.repeat(np.arange(len(sizes)), sizes)
    R[lab[:, None] == lab[None, :]] = 1.0
    return R, lab


def test_blocks_of_identical_rows_give_one_clump_each_led_by_the_largest_key():
    R, lab = _blocks([3, 1, 4])
    key = np.array([1.0, 9.0, 2.0, 5.0, 3.0, 3.5, 8.0, 1.5])
    out = cr.replay(R, np.arange(8) * 10, key, 1000, 0.5, 0.0, 0.0)
    assert out["n_clumps"] == 3
    assert out["owner"].tolist() == [1, 1, 1, 3, 6, 6, 6, 6]
    assert out["rank"].tolist() == [0, 1, 0, 3, 0, 0, 2, 0]
    assert np.all(out["r2"] == 1.0)
    assert cr.same(out, cr.plain(R, np.arange(8) * 10, key, 1000, 0.5, 0.0, 0.0))


def test_equal_keys_give_the_lead_to_the_lower_row():
    R, _ = _blocks([3])
    out = cr.replay(R, [5, 6, 7], [4.0, 4.0, 4.0], 10, 0.5, 1.0, 1.0)
    assert out["owner"].tolist() == [0, 0, 0] and out["rank"].tolist() == [1, 0, 0]


def test_the_first_index_keeps_a_snp_that_correlates_more_with_a_later_one():
    R = np.array([[1.0, 0.8, 0.1], [0.8, 1.0, 0.95], [0.1, 0.95, 1.0]])
    out = cr.replay(R, [1, 2, 3], [9.0, 1.0, 8.0], 10, 0.5, 0.0, 0.0)
    assert out["owner"].tolist() == [0, 0, 2] and out["r2"][1] == 0.8 * 0.8 and out["n_clumps"] == 2


def test_radius_zero_clumps_one_position_only():
    R, _ = _blocks([2])
    assert cr.replay(R, [7, 7], [2.0, 1.0], 0, 0.5, 0.0, 0.0)["owner"].tolist() == [0, 0]
    assert cr.replay(R, [7, 8], [2.0, 1.0], 0, 0.5, 0.0, 0.0)["owner"].tolist() == [0, 1]


def test_a_row_below_key_member_stays_out_and_its_neighbours_clump():
    R, _ = _blocks([3])
    out = cr.replay(R, [1, 2, 3], [9.0, 0.5, 3.0], 10, 0.5, 5.0, 1.0)
    assert out["owner"].tolist() == [0, -1, 0] and np.isnan(out["r2"][1]) and out["rank"].tolist() == [1, 0, 0]


def test_a_nan_key_or_a_nan_row_of_r_touches_nothing_else():
    R, _ = _blocks([4])
    base = cr.replay(R, [1, 2, 3, 4], [9.0, 1.0, 3.0, 2.0], 10, 0.5, 0.0, 0.0)
    out = cr.replay(R, [1, 2, 3, 4], [9.0, np.nan, 3.0, 2.0], 10, 0.5, 0.0, 0.0)
    assert out["owner"].tolist() == [0, -1, 0, 0] and out["n_clumps"] == 1 == base["n_clumps"]
    Rn = R.copy()
    Rn[2, :] = Rn[:, 2] = np.nan
    Rn[2, 2] = 1.0
    out = cr.replay(Rn, [1, 2, 3, 4], [9.0, 1.0, 3.0, 2.0], 10, 0.5, 0.0, 0.0)
    assert out["owner"].tolist() == [0, 0, 2, 0] and out["rank"].tolist() == [1, 0, 2, 0]      # it leads, and leads alone
    out = cr.replay(Rn, [1, 2, 3, 4], [1.0, 2.0, 9.0, 3.0], 10, 0.5, 0.0, 0.0)
    assert out["owner"].tolist() == [3, 3, 2, 3] and out["rank"].tolist() == [0, 0, 1, 2]


def test_r2_min_equal_to_an_entrys_own_square_includes_it():
    r = 0.3 + 2.0 ** -30
    R = np.array([[1.0, r], [r, 1.0]])
    assert cr.replay(R, [1, 2], [2.0, 1.0], 10, r * r, 0.0, 0.0)["owner"].tolist() == [0, 0]
    assert cr.replay(R, [1, 2], [2.0, 1.0], 10, np.nextafter(r * r, 1.0), 0.0, 0.0)["owner"].tolist() == [0, 1]


def test_key_index_above_every_key_gives_nothing():
    R, _ = _blocks([3])
    out = cr.replay(R, [1, 2, 3], [1.0, 2.0, 3.0], 10, 0.5, 4.0, 0.0)
    assert out["n_clumps"] == 0 and out["owner"].tolist() == [-1] * 3 and out["rank"].tolist() == [0] * 3 and np.all(np.isnan(out["r2"]))
    assert cr.same(out, cr.plain(R, [1, 2, 3], [1.0, 2.0, 3.0], 10, 0.5, 4.0, 0.0))


def test_every_trait_equals_its_own_run():
    c = cr.random_case(12345, M=30, T=3)
    all3 = cr.replay(**c)
    assert all3["owner"].shape == (3, 30) and all3["n_clumps"].shape == (3,)
    for t in range(3):
        one = cr.replay(**dict(c, key=c["key"][t]))
        assert cr.same(one, dict(owner=all3["owner"][t], rank=all3["rank"][t], r2=all3["r2"][t], n_clumps=all3["n_clumps"][t])), t
