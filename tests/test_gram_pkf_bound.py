"""The sub-flush interval of the packed f32 Gram routine by the codes of the run (k_gram.hip: PK_F / PK_F_GENO), without a GPU.

The accumulator S + 4096 S' of two rows is exact while S and S' stay below 4096.  A 2-bit source CAN hold a 3 (product 9:
7 chunks of 64 samples, 9 * 448 = 4032), a genotype panel holds 0, 1, 2 (product 4: 15 chunks, 4 * 960 = 3840).  The pack
kernel tells the Gram launch of the same run which of the two holds."""
import os
import re

import numpy as np

KC = 64


def _packed_chain(a, a2, b, acc=0.0):
    """float32 chain acc = fma((a + 4096 a'), b, acc) in k order; every product here is an exact float32, so a rounded add is the fma."""
    fa = (a.astype(np.float32) + np.float32(4096.0) * a2.astype(np.float32)).astype(np.float32)
    acc = np.float32(acc)
    for x, y in zip(fa, b.astype(np.float32)):
        acc = np.float32(acc + np.float32(x * y))
        assert float(acc) == int(acc)              # every partial sum is an integer the format holds
    return acc


def _split(acc):
    u = int(acc)
    return u & 4095, u >> 12


def _segment(a, a2, b, interval):
    """A segment as the kernel walks it: the accumulator is split into the two rows' running sums every `interval` chunks and at the end."""
    lo = hi = 0
    for k0 in range(0, len(a), interval * KC):
        s = slice(k0, k0 + interval * KC)
        x, y = _split(_packed_chain(a[s], a2[s], b[s]))
        lo += x
        hi += y
    return lo, hi


def test_codes_up_to_2_are_exact_with_15_chunks_between_two_splits():
    n = 15 * KC
    two = np.full(n, 2)
    assert _split(_packed_chain(two, two, two)) == (4 * n, 4 * n) == (3840, 3840)      # the all-2 rows: every product is 4
    zero = np.zeros(n, dtype=int)
    assert _split(_packed_chain(two, zero, two)) == (3840, 0)
    assert _split(_packed_chain(zero, two, two)) == (0, 3840)
    rng = np.random.default_rng(15)
    for _ in range(10):
        a, a2, b = (rng.integers(0, 3, size=n) for _ in range(3))
        assert _split(_packed_chain(a, a2, b)) == (int(a @ b), int(a2 @ b))
    # a segment longer than one interval: 31 chunks = 15 + 15 + 1
    n = 31 * KC
    a, a2, b = (rng.integers(0, 3, size=n) for _ in range(3))
    assert _segment(a, a2, b, 15) == (int(a @ b), int(a2 @ b))
    two = np.full(n, 2)
    assert _segment(two, two, two, 15) == (4 * n, 4 * n)


def test_16_chunks_of_code_2_are_the_first_collision():
    n = 16 * KC
    assert 4 * n == 4096
    two = np.full(n, 2)
    assert _split(_packed_chain(two, two, two)) != (4 * n, 4 * n)
    # ... and only the last sample does it: one product less and the fields are still apart
    a = two.copy()
    a[-1] = 0
    assert _split(_packed_chain(a, two, two)) == (4 * n - 4, 4 * n)


def test_a_code_3_needs_the_short_interval():
    n = 15 * KC
    three = np.full(n, 3)
    assert 9 * n > 4096
    assert _segment(three, three, three, 15) != (9 * n, 9 * n)          # why the fallback exists
    assert _segment(three, three, three, 7) == (9 * n, 9 * n)
    # one row with 3s is enough: its products with a row of 2s are 6, and 6 * 960 = 5760
    two = np.full(n, 2)
    assert _segment(three, two, two, 15) != (6 * n, 4 * n)
    assert _segment(three, two, two, 7) == (6 * n, 4 * n)
    rng = np.random.default_rng(7)
    for _ in range(10):
        a, a2, b = (rng.integers(0, 4, size=n) for _ in range(3))
        assert _segment(a, a2, b, 7) == (int(a @ b), int(a2 @ b))


def test_both_intervals_follow_from_the_code_bound_in_the_kernel_source():
    shift = 12
    for code_max, f in ((3, 7), (2, 15)):
        assert ((1 << shift) - 1) // (code_max * code_max * KC) == f
        assert code_max * code_max * KC * f < (1 << shift) <= code_max * code_max * KC * (f + 1)
    src = open(os.path.join(os.path.dirname(__file__), "..", "gauss_amd", "csrc", "k_gram.hip")).read()
    assert re.search(r"constexpr int PK_CODE_GENO = 2;", src)
    assert "PK_F_GENO = ((1 << PK_SHIFT) - 1) / (PK_CODE_GENO * PK_CODE_GENO * KC)" in src
    assert re.search(r"static_assert\(PK_F_GENO == 15 && PK_CODE_GENO \* PK_CODE_GENO \* KC \* PK_F_GENO < \(1 << PK_SHIFT\)", src)
    assert re.search(r"static_assert\(PK_F == 7 && PK_CODE_MAX \* PK_CODE_MAX \* KC \* PK_F < \(1 << PK_SHIFT\)", src)


def test_the_pack_kernels_word_test_finds_exactly_the_threes():
    """(w & (w >> 1)) & 0x55555555 on a word of sixteen 2-bit codes (k_pack_epilogue.hip) is non-zero exactly when a code is 3."""
    rng = np.random.default_rng(2)
    for _ in range(200):
        codes = rng.integers(0, 3, size=16)
        w = int(sum(int(c) << (2 * i) for i, c in enumerate(codes)))
        assert (w & (w >> 1)) & 0x55555555 == 0
        codes[rng.integers(16)] = 3
        w = int(sum(int(c) << (2 * i) for i, c in enumerate(codes)))
        assert (w & (w >> 1)) & 0x55555555 != 0
