"""The arithmetic behind the packed f32 Gram routine (k_gram.hip: chunk_mfma_packed), without a GPU.

The kernel feeds the fp32 MFMA -- bitwise a k-ordered fmaf chain -- the A operand a + 4096 a' of two rows and splits the
accumulator S + 4096 S' every PK_F = 7 chunks of 64 samples.  That is exact while S and S' stay below 4096; with codes <= 3
a sample adds at most 9, so 448 samples (9 * 448 = 4032) is the last multiple of a chunk that is safe."""
import numpy as np


def _packed_chain(a, a2, b):
    """float32 chain acc = fma((a + 4096 a'), b, acc) in k order; every product here is an exact float32, so a rounded add is the fma."""
    fa = (a.astype(np.float32) + np.float32(4096.0) * a2.astype(np.float32)).astype(np.float32)
    acc = np.float32(0.0)
    for x, y in zip(fa, b.astype(np.float32)):
        acc = np.float32(acc + np.float32(x * y))
    return acc


def _split(acc):
    u = int(acc)
    return u & 4095, u >> 12


def test_packed_accumulation_is_exact_up_to_448_samples_of_code_3():
    for n in (64, 447, 448):
        a = np.full(n, 3)
        assert _split(_packed_chain(a, a, a)) == (9 * n, 9 * n)
    rng = np.random.default_rng(3)
    for _ in range(20):
        a, a2, b = (rng.integers(0, 4, size=448) for _ in range(3))
        assert _split(_packed_chain(a, a2, b)) == (int(a @ b), int(a2 @ b))


def test_packed_accumulation_first_fails_where_the_bound_says():
    """9 n < 4096 holds up to n = 455; at 456 samples of code 3 the low row's sum (4104) runs into the high row's field."""
    a = np.full(455, 3)
    assert _split(_packed_chain(a, a, a)) == (9 * 455, 9 * 455)
    a = np.full(456, 3)
    assert 9 * 456 == 4104
    assert _split(_packed_chain(a, a, a)) != (9 * 456, 9 * 456)


def test_sub_flush_interval_follows_from_the_code_bound():
    """PK_F of k_gram.hip: the largest number of 64-sample chunks whose sum of products of codes <= 3 stays below 2^12, and the
    whole accumulator then stays an exact float32 integer (below 2^24)."""
    import os
    import re
    kc, code_max, shift = 64, 3, 12
    f = ((1 << shift) - 1) // (code_max * code_max * kc)
    assert f == 7 and code_max * code_max * kc * f < (1 << shift) <= code_max * code_max * kc * (f + 1)
    assert ((1 << shift) - 1) * ((1 << shift) + 1) < 1 << 24
    src = open(os.path.join(os.path.dirname(__file__), "..", "gauss_amd", "csrc", "k_gram.hip")).read()
    assert re.search(r"constexpr int PK_SHIFT = 12;", src) and re.search(r"constexpr int PK_CODE_MAX = 3;", src)
    assert "PK_F = ((1 << PK_SHIFT) - 1) / (PK_CODE_MAX * PK_CODE_MAX * KC)" in src
    # a 16-bit-slab segment (gauss_plan.cpp: at most 7168 samples) fits the running registers' 16-bit halves
    assert code_max * code_max * 7168 < 1 << 16
