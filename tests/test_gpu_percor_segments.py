"""GPU suite: the per-population readers of the Gram slab -- pop_cor_kernel, pair_cor_kernel (k_pack_epilogue.hip) and
zm_partial_kernel / zm_final_kernel (k_zmix.hip) -- on populations that the planner cuts into SEVERAL K segments, against the exact
integer reference of tests/percor_ref.py.  The population tables sit on the planner's cuts (the rule is stated beside them in
percor_ref.py: 384 samples a segment for the every-pair calls at these sizes, 2 048 for a listed-pair call), the SNP counts on the
tile edges; tests/test_percor_ref.py checks on the CPU that the inputs are what they are meant to be.

Bounds (derived, not measured).  Correlations: numer and both variance terms are exact integers below 2^53 in fp64; the tail is
two square roots, one product and one division, each within 2^-53 relative (no contraction), the reference is rounded once:
|got - ref| <= 2^-50 |ref|, and the same NaN pattern.  Normal equations: summing n_rows products in any order errs by at most
gamma_n sum |x_a x_b|, every r carries at most 2^-50 relative error: 2 (n_rows 2^-53 + 2^-49) A_ab, the factor 2 for the
second-order terms; the kept-row count is decided by exact integers and must be equal.  Both Gram dtypes, a second run and another
cut of the same samples must give the same bits."""
import ctypes as C
import os

import numpy as np
import pytest

import percor_ref as pr
from gauss_amd import hotpath

pytestmark = pytest.mark.gpu

REL = 2.0 ** -50
_ip = C.POINTER(C.c_int32)
_dp = C.POINTER(C.c_double)
ALL_CASES = pr.EVERY_PAIR_CASES + pr.LISTED_CASES


def _ld_pairs(ctx, G, off, grp, pi, pj):
    """gauss_ld_per_pop_pairs: [n_group, n_pairs]."""
    off = np.ascontiguousarray(off, dtype=np.int32)
    P = len(off) - 1
    grp = None if grp is None else np.ascontiguousarray(grp, dtype=np.int32)
    ng = P if grp is None else int(grp.max()) + 1
    out = np.full((ng, len(pi)), -7.0)
    rc = ctx.lib.gauss_ld_per_pop_pairs(ctx.handle, G.ctypes.data, G.shape[0], G.strides[0], off.ctypes.data_as(_ip), P,
                                        None if grp is None else grp.ctypes.data_as(_ip), ng, pi.ctypes.data_as(_ip),
                                        pj.ctypes.data_as(_ip), len(pi), out.ctypes.data_as(_dp))
    assert rc == 0, ctx.lib.gauss_last_error()
    return out


def _bytes(v):
    return tuple(_bytes(x) for x in v) if isinstance(v, tuple) else np.asarray(v).tobytes()


def _both_dtypes(ctx, fn):
    """fn() under the f32 and the i8 Gram kernels (the slabs hold the same integers, as f32 or as int32 bit patterns): the same
    bits; returns the f32 result."""
    out = {}
    try:
        for dt in ("f32", "i8"):
            ctx.set_gram_dtype(dt)
            out[dt] = fn()
    finally:
        ctx.set_gram_dtype(os.environ.get("GAUSS_GRAM_DTYPE", "f32"))      # (back to the session's form)
    assert _bytes(out["f32"]) == _bytes(out["i8"]), "f32 and i8 Gram slabs gave different bits"
    return out["f32"]


def _labels(c, grouped):
    """A name for every output row: the samples of the population (or of the group's populations) with the segments they are cut
    into at 384 | 2 048 samples a segment."""
    pop = [f"{m}[{len(pr.segment_chunks(m, pr.SEG_EVERY_PAIR))}|{len(pr.segment_chunks(m, pr.SEG_LISTED))}]" for m in c["sizes"]]
    if not grouped:
        return pop
    return ["+".join(pop[p] for p in range(len(pop)) if c["grp"][p] == g) for g in range(int(c["grp"].max()) + 1)]


def _check_r(got, ref, what, labels):
    """The same NaN pattern, everything else finite and within 2^-50 relative; a failure names the rows (populations) it is in."""
    assert got.shape == ref.shape
    nan = np.isnan(ref)
    ok = ~nan & np.isfinite(got)
    err = np.where(ok, np.abs(got - np.where(nan, 0.0, ref)), 0.0)
    scale = np.where(ok, np.abs(ref), 0.0)
    worst = float(np.max(err[scale > 0] / scale[scale > 0])) if (scale > 0).any() else 0.0
    print(f"{what}: {int((~nan).sum())} finite, {int(nan.sum())} NaN, max rel err {worst:.3e} (bound {REL:.3e})")
    bad = [labels[g] for g in range(len(ref)) if not np.array_equal(np.isnan(got[g]), nan[g]) or not np.all(np.isfinite(got[g][~nan[g]]))
           or not np.all(err[g] <= REL * scale[g])]
    assert not bad, (what, "rows failing: samples[segments at 384|2048]", bad, worst)


@pytest.mark.parametrize("name", ALL_CASES)
def test_ld_per_pop_against_exact_reference(ctx, name):
    c = pr.case(name)
    got = _both_dtypes(ctx, lambda: hotpath.ld_per_pop(c["G"], c["off"], ctx=ctx))
    _check_r(got, pr.case_rows(name, False)[:, 1:].T, f"ld_per_pop {name}", _labels(c, False))


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("name", ALL_CASES)
def test_ld_per_pop_pairs_against_exact_reference(ctx, name, grouped):
    c = pr.case(name)
    G, off, S = c["G"], c["off"], c["S"]
    grp = c["grp"] if grouped else None
    pi, pj = pr.pair_list(S)
    idx = pr.pair_row_index(S, pi, pj)
    got = _both_dtypes(ctx, lambda: _ld_pairs(ctx, G, off, grp, pi, pj))
    _check_r(got, pr.case_rows(name, grouped)[idx, 1:].T, f"ld_per_pop_pairs {name} grouped={grouped}",
             _labels(c, grouped))
    if not grouped:
        # one population per group: gauss_ld_per_pop's bits on the same pairs, whichever way the populations were cut (384-sample
        # segments there, 2 048-sample segments here) and whether the groups are implied or spelled out
        every = hotpath.ld_per_pop(G, off, ctx=ctx)[:, idx]
        assert got.tobytes() == every.tobytes()
        own = _ld_pairs(ctx, G, off, np.arange(len(off) - 1, dtype=np.int32), pi, pj)
        assert got.tobytes() == own.tobytes()


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("name", ALL_CASES)
def test_zmix_normal_eq_against_exact_reference(ctx, name, grouped):
    c = pr.case(name)
    grp = c["grp"] if grouped else None
    run = lambda: hotpath.zmix_normal_eq(c["G"], c["off"], c["z"], pop_group=grp, ctx=ctx)
    xtx, xty, yty, n_rows = _both_dtypes(ctx, run)
    assert _bytes(run()) == _bytes((xtx, xty, yty, n_rows))                    # a second run: identical bytes
    want = pr.case_normal_eq(name, grouped)
    assert n_rows == want["n_rows"]                                            # finiteness is decided by exact integers
    assert np.array_equal(xtx, xtx.T)
    A = want["A"]
    bound = pr.normal_eq_bound(n_rows, A, factor=2.0)
    level = 0.0
    for got, ref, b, a in ((xtx, want["xtx"], bound[1:, 1:], A[1:, 1:]), (xty, want["xty"], bound[0, 1:], A[0, 1:]),
                           (np.array([yty]), np.array([want["yty"]]), bound[:1, 0], A[:1, 0])):
        err = np.abs(got - ref)
        level = max(level, float(np.max(err / np.maximum(a, 1e-300))))
        assert np.all(err <= b), (level, err, b)
    print(f"zmix_normal_eq {name} grouped={grouped}: {n_rows} rows kept of {c['S'] * (c['S'] - 1) // 2}, max |err| / A = {level:.3e} "
          f"(bound {2.0 * (n_rows * 2.0 ** -53 + 2.0 ** -49):.3e})")


@pytest.mark.parametrize("S", [129, 300])
def test_bits_do_not_depend_on_the_population_cut(ctx, S):
    """The 1 000-sample population alone (one segment in a listed-pair call, three in an every-pair call), and the same columns
    declared as three populations of 384 + 384 + 232 pooled into one group: identical bits."""
    c = pr.case(f"lead_1000-S{S}")
    assert c["sizes"][0] == 1000
    G = np.ascontiguousarray(c["G"][:, :1000])
    one, three, grp = np.array([0, 1000], dtype=np.int32), np.array([0, 384, 768, 1000], dtype=np.int32), np.zeros(3, dtype=np.int32)
    iu, ju = np.triu_indices(S, 1)
    pi, pj = iu.astype(np.int32), ju.astype(np.int32)

    def run():
        return (_ld_pairs(ctx, G, one, None, pi, pj), _ld_pairs(ctx, G, three, grp, pi, pj),
                hotpath.zmix_normal_eq(G, one, c["z"], ctx=ctx), hotpath.zmix_normal_eq(G, three, c["z"], pop_group=grp, ctx=ctx))

    r1, r3, z1, z3 = _both_dtypes(ctx, run)
    assert r1.shape == r3.shape == (1, len(pi)) and np.isfinite(r1).any() and np.isnan(r1).any()
    _check_r(r1, pr.case_rows(c["name"], False)[:, 1:2].T, f"ld_per_pop_pairs {c['name']} population 0 alone", ["1000[3|1]"])
    assert r1.tobytes() == r3.tobytes()
    assert r1.tobytes() == hotpath.ld_per_pop(G, one, ctx=ctx).tobytes()
    assert _bytes(z1) == _bytes(z3)
    assert 0 < z1[3] < len(pi)
