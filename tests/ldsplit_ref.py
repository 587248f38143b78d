"""Two numpy statements of the LD-splitting rule of include/gauss_hip.h (gauss_ld_split_rows), independent of each other.

(a) replay(): the rule literally -- per row the band, e = r * r, the reversed cumsum for S and the reversed running max for SM; per
    boundary the cumsum over k for T and the max for Mx; the dynamic programme as a loop with np.argmin (the first minimum: the
    smallest a).  np.cumsum of a 1-D array adds in index order, one rounding per step: the bits are the kernels'.
(b) cross_cost() / exhaustive(): for a given set of boundaries the sum of e over the band pairs whose ends lie in different blocks, by
    math.fsum (no order); for the optimum every admissible composition of M into K parts.  M <= 12 only."""
import itertools
import math

import numpy as np

INF = np.inf


def band_end(bp, i, W, radius):
    """one past the last band column of row i: j - i < W and bp_j - bp_i <= radius"""
    M = len(bp)
    hi = i + 1
    while hi < M and hi - i < W and int(bp[hi]) - int(bp[i]) <= radius:
        hi += 1
    return hi


def pair_values(R, bp, W, radius, thr_r2):
    """E (thresholded, 0 outside the band and where r is not finite), E0 (un-thresholded), hi [M], n_nonfinite"""
    M = len(bp)
    E, E0 = np.zeros((M, M)), np.zeros((M, M))
    hi = np.zeros(M, dtype=np.int64)
    bad = 0
    for i in range(M):
        hi[i] = band_end(bp, i, W, radius)
        for j in range(i + 1, int(hi[i])):
            r = R[i, j]
            if not np.isfinite(r):
                bad += 1
                continue
            e = r * r
            E0[i, j] = e
            E[i, j] = 0.0 if e < thr_r2 else e
    return E, E0, hi, bad


def replay(R, bp, radius, thr_r2, min_size, max_size, max_K, max_r2):
    """dict(cost [max_K], prev [max_K, M + 1] int32, max_r2 [M + 1], n_nonfinite, splits {K: ends or None})"""
    R = np.asarray(R, dtype=np.float64)
    M = R.shape[0]
    W = int(max_size)
    E, E0, hi, bad = pair_values(R, bp, W, radius, thr_r2)
    S, SM = np.zeros((M, M + 1)), np.zeros((M, M + 1))         # S[i][b], b = i + 1 .. hi_i; 0 from hi_i on
    for i in range(M):
        h = int(hi[i])
        if h > i + 1:
            S[i, i + 1:h] = np.cumsum(E[i, i + 1:h][::-1])[::-1]
            SM[i, i + 1:h] = np.maximum.accumulate(E0[i, i + 1:h][::-1])[::-1]
    T = np.zeros((M + 1, min(W, M) + 1))                         # T[b][k], k = 0 .. min(W, b)
    Mx = np.zeros(M + 1)
    for b in range(1, M + 1):
        kmax = min(W, b)
        ks = np.arange(1, kmax + 1)
        T[b, 1:kmax + 1] = np.cumsum(S[b - ks, b])
        Mx[b] = SM[b - ks, b].max()
    cost = np.full(max_K, INF)
    prev = np.full((max_K, M + 1), -1, dtype=np.int32)
    C = np.full(M + 1, INF)
    C[0] = 0.0
    for k in range(1, max_K + 1):
        Cn = np.full(M + 1, INF)
        for b in range(1, M + 1):
            if b < M and not Mx[b] <= max_r2:
                continue
            lo, up = max(0, b - int(max_size)), b - int(min_size)
            if up < lo:
                continue
            a = np.arange(lo, up + 1)
            v = C[a] + T[b, b - a]
            q = int(np.argmin(v))
            if v[q] < INF:
                Cn[b], prev[k - 1, b] = v[q], a[q]
        C = Cn
        cost[k - 1] = C[M]
    return dict(cost=cost, prev=prev, max_r2=Mx, n_nonfinite=bad, splits={k: backtrack(cost, prev, k) for k in range(1, max_K + 1)})


def backtrack(cost, prev, K):
    if not np.isfinite(cost[K - 1]):
        return None
    b = prev.shape[1] - 1
    ends = np.empty(K, dtype=np.int64)
    for k in range(K, 0, -1):
        ends[k - 1] = b
        b = int(prev[k - 1, b])
    assert b == 0
    return ends


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
def n_band_pairs(bp, max_size, radius):
    return int(sum(band_end(bp, i, int(max_size), radius) - i - 1 for i in range(len(bp))))


def cross_cost(R, bp, ends, radius, thr_r2, max_size):
    """the sum, by math.fsum, of e over the band pairs (i, j) that the boundaries `ends` (exclusive block ends, the last is M) put
    into different blocks; and the largest un-thresholded e among them"""
    R = np.asarray(R, dtype=np.float64)
    M = R.shape[0]
    block = np.zeros(M, dtype=np.int64)
    start = 0
    for k, e in enumerate(ends):
        block[start:int(e)] = k
        start = int(e)
    terms, top = [], 0.0
    for i in range(M):
        for j in range(i + 1, band_end(bp, i, int(max_size), radius)):
            if block[i] == block[j] or not np.isfinite(R[i, j]):
                continue
            e = float(R[i, j]) * float(R[i, j])
            top = max(top, e)
            if not e < thr_r2:
                terms.append(e)
    return math.fsum(terms), top


def compositions(M, K, min_size, max_size):
    """every way to write M as K ordered parts in min_size .. max_size, as tuples of block ends"""
    if K == 1:
        if min_size <= M <= max_size:
            yield (M,)
        return
    for cuts in itertools.combinations(range(1, M), K - 1):
        ends = cuts + (M,)
        sizes = np.diff((0,) + ends)
        if sizes.min() >= min_size and sizes.max() <= max_size:
            yield ends


def exhaustive(R, bp, K, radius, thr_r2, min_size, max_size, max_r2):
    """(best cost, [every split whose cost is within 1e-12 relative of it]) over the admissible compositions; (inf, []) for none"""
    assert len(bp) <= 12
    found = []
    for ends in compositions(len(bp), K, min_size, max_size):
        c, top = cross_cost(R, bp, ends, radius, thr_r2, max_size)
        if K > 1 and not top <= max_r2:
            continue
        found.append((c, ends))
    if not found:
        return INF, []
    best = min(c for c, _ in found)
    return best, [e for c, e in found if c - best <= 1e-12 * max(best, 1.0)]
