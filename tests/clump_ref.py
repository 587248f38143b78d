"""LD clumping (include/gauss_hip.h: gauss_ld_clump_rows) stated twice in numpy, for the tests to hold the library against.

`replay` is the header's loop, literal.  `plain` states the same rule another way: the rows sorted once, and boolean masks over a
precomputed band matrix of `R * R >= r2_min`.  tests/test_clump_ref.py holds the two equal; the outputs are integers and copied
products, so equal means equal."""
import numpy as np


def _one(R, bp, key, radius, r2_min, key_index, key_member):
    """replay for one trait: (owner, rank, r2, n)"""
    M = len(bp)
    owner = np.full(M, -1, dtype=np.int32)
    rank = np.zeros(M, dtype=np.int32)
    r2 = np.full(M, np.nan)
    n = 0
    order = [i for i in range(M) if key[i] >= key_index]                # (a NaN key compares false)
    order.sort(key=lambda i: (-key[i], i))
    for i in order:
        if owner[i] != -1:
            continue
        n += 1
        owner[i], rank[i], r2[i] = i, n, 1.0
        for j in range(M):
            if j == i or abs(int(bp[j]) - int(bp[i])) > radius or owner[j] != -1 or not key[j] >= key_member:
                continue
            t2 = R[i, j] * R[i, j]
            if t2 >= r2_min:
                owner[j], r2[j] = i, t2
    return owner, rank, r2, n


def _pack(outs, one):
    owner, rank, r2, n = (np.array(x) for x in zip(*outs))
    if one:
        return dict(owner=owner[0], rank=rank[0], r2=r2[0], n_clumps=int(n[0]))
    return dict(owner=owner, rank=rank, r2=r2, n_clumps=n.astype(np.int32))


def replay(R, bp, key, radius, r2_min, key_index, key_member):
    """The header's loop for every trait of key ([M] or [T, M]); dict(owner, rank, r2, n_clumps) shaped like hotpath.ld_clump's."""
    R, bp, key = np.asarray(R, dtype=np.float64), np.asarray(bp), np.asarray(key, dtype=np.float64)
    one = key.ndim == 1
    K = key.reshape(1, -1) if one else key
    return _pack([_one(R, bp, k, int(radius), float(r2_min), float(key_index), float(key_member)) for k in K], one)


def plain(R, bp, key, radius, r2_min, key_index, key_member):
    """The same rule from masks: C[i, j] says that lead i would take j (in its band, not itself, r^2 large enough -- a NaN is not);
    walking the rows in (key descending, row ascending) order, a free row above key_index takes every free, eligible row of its mask."""
    R, bp, key = np.asarray(R, dtype=np.float64), np.asarray(bp, dtype=np.int64), np.asarray(key, dtype=np.float64)
    one = key.ndim == 1
    K = key.reshape(1, -1) if one else key
    M = len(bp)
    with np.errstate(invalid="ignore"):
        R2 = R * R
        C = (np.abs(bp[:, None] - bp[None, :]) <= int(radius)) & (R2 >= r2_min) & ~np.eye(M, dtype=bool)
    outs = []
    for k in K:
        with np.errstate(invalid="ignore"):
            lead_ok, member_ok = k >= key_index, k >= key_member
        free = np.ones(M, dtype=bool)
        owner, rank, r2 = np.full(M, -1, dtype=np.int32), np.zeros(M, dtype=np.int32), np.full(M, np.nan)
        # lexsort: the last key is the primary one; NaN keys sort last and are not leads anyway
        idx = np.lexsort((np.arange(M), -np.where(np.isnan(k), -np.inf, k)))
        n = 0
        for i in idx[lead_ok[idx]]:
            if not free[i]:
                continue
            n += 1
            take = C[i] & free & member_ok
            take[i] = False
            owner[take], r2[take] = i, R2[i, take]
            owner[i], rank[i], r2[i] = i, n, 1.0
            free &= ~take
            free[i] = False
        outs.append((owner, rank, r2, n))
    return _pack(outs, one)


def same(a, b):
    """two results are equal: integers equal, r2 bit for bit (NaN where both are NaN)"""
    return (np.array_equal(a["owner"], b["owner"]) and np.array_equal(a["rank"], b["rank"]) and
            np.array_equal(np.asarray(a["n_clumps"]), np.asarray(b["n_clumps"])) and
            np.array_equal(np.isnan(a["r2"]), np.isnan(b["r2"])) and
            np.array_equal(np.nan_to_num(a["r2"], nan=-1.0), np.nan_to_num(b["r2"], nan=-1.0)))


def random_case(seed, M=None, T=None):
    """A seeded case with everything the rule can meet: tied keys, tied positions, NaN keys, a NaN row of R, r^2 exactly at r2_min"""
    rng = np.random.default_rng(seed)
    M = M or int(rng.integers(1, 41))
    T = T or int(rng.integers(1, 4))
    X = rng.standard_normal((M, 12))
    for i in range(1, M):
        if rng.random() < 0.5:
            X[i] = X[int(rng.integers(0, i))] + rng.standard_normal(12) * rng.choice([0.0, 0.3, 1.0])
    with np.errstate(invalid="ignore", divide="ignore"):
        R = np.corrcoef(X) if M > 1 else np.ones((1, 1))
    R = np.atleast_2d(R)
    if M > 3 and rng.random() < 0.3:
        d = int(rng.integers(0, M))
        R[d, :] = np.nan
        R[:, d] = np.nan
    np.fill_diagonal(R, 1.0)
    bp = np.sort(rng.integers(0, 3000, M)).astype(np.int32)
    key = np.round(rng.chisquare(1, (T, M)) * 4, int(rng.integers(0, 3)))      # rounded: ties
    key[rng.random((T, M)) < 0.05] = np.nan
    radius = int(rng.choice([0, 50, 400, 10_000]))
    r2_min = float(rng.choice([0.0, 0.2, 0.5, 0.8, 1.0]))
    if M > 1 and rng.random() < 0.3:
        i, j = rng.choice(M, 2, replace=False)
        if np.isfinite(R[i, j]):
            r2_min = min(float(R[i, j] * R[i, j]), 1.0)
    ki = float(rng.choice([0.0, 2.0, 6.0]))
    km = float(rng.choice([0.0, 1.0, ki])) if ki > 0 else 0.0
    return dict(R=R, bp=bp, key=key if T > 1 else key[0], radius=radius, r2_min=r2_min, key_index=ki, key_member=min(km, ki))
