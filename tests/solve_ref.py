"""References and inputs for the window solve on an ill-conditioned B11 (k_solve.hip, k_solve_lite.hip, solve_kernel).  Plain
numpy / scipy / mpmath and Python integers, no GPU.

* truth_solve: B11^-1 [B21^T | z1] for the exact doubles passed in, by iterative refinement whose residual is formed exactly
  (a double is an integer times a power of two; numpy object arrays of Python integers in fixed point) until it is below
  1e-30, and z and info from it by the oracle's formulas (dist.cpp:193-202 as oracle.run_impute states them), the sums exact,
  the square root and the quotient in mpmath.
* chol_route: the kernel's own algebra in fp64 with LAPACK -- L = chol(B11), X = L^-1, y = X z1, w_u = X b21_u^T,
  z_u = w_u . y / sqrt(info_u), info_u = w_u . w_u.  Its error against the truth is the yardstick of the GPU's bounds.
* chol_route_blocked: the same algebra in 64-row factor blocks with reciprocal-square-root pivots, stated so that single
  steps can be made subtly wrong (MUTATIONS); tests/test_solve_ref.py shows that the bounds reject each of them.
* the seeded, named cases that tests/test_solve_ref.py (CPU) and tests/test_gpu_solve_illcond.py (the kernels) share.  The
  conditioning is planted through exact duplicates among the measured rows: the LD matrix is then singular up to rounding, so
  lambda_min(B11) = lam and lam alone steers cond(B11) (2e3 .. 3e5 here: lambda_max is about 3) and the MakePosDef decision.  z1 is drawn
  independently for every row, duplicates included, so the right-hand side has a component along the small eigenvector.
* measure_levels(): `python tests/solve_ref.py` writes the errors of both CPU routes against the truth, and the clamped
  cases' levels in the convention of clamp_ref.py, to tests/golden/solve_levels.json.
"""
import collections
import contextlib
import functools
import json
import os
import sys

import numpy as np
import scipy.linalg

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import clamp_ref as cr  # noqa: E402
import oracle  # noqa: E402

NB = cr.NB
LEVELS_PATH = os.path.join(HERE, "golden", "solve_levels.json")
FACTOR, FLOOR, CEILING = 16.0, 1e-13, 1e-8       # clamp_levels.json's convention; the ceiling is the suite's Z_TOL
FRAC_BITS = 192                                   # fixed point of the refined solution: 2^-192 = 1.6e-58
RESID_TOL = 1e-30


def bound(level):
    """The GPU's bound for a quantity that chol_route gets wrong by `level`."""
    return min(CEILING, max(FLOOR, FACTOR * level))


# ---- exact arithmetic on doubles ---------------------------------------------------------------------------------------------
_shift = np.frompyfunc(lambda m, s: m << s if s >= 0 else m >> -s, 2, 1)
_tofloat = np.frompyfunc(float, 1, 1)


def exact_ints(a):
    """Finite doubles as Python integers times one power of two: (object array, exponent)."""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)
    e = np.where(a == 0.0, 0, e.astype(np.int64) - 53)
    emin = int(e.min()) if a.size else 0
    return _shift(np.ldexp(m, 53).astype(np.int64).astype(object), (e - emin).astype(object)), emin


def _to_fixed(d, frac_bits):
    """round-towards-minus-infinity(d * 2^frac_bits) as Python integers."""
    m, e = np.frexp(np.asarray(d, dtype=np.float64))
    return _shift(np.ldexp(m, 53).astype(np.int64).astype(object), (e.astype(np.int64) - 53 + frac_bits).astype(object))


def _residual(ai, ea, bs, x, frac_bits):
    """B - A X, formed exactly, rounded once to double.  bs = B in units of 2^(ea - frac_bits)."""
    r = bs - ai.dot(x)
    return np.ldexp(_tofloat(r).astype(np.float64), ea - frac_bits)


def refine(a, b, frac_bits=FRAC_BITS, tol=RESID_TOL, max_pass=12):
    """A^-1 B for the exact doubles in a [n, n] and b [n, r]: one LAPACK LU in fp64, then X += LU^-1 (B - A X) with the residual
    exact and X in fixed point, until max |B - A X| < tol.  At cond(A) <= 1e8 a pass gains at least 8 digits.
    Returns (X as integers, frac_bits, the residual reached, passes)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ai, ea = exact_ints(a)
    bi, eb = exact_ints(b)
    if eb - ea + frac_bits < 0:
        raise ValueError("frac_bits too small for these magnitudes")
    bs = _shift(bi, np.full(bi.shape, eb - ea + frac_bits, dtype=object))
    lu = scipy.linalg.lu_factor(a)
    x = np.zeros(b.shape, dtype=object)
    x[...] = 0
    for k in range(max_pass):
        r = _residual(ai, ea, bs, x, frac_bits)
        res = float(np.max(np.abs(r)))
        if res < tol:
            return x, frac_bits, res, k
        x = x + _to_fixed(scipy.linalg.lu_solve(lu, r), frac_bits)
    raise RuntimeError(f"refinement stalled at residual {res}")


def exact_residual(a, b, x, frac_bits):
    """max |B - A X| for a fixed-point X, formed exactly (independent entry point for the tests)."""
    ai, ea = exact_ints(a)
    bi, eb = exact_ints(b)
    bs = _shift(bi, np.full(bi.shape, eb - ea + frac_bits, dtype=object))
    return float(np.max(np.abs(_residual(ai, ea, bs, x, frac_bits))))


def truth_solve(b11, b21, z1, frac_bits=FRAC_BITS):
    """dict(z, info [U] rounded once to double; x = B11^-1 [B21^T | z1] in fixed point, frac_bits, resid, passes)."""
    import mpmath as mp
    b11, b21, z1 = (np.asarray(v, dtype=np.float64) for v in (b11, b21, z1))
    U = b21.shape[0]
    rhs = np.column_stack([b21.T, z1])
    x, fb, res, passes = refine(b11, rhs, frac_bits)
    ri, er = exact_ints(rhs)
    q = (ri[:, :U] * x[:, :U]).sum(0)                       # b21_u . B11^-1 b21_u^T      (dist.cpp:197), exact
    t = (ri[:, :U] * x[:, U:U + 1]).sum(0)                  # b21_u . B11^-1 z1           (dist.cpp:194), exact
    z, info = np.empty(U), np.empty(U)
    with mp.workdps(50):
        for u in range(U):
            iu = abs(mp.ldexp(mp.mpf(int(q[u])), er - fb))                                   # dist.cpp:198
            info[u] = float(iu)
            z[u] = float(mp.ldexp(mp.mpf(int(t[u])), er - fb) / mp.sqrt(iu))             # dist.cpp:200
    return dict(z=z, info=info, x=x, frac_bits=fb, resid=res, passes=passes)


def fixed_to_float(x, frac_bits):
    return np.ldexp(_tofloat(x).astype(np.float64), -frac_bits)


# ---- the kernel's algebra in fp64 ---------------------------------------------------------------------------------------------
def _one_blas_thread():
    """The recorded levels are single rounding instances: keep the summation order independent of the CPU count where
    threadpoolctl is there to ask for it."""
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1, user_api="blas")
    except ImportError:
        return contextlib.nullcontext()


def chol_route(b11, b21, z1):
    """(z, info) by the kernel's algebra with LAPACK: the yardstick."""
    with _one_blas_thread():
        L = np.linalg.cholesky(np.asarray(b11, dtype=np.float64))
        X = scipy.linalg.solve_triangular(L, np.eye(len(L)), lower=True)
        y = X @ np.asarray(z1, dtype=np.float64)
        W = X @ np.asarray(b21, dtype=np.float64).T
        info = np.einsum("ku,ku->u", W, W)
        return (W.T @ y) / np.sqrt(info), info


MUTATIONS = ("rsqrt_2m40", "f32_block_inverse", "info_kblock_twice", "y_entry_dropped", "wy_in_f32")


def chol_route_blocked(b11, b21, z1, mutation=None, nb=NB):
    """The same algebra in factor blocks of nb rows: the diagonal block by a column Cholesky whose pivots are multiplied by
    1 / sqrt(pivot), its inverse, the panel below it, the trailing update; the rows of X = L^-1 block by block; info as a sum
    of nb-wide k blocks.  mutation (one of MUTATIONS) makes one step subtly wrong:
      rsqrt_2m40         every 1 / sqrt(pivot) carries a relative error of 2^-40 (one Newton step too few)
      f32_block_inverse  the inverse of the last diagonal factor block is rounded to fp32
      info_kblock_twice  the partial sum of info's first k block is added a second time with weight 1e-9
      y_entry_dropped    y is built from z1 with one entry of the last block left out
      wy_in_f32          w_u . y is accumulated in float32"""
    assert mutation is None or mutation in MUTATIONS
    A = np.array(b11, dtype=np.float64)
    z1 = np.array(z1, dtype=np.float64)
    b21 = np.asarray(b21, dtype=np.float64)
    M = len(A)
    blocks = [(s, min(s + nb, M)) for s in range(0, M, nb)]
    L = np.zeros((M, M))
    Xd = []
    for bi, (s, e) in enumerate(blocks):
        D = A[s:e, s:e].copy()
        n = e - s
        for j in range(n):
            r = 1.0 / np.sqrt(D[j, j])
            if mutation == "rsqrt_2m40":
                r *= 1.0 + 2.0 ** -40
            D[j:, j] *= r
            D[j + 1:, j + 1:] -= np.outer(D[j + 1:, j], D[j + 1:, j])
        D = np.tril(D)
        Xi = scipy.linalg.solve_triangular(D, np.eye(n), lower=True)
        if mutation == "f32_block_inverse" and bi == len(blocks) - 1:
            Xi = Xi.astype(np.float32).astype(np.float64)
        Xd.append(Xi)
        L[s:e, s:e] = D
        if e < M:
            L[e:, s:e] = A[e:, s:e] @ Xi.T
            A[e:, e:] -= L[e:, s:e] @ L[e:, s:e].T
    X = np.zeros((M, M))
    for bi, (s, e) in enumerate(blocks):
        T = np.zeros((e - s, M))
        T[:, s:e] = np.eye(e - s)
        for (s2, e2) in blocks[:bi]:
            T -= L[s:e, s2:e2] @ X[s2:e2]
        X[s:e] = Xd[bi] @ T
    if mutation == "y_entry_dropped":
        z1[blocks[-1][0] + (M - blocks[-1][0]) // 2] = 0.0
    y = X @ z1
    W = X @ b21.T
    info = np.zeros(b21.shape[0])
    for (s, e) in blocks:
        info += np.einsum("ku,ku->u", W[s:e], W[s:e])
    if mutation == "info_kblock_twice":
        info += 1e-9 * np.einsum("ku,ku->u", W[:blocks[0][1]], W[:blocks[0][1]])
    if mutation == "wy_in_f32":
        num = np.sum((W * y[:, None]).astype(np.float32), axis=0, dtype=np.float32).astype(np.float64)
    else:
        num = W.T @ y
    return num / np.sqrt(info), info


def errors(z, info, truth):
    """The suite's measures: info relatively, z as |dz| / max(1, |z|)."""
    return dict(z=cr.zerr(np.asarray(z), truth["z"]), info=cr.relerr(np.asarray(info), truth["info"]))


# ---- the cases ---------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name M U mode place lam eps seed")
N_SAMPLES = 500                                 # mode 0: one pooled population (1 500 at M = 640: more samples than rows, B11 of full rank)
POP_SIZES = (120, 90, 150, 140)                 # mode 1: four populations with allele frequencies of their own
W_SUM = 1.061                                   # un-normalised like the PGC2 weights


def duplicates(place, M):
    """[(row, the row it copies, genotypes changed)] of a placement."""
    if place == "first":                         # tiny pivot in the first block, carried through every trailing update
        return [(1, 0, 0)]
    if place == "last":                          # tiny pivot in the last block
        return [(M - 1, 0, 0)]
    if place == "straddle":                      # the pair sits on either side of the edge between the first two factor blocks
        return [(NB, NB - 1, 0)]
    if place == "blockend":                      # the pair is the last two rows of the first factor block
        return [(NB - 1, NB - 2, 0)]
    if place == "three":                         # three duplicates whose tiny pivots fall into three different blocks
        return [(NB // 2, 1, 0), (NB + NB // 2, 2, 0), (M - 1, 3, 0)]
    if place == "near":                          # one exact pair and 8 near copies: a cluster of eigenvalues between lam and 1e-2
        step = (M - 12) // 8
        return [(M - 1, 0, 0)] + [(11 + k * step, 1 + k, 1 + k % 3) for k in range(8)]
    raise ValueError(place)


@functools.lru_cache(maxsize=None)
def _rows(M, U, mode, place, seed):
    rng = np.random.default_rng(seed)
    if mode == 0:
        n = N_SAMPLES if M < N_SAMPLES else 3 * N_SAMPLES
        G = cr.rand_geno(rng, M + U, n)
        off, w = np.array([0, n], dtype=np.int32), None
    else:
        off = np.concatenate([[0], np.cumsum(POP_SIZES)]).astype(np.int32)
        base = rng.uniform(0.1, 0.9, size=(M + U, 1))
        G = np.zeros((M + U, int(off[-1])), dtype=np.uint8)
        for p, m in enumerate(POP_SIZES):
            af = np.clip(base + rng.normal(0, 0.08, size=(M + U, 1)), 0.05, 0.95)
            G[:, off[p]:off[p + 1]] = (rng.random((M + U, m)) < af).astype(np.uint8) + (rng.random((M + U, m)) < af).astype(np.uint8)
            for r in range(M + U):               # polymorphic inside every population
                blk = G[r, off[p]:off[p + 1]]
                if blk.min() == blk.max():
                    blk[0], blk[1] = 0, 1
        w = rng.uniform(0.5, 1.5, len(POP_SIZES))
        w *= W_SUM / w.sum()
    gm = G[:M].copy()
    for row, src, changed in duplicates(place, M):
        gm[row] = gm[src]
        cols = rng.choice(G.shape[1], size=changed, replace=False)
        gm[row, cols] = (gm[row, cols] + 1) % 3
    for p in range(len(off) - 1):                # a near copy is still polymorphic inside every population
        blk = gm[:, off[p]:off[p + 1]]
        assert np.all(blk.min(1) != blk.max(1))
    return np.ascontiguousarray(gm), np.ascontiguousarray(G[M:]), off, w, rng.standard_normal(M) * 2


def window(case):
    gm, gu, off, w, z1 = _rows(case.M, case.U, case.mode, case.place, case.seed)
    return dict(mode=case.mode, geno_m=gm, geno_u=gu, pop_off=off, pop_wgt=w, z1=z1, lam=float(case.lam), min_abs_eig=float(case.eps))


def _cases():
    eps = cr.EPS
    specs = [  # (M, U, mode, place, [lam, ...])        lam 1 % on either side of eps: the decision pairs, one per placement
        (63, 33, 0, "first", [1.01e-5, 0.99e-5]),
        (63, 130, 1, "first", [1e-4]),
        (64, 130, 1, "last", [1.01e-5, 0.99e-5]),
        (64, 33, 0, "blockend", [1.01e-5, 0.99e-5, 1e-3]),
        (65, 33, 0, "straddle", [1.01e-5, 0.99e-5, 0.0]),
        (65, 130, 1, "last", [1.01e-5, 0.99e-5, 0.0, 1e-4]),
        (129, 33, 1, "straddle", [1.01e-5, 0.99e-5, 0.0]),
        (129, 130, 0, "three", [1.01e-5, 0.99e-5, 0.0, 1e-3]),
        (129, 33, 0, "near", [1.01e-5, 1e-4]),
        (200, 33, 0, "blockend", [1.01e-5, 0.99e-5, 0.0]),
        (200, 130, 1, "three", [1.01e-5, 0.99e-5, 0.0]),
        (200, 130, 0, "near", [1.01e-5, 0.99e-5, 1e-3]),
        (200, 33, 1, "straddle", [1e-4]),
        (640, 16, 0, "last", [1.01e-5]),
    ]
    out = {}
    for M, U, mode, place, lams in specs:
        for lam in lams:
            name = f"m{mode}_{M}x{U}_{place}_{lam:g}"
            out[name] = Case(name, M, U, mode, place, lam, eps, 1000 + 7 * M + U + mode)
    for lam in (1.01e-3, 0.99e-3):               # a min_abs_eig of the caller's own: eps is not hard-wired
        name = f"m0_129x33_straddle_eps1e-3_{lam:g}"
        out[name] = Case(name, 129, 33, 0, "straddle", lam, 1e-3, 1000 + 7 * 129 + 33 + 5)
    return out


CASES = _cases()
UNCLAMPED = [n for n, c in CASES.items() if c.lam > c.eps]
CLAMPED = [n for n, c in CASES.items() if c.lam < c.eps]
SMALL_LAM = [n for n in UNCLAMPED if CASES[n].lam / CASES[n].eps < 1.02]


def twin(name, side):
    """The case on the other side of eps on the same window: side 'above' or 'below' (None where the list has none)."""
    c = CASES[name]
    for n, d in CASES.items():
        if d[1:5] == c[1:5] and d.eps == c.eps and d.seed == c.seed and abs(d.lam / d.eps - 1.0) < 0.02 and (d.lam > d.eps) == (side == "above"):
            return n
    return None


PAIRS = [(n, twin(n, "below")) for n in SMALL_LAM if twin(n, "below")]
# the windows that the GPU tests run in every launch form -- every unclamped case of these sizes, whatever its lam, placement
# and min_abs_eig -- and the clamped ones they check against clamp_ref.py
FORMS = [n for n in UNCLAMPED if CASES[n].M in (65, 129, 200)]
FORMS_BELOW = sorted({twin(n, "below") for n in FORMS} - {None})      # the same windows just below eps, where the list has one
CLAMP_CHECKED = [n for n in CLAMPED if CASES[n].M in (65, 129, 200)]


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    w = window(CASES[name])
    return oracle.run_impute(w["mode"], w["geno_m"], w["geno_u"], w["pop_off"], w["pop_wgt"], w["z1"], lam=w["lam"],
                             min_abs_eig=w["min_abs_eig"], want_mats=True)


@functools.lru_cache(maxsize=None)
def oracle_truth(name):
    o = oracle_run(name)
    return truth_solve(o["b11"], o["b21"], window(CASES[name])["z1"])


def cert_threshold(win):
    """The lam at which shift_cert_kernel's bound equals eps (the comment above it in k_solve.hip):
    lam - (W - 1)+ sum_p w_p sum_i (mu_p(i) / sd_i)^2 - M 1e-10 = eps, with mu_p(i) the mean genotype of row i in population p
    and sd_i^2 the weighted covariance of row i with itself (util.cpp:103-124)."""
    from oracle import oracle_np
    gm = win["geno_m"].astype(np.float64)
    M = gm.shape[0]
    if win["mode"] == 0:
        return win["min_abs_eig"] + 1e-10 * M
    off, w = win["pop_off"], win["pop_wgt"]
    var = np.diag(oracle_np.weighted_cov(gm, None, off, w))
    s = sum(w[p] * np.sum(gm[:, off[p]:off[p + 1]].mean(1) ** 2 / var) for p in range(len(w)))
    return win["min_abs_eig"] + max(float(np.sum(w)) - 1.0, 0.0) * float(s) + 1e-10 * M


# ---- the levels --------------------------------------------------------------------------------------------------------------
def solve_level(name):
    """Errors against the truth of chol_route and of the oracle's own route (full-pivot-LU inverse), both on the oracle's B11
    and B21, with the smallest eigenvalue and the condition number."""
    c = CASES[name]
    o, t = oracle_run(name), oracle_truth(name)
    ev = np.linalg.eigvalsh(o["b11"])
    zc, ic = chol_route(o["b11"], o["b21"], window(c)["z1"])
    ec, eo = errors(zc, ic, t), errors(o["z"], o["info"], t)
    return dict(M=c.M, U=c.U, lam=c.lam, lam_min=float(ev[0]), cond=float(ev[-1] / ev[0]), mpd=int(o["mpd"]), passes=int(t["passes"]),
                z=ec["z"], info=ec["info"], z_oracle=eo["z"], info_oracle=eo["info"])


def clamp_level(name):
    """A clamped case in clamp_ref.b11_level's terms: the oracle (Jacobi, full-pivot LU) against numpy (eigh, inv), and two
    operation orders of the solve on one matrix."""
    c = CASES[name]
    win, o = window(c), oracle_run(name)
    A, b21 = cr.raw_b11(win)
    X, lam = cr.clamp_numpy(A, c.eps)
    z, info = cr.solve_inv(X, b21, win["z1"])
    zc, ic = cr.solve_chol(X, b21, win["z1"])
    cert = max(cr.certificate_level(cr.clamp_certificate(A, m, c.eps)) for m in (X, o["b11"]))
    return dict(M=c.M, lifted=int(np.sum(lam < c.eps)), lam_min=float(lam[0]), mpd=int(o["mpd"]), b11=float(np.max(np.abs(o["b11"] - X))),
                cert=float(cert), info=cr.relerr(o["info"], info), z=cr.zerr(o["z"], z), info_own=cr.relerr(ic, info), z_own=cr.zerr(zc, z))


def measure_levels():
    return dict(solve={n: solve_level(n) for n in UNCLAMPED}, clamp={n: clamp_level(n) for n in CLAMP_CHECKED})


def load_levels():
    with open(LEVELS_PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    levels = measure_levels()
    with open(LEVELS_PATH, "w") as f:
        json.dump(levels, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(levels, indent=1, sort_keys=True))
