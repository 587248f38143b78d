"""numpy replay of the gene-based sum-of-chi2 test (include/gauss_hip.h: gauss_gene_sumchi2; include/gauss_host.h:
gauss_host_sumchi2_pval), literal: the pruning loop, the Jacobi solve with k_sumchi2.hip's rotation order, skip rule and summation
order of the Frobenius norm, the saddlepoint p-value with its bracket and its 100 bisection steps; and `imhof`, the numerical
inversion the saddlepoint is judged against.  Every fp64 product and sum is a separate rounded operation, as in the kernel (it is
compiled without contraction), so `prune`, `jacobi` and `qstat` give the kernel's bits."""
import math

import numpy as np

MAX_KEPT, MAX_N, MAX_SWEEPS, T = 128, 1024, 30, 256
ST_NOCONV, ST_TOOLARGE, ST_EMPTY = 4, 128, 256
EDGE, BISECT = 1e-3, 100


def prune(R, r2):
    """(kept [n] 0/1, n_nan): rows in order; a row whose off-diagonal entries are all NaN (n > 1) is dropped and counted; a row not
    yet dropped is kept and drops every later row j with R_ij * R_ij > r2 (strict; a NaN compares false)."""
    R = np.asarray(R, dtype=np.float64)
    n = R.shape[0]
    drop = np.zeros(n, dtype=np.int32)
    if n > 1:
        off = ~np.eye(n, dtype=bool)
        drop[np.all(np.isnan(R) | ~off, axis=1)] = 2
    for i in range(n):
        if drop[i]:
            continue
        row = R[i, i + 1:]
        with np.errstate(invalid="ignore"):
            hit = (row * row) > r2
        drop[i + 1:][hit & (drop[i + 1:] == 0)] = 1
    return (drop == 0).astype(np.int32), int((drop == 2).sum())


def _frob(A, k):
    """sum of the squares of the k x k block as the kernel adds them: thread t takes entries t, t + 256, ... in row-major order,
    then 8 halving steps over the 256 partial sums"""
    v = (A[:k, :k] * A[:k, :k]).reshape(-1)
    pad = np.zeros(-(-v.size // T) * T)
    pad[:v.size] = v
    part = np.zeros(T)
    for row in pad.reshape(-1, T):
        part = part + row
    s = T // 2
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def jacobi(A):
    """(eigenvalues descending [k], sweeps, converged) of the symmetric k x k matrix A by the kernel's cyclic two-sided Jacobi"""
    A = np.array(A, dtype=np.float64)
    k = A.shape[0]
    m = k + (k & 1)
    W = np.zeros((m, m))
    W[:k, :k] = A
    tol = 8.881784197001252e-16 * math.sqrt(_frob(W, k))
    converged, sweeps = False, 0
    half = m // 2
    for sweep in range(MAX_SWEEPS):
        rotated = False
        for rnd in range(m - 1):
            P, Q, Cc, Ss = [], [], [], []
            for t in range(half):
                if t == 0:
                    p, q = m - 1, rnd
                else:
                    p, q = (rnd + t) % (m - 1), (rnd - t + m - 1) % (m - 1)
                if p > q:
                    p, q = q, p
                c, s = 1.0, 0.0
                if q < k:
                    apq = W[p, q]
                    if abs(apq) > tol:
                        tau = (W[q, q] - W[p, p]) / (2.0 * apq)
                        if abs(tau) > 1e150:
                            tt = 0.5 / tau
                        else:
                            tt = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + math.sqrt(1.0 + tau * tau))
                        c = 1.0 / math.sqrt(1.0 + tt * tt)
                        s = tt * c
                        rotated = True
                if s != 0.0:
                    P.append(p); Q.append(q); Cc.append(c); Ss.append(s)
            if not P:
                continue
            P, Q = np.array(P), np.array(Q)
            c, s = np.array(Cc)[:, None], np.array(Ss)[:, None]
            x, y = W[P, :].copy(), W[Q, :].copy()                  # rows p, q <- J^T A
            W[P, :] = c * x - s * y
            W[Q, :] = s * x + c * y
            x, y = W[:, P].copy(), W[:, Q].copy()                  # columns p, q <- A J
            W[:, P] = c.T * x - s.T * y
            W[:, Q] = s.T * x + c.T * y
        sweeps = sweep + 1
        if not rotated:
            converged = True
            break
    if not converged:
        return np.full(k, np.nan), sweeps, False
    d = np.diagonal(W)[:k].copy()
    order = sorted(range(k), key=lambda i: (-d[i], i))            # descending, ties: the smaller index first
    return d[order], sweeps, True


def qstat(z, kept):
    """sum of z_i^2 over the kept rows, added in ascending row order"""
    q = 0.0
    for i in np.flatnonzero(kept):
        q = q + z[i] * z[i]
    return q


def top_row(z):
    """the row with the largest z^2 among the finite z (ties: the smaller row); -1: none"""
    z = np.asarray(z, dtype=np.float64)
    ok = np.isfinite(z)
    if not ok.any():
        return -1
    with np.errstate(over="ignore", invalid="ignore"):
        z2 = np.where(ok, z * z, -1.0)
    return int(np.argmax(z2))                                      # (argmax returns the first of equal maxima)


def gene(R, Z, r2):
    """One gene as gauss_gene_sumchi2 reports it: dict(kept, n_kept, lam [128], q [T], top [T], status, sweeps).  Z [T, n]."""
    R = np.asarray(R, dtype=np.float64)
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    kept, _ = prune(R, r2) if R.shape[0] else (np.zeros(0, np.int32), 0)
    k = int(kept.sum())
    lam, status, sweeps = np.full(MAX_KEPT, np.nan), 0, 0
    if k == 0:
        status = ST_EMPTY
    elif k > MAX_KEPT:
        status = ST_TOOLARGE
    else:
        idx = np.flatnonzero(kept)
        ev, sweeps, ok = jacobi(R[np.ix_(idx, idx)])
        lam[:k] = ev
        status = 0 if ok else ST_NOCONV
    return dict(kept=kept, n_kept=k, lam=lam, q=np.array([qstat(z, kept) for z in Z]), top=np.array([top_row(z) for z in Z]),
                status=status, sweeps=sweeps)


def pnorm_upper(x):
    return 0.5 * math.erfc(x / 1.4142135623730951)


def saddle(lam, q, edge=EDGE, branch=None):
    """P(sum lam_i chi2_1 > q) as gauss_host_sumchi2_pval computes it.  branch="saddle" / "edgeworth" forces one formula (the test
    of their agreement at the switch)."""
    l = [float(v) for v in np.asarray(lam, dtype=np.float64).reshape(-1) if v > 0.0]
    k = len(l)
    if k == 0 or math.isnan(q):
        return math.nan
    if q <= 0.0:
        return 1.0
    if k == 1:
        return 2 * pnorm_upper(math.sqrt(q / l[0]))
    s1 = s2 = s3 = lmax = 0.0
    for v in l:
        s1 += v; s2 += v * v; s3 += v * v * v; lmax = max(lmax, v)
    x = (q - s1) / math.sqrt(2 * s2)
    if branch == "edgeworth" or (branch is None and abs(x) < edge):
        k3 = 8 * s3 / ((2 * s2) * math.sqrt(2 * s2))
        return pnorm_upper(x) + math.exp(-0.5 * x * x) / 2.5066282746310002 * (k3 / 6) * (x * x - 1)
    lo, hi = (0.0, 0.5 / lmax) if q > s1 else (-0.5 * k / q, 0.0)
    for _ in range(BISECT):
        mid = 0.5 * (lo + hi)
        k1 = 0.0
        bad = not (1 - 2 * mid * lmax > 0)
        if not bad:
            for v in l:
                k1 += v / (1 - 2 * mid * v)
        if bad or k1 > q:
            hi = mid
        else:
            lo = mid
    zeta = 0.5 * (lo + hi)
    K = K2 = 0.0
    for v in l:
        d = 1 - 2 * zeta * v
        K += math.log1p(-2 * zeta * v); K2 += 2 * v * v / (d * d)
    K *= -0.5
    try:
        w = (-1.0 if zeta < 0 else 1.0) * math.sqrt(2 * (zeta * q - K))
        p = pnorm_upper(w + math.log(zeta * math.sqrt(K2) / w) / w)
    except (ValueError, ZeroDivisionError):
        return math.nan
    return p if math.isfinite(p) else math.nan


def imhof(lam, q):
    """(p, quad's error estimate): P(sum lam_i chi2_1 > q) by Imhof's numerical inversion (Biometrika 48, 1961) with
    scipy.integrate.quad: p = 1/2 + 1/pi int_0^inf sin(theta(u)) / (u rho(u)) du, theta = 1/2 sum atan(lam u) - q u / 2,
    rho = prod (1 + lam^2 u^2)^(1/4)"""
    from scipy.integrate import quad
    l = np.array([v for v in np.asarray(lam, dtype=np.float64).reshape(-1) if v > 0.0])
    l = l[l > 1e-10 * l.max()]      # (a rank-deficient block's rounding-level eigenvalues: their part of Q is below 1e-10 of it)

    def f(u):
        if u == 0.0:
            return 0.5 * (l.sum() - q)
        th = 0.5 * np.arctan(l * u).sum() - 0.5 * q * u
        return math.sin(th) / (u * math.exp(0.25 * np.log1p(l * l * u * u).sum()))
    # rho(u) > prod (lam u)^(1/2): the tail beyond U is below (2 / k) U^(-k/2) / prod sqrt(lam); U is chosen so that it is < 1e-14
    k = len(l)
    logc = -0.5 * np.log(l).sum() + math.log(2.0 / k)
    U = math.exp((logc + 14 * math.log(10)) / (0.5 * k))
    v, err = quad(f, 0.0, U, limit=2000, epsabs=1e-13, epsrel=1e-10)
    return 0.5 + v / math.pi, err / math.pi
