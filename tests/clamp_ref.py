"""References for the two device eigenvalue-clamp solvers: MakePosDef / CountPC on a window's B11 (k_misc.hip, one-sided
Jacobi) and the population-weight solver (k_popwgt.hip, two-sided Jacobi, clamp, Cholesky solve).  Plain numpy and mpmath, no GPU.

* clamp_numpy / clamp_certificate: the clamp V max(L, eps) V^T stated with LAPACK, and residuals that pin a clamped matrix
  without naming an eigenvector basis (hundreds of equal eigenvalues leave the basis inside the cluster free).
* popwgt_mp: the whole pw_* pipeline of one interval in mpmath (exact cross sums, eigsy, the clamp rule of util.cpp:302-318,
  the solve).
* seeded input builders and the table of cases that tests/test_clamp_ref.py (CPU: the cases are well posed, the certificate
  can fail) and tests/test_gpu_clamp.py (the kernels) share.
* measure_levels(): how far the two CPU statements of every case disagree.  `python tests/clamp_ref.py` writes them to
  tests/golden/clamp_levels.json; the GPU is allowed FACTOR times that, never less than FLOOR, never more than CEILING.
"""
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

import oracle  # noqa: E402
from oracle import oracle_np  # noqa: E402

NB = 64                      # factor block and padding unit of B11 (gauss_internal.h): Mld = M rounded up to NB
EPS = 1e-5                   # min_abs_eig
QCAT_CUTOFF = 0.01
LEVELS_PATH = os.path.join(HERE, "golden", "clamp_levels.json")
FACTOR, FLOOR = 16.0, 1e-13
# today's bounds on a clamped window (test_gpu_parity.py::test_makeposdef_clamp_path: b11 1e-9, z and info 1e-5) and on the weights
# (test_gpu_popwgt.py::_check: 1e-8 x scale): never exceeded.  The solve on the GPU's own matrices has no bound of its own today on
# a clamped B11 (condition 1e5); it gets the ceiling of z and info, and its level -- two operation orders of the solve on one and
# the same matrix -- is what decides.
CEILING = dict(b11=1e-9, cert=1e-9, info=1e-5, z=1e-5, info_own=1e-5, z_own=1e-5, w=1e-8)
RANK_TOL = 1e-8              # an eigenvalue of X - A above this counts as a lift: the smallest lift of any case is EPS * 1e-2


def bound(level, what):
    """The GPU's bound for a quantity whose two CPU statements disagree by `level`."""
    return min(CEILING[what], max(FLOOR, FACTOR * level))


# ---- the clamp ---------------------------------------------------------------------------------------------------------------
def clamp_numpy(A, eps=EPS):
    """(V max(L, eps) V^T, L) with numpy.linalg.eigh; A itself where no eigenvalue is below eps (MakePosDef leaves it alone)."""
    A = np.asarray(A, dtype=np.float64)
    lam, V = np.linalg.eigh(A)
    if lam[0] >= eps:
        return A.copy(), lam
    return (V * np.maximum(lam, eps)) @ V.T, lam


def clamp_certificate(A, X, eps=EPS, rank_tol=RANK_TOL):
    """Residuals that are all small for X = clamp(A) and only for it, whatever basis was chosen inside a cluster of equal
    eigenvalues: X is symmetric, commutes with A (shares its eigenspaces), has the spectrum sort(max(L, eps)), and X - A is
    positive semidefinite of rank #{L < eps}.  Norms: asym and spectrum are max-abs, commute is Frobenius / max |L|."""
    A = np.asarray(A, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    lam = np.linalg.eigvalsh(A)
    want = np.sort(np.maximum(lam, eps)) if lam[0] < eps else lam
    Xs = 0.5 * (X + X.T)
    d = np.linalg.eigvalsh(Xs - A)
    return dict(asym=float(np.max(np.abs(X - X.T))),
                commute=float(np.linalg.norm(Xs @ A - A @ Xs) / max(1.0, float(np.max(np.abs(lam))))),
                spectrum=float(np.max(np.abs(np.linalg.eigvalsh(Xs) - want))),
                rank=int(np.sum(d > rank_tol)), rank_want=int(np.sum(lam < eps)) if lam[0] < eps else 0,
                min_eig=float(d[0]))


def certificate_level(c):
    return max(c["asym"], c["commute"], c["spectrum"], -c["min_eig"])


def certificate_ok(c, tol):
    return certificate_level(c) <= tol and c["rank"] == c["rank_want"]


def solve_inv(b11, b21, z1):
    """(z, info) of run_dist / run_distmix from B11 and B21 with numpy's inverse (dist.cpp:193-202)."""
    y = b21 @ np.linalg.inv(b11)
    info = np.abs(np.einsum("ij,ij->i", y, b21))
    return (y @ np.asarray(z1, dtype=np.float64)) / np.sqrt(info), info


def solve_chol(b11, b21, z1):
    """The same numbers in another valid operation order: Cholesky factor and two triangular solves."""
    L = np.linalg.cholesky(b11)
    v = np.linalg.solve(L, b21.T)
    info = np.abs(np.einsum("ij,ij->j", v, v))
    return (np.linalg.solve(L, np.asarray(z1, dtype=np.float64)) @ v) / np.sqrt(info), info


def zerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


# ---- window builders ---------------------------------------------------------------------------------------------------------
def rand_geno(rng, rows, n, lo=0.05, hi=0.95):
    af = rng.uniform(lo, hi, size=(rows, 1))
    g = (rng.random((rows, n)) < af).astype(np.uint8) + (rng.random((rows, n)) < af).astype(np.uint8)
    for r in range(rows):                      # no monomorphic rows
        if g[r].min() == g[r].max():
            g[r, 0], g[r, 1] = 0, 2
    return g


def _window(mode, gm, gu, off, w, z1, lam):
    return dict(mode=mode, geno_m=np.ascontiguousarray(gm), geno_u=np.ascontiguousarray(gu), pop_off=np.asarray(off, dtype=np.int32),
                pop_wgt=w, z1=np.ascontiguousarray(z1), lam=float(lam))


def window_rank_deficient(M, N, seed, U=24, lam=0.0):
    """One pooled population of N < M samples: B11 has rank N - 1, M - N + 1 eigenvalues sit at lam."""
    rng = np.random.default_rng(seed)
    G = rand_geno(rng, M + U, N)
    return _window(0, G[:M], G[M:], [0, N], None, rng.standard_normal(M) * 2, lam)


def window_duplicated(M, N, k, seed, U=24, lam=0.0):
    """N > M samples, the last k measured rows repeat the first k: k eigenvalues sit at lam."""
    rng = np.random.default_rng(seed)
    G = rand_geno(rng, M - k + U, N)
    gm = np.vstack([G[:M - k], G[:k]])
    z = rng.standard_normal(M - k) * 2
    return _window(0, gm, G[M - k:], [0, N], None, np.concatenate([z, z[:k]]), lam)


def window_mixed(M, sizes, wsum, seed, U=24, lam=0.0):
    """Mode 1 (weighted estimator, util.cpp:103-124): populations with allele frequencies of their own, fewer samples than
    measured rows, weights summing to wsum.  Above 1 the estimator's mean term turns negative (k_solve.hip: shift_cert_kernel),
    so B11 is indefinite; low allele frequencies keep every self-covariance positive (no NaN row)."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    base = rng.uniform(0.08, 0.3, size=(M + U, 1))
    G = np.zeros((M + U, int(off[-1])), dtype=np.uint8)
    for p, m in enumerate(sizes):
        af = np.clip(base + rng.normal(0, 0.04, size=(M + U, 1)), 0.04, 0.4)
        G[:, off[p]:off[p + 1]] = (rng.random((M + U, m)) < af).astype(np.uint8) + (rng.random((M + U, m)) < af).astype(np.uint8)
        for r in range(M + U):                 # polymorphic inside every population
            blk = G[r, off[p]:off[p + 1]]
            if blk.min() == blk.max():
                blk[0], blk[1] = 0, 1
    w = rng.uniform(0.5, 1.5, len(sizes))
    w *= wsum / w.sum()
    return _window(1, G[:M], G[M:], off, w, rng.standard_normal(M) * 2, lam)


def raw_b11(win, lam=None):
    """B11 (diagonal 1 + lam) and B21 before MakePosDef, in Gram form with numpy (oracle/oracle_np.py): a statement of the LD
    that shares no operation order with the loop-literal C oracle, so that the recorded levels include the LD's own rounding."""
    lam = win["lam"] if lam is None else lam
    gm, gu = win["geno_m"], win["geno_u"]
    if win["mode"] == 0:
        b11, b21 = oracle_np.pooled_cor(gm), oracle_np.pooled_cor(gu, gm)
    else:
        b11 = oracle_np.weighted_cor(gm, None, win["pop_off"], win["pop_wgt"])
        b21 = oracle_np.weighted_cor(gu, gm, win["pop_off"], win["pop_wgt"])
    b11 = 0.5 * (b11 + b11.T)
    np.fill_diagonal(b11, 1.0 + lam)
    return b11, b21


def lam_for(A0, r, margin, eps=EPS):
    """A0: B11 with lam = 0.  The diagonal of B11 is 1 + lam, so lam shifts the whole spectrum exactly.  Returns the lam that
    puts exactly r eigenvalues below eps, the nearest one at eps (1 - margin); for r = 0 the smallest one at eps (1 + margin)."""
    mu = np.linalg.eigvalsh(np.asarray(A0, dtype=np.float64))
    lam = eps * (1.0 + margin) - mu[0] if r == 0 else eps * (1.0 - margin) - mu[r - 1]
    if 0 < r < len(mu) and not mu[r] + lam > eps * (1.0 + margin):
        raise ValueError(f"eigenvalue {r} of A0 is not clear of eps: {mu[r] + lam}")
    return float(lam)


def window_near_eps(r, margin, seed=77):
    """M = 2 NB + 2 with two duplicated rows (two eigenvalues of A0 at 0 up to rounding) and the lam that lam_for chooses."""
    win = window_duplicated(2 * NB + 2, 300, 2, seed)
    A0, _ = raw_b11(win, lam=0.0)
    win["lam"] = lam_for(A0, r, margin)
    return win


# name -> (builder, MakePosDef acts, no eigenvalue within this relative margin of eps, B11 indefinite)
SIZES_FEW = [(NB - 1, 300), (NB, 300), (NB + 1, 300), (2 * NB + 2, 300), (640, 1500), (1200, 2500)]
SIZES_MANY = [(NB - 1, 40), (NB, 40), (NB + 1, 40), (2 * NB + 2, 80), (640, 200), (1200, 500)]
CASES = {}
for _k, (_M, _N) in enumerate(SIZES_FEW):
    CASES[f"few_{_M}"] = (functools.partial(window_duplicated, _M, _N, 1 + _k % 3, 100 + _M), True, 0.5, False)
for _M, _N in SIZES_MANY:
    CASES[f"many_{_M}"] = (functools.partial(window_rank_deficient, _M, _N, 200 + _M), True, 0.5, False)
for _ws in (1.0, 1.061, 1.5):
    CASES[f"mix_w{int(round(_ws * 1000))}"] = (functools.partial(window_mixed, 2 * NB + 2, [25, 20, 30, 25], _ws, 300), True, 0.5, _ws > 1.4)
CASES["near_below"] = (functools.partial(window_near_eps, 2, 1e-2), True, 1e-2, False)
CASES["near_above"] = (functools.partial(window_near_eps, 0, 1e-2), False, 1e-2, False)
BIG = ("few_640", "many_640", "few_1200", "many_1200")

# CountPC: rank deficient, lam small: hundreds of eigenvalues sit at lam, far under the cutoff
QCAT_CASES = {"qcat_130": (2 * NB + 2, 80, 1e-3), "qcat_640": (640, 200, 1e-3)}
QCAT_HEAD, QCAT_PRED = 4, 20


def qcat_window(name):
    M, N, lam = QCAT_CASES[name]
    return window_rank_deficient(M, N, 400 + M, lam=lam)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the CPU knows about a B11 case: the window, B11 before the clamp, the oracle's run and numpy's."""
    win = CASES[name][0]()
    A, b21 = raw_b11(win)
    X, lam = clamp_numpy(A)
    z, info = solve_inv(X, b21, win["z1"])
    orc = oracle.run_impute(win["mode"], win["geno_m"], win["geno_u"], win["pop_off"], win["pop_wgt"], win["z1"], lam=win["lam"],
                            want_mats=True)
    return dict(win=win, A=A, b21=b21, X=X, lam=lam, z=z, info=info, oracle=orc)


# ---- population weights ------------------------------------------------------------------------------------------------------
def balding_nichols(sizes, P, seed, twin=None, noise=0.01):
    """Interval-major rows [study, AF_0 .. AF_(P-1)] of Balding-Nichols allele frequencies: ancestral frequency U(0.05, 0.95);
    super-populations drift from it with F_ST 0.1 .. 0.02, the populations of a super-population drift from ITS frequency with
    F_ST between 0.002 and 0.1, so columns inside a super-population correlate above 0.99 at the low end.  twin = interval whose
    last population is the first one again (F_ST = 0 between them) observed through sampling noise of sd 1e-3: nearly, not
    exactly, collinear."""
    rng = np.random.default_rng(seed)
    n_super = min(5, P)
    sup = np.arange(P) % n_super
    f_sup = np.geomspace(0.1, 0.02, n_super)
    f_pop = np.geomspace(0.1, 0.002, P)[rng.permutation(P)] if P > 1 else np.array([0.05])
    blocks = []
    for i, n in enumerate(sizes):
        anc = rng.uniform(0.05, 0.95, n)
        ps = np.empty((n, n_super))
        for s in range(n_super):
            c = (1 - f_sup[s]) / f_sup[s]
            ps[:, s] = np.clip(rng.beta(anc * c, (1 - anc) * c), 0.01, 0.99)
        af = np.empty((n, P))
        for k in range(P):
            c = (1 - f_pop[k]) / f_pop[k]
            af[:, k] = rng.beta(ps[:, sup[k]] * c, (1 - ps[:, sup[k]]) * c)
        if twin == i:
            af[:, -1] = np.clip(af[:, 0] + rng.normal(0, 1e-3, n), 0, 1)
        w = rng.dirichlet(np.ones(P))
        study = np.clip(af @ w + rng.normal(0, noise, n), 0, 1)
        blocks.append(np.column_stack([study, af]))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.ascontiguousarray(np.vstack(blocks)), off


PW_CASES = {f"bn_P{P}": functools.partial(balding_nichols, [1000, 3000], P, 500 + P) for P in (5, 26, 29, 64)}
PW_CASES["bn_twin"] = functools.partial(balding_nichols, [1000], 26, 561, twin=0)


def _exact_ints(r):
    """Finite doubles as Python integers times one power of two: (object array, exponent)."""
    m, e = np.frexp(r)
    e = e.astype(np.int64) - 53
    mi = np.ldexp(m, 53).astype(np.int64)
    emin = int(e.min())
    out = np.empty(r.shape, dtype=object)
    for idx in np.ndindex(r.shape):
        out[idx] = int(mi[idx]) << int(e[idx] - emin)
    return out, emin


def popwgt_mp(x, off, eps=EPS, dps=40):
    """The pw_* pipeline of every interval in mpmath at `dps` digits: column means, cross sums of the centred columns divided by
    n - 1 (from exact integer sums: sum (x - mx)(y - my) = sum xy - sum x sum y / n), eigsy on Cxx, the clamp rule of
    util.cpp:302-318 (when the smallest eigenvalue is below eps, every eigenvalue below eps becomes eps), and
    W = V diag(1 / L) V^T Cxy.  Returns (W [n_int, P] as float64, status, smallest eigenvalue of Cxx); an interval with fewer
    than two rows or a non-finite value is NaN with ST_NONFINITE, as in popwgt_ref.interval_weights."""
    import pytest
    mp = pytest.importorskip("mpmath")
    from popwgt_ref import ST_CLAMPED, ST_NONFINITE
    n_int, P = len(off) - 1, x.shape[1] - 1
    W = np.full((n_int, P), np.nan)
    st = np.zeros(n_int, dtype=np.int32)
    lmin = np.full(n_int, np.nan)
    with mp.workdps(dps):
        for i in range(n_int):
            r = np.asarray(x[off[i]:off[i + 1]], dtype=np.float64)
            n = r.shape[0]
            if n < 2 or not np.all(np.isfinite(r)):
                st[i] = ST_NONFINITE
                continue
            xi, e = _exact_ints(r)
            sxy = xi.T @ xi
            sx = xi.sum(0)
            C = mp.matrix(P + 1, P + 1)
            for a in range(P + 1):
                for b in range(a, P + 1):
                    C[a, b] = C[b, a] = mp.ldexp(mp.mpf(int(sxy[a, b])) - mp.mpf(int(sx[a])) * int(sx[b]) / n, 2 * e) / (n - 1)
            lam, Q = mp.eigsy(C[1:, 1:])
            lam = [lam[k] for k in range(P)]
            lmin[i] = float(min(lam))
            if min(lam) < eps:
                st[i] = ST_CLAMPED
                lam = [mp.mpf(eps) if v < eps else v for v in lam]
            w = [mp.mpf(0)] * P
            for k in range(P):
                proj = sum(Q[a, k] * C[a + 1, 0] for a in range(P)) / lam[k]
                for a in range(P):
                    w[a] += Q[a, k] * proj
            W[i] = [float(v) for v in w]
    return W, st, lmin


@functools.lru_cache(maxsize=None)
def pw_reference(name):
    from popwgt_ref import interval_weights
    x, off = PW_CASES[name]()
    return dict(x=x, off=off, np=interval_weights(x, off), mp=popwgt_mp(x, off))


def werr(got, want):
    """Per interval max |got - want| / max(1, max |want|): the scale of test_gpu_popwgt.py::_check."""
    return np.array([np.max(np.abs(g - w)) / max(1.0, float(np.max(np.abs(w)))) for g, w in zip(got, want)])


# ---- the levels --------------------------------------------------------------------------------------------------------------
def b11_level(name):
    """How far the oracle (hand-written Jacobi and full-pivot LU) and numpy (eigh, inv) disagree on one case, and how far two
    operation orders of the solve disagree on one and the same matrix."""
    ref = reference(name)
    o = ref["oracle"]
    zc, ic = solve_chol(ref["X"], ref["b21"], ref["win"]["z1"])
    cert = max(certificate_level(clamp_certificate(ref["A"], m)) for m in (ref["X"], o["b11"]))
    return dict(M=int(ref["A"].shape[0]), lifted=int(np.sum(ref["lam"] < EPS)), lam_min=float(ref["lam"][0]), mpd=int(o["mpd"]),
                b11=float(np.max(np.abs(o["b11"] - ref["X"]))), cert=float(cert), info=relerr(o["info"], ref["info"]),
                z=zerr(o["z"], ref["z"]), info_own=relerr(ic, ref["info"]), z_own=zerr(zc, ref["z"]))


def qcat_level(name):
    win = qcat_window(name)
    A, _ = raw_b11(win)
    lam = np.linalg.eigvalsh(A)
    o = oracle.run_qcat(win["mode"], win["geno_m"], win["geno_u"], win["pop_off"], None, win["z1"], QCAT_HEAD, QCAT_PRED, lam=win["lam"],
                        eig_cutoff=QCAT_CUTOFF)
    return dict(M=int(A.shape[0]), below=int(np.sum(lam < QCAT_CUTOFF)), num_eig=int(A.shape[0] - np.sum(lam < QCAT_CUTOFF)),
                oracle_num_eig=int(o["num_eig"]), nearest=float(np.min(np.abs(lam / QCAT_CUTOFF - 1.0))))


def pw_level(name):
    ref = pw_reference(name)
    return dict(w=float(np.max(werr(ref["np"][0], ref["mp"][0]))), lam_min=[float(v) for v in ref["mp"][2]],
                clamped=[int(v) for v in ref["mp"][1]])


def measure_levels():
    return dict(b11={k: b11_level(k) for k in CASES}, qcat={k: qcat_level(k) for k in QCAT_CASES},
                popwgt={k: pw_level(k) for k in PW_CASES})


def load_levels():
    with open(LEVELS_PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    levels = measure_levels()
    with open(LEVELS_PATH, "w") as f:
        json.dump(levels, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(levels, indent=1, sort_keys=True))
