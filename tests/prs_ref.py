"""The polygenic score weights of a window (include/gauss_hip.h, prs_*) in numpy, stated twice on given (B, z): B = B11 with the ridge
on its diagonal, z = z1.  r_j = z_j / sqrt(n - 2 + z_j^2); a SNP whose z is not finite is frozen (r = 0, beta = 0, never updated).  For
each s a chain starts from beta = 0 and takes the penalties in the order given, each from the solution of the one before.  One sweep,
j = 0 .. M - 1 in order, frozen j skipped:
    u = r_j - (1 - s) ((B beta)_j - B_jj beta_j);   b' = sign(u) (|u| - lam) / ((1 - s) B_jj + s) if |u| > lam else 0;   beta_j = b'
delta = the largest |b' - beta_j| of the sweep; the penalty is left when delta < tol * r_max (or r_max = 0), or after max_sweeps sweeps.

fit_cov carries g = B beta and updates it with one multiply and one add per entry, which is what the kernel does, in the kernel's order.
fit_textbook carries nothing: it forms B_j . beta with np.dot at every coordinate.  e_ref(a, b) is the largest gap between the two on a
case: what the order of the sums is worth there."""
import math

import numpy as np

DEFAULT_S = (0.2, 0.5, 0.9, 1.0)
DEFAULT_LAM = tuple(float(v) for v in np.exp(np.linspace(np.log(0.1), np.log(0.001), 20)))      # lassosum's path
DEFAULTS = dict(s=DEFAULT_S, lam=DEFAULT_LAM, tol=1e-4, max_sweeps=100)
ONE_CELL = dict(s=(0.5,), lam=(0.02,))
N_STUDY = 5000.0                             # the sample size of the test studies: a planted z of 10 is a correlation of 0.14
VALUE_KEYS = ("beta", "br", "bg", "delta")
EXACT_KEYS = ("nnz", "sweeps", "noconv")


def args_of(**kw):
    a = dict(DEFAULTS)
    a.update(kw)
    a["s"], a["lam"] = tuple(float(v) for v in a["s"]), tuple(float(v) for v in a["lam"])
    return a


def p2cor(z, n):
    """(r, frozen): lassosum's p2cor; a frozen SNP has r = 0"""
    z = np.asarray(z, dtype=np.float64)
    frozen = ~np.isfinite(z)
    with np.errstate(invalid="ignore"):
        r = z / np.sqrt(n - 2 + z ** 2)
    r[frozen] = 0.0
    return r, frozen


def kkt(B, r, s, lam, beta, frozen=None):
    """The largest KKT residual of beta at (s, lam), from a fresh B beta: |q_j - lam sign(beta_j)| on the support, max(0, |q_j| - lam)
    off it, q = r - (1 - s) B beta - s beta.  Also returns the residual per SNP and the sum of the absolute terms of q_j (its rounding)."""
    q = r - (1.0 - s) * (B @ beta) - s * beta
    res = np.where(beta != 0, np.abs(q - lam * np.sign(beta)), np.maximum(0.0, np.abs(q) - lam))
    mag = np.abs(r) + (1.0 - s) * (np.abs(B) @ np.abs(beta)) + s * np.abs(beta) + lam
    if frozen is not None:
        res = np.where(frozen, 0.0, res)
    return float(res.max(initial=0.0)), res, mag


def _fit(B, z, n, textbook, **kw):
    a = args_of(**kw)
    B = np.ascontiguousarray(B, dtype=np.float64)
    M = B.shape[0]
    r_arr, frozen = p2cor(z, n)
    r = [float(v) for v in r_arr]
    live = [j for j in range(M) if not frozen[j]]
    diag = [float(B[j, j]) for j in range(M)]
    rmax = max([abs(r[j]) for j in live], default=0.0)
    thr = a["tol"] * rmax
    ns, nl = len(a["s"]), len(a["lam"])
    out = dict(beta=np.zeros((ns, nl, M)), nnz=np.zeros((ns, nl), dtype=np.int64), sweeps=np.zeros((ns, nl), dtype=np.int64),
               delta=np.zeros((ns, nl)), br=np.zeros((ns, nl)), bg=np.zeros((ns, nl)), kkt=np.zeros((ns, nl)),
               noconv=np.zeros((ns, nl), dtype=bool), margin=np.full((ns, nl), np.inf), deltas=[[None] * nl for _ in range(ns)],
               r=r_arr, frozen=frozen, rmax=rmax, thr=thr, coord_steps=0, row_updates=0)
    for i_s, s in enumerate(a["s"]):
        oms = 1.0 - s
        beta = np.zeros(M)
        g = np.zeros(M)
        for i_l, lam in enumerate(a["lam"]):
            deltas = []
            for sw in range(a["max_sweeps"]):
                delta, margin = 0.0, math.inf
                for j in live:
                    bj, bjj = float(beta[j]), diag[j]
                    gj = float(np.dot(B[j], beta)) if textbook else float(g[j])
                    u = r[j] - oms * (gj - bjj * bj)
                    au = abs(u)
                    margin = min(margin, abs(au - lam))
                    bn = math.copysign(au - lam, u) / (oms * bjj + s) if au > lam else 0.0
                    d = bn - bj
                    out["coord_steps"] += 1
                    if d != 0.0:
                        if not textbook:
                            g += d * B[j]
                        beta[j] = bn
                        delta = max(delta, abs(d))
                        out["row_updates"] += 1
                deltas.append(delta)
                if delta < thr or rmax == 0.0:
                    break
            gg = B @ beta if textbook else g
            br = bg = 0.0
            for j in range(M):
                br += float(beta[j]) * r[j]
                bg += float(beta[j]) * float(gg[j])
            q = r_arr - oms * gg - s * beta
            res = np.where(beta != 0, np.abs(q - np.copysign(lam, beta)), np.maximum(0.0, np.abs(q) - lam))
            res[frozen] = 0.0
            out["beta"][i_s, i_l] = beta
            out["nnz"][i_s, i_l] = int(np.count_nonzero(beta))
            out["sweeps"][i_s, i_l] = len(deltas)
            out["delta"][i_s, i_l] = deltas[-1]
            out["br"][i_s, i_l], out["bg"][i_s, i_l] = br, bg
            out["kkt"][i_s, i_l] = float(res.max(initial=0.0))
            out["noconv"][i_s, i_l] = not (deltas[-1] < thr or rmax == 0.0)
            out["margin"][i_s, i_l] = margin           # the smallest | |u| - lam | of the last sweep
            out["deltas"][i_s][i_l] = deltas
    return out


def fit_cov(B, z, n, **kw):
    """Exactly the update of the definition, with g = B beta carried"""
    return _fit(B, z, n, False, **kw)


def fit_textbook(B, z, n, **kw):
    """The same coordinate descent with B_j . beta recomputed by np.dot at every coordinate; no g"""
    return _fit(B, z, n, True, **kw)


def e_ref(x, y):
    """The largest gap between two fits of one case over beta, br, bg and delta"""
    return max(float(np.max(np.abs(x[k] - y[k]), initial=0.0)) for k in VALUE_KEYS)


def value_tol(res, e):
    """The absolute bound on beta, br, bg and delta: ten times the gap between the reference's two statements, or the project's fp64
    bound 1e-8 relative to the largest weight"""
    return max(10.0 * e, 1e-8 * max(1.0, float(np.max(np.abs(res["beta"]), initial=0.0))))


def borderline(B, z, n, **kw):
    """(list of the decisions of the case that rounding could turn, fit_cov's result, e_ref).  A sweep's delta within 10 e_ref of the
    stop threshold could end a penalty a sweep earlier or later; a | |u| - lam | of a last sweep within the value bound of 0 is a
    support decision."""
    want, tb = fit_cov(B, z, n, **kw), fit_textbook(B, z, n, **kw)
    e = e_ref(want, tb)
    tol_v = value_tol(want, e)
    out = []
    for k in EXACT_KEYS:
        if not np.array_equal(want[k], tb[k]):
            out.append(f"the two statements differ in {k}")
    ns, nl = want["nnz"].shape
    for i_s in range(ns):
        for i_l in range(nl):
            if want["rmax"] > 0 and any(abs(d - want["thr"]) <= 10.0 * e for d in want["deltas"][i_s][i_l]):
                out.append(f"stop: a delta of cell ({i_s}, {i_l}) within 10 e_ref of tol r_max")
            if want["margin"][i_s, i_l] <= tol_v:
                out.append(f"support: | |u| - lam | = {want['margin'][i_s, i_l]:.1e} in the last sweep of cell ({i_s}, {i_l})")
    return out, want, e


# ---- the windows of tests/test_gpu_prs.py, built here so that tests/test_prs_ref.py can vet them on the CPU ---------------------
def mats(mode, gm, gu, off, w, lam=0.1):
    from cond_ref import window_mats
    return window_mats(mode, gm, gu, off, w) if lam == 0.1 else window_mats(mode, gm, gu, off, w, lam)


def small_window(M, U, seed):
    """(p, gm, gu, z1): cs_ref's window with three planted measured signals"""
    import cs_ref
    p, gm, gu = cs_ref.window(M, U)
    return p, gm, gu, cs_ref.planted(gm, seed=seed)


# (M, U, grid, seed of the Z-scores, mode): M on either side of a wave's 64 lanes and of the workgroup's 256, one SNP, two SNPs, more
# than one pass of the workgroup over a row (300); each on pooled (0) and weighted (1) LD, with the default grid and with one cell
# from a cold start.  tests/test_prs_ref.py vets every (case, seed) on the CPU.
SHAPES = (1, 2, 63, 64, 65, 255, 256, 257, 300)
SEEDS = {}
SMALL_CASES = [(M, 3, grid, SEEDS.get((M, mode, gi), 100 + M + mode), mode)
               for M in SHAPES for mode in (0, 1) for gi, grid in enumerate((dict(), dict(ONE_CELL)))]
LARGE_CASE = (1213, 2512, dict(), 1215)      # chr22's largest window, weighted LD, default grid
NOCONV_CASE = (129, 5, dict(max_sweeps=2), 14)
FROZEN_CASE = (65, 4, dict(), 9, (5, 40))    # ..., the SNPs whose z is NaN / inf


def case_id(c):
    return f"M{c[0]}-U{c[1]}-{'one' if c[2].get('lam') else 'grid'}-mode{c[4]}"
