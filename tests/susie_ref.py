"""Reference statements of the multi-causal fine-mapping of a window (test infrastructure, numpy only).

Definition (include/gauss_hip.h, susie_*): B = B11 [M x M] of a window (lambda on the diagonal), C = B21 [U x M], z = z1,
A = [B | C^T], R = A^T B^-1 A, zhat = A^T B^-1 z = [z ; m], d = diag(R).  The candidates are the M measured SNPs, then the U
unmeasured ones.  The fit is IBSS with Gauss-Seidel sweeps over l = 1 .. L; the sets, their purity, `kept` and the per-SNP summaries
follow from the final alpha.  Two statements of the same fit:

* ``fit_textbook`` forms R and zhat explicitly with np.linalg.solve and multiplies by R;
* ``fit_w`` states what the kernels evaluate: W = B^-1 C^T once, then v = bbar_meas + W bbar_unmeas, R bbar = [B v ; C v]; the
  purity's R_ij are B_ij, C_ui and c_u . W_v.

``plain_rss`` is an independent plain SuSiE-RSS loop on (z, B) alone that shares no helper with them: with measured_only the two
statements must return its alpha.

``borderline`` lists the decisions a rounding error could turn (tests/test_susie_ref.py vets every committed case): a null check
with |lse(V')| <= 1e-6, a stop with |delta - tol| <= 1e-3 tol, a purity within 1e-6 of min_abs_corr, a membership whose mass ahead
is within the value tolerance of rho (cs_ref.borderline's rule).
"""
import numpy as np

DEFAULTS = dict(L=10, coverage=0.95, prior_var=25.0, tol=1e-4, max_sweeps=100, min_abs_corr=0.5, estimate_var=True, measured_only=False)
PURITY_N = 128


def args_of(**kw):
    a = dict(DEFAULTS)
    a.update(kw)
    return a


def _lbf(r, d, V):
    if V == 0.0:
        return np.zeros_like(r)
    return 0.5 * (r * r * V / (1.0 + V * d) - np.log1p(V * d))


def _ser(r, d, adm, V):
    """One single-effect update: (alpha, mu, lbf, lse, s2) over the admissible candidates, zeros elsewhere"""
    T = len(r)
    alpha, mu, lbf, s2 = np.zeros(T), np.zeros(T), np.full(T, -np.inf), np.zeros(T)
    n_adm = int(adm.sum())
    if n_adm == 0:
        return alpha, mu, lbf, np.nan, s2
    lb = _lbf(r[adm], d[adm], V)
    mx = lb.max()
    e = np.exp(lb - mx)
    tot = e.sum()
    alpha[adm] = e / tot
    s2[adm] = V / (1.0 + V * d[adm])
    mu[adm] = s2[adm] * r[adm]
    lbf[adm] = lb
    return alpha, mu, lbf, mx + np.log(tot / n_adm), s2


def _ibss(zhat, d, adm, rmul, a):
    """The fit given zhat, d, the admissibility flags and b -> R b.  Records every null check and the delta of every sweep."""
    T, L = len(zhat), a["L"]
    alpha, mu, lbf = np.zeros((L, T)), np.zeros((L, T)), np.full((L, T), -np.inf)
    rb, f = np.zeros((L, T)), np.zeros(T)
    V, lse = np.full(L, float(a["prior_var"])), np.full(L, np.nan)
    null_lse, deltas = [], []
    sweeps, converged = 0, False
    for _ in range(a["max_sweeps"]):
        Vn, prev = V.copy(), alpha.copy()
        for l in range(L):
            with np.errstate(invalid="ignore"):
                r = zhat - (f - rb[l])
            alpha[l], mu[l], lbf[l], lse[l], s2 = _ser(r, d, adm, V[l])
            new = rmul(alpha[l] * mu[l])
            f = (f - rb[l]) + new
            rb[l] = new
            if a["estimate_var"] and V[l] != 0.0:
                v1 = float(np.sum(alpha[l][adm] * (mu[l][adm] ** 2 + s2[adm])))
                l1 = _ser(r, d, adm, v1)[3]
                null_lse.append(l1)
                Vn[l] = 0.0 if l1 <= 0.0 else v1
        V = Vn
        sweeps += 1
        deltas.append(float(np.max(np.abs(alpha - prev))))
        if deltas[-1] < a["tol"]:
            converged = True
            break
    with np.errstate(invalid="ignore", divide="ignore"):
        rmax = float(np.nanmax(np.abs(zhat[adm]) / np.sqrt(d[adm]))) if adm.any() else 0.0
    return dict(alpha=alpha, mu=mu, lbf=lbf, V=V, lse=lse, sweeps=sweeps, delta=deltas[-1], deltas=deltas, converged=converged,
                null_lse=np.array(null_lse), rmax=rmax, adm=adm, d=d, zhat=zhat)


def _sets(res, rij, a, M):
    """Sets, purity, kept and the per-SNP summaries from the final alpha; rij(i, j) = R_ij"""
    alpha, V, d = res["alpha"], res["V"], res["d"]
    L, T = alpha.shape
    rho = a["coverage"]
    idx = np.arange(T)
    member, ahead = np.zeros((L, T), dtype=bool), np.zeros((L, T))
    purity, kept = np.full(L, np.nan), np.zeros(L, dtype=bool)
    for l in range(L):
        order = np.lexsort((idx, -alpha[l]))
        ahead[l, order] = np.concatenate([[0.0], np.cumsum(alpha[l][order])[:-1]])
        member[l] = (alpha[l] > 0) & ((ahead[l] < rho) | (rho >= 1.0))
        top = [int(j) for j in order[: min(int(member[l].sum()), PURITY_N)]]
        if len(top) == 1:
            purity[l] = 1.0
        elif len(top) > 1:
            purity[l] = min(abs(rij(i, j)) / np.sqrt(d[i] * d[j]) for k, i in enumerate(top) for j in top[k + 1:])
        kept[l] = V[l] > 0 and purity[l] >= a["min_abs_corr"] and not any(kept[k] and np.array_equal(member[k], member[l]) for k in range(l))
    keep, sset, set_pip = np.ones(T), np.full(T, -1, dtype=np.int64), np.zeros(T)
    for l in range(L):
        if V[l] > 0:
            keep = keep * (1.0 - alpha[l])
        better = kept[l] & member[l] & ((sset < 0) | (alpha[l] > set_pip))
        sset[better] = l
        set_pip[better] = alpha[l][better]
    res.update(member=member, ahead=ahead, purity=purity, kept=kept, pip=1.0 - keep, set=sset, set_pip=set_pip,
               size=member.sum(axis=1).astype(np.int64), mass=np.where(member, alpha, 0.0).sum(axis=1), M=M)
    return res


def _admissible(zhat, d, M, z, a):
    with np.errstate(invalid="ignore"):
        adm = np.isfinite(zhat) & np.isfinite(d) & (d > 0)
    if a["measured_only"] or not np.all(np.isfinite(z)):
        adm[M:] = False
    return adm


def fit_textbook(B, C, z, **kw):
    a = args_of(**kw)
    B, C, z = np.asarray(B, dtype=np.float64), np.asarray(C, dtype=np.float64), np.asarray(z, dtype=np.float64)
    M = len(z)
    A = np.hstack([B, C.T])
    R = A.T @ np.linalg.solve(B, A)
    zhat = A.T @ np.linalg.solve(B, z)
    zhat[:M] = z                                                # (B B^-1 z: the measured part is z itself, to the bit)
    d = np.diag(R).copy()
    adm = _admissible(zhat, d, M, z, a)
    Rs = R.copy()
    Rs[:, ~adm] = 0.0                                           # an inadmissible candidate's bbar is 0: its (possibly non-finite) column is not read
    res = _ibss(zhat, d, adm, lambda b: Rs @ b, a)
    return _sets(res, lambda i, j: R[i, j], a, M)


def fit_w(B, C, z, **kw):
    a = args_of(**kw)
    B, C, z = np.asarray(B, dtype=np.float64), np.asarray(C, dtype=np.float64), np.asarray(z, dtype=np.float64)
    M = len(z)
    W = np.linalg.solve(B, C.T)                                 # [M, U]
    info = np.einsum("um,mu->u", C, W)
    zhat = np.concatenate([z, C @ np.linalg.solve(B, z)])
    d = np.concatenate([np.diag(B), info])
    adm = _admissible(zhat, d, M, z, a)

    def rmul(b):
        v = b[:M] + W @ b[M:]
        return np.concatenate([B @ v, C @ v])

    def rij(i, j):
        i, j = min(i, j), max(i, j)
        if j < M:
            return B[i, j]
        if i < M:
            return C[j - M, i]
        return float(C[i - M] @ W[:, j - M])

    res = _ibss(zhat, d, adm, rmul, a)
    return _sets(res, rij, a, M)


def plain_rss(z, R, L, prior_var, max_sweeps, tol, estimate_var):
    """SuSiE-RSS on (z, R) as the paper writes it -- residual variance 1, uniform prior, EM update of the prior variance with the null
    check -- in plain loops, sharing nothing with the functions above.  Returns alpha [L, M]."""
    M = len(z)
    alpha = [[0.0] * M for _ in range(L)]
    post = [[0.0] * M for _ in range(L)]
    V = [float(prior_var)] * L

    def bf(r, V_):
        out = []
        for j in range(M):
            out.append(0.0 if V_ == 0.0 else 0.5 * (r[j] ** 2 * V_ / (1.0 + V_ * R[j][j]) - np.log1p(V_ * R[j][j])))
        return out

    for _ in range(max_sweeps):
        Vn, old = list(V), [list(row) for row in alpha]
        for l in range(L):
            others = [sum(alpha[k][j] * post[k][j] for k in range(L) if k != l) for j in range(M)]
            r = [z[i] - sum(R[i][j] * others[j] for j in range(M)) for i in range(M)]
            lb = bf(r, V[l])
            top = max(lb)
            w = [np.exp(x - top) for x in lb]
            tot = sum(w)
            for j in range(M):
                s2 = V[l] / (1.0 + V[l] * R[j][j])
                alpha[l][j], post[l][j] = w[j] / tot, s2 * r[j]
            if estimate_var and V[l] != 0.0:
                v1 = sum(alpha[l][j] * (post[l][j] ** 2 + V[l] / (1.0 + V[l] * R[j][j])) for j in range(M))
                lb1 = bf(r, v1)
                top1 = max(lb1)
                Vn[l] = 0.0 if top1 + np.log(sum(np.exp(x - top1) for x in lb1) / M) <= 0.0 else v1
        V = Vn
        if max(abs(alpha[l][j] - old[l][j]) for l in range(L) for j in range(M)) < tol:
            break
    return np.array(alpha)


VALUE_KEYS = ("alpha", "mu", "pip", "set_pip", "mass", "lse", "V", "purity")
EXACT_KEYS = ("size", "set", "kept", "sweeps")


def gap(x, y):
    """Largest absolute difference of the value outputs of two results (NaN against NaN counts as equal)"""
    g = 0.0
    for k in VALUE_KEYS:
        p, q = np.asarray(x[k], dtype=np.float64), np.asarray(y[k], dtype=np.float64)
        both = np.isnan(p) & np.isnan(q)
        with np.errstate(invalid="ignore"):
            dlt = np.where(both, 0.0, np.abs(p - q))
        g = max(g, float(np.max(dlt)) if dlt.size else 0.0)
    return g


def value_tol(res, e_ref):
    """The bound on alpha, mu, pip, set_pip, mass, lse, V and purity: ten times the gap between the two statements of the reference (the
    GPU's sums have a third order of their own), or the project's 1e-8 on solve outputs carried through a Bayes factor (cs_ref.pip_tol's
    reasoning): a residual r_j / sqrt(d_j) off by 1e-8 max(1, |.|) moves lbf by at most max(1, r_max^2) 1e-8, a pip by twice that."""
    return max(10.0 * e_ref, 2.0 * max(1.0, res["rmax"] ** 2) * 1e-8)


def borderline(res, a, tol_v):
    """The decisions of a fit that a rounding error could turn, as a list of strings (empty: none)"""
    a = args_of(**a)
    out = []
    if res["null_lse"].size and np.any(np.abs(res["null_lse"]) <= 1e-6):
        out.append("null check: |lse(V')| <= 1e-6")
    if a["tol"] > 0:
        for s, dlt in enumerate(res["deltas"]):
            if abs(dlt - a["tol"]) <= 1e-3 * a["tol"]:
                out.append(f"stop: delta of sweep {s + 1} within 1e-3 tol of tol")
    rho = a["coverage"]
    for l in range(res["alpha"].shape[0]):
        p = res["alpha"][l]
        if np.isfinite(res["purity"][l]) and res["V"][l] > 0 and abs(res["purity"][l] - a["min_abs_corr"]) <= 1e-6:
            out.append(f"purity of set {l} within 1e-6 of min_abs_corr")
        if rho >= 1.0:
            with np.errstate(invalid="ignore", divide="ignore"):
                lp = np.log(p[res["adm"]])
            if np.any((lp > -760.0) & (lp < -700.0)):
                out.append(f"set {l}: an alpha at the edge of the double range")
            continue
        order = np.argsort(p, kind="stable")
        ps = p[order]
        csum = np.concatenate([[0.0], np.cumsum(ps)])
        lo, hi = np.searchsorted(ps, ps - tol_v, side="left"), np.searchsorted(ps, ps + tol_v, side="right")
        near = np.zeros(len(p))
        near[order] = csum[hi] - csum[lo] - ps
        turn = (p > 0) & (np.abs(rho - res["ahead"][l]) <= max(tol_v, 1e-6) + near)
        if res["V"][l] > 0 and np.any(turn):                   # (a set of V_l = 0 is never kept: its members decide nothing)
            out.append(f"set {l}: the mass ahead of SNP {int(np.flatnonzero(turn)[0])} within the tolerance of rho")
    return out


# ---- the windows of tests/test_gpu_susie.py, built here so that tests/test_susie_ref.py can vet them on the CPU ----------------------
def mats(mode, gm, gu, off, w, lam=0.1):
    from cond_ref import window_mats
    return window_mats(mode, gm, gu, off, w) if lam == 0.1 else window_mats(mode, gm, gu, off, w, lam)


def small_window(M, U, seed):
    """(p, gm, gu, z1): cs_ref's window with three planted measured signals"""
    import cs_ref
    p, gm, gu = cs_ref.window(M, U)
    return p, gm, gu, cs_ref.planted(gm, seed=seed)


# (M, U, susie arguments, (seed of the Z-scores under pooled LD, under weighted LD)).  T = 2, 5, 23; rows of M on either side of
# SUSIE_VR = 8 (7, 8, 9) and of the wave's 64 columns (63, 65); T on either side of SUSIE_RR = 8 (M + U = 7, 8, 9), of SUSIE_T = 256
# (255, 257), of cs_tld's 16, of SUSIE_CH = 1024 unmeasured candidates (U = 1023, 1024, 1025) and of the CS_LDS_T = 4096 candidates
# cs_set_row keeps in LDS (T = 4096, 4104); candidate blocks of 256 that straddle M (M = 250, U = 30); L = 1, 10, 32; tol = 0 with 1, 2,
# 5, 30 sweeps; estimate_var on and off (off with as many effects as signals: an effect that cannot switch off spreads over the whole
# window, and a set of hundreds of near-equal alpha has borderline members); measured_only.  Every case runs on pooled and on weighted
# LD; each (case, mode) has the seed tests/test_susie_ref.py vets.  (L = 32 on 129 + 129 runs 30 sweeps: under weighted LD, whose
# weights do not sum to one, the noise keeps the spare effects alive, and after 5 sweeps their sets are still borderline.)
SMALL_CASES = [
    (1, 1, dict(L=1, tol=0.0, max_sweeps=1), (3, 3)),
    (2, 3, dict(L=10, tol=0.0, max_sweeps=2), (4, 4)),
    (12, 11, dict(L=10, tol=0.0, max_sweeps=5), (14, 14)),
    (3, 4, dict(L=1, tol=0.0, max_sweeps=5, estimate_var=False), (5, 5)),
    (7, 1, dict(L=3, tol=0.0, max_sweeps=2), (6, 6)),
    (8, 1, dict(L=3, tol=0.0, max_sweeps=5), (7, 7)),
    (9, 7, dict(L=32, tol=0.0, max_sweeps=2), (8, 8)),
    (63, 192, dict(L=10, tol=0.0, max_sweeps=5), (10, 10)),
    (65, 192, dict(L=10, tol=0.0, max_sweeps=30), (10, 11)),
    (250, 30, dict(L=3, tol=0.0, max_sweeps=5, estimate_var=False), (11, 11)),
    (127, 128, dict(L=10, tol=0.0, max_sweeps=30, measured_only=True), (12, 12)),
    (129, 129, dict(L=32, tol=0.0, max_sweeps=30), (13, 16)),
    (40, 1023, dict(L=10, tol=0.0, max_sweeps=2), (15, 19)),
    (40, 1024, dict(L=10, tol=0.0, max_sweeps=2), (15, 15)),
    (40, 1025, dict(L=5, tol=0.0, max_sweeps=5), (16, 22)),
    (56, 4040, dict(L=2, tol=0.0, max_sweeps=1), (20, 20)),
    (64, 4040, dict(L=2, tol=0.0, max_sweeps=2), (21, 21)),
]
SMALL_CASE_MODES = [(c[0], c[1], c[2], c[3][mode], mode) for c in SMALL_CASES for mode in (0, 1)]
# (L = 4: with ten effects on three planted signals the spare ones are still spread over the window after 5 sweeps, and a set of a
# thousand near-equal alpha has borderline members)
LARGE_CASE = (1213, 2512, dict(L=4, tol=0.0, max_sweeps=5), 1214)
CONVERGENCE_CASE = (129, 129, dict(L=10), 13)
COVERAGE_CASES = [dict(coverage=0.5), dict(coverage=1.0)]
COVERAGE_WINDOW = (127, 128, 17)
NOCONV_CASE = (129, 129, dict(L=10, max_sweeps=2), 14)


def tag_window(seed=3):
    """Planted window (a): two causal SNPs that share one measured tag with the largest marginal |z|.  The causal SNPs c1, c2 are
    measured and uncorrelated (|r| < 0.05); the tag's genotypes are their clipped sum with 15 % of the samples shuffled: r = 0.60 and
    0.58 with them, so its marginal z is about 1.2 times theirs -- but it is NOT their sum, and the two-SNP model fits better.  (With
    an exact sum the tag alone and the pair are the same model; with 10 % shuffled IBSS stays at the tag; at 25 % the tag no longer
    leads.)  Returns (p, gm, gu, z1, (c1, c2, tag)) -- pooled LD."""
    from cond_ref import window_mats
    from helpers import small_panel, split_window
    p = small_panel(n_snp=160, scale=0.02, seed=29)
    gm, gu, _ = split_window(dict(G=p["G"][:150]), 100)
    c1, c2, tag = 52, 70, 97
    rng = np.random.default_rng(1)
    t = np.clip(gm[c1].astype(np.int64) + gm[c2].astype(np.int64), 0, 2)
    pick = rng.random(t.size) < 0.15
    t2 = t.copy()
    t2[pick] = rng.permutation(t)[pick]
    gm = gm.copy()
    gm[tag] = t2.astype(gm.dtype)
    B, _ = window_mats(0, gm, gu, p["off"], None)
    z1 = B[:, [c1, c2]] @ np.array([9.0, 9.0]) + 0.5 * np.random.default_rng(seed).standard_normal(gm.shape[0])
    return p, np.ascontiguousarray(gm), gu, z1, (c1, c2, tag)
