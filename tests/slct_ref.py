"""Reference statements of the stepwise conditional signal selection (test infrastructure, numpy only).

Definition (include/gauss_hip.h, slct_*): with B = B11 of a window (lambda on the diagonal, repaired if MakePosDef acted), z = z1
and S the ordered set of selected SNPs, the statistic of SNP i given S is

    zc_i = (z_i - B_iS B_SS^-1 z_S) / sqrt(B_ii - B_iS B_SS^-1 B_Si)

and selection is greedy: forced SNPs first, then at every step the admissible SNP (not selected, variance left above
min_var_frac * B_ii) with the largest zc_i^2 (ties: the smallest index; a NaN never wins) until the largest falls below chi2_stop
or K SNPs are in.  Two routes with no shared arithmetic:

* ``slct_recurrence`` is the partial Cholesky recurrence the GPU kernel evaluates (k_slct.hip);
* ``slct_by_definition`` takes every step's statistics from ``np.linalg.solve`` on B_SS and the joint z from ``np.linalg.inv``.

Both return, per step, ``margin``: the smallest relative distance of the chosen chi^2 from the runner-up, of the chosen (at the
stopping step: the best) chi^2 from chi2_stop, and of every unselected SNP's variance left from its guard -- the room a rounding
error has before it changes a decision.  Exact equality of the selected indices means something only while it is positive.
"""
import numpy as np


def _pick(chi2, adm):
    """(index of the best admissible chi^2 or -1, its value, the runner-up's value or None): ties to the smaller index, NaN never wins."""
    cand = np.nonzero(adm & ~np.isnan(chi2))[0]
    if len(cand) == 0:
        return -1, None, None
    c = chi2[cand]
    k = int(np.argmax(c))                                  # first maximum = smallest index
    rest = np.delete(c, k)
    return int(cand[k]), float(c[k]), (float(rest.max()) if len(rest) else None)


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def _guard_margin(v, diag, sel, mvf):
    """every unselected SNP's variance left against its guard, relative to B_ii (v / B_ii is a share in [0, 1])"""
    free = np.ones(len(v), dtype=bool)
    free[list(sel)] = False
    d = np.abs(v[free] / diag[free] - mvf)
    d = d[~np.isnan(d)]
    return float(d.min()) if len(d) else np.inf


def _run(B, z, K, chi2_stop, min_var_frac, forced, state, enter):
    """The greedy rule, shared: `state(sel)` returns (r, v) given the selected list, `enter(j)` records SNP j.  Only the bookkeeping
    is common to the two routes -- what r and v are is theirs."""
    M = len(z)
    diag = np.diag(B).copy()
    sel, zin, margin = [], [], []
    skipped = 0
    forced = [int(f) for f in forced]
    r, v = state(sel)
    for t in range(K):
        with np.errstate(invalid="ignore", divide="ignore"):
            adm = v > min_var_frac * diag
            if sel:
                adm[sel] = False
            chi2 = r * r / v
        m = _guard_margin(v, diag, sel, min_var_frac)
        if t < len(forced):
            j = forced[t]
            margin.append(m)
            if not adm[j]:
                skipped = 1
                continue
        else:
            j, best, second = _pick(chi2, adm)
            if j < 0:
                margin.append(m)
                break
            m = min(m, _rel(best, chi2_stop))
            if best < chi2_stop:
                margin.append(m)
                break
            if second is not None:
                m = min(m, _rel(best, second))
            margin.append(m)
        with np.errstate(invalid="ignore"):
            zin.append(r[j] / np.sqrt(v[j]))
        sel.append(j)
        enter(j)
        r, v = state(sel)
    margin.append(_guard_margin(v, diag, sel, min_var_frac))      # the final state decides where zc is NaN
    with np.errstate(invalid="ignore", divide="ignore"):
        adm = v > min_var_frac * diag
        if sel:
            adm[sel] = False
        zc = np.where(adm, r / np.sqrt(v), np.nan)
        var_left = v / diag
    return dict(n=len(sel), idx=np.array(sel, dtype=np.int64), zin=np.array(zin), zc=zc, var=var_left, skipped=skipped,
                margin=margin, min_margin=float(min(margin)))


def slct_recurrence(B, z, K, chi2_stop, min_var_frac, forced=()):
    """The partial Cholesky factorisation whose pivot is the largest conditional chi^2: r, v and the selected columns W are updated
    step by step, the sums in ascending order of s; joint z by substitution on L = [W[b][sel[a]]]."""
    B = np.asarray(B, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    M = len(z)
    st = dict(r=z.copy(), v=np.diag(B).copy(), W=[], sel=[])

    def enter(j):
        r, v, W = st["r"], st["v"], st["W"]
        sq = np.sqrt(v[j])
        zin = r[j] / sq
        s = np.zeros(M)
        for ws in W:
            s = s + ws * ws[j]
        w = (B[j] - s) / sq
        st["r"] = r - w * zin
        st["v"] = v - w * w
        W.append(w)
        st["sel"].append(j)

    out = _run(B, z, K, chi2_stop, min_var_frac, forced, lambda sel: (st["r"], st["v"]), enter)
    n = out["n"]
    L = np.array([[st["W"][b][st["sel"][a]] if b <= a else 0.0 for b in range(n)] for a in range(n)]).reshape(n, n)
    joint = np.zeros(n)
    y = out["zin"]                                         # L y = z_S: the forward substitution the selection has done
    for a in range(n):                                     # column a of L^-1 by forward substitution
        x = np.zeros(n)
        x[a] = 1.0 / L[a, a]
        for b in range(a + 1, n):
            x[b] = -np.dot(L[b, a:b], x[a:b]) / L[b, b]
        joint[a] = np.dot(x, y) / np.sqrt(np.dot(x, x))
    out["joint"] = joint
    return out


def slct_by_definition(B, z, K, chi2_stop, min_var_frac, forced=()):
    """Every step's r_i = z_i - B_iS B_SS^-1 z_S and v_i = B_ii - B_iS B_SS^-1 B_Si from np.linalg.solve on the submatrix, for
    every SNP; joint z from np.linalg.inv(B_SS)."""
    B = np.asarray(B, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    diag = np.diag(B).copy()

    def state(sel):
        if not sel:
            return z.copy(), diag.copy()
        S = np.array(sel)
        X = np.linalg.solve(B[np.ix_(S, S)], B[S, :])      # B_SS^-1 B_S.
        return z - z[S] @ X, diag - np.einsum("si,si->i", B[S, :], X)

    out = _run(B, z, K, chi2_stop, min_var_frac, forced, state, lambda j: None)
    if out["n"]:
        S = out["idx"]
        inv = np.linalg.inv(B[np.ix_(S, S)])
        out["joint"] = (inv @ z[S]) / np.sqrt(np.diag(inv))
    else:
        out["joint"] = np.zeros(0)
    return out


def planted_z(B, causal, effect, seed, noise=1.0):
    """Z-scores with signals at the `causal` SNPs: z = B[:, causal] @ effect + noise * N(0, 1) -- what marginal statistics look like
    when a few SNPs carry an effect and their neighbours inherit it through LD."""
    rng = np.random.default_rng(seed)
    B = np.asarray(B, dtype=np.float64)
    return B[:, list(causal)] @ np.asarray(effect, dtype=np.float64) + noise * rng.standard_normal(B.shape[0])


def min_var_frac(collin, lam):
    """The guard a caller who means "un-ridged r^2 >= collin" passes: two identical rows have B_ij = 1, B_ii = 1 + lam, so one
    explains 1 / (1 + lam)^2 of the other, not 1."""
    return 1.0 - collin / (1.0 + lam) ** 2
