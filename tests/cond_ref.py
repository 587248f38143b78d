"""Reference statements of the imputed SNPs conditioned on the selected signals (test infrastructure, numpy only).

Definition (include/gauss_hip.h, out_cond_*): with B = B11 of a window (lambda on the diagonal, repaired if MakePosDef acted),
z = z1, S the ordered set of selected SNPs, b_u row u of B21, m_u = b_u B^-1 z and info_u = |b_u B^-1 b_u^T|,

    cond_z_u   = (m_u - b_u[S] B_SS^-1 z_S) / sqrt(info_u - b_u[S] B_SS^-1 b_u[S]^T)
    cond_var_u = (info_u - b_u[S] B_SS^-1 b_u[S]^T) / info_u

cond_z_u is NaN unless info_u - b_u[S] B_SS^-1 b_u[S]^T > mvf_u * info_u; cond_var_u is always given.  Under z ~ N(0, B),
cov(m_u, z_S) = b_u B^-1 B_:S = b_u[S], so the numerator's variance is the denominator's radicand and cond_z is N(0, 1) where S
explains everything.  S empty: cond_z = m / sqrt(info), cond_var = 1.  Three routes:

* ``cond_by_definition``: np.linalg.solve on B_SS and on B (the primary reference);
* ``cond_by_residual``: the numerator as the imputation of the residual r = z - B_:S B_SS^-1 z_S -- B^-1 B_:S = E_S, so
  b_u B^-1 r = m_u - b_u[S] B_SS^-1 z_S -- through any imputer (default B21 @ solve(B, r); the oracle's run_impute in the GPU
  tests), the variance through a Cholesky factor of B_SS;
* ``cond_by_augmented``: ``slct_by_definition`` with S forced on the bordered matrix [[B, b_u^T], [b_u, info_u]] and z extended
  by m_u: the imputed SNP treated as one more SNP whose variance is info_u, which is the whole point.

Each returns ``margin``: the smaller of the smallest |cond_var_u - mvf_u| (the room a rounding error has before the guard decides
otherwise) and the smallest info_u.  Where cond_z is NaN means something only while that is positive.

The null check the definition rests on (not a test, it is randomised): M = 65, U = 40, lambda = 0.1, 4 000 draws z ~ N(0, B),
the variance of cond_z came out at 0.99 - 1.02 for every u.
"""
import numpy as np

from slct_ref import slct_by_definition


def _impute(B, B21, z):
    """(m, info, Y): m_u = b_u B^-1 z, info_u = |b_u B^-1 b_u^T|."""
    Y = np.linalg.solve(B, B21.T).T                        # row u = B^-1 b_u^T
    return B21 @ np.linalg.solve(B, z), np.abs(np.einsum("um,um->u", B21, Y))


def _finish(num, info, expl, mvf_u):
    with np.errstate(invalid="ignore", divide="ignore"):
        left = info - expl
        var = left / info
        cz = np.where(left > mvf_u * info, num / np.sqrt(left), np.nan)
    d = np.abs(var - mvf_u)
    d = d[~np.isnan(d)]
    margin = min(float(d.min()) if len(d) else np.inf, float(info.min()) if len(info) else np.inf)
    return dict(z=cz, var=var, margin=margin)


def cond_by_definition(B, B21, z, S, mvf_u):
    B, B21, z = np.asarray(B, dtype=np.float64), np.asarray(B21, dtype=np.float64), np.asarray(z, dtype=np.float64)
    S = np.asarray(S, dtype=np.int64)
    m, info = _impute(B, B21, z)
    if len(S) == 0:
        with np.errstate(invalid="ignore", divide="ignore"):
            return dict(z=m / np.sqrt(info), var=np.ones(len(m)), margin=min(1.0 - mvf_u, float(info.min())))
    bS = B21[:, S]
    X = np.linalg.solve(B[np.ix_(S, S)], bS.T)             # [n, U]: B_SS^-1 b_u[S]^T
    return _finish(m - z[S] @ X, info, np.einsum("un,nu->u", bS, X), mvf_u)


def cond_by_residual(B, B21, z, S, mvf_u, impute=None):
    """impute(r) -> (mean, info) of the window with z1 = r; None: B21 @ solve(B, r)."""
    B, B21, z = np.asarray(B, dtype=np.float64), np.asarray(B21, dtype=np.float64), np.asarray(z, dtype=np.float64)
    S = np.asarray(S, dtype=np.int64)
    if impute is None:
        impute = lambda r: _impute(B, B21, r)
    if len(S) == 0:
        m, info = impute(z)
        with np.errstate(invalid="ignore", divide="ignore"):
            return dict(z=m / np.sqrt(info), var=np.ones(len(m)), margin=min(1.0 - mvf_u, float(info.min())))
    L = np.linalg.cholesky(B[np.ix_(S, S)])
    y = np.linalg.solve(L, z[S])
    r = z - B[:, S] @ np.linalg.solve(L.T, y)
    num, info = impute(r)
    Wt = np.linalg.solve(L, B21[:, S].T)                   # [n, U]: column u = L^-1 b_u[S]^T
    return _finish(num, info, np.sum(Wt * Wt, axis=0), mvf_u)


def cond_by_augmented(B, B21, z, S, mvf_u):
    B, B21, z = np.asarray(B, dtype=np.float64), np.asarray(B21, dtype=np.float64), np.asarray(z, dtype=np.float64)
    S = [int(s) for s in S]
    M, U = len(z), B21.shape[0]
    m, info = _impute(B, B21, z)
    cz, var = np.zeros(U), np.zeros(U)
    Ba = np.zeros((M + 1, M + 1))
    Ba[:M, :M] = B
    za = np.append(z, 0.0)
    for u in range(U):
        Ba[M, :M] = Ba[:M, M] = B21[u]
        Ba[M, M] = info[u]
        za[M] = m[u]
        # (the guard of the run is the imputed SNP's; a forced SNP that sits in S has passed the selection's own, stricter one)
        r = slct_by_definition(Ba, za, len(S), 0.0, mvf_u, forced=S)
        assert r["n"] == len(S) and list(r["idx"]) == S, "a forced SNP failed the imputed SNPs' guard"
        cz[u], var[u] = r["zc"][M], r["var"][M]
    d = np.abs(var - mvf_u)
    d = d[~np.isnan(d)]
    return dict(z=cz, var=var, margin=min(float(d.min()) if len(d) else np.inf, float(info.min())))


def window_mats(mode, geno_m, geno_u, pop_off, pop_wgt, lam=0.1):
    """B11 (lambda on the diagonal, before MakePosDef) and B21 of a window as the numpy oracle forms them."""
    from oracle import oracle_np
    if mode == 0:
        b11, b21 = oracle_np.pooled_cor(geno_m), oracle_np.pooled_cor(geno_u, geno_m)
    else:
        b11 = oracle_np.weighted_cor(geno_m, None, pop_off, pop_wgt)
        b21 = oracle_np.weighted_cor(geno_u, geno_m, pop_off, pop_wgt)
    np.fill_diagonal(b11, 1.0 + lam)
    return b11, b21
