"""Reference statements of further traits that lack some of the window's measured SNPs (test infrastructure, numpy only).

Definition (include/gauss_hip.h, miss_more): for further trait t that lacks the measured SNPs D, the outputs are what run_dist /
run_distmix (dist.cpp:129-227, distmix.cpp:138-253) return for that trait alone when the window's measured set is the M - |D| other
SNPs and the SNPs of D are further unmeasured SNPs.  Two routes to it:

* ``miss_by_oracle`` does exactly that, one oracle call per trait (the primary reference);
* ``miss_closed_form`` is the rank-|D| downdate the GPU kernels evaluate, in LAPACK, on the b11 / b21 of
  ``oracle.run_impute(..., want_mats=True)`` for the FULL measured set (b11 as repaired by MakePosDef when it acted).

Both return z [T, U], info [T, U] and dense z_miss / info_miss [T, M], NaN where nothing is missing.
"""
import numpy as np


def miss_closed_form(b11, b21, Z, mask):
    """b11 [M, M] with lambda on the diagonal (repaired if MakePosDef acted), b21 [U, M], Z [T, M], mask [T, M] (non-zero: no score).
    With A = b11^-1, z0 = Z[t] with zeros on D, g0 = A z0, y_u = A b_u^T and L_D L_D^T = A_DD:
    c = -A_DD^-1 g0_D;  mean_u = b_u . g0 + y_u[D] . c;  info_ut = |b_u . y_u - ||L_D^-1 y_u[D]||^2|;  z = mean / sqrt(info);
    for d in D: mean_d = c_d, info_dt = |b11_dd - (A_DD^-1)_dd|."""
    b11 = np.asarray(b11, dtype=np.float64)
    b21 = np.asarray(b21, dtype=np.float64)
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    mask = np.atleast_2d(np.asarray(mask)) != 0
    T, M = Z.shape
    U = b21.shape[0]
    A = np.linalg.inv(b11)
    A = 0.5 * (A + A.T)
    Y = b21 @ A                                                       # row u = y_u
    by = np.einsum("um,um->u", b21, Y)
    z, info = np.zeros((T, U)), np.zeros((T, U))
    z_miss, info_miss = np.full((T, M), np.nan), np.full((T, M), np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T):
            D = np.nonzero(mask[t])[0]
            z0 = np.where(mask[t], 0.0, Z[t])
            g0 = A @ z0
            mean = b21 @ g0
            if len(D) == 0:
                info[t] = np.abs(by)
                z[t] = mean / np.sqrt(info[t])
                continue
            L = np.linalg.cholesky(A[np.ix_(D, D)])
            c = -np.linalg.solve(L.T, np.linalg.solve(L, g0[D]))
            V = np.linalg.solve(L, Y[:, D].T)                         # [k, U]
            info[t] = np.abs(by - np.sum(V * V, axis=0))
            z[t] = (mean + Y[:, D] @ c) / np.sqrt(info[t])
            Li = np.linalg.inv(L)
            info_miss[t, D] = np.abs(np.diag(b11)[D] - np.sum(Li * Li, axis=0))
            z_miss[t, D] = c / np.sqrt(info_miss[t, D])
    return dict(z=z, info=info, z_miss=z_miss, info_miss=info_miss)


def miss_by_oracle(mode, gm, gu, off, w, Z, mask, lam=0.1, min_abs_eig=1e-5, run_impute=None):
    """One run of the oracle per trait (default: the loop-literal C oracle): measured rows gm[S], unmeasured rows vstack(gu, gm[D]),
    scores Z[t][S].  `mpd` counts the runs in which MakePosDef acted."""
    if run_impute is None:
        import oracle
        run_impute = oracle.run_impute
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    mask = np.atleast_2d(np.asarray(mask)) != 0
    T, M = Z.shape
    U = gu.shape[0]
    z, info = np.zeros((T, U)), np.zeros((T, U))
    z_miss, info_miss = np.full((T, M), np.nan), np.full((T, M), np.nan)
    mpd = 0
    for t in range(T):
        D, S = np.nonzero(mask[t])[0], np.nonzero(~mask[t])[0]
        r = run_impute(mode, np.ascontiguousarray(gm[S]), np.ascontiguousarray(np.vstack([gu, gm[D]])), off, w, Z[t][S],
                       lam=lam, min_abs_eig=min_abs_eig)
        z[t], info[t] = r["z"][:U], r["info"][:U]
        z_miss[t, D], info_miss[t, D] = r["z"][U:], r["info"][U:]
        mpd += int(r["mpd"])
    return dict(z=z, info=info, z_miss=z_miss, info_miss=info_miss, mpd=mpd)


def random_mask(T, M, ks, seed=0):
    """mask [T, M]: trait t lacks ks[t] random SNPs."""
    rng = np.random.default_rng(seed)
    mask = np.zeros((T, M), dtype=np.uint8)
    for t, k in enumerate(ks):
        mask[t, rng.choice(M, size=k, replace=False)] = 1
    return mask


def cyclic_mask(M, ks, n_union, seed=0):
    """mask [len(ks), M]: trait t lacks ks[t] SNPs, consecutive members of one random set E of n_union SNPs, each trait starting where the
    one before it ended and wrapping around: exactly n_union distinct SNPs are missing, and once sum(ks) > n_union traits share SNPs."""
    ks = list(ks)
    assert max(ks) <= n_union <= min(sum(ks), M)
    E = np.sort(np.random.default_rng(seed).choice(M, size=n_union, replace=False))
    mask = np.zeros((len(ks), M), dtype=np.uint8)
    at = 0
    for t, k in enumerate(ks):
        mask[t, E[(at + np.arange(k)) % n_union]] = 1
        at += k
    assert int(mask.any(axis=0).sum()) == n_union and np.array_equal(mask.sum(axis=1), ks)
    return mask
