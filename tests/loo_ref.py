"""Reference statements of the leave-one-out re-imputation of measured SNPs (test infrastructure, numpy only).

Definition (include/gauss_hip.h, out_loo_*): for measured SNP i of a window, the values run_dist / run_distmix
(dist.cpp:129-227, distmix.cpp:138-253) return for SNP i when it is presented as the only unmeasured SNP and the other
M - 1 are the measured set.  Two independent routes to it:

* ``loo_by_deletion`` does exactly that, one oracle call per SNP;
* ``loo_closed_form`` is the rank-one downdate of B^-1 that the GPU kernel evaluates, in LAPACK form.
"""
import numpy as np


def loo_closed_form(b11, z1):
    """b11: the window's B11 (lambda on the diagonal, repaired if MakePosDef acted), z1 [M].
    d = diag(B^-1), g = B^-1 z1;  mean = z1 - g / d;  info = |B_ii - 1 / d|;  z = mean / sqrt(info);  t = g / sqrt(d)."""
    b11 = np.asarray(b11, dtype=np.float64)
    z1 = np.asarray(z1, dtype=np.float64)
    inv = np.linalg.inv(b11)
    d = np.diag(inv).copy()
    g = inv @ z1
    mean = z1 - g / d
    info = np.abs(np.diag(b11) - 1.0 / d)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = mean / np.sqrt(info)
    t = g / np.sqrt(d)
    if len(z1) == 1:                      # nothing to impute from: b is empty
        info, z = np.zeros(1), np.full(1, np.nan)
    return dict(z=z, info=info, t=t, mean=mean)


def loo_by_deletion(mode, geno_m, pop_off, pop_wgt, z1, lam=0.1, min_abs_eig=1e-5, idx=None, run_impute=None):
    """SNP i deleted from the measured set and imputed from the others by the oracle's run_impute (default: the
    numpy / LAPACK oracle; pass oracle.run_impute for the loop-literal C one).  idx: the SNPs to do (default all).
    Returns z, info, t [len(idx)]; t = (z1_i - mean_i) / sqrt(B_ii - info_i) with B_ii = 1 + lam, valid while
    MakePosDef stays silent (the returned `mpd` counts the deletions where it did not)."""
    if run_impute is None:
        from oracle import oracle_np
        run_impute = oracle_np.run_impute
    geno_m = np.asarray(geno_m)
    z1 = np.asarray(z1, dtype=np.float64)
    M = len(z1)
    idx = np.arange(M) if idx is None else np.asarray(idx)
    z, info, t = np.zeros(len(idx)), np.zeros(len(idx)), np.zeros(len(idx))
    mpd = 0
    for k, i in enumerate(idx):
        keep = np.r_[0:i, i + 1:M]
        r = run_impute(mode, np.ascontiguousarray(geno_m[keep]), np.ascontiguousarray(geno_m[i:i + 1]), pop_off, pop_wgt, z1[keep],
                       lam=lam, min_abs_eig=min_abs_eig)
        z[k], info[k] = r["z"][0], r["info"][0]
        mean = z[k] * np.sqrt(info[k])
        t[k] = (z1[i] - mean) / np.sqrt(1.0 + lam - info[k])
        mpd += int(r["mpd"])
    return dict(z=z, info=info, t=t, mpd=mpd)


def window_b11(mode, geno_m, pop_off, pop_wgt, lam=0.1):
    """B11 of a window as the oracle forms it (before MakePosDef)."""
    from oracle import oracle_np
    b11 = oracle_np.pooled_cor(geno_m) if mode == 0 else oracle_np.weighted_cor(geno_m, None, pop_off, pop_wgt)
    np.fill_diagonal(b11, 1.0 + lam)
    return b11
