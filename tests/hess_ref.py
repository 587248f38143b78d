"""Two numpy statements of the hess rule of include/gauss_hip.h (gauss_ld_hess_rows) and of the estimators of api.hess_estimates.

(a) rule(): the repair, then np.linalg.eigh on the repaired matrix, n_pos and the projections; estimates(): the estimators in vectorised
    numpy (cumulative sums).
(b) estimates_loops(): the estimators through explicit loops with math.fsum, written from the formulas and sharing no line with (a).
replay_proj() is the order of hess_proj_kernel (k_hess.hip) on the vectors the GPU returned."""
import math

import numpy as np


def repair(R):
    """(R', mono, n_nonfinite): a SNP whose every off-diagonal entry is NaN (M > 1) has its row, column and diagonal set to 0; any other
    non-finite entry counts as 0 and once per pair i <= j in n_nonfinite"""
    R = np.array(R, dtype=np.float64)
    M = len(R)
    off = ~np.eye(M, dtype=bool)
    mono = np.array([M > 1 and bool(np.all(np.isnan(R[i][off[i]]))) for i in range(M)])
    live = ~mono[:, None] & ~mono[None, :]
    bad = ~np.isfinite(R) & live
    n_bad = int(np.triu(bad).sum())
    R[bad] = 0.0
    R[~live] = 0.0
    return R, mono, n_bad


def repair_z(z, mono):
    z = np.array(z, dtype=np.float64).reshape(-1, len(mono))
    z[~np.isfinite(z)] = 0.0
    z[:, mono] = 0.0
    return z


def n_pos_of(lam, eig_min):
    if not np.all(np.isfinite(lam)):
        return 0
    return int(sum(1 for x in lam if x > eig_min * lam[0] and x > 0.0))


def rule(R, z, k_max, eig_min=1e-6):
    """dict(lam [M] descending, vectors [M, M] (row i = v_i), n_pos, proj [T, k_max], n_nonfinite, mono) through eigh"""
    Rp, mono, n_bad = repair(R)
    zr = repair_z(z, mono)
    w, v = np.linalg.eigh(Rp)
    lam, vec = w[::-1].copy(), v[:, ::-1].T.copy()
    n_pos = n_pos_of(lam, eig_min)
    kk = min(k_max, n_pos)
    proj = np.full((len(zr), k_max), np.nan)
    proj[:, :kk] = (zr @ vec[:kk].T) / np.sqrt(lam[:kk])
    return dict(lam=lam, vectors=vec, n_pos=n_pos, proj=proj, n_nonfinite=n_bad, mono=mono, R=Rp, z=zr)


def replay_proj(vectors, lam, z, mono, k_max, n_pos):
    """hess_proj_kernel's sums on the returned vectors: lane l adds the products of the rows l, l + 64, ... in ascending order, then six
    halving steps; one correctly rounded square root and division"""
    zr = repair_z(z, mono)
    T, M = zr.shape
    ldn = (M + 63) // 64 * 64
    kk = min(k_max, n_pos)
    out = np.full((T, k_max), np.nan)
    V = np.zeros((kk, ldn))
    V[:, :M] = vectors[:kk]
    for t in range(T):
        zt = np.zeros(ldn)
        zt[:M] = zr[t]
        prod = (V * zt[None, :]).reshape(kk, ldn // 64, 64)
        part = np.zeros((kk, 64))
        for c in range(ldn // 64):
            part = part + prod[:, c, :]
        h = 32
        while h:
            part = part[:, :h] + part[:, h:2 * h]
            h //= 2
        out[t, :kk] = part[:, 0] / np.sqrt(lam[:kk])
    return out


def choose_k(lam, k_max, n_pos, k=None, var_frac=0.99):
    cap = min(k_max, n_pos)
    if k is not None:
        return min(int(k), cap)
    tot = 0.0
    for x in lam:
        tot = tot + x
    run = 0.0
    for i in range(cap):
        run = run + lam[i]
        if run / tot >= var_frac:
            return i + 1
    return cap


def estimates(lam, proj, n, k=None, var_frac=0.99, overlap=None, eig_min=1e-6):
    """(a): vectorised"""
    lam, p = np.asarray(lam, dtype=np.float64), np.asarray(proj, dtype=np.float64)
    T, k_max = p.shape
    nn = np.broadcast_to(np.asarray(n, dtype=np.float64), (T,)).copy()
    kk = choose_k(lam, k_max, n_pos_of(lam, eig_min), k, var_frac)
    s = np.zeros((T, T)) if overlap is None else np.broadcast_to(np.asarray(overlap, dtype=np.float64), (T, T))
    H = np.cumsum(p[:, :kk] ** 2, axis=1)[:, -1]
    h2 = (H - kk) / (nn - kk)
    with np.errstate(invalid="ignore"):
        se = np.sqrt((nn / (nn - kk)) ** 2 * (2 * kk * (1 - h2) / nn + 4 * h2) * (1 - h2) / nn)
    Cm = p[:, :kk] @ p[:, :kk].T
    cov = (Cm - kk * s) / np.sqrt(np.outer(nn, nn))
    with np.errstate(invalid="ignore"):
        rg = cov / np.sqrt(np.outer(h2, h2))
    rg[~((h2[:, None] > 0) & (h2[None, :] > 0))] = np.nan
    return dict(k=kk, H=H, h2=h2, se=se, C=Cm, cov=cov, rg=rg)


def estimates_loops(lam, proj, n, k=None, var_frac=0.99, overlap=None, eig_min=1e-6):
    """(b): explicit loops, math.fsum"""
    T, k_max = len(proj), len(proj[0])
    nn = [float(n)] * T if np.ndim(n) == 0 else [float(x) for x in n]
    kk = choose_k(lam, k_max, n_pos_of(lam, eig_min), k, var_frac)
    H, h2, se = [], [], []
    for t in range(T):
        Ht = math.fsum(float(proj[t][i]) * float(proj[t][i]) for i in range(kk))
        h = (Ht - kk) / (nn[t] - kk)
        v = (nn[t] / (nn[t] - kk)) ** 2 * (2.0 * kk * (1.0 - h) / nn[t] + 4.0 * h) * (1.0 - h) / nn[t]
        H.append(Ht), h2.append(h), se.append(math.sqrt(v) if v >= 0 else math.nan)
    Cm, cov, rg = np.zeros((T, T)), np.zeros((T, T)), np.full((T, T), np.nan)
    for a in range(T):
        for b in range(T):
            sab = 0.0 if overlap is None else float(overlap if np.ndim(overlap) == 0 else overlap[a][b])
            Cm[a, b] = math.fsum(float(proj[a][i]) * float(proj[b][i]) for i in range(kk))
            cov[a, b] = (Cm[a, b] - kk * sab) / math.sqrt(nn[a] * nn[b])
            if h2[a] > 0 and h2[b] > 0:
                rg[a, b] = cov[a, b] / math.sqrt(h2[a] * h2[b])
    return dict(k=kk, H=np.array(H), h2=np.array(h2), se=np.array(se), C=Cm, cov=cov, rg=rg)
