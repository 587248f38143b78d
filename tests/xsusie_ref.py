"""Reference statements of the joint fine-mapping across studies (test infrastructure, numpy only).

Definition (include/gauss_hip.h, xs_group): K studies, each a window with its own B_k = B11, C_k = B21 and z_k; study k has the
quantities of tests/susie_ref.py in its own candidate order (measured first): zhat_k, d_k, adm_k, R_k.  Study 1 leads; ``maps[k]``
takes leader candidate j to study k's index (-1: absent; None: the same index).  The joint candidates are the leader's candidates
present and admissible in every study.  One alpha_l is shared, residuals, mu and V are per study; every sum over candidates runs in
leader order, over studies ascending.  Two statements of the same fit:

* ``fit_textbook`` forms every R_k = A_k^T B_k^-1 A_k and zhat_k explicitly;
* ``fit_w`` states what the kernels evaluate: W_k = B_k^-1 C_k^T, v = bbar_meas + W_k bbar_unmeas, R_k bbar = [B_k v ; C_k v].

``plain_measured`` is an independent plain loop for measured_only that shares no helper with them.

``borderline`` lists the decisions a rounding error could turn, susie_ref.borderline's rules with the joint null check in the place of
the single one and every study's purity beside their maximum.
"""
import numpy as np

import susie_ref as sr

PURITY_N = sr.PURITY_N
VALUE_KEYS = ("alpha", "mu", "pip", "set_pip", "mass", "lse", "V", "purity", "xs_V", "xs_purity", "xs_mu")
EXACT_KEYS = ("size", "set", "kept", "sweeps", "xs_n")


def _study_textbook(B, C, z, a):
    M = len(z)
    A = np.hstack([B, C.T])
    R = A.T @ np.linalg.solve(B, A)
    zhat = A.T @ np.linalg.solve(B, z)
    zhat[:M] = z
    d = np.diag(R).copy()
    adm = sr._admissible(zhat, d, M, z, a)
    Rs = R.copy()
    Rs[:, ~adm] = 0.0
    return dict(zhat=zhat, d=d, adm=adm, rmul=lambda b: Rs @ b, rij=lambda i, j: R[i, j], T=len(zhat))


def _study_w(B, C, z, a):
    M = len(z)
    W = np.linalg.solve(B, C.T)
    info = np.einsum("um,mu->u", C, W)
    zhat = np.concatenate([z, C @ np.linalg.solve(B, z)])
    d = np.concatenate([np.diag(B), info])
    adm = sr._admissible(zhat, d, M, z, a)

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

    return dict(zhat=zhat, d=d, adm=adm, rmul=rmul, rij=rij, T=len(zhat))


def _lse_of(lb, n):
    mx = lb.max()
    return mx + np.log(np.exp(lb - mx).sum() / n)


def _joint(st, maps, a):
    K, TL, L = len(st), st[0]["T"], a["L"]
    idx = [np.arange(TL) if m is None else np.asarray(m, dtype=np.int64) for m in maps]
    jadm = np.ones(TL, dtype=bool)
    for k in range(K):
        jadm &= idx[k] >= 0
    for k in range(K):
        jadm[jadm] &= st[k]["adm"][idx[k][jadm]]
    J = np.flatnonzero(jadm)                                    # the joint admissible candidates, in leader order
    own = [idx[k][J] for k in range(K)]
    n = len(J)
    alpha, lbf = np.zeros((L, TL)), np.full((L, TL), -np.inf)
    mu = np.zeros((K, L, TL))                                   # every study's mu in leader order
    rb = [np.zeros((L, s["T"])) for s in st]
    f = [np.zeros(s["T"]) for s in st]
    V, lse = np.full((L, K), float(a["prior_var"])), np.full(L, np.nan)
    null_lse, deltas = [], []
    sweeps = 0

    def lbf_sum(r, Vl):
        tot = None
        for k in range(K):
            t = sr._lbf(r[k][own[k]], st[k]["d"][own[k]], float(Vl[k]))
            tot = t if tot is None else tot + t
        return tot

    for _ in range(a["max_sweeps"]):
        Vn, prev = V.copy(), alpha.copy()
        for l in range(L):
            with np.errstate(invalid="ignore"):
                r = [st[k]["zhat"] - (f[k] - rb[k][l]) for k in range(K)]
            aJ = np.zeros(0)
            alpha[l], lbf[l], lse[l] = 0.0, -np.inf, np.nan
            if n:
                lb = lbf_sum(r, V[l])
                mx = lb.max()
                e = np.exp(lb - mx)
                tot = e.sum()
                aJ = e / tot
                alpha[l, J], lbf[l, J], lse[l] = aJ, lb, mx + np.log(tot / n)
            v1 = np.zeros(K)
            for k in range(K):
                dk = st[k]["d"][own[k]]
                s2 = V[l, k] / (1.0 + V[l, k] * dk)
                m = s2 * r[k][own[k]]
                mu[k, l] = 0.0
                mu[k, l, J] = m
                b = np.zeros(st[k]["T"])
                b[own[k]] = aJ * m
                new = st[k]["rmul"](b)
                f[k] = (f[k] - rb[k][l]) + new
                rb[k][l] = new
                v1[k] = float(np.sum(aJ * (m ** 2 + s2)))
            if a["estimate_var"] and np.any(V[l] != 0.0):
                l1 = _lse_of(lbf_sum(r, v1), n) if n else np.nan
                null_lse.append(l1)
                Vn[l] = 0.0 if (l1 <= 0.0 or n == 0) else v1
        V = Vn
        sweeps += 1
        deltas.append(float(np.max(np.abs(alpha - prev))))
        if deltas[-1] < a["tol"]:
            break
    rmax = 0.0
    for s in st:
        if s["adm"].any():
            with np.errstate(invalid="ignore", divide="ignore"):
                rmax = max(rmax, float(np.nanmax(np.abs(s["zhat"][s["adm"]]) / np.sqrt(s["d"][s["adm"]]))))
    return dict(alpha=alpha, lbf=lbf, xs_mu=mu, mu=mu[0], xs_V=V.T.copy(), V=V[:, 0].copy(), lse=lse, sweeps=sweeps, delta=deltas[-1],
                deltas=deltas, null_lse=np.array(null_lse), rmax=rmax, adm=jadm, xs_n=n, idx=idx, K=K)


def _sets(res, st, a):
    alpha, K = res["alpha"], res["K"]
    L, T = alpha.shape
    rho = a["coverage"]
    ar = np.arange(T)
    member, ahead = np.zeros((L, T), dtype=bool), np.zeros((L, T))
    xs_purity, purity, kept = np.full((K, L), np.nan), np.full(L, np.nan), np.zeros(L, dtype=bool)
    for l in range(L):
        order = np.lexsort((ar, -alpha[l]))
        ahead[l, order] = np.concatenate([[0.0], np.cumsum(alpha[l][order])[:-1]])
        member[l] = (alpha[l] > 0) & ((ahead[l] < rho) | (rho >= 1.0))
        top = [int(j) for j in order[: min(int(member[l].sum()), PURITY_N)]]
        for k in range(K):
            own, d, rij = res["idx"][k], st[k]["d"], st[k]["rij"]
            if len(top) == 1:
                xs_purity[k, l] = 1.0
            elif len(top) > 1:
                xs_purity[k, l] = min(abs(rij(int(own[i]), int(own[j]))) / np.sqrt(d[own[i]] * d[own[j]]) for q, i in enumerate(top) for j in top[q + 1:])
        if top:
            purity[l] = xs_purity[:, l].max()
        kept[l] = np.any(res["xs_V"][:, l] > 0) and purity[l] >= a["min_abs_corr"] and \
            not any(kept[k] and np.array_equal(member[k], member[l]) for k in range(l))
    keep, sset, set_pip = np.ones(T), np.full(T, -1, dtype=np.int64), np.zeros(T)
    for l in range(L):
        if res["V"][l] > 0:
            keep = keep * (1.0 - alpha[l])
        better = kept[l] & member[l] & ((sset < 0) | (alpha[l] > set_pip))
        sset[better] = l
        set_pip[better] = alpha[l][better]
    res.update(member=member, ahead=ahead, purity=purity, xs_purity=xs_purity, kept=kept, pip=1.0 - keep, set=sset, set_pip=set_pip,
               size=member.sum(axis=1).astype(np.int64), mass=np.where(member, alpha, 0.0).sum(axis=1))
    return res


def _fit(one, studies, maps, kw):
    a = sr.args_of(**kw)
    st = [one(np.asarray(B, dtype=np.float64), np.asarray(C, dtype=np.float64), np.asarray(z, dtype=np.float64), a) for B, C, z in studies]
    maps = list(maps) if maps is not None else [None] * len(st)
    return _sets(_joint(st, maps, a), st, a)


def fit_textbook(studies, maps=None, **kw):
    """studies: [(B_k, C_k, z_k)]; maps: [None, from_lead_1, ..] (None: the same index)"""
    return _fit(_study_textbook, studies, maps, kw)


def fit_w(studies, maps=None, **kw):
    return _fit(_study_w, studies, maps, kw)


def plain_measured(zs, Bs, maps, L, prior_var, max_sweeps, tol, estimate_var):
    """The joint fit of the measured SNPs alone in plain loops: zs[k], Bs[k] a study's scores and B11, maps[k][j] the place of leader SNP
    j among study k's measured SNPs (-1 or beyond them: not measured there).  Residual variance 1, uniform prior over the SNPs
    measured in every study, one prior variance per (effect, study), the joint null check.  Returns alpha [L, M_lead]."""
    K, ML = len(zs), len(zs[0])
    where = []
    for j in range(ML):
        at = []
        for k in range(K):
            c = j if maps[k] is None else int(maps[k][j])
            at.append(c if 0 <= c < len(zs[k]) else -1)
        where.append(at)
    cand = [j for j in range(ML) if min(where[j]) >= 0]
    alpha = [[0.0] * ML for _ in range(L)]
    post = [[[0.0] * ML for _ in range(L)] for _ in range(K)]
    V = [[float(prior_var)] * K for _ in range(L)]

    def bf(r, Vl):
        out = []
        for j in cand:
            t = 0.0
            for k in range(K):
                c = where[j][k]
                dk = Bs[k][c][c]
                t += 0.0 if Vl[k] == 0.0 else 0.5 * (r[k][c] ** 2 * Vl[k] / (1.0 + Vl[k] * dk) - np.log1p(Vl[k] * dk))
            out.append(t)
        return out

    for _ in range(max_sweeps):
        Vn, old = [list(v) for v in V], [list(row) for row in alpha]
        for l in range(L):
            r = []
            for k in range(K):
                Mk = len(zs[k])
                others = [0.0] * Mk
                for j in cand:
                    others[where[j][k]] = sum(alpha[q][j] * post[k][q][j] for q in range(L) if q != l)
                r.append([zs[k][i] - sum(Bs[k][i][c] * others[c] for c in range(Mk)) for i in range(Mk)])
            lb = bf(r, V[l])
            top = max(lb)
            w = [np.exp(x - top) for x in lb]
            tot = sum(w)
            for n, j in enumerate(cand):
                alpha[l][j] = w[n] / tot
                for k in range(K):
                    c = where[j][k]
                    post[k][l][j] = V[l][k] / (1.0 + V[l][k] * Bs[k][c][c]) * r[k][c]
            if estimate_var and any(v != 0.0 for v in V[l]):
                v1 = [sum(alpha[l][j] * (post[k][l][j] ** 2 + V[l][k] / (1.0 + V[l][k] * Bs[k][where[j][k]][where[j][k]])) for j in cand)
                      for k in range(K)]
                lb1 = bf(r, v1)
                top1 = max(lb1)
                Vn[l] = [0.0] * K if top1 + np.log(sum(np.exp(x - top1) for x in lb1) / len(cand)) <= 0.0 else v1
        V = Vn
        if max(abs(alpha[l][j] - old[l][j]) for l in range(L) for j in range(ML)) < tol:
            break
    return np.array(alpha)


def gap(x, y):
    g = 0.0
    for k in VALUE_KEYS:
        p, q = np.asarray(x[k], dtype=np.float64), np.asarray(y[k], dtype=np.float64)
        both = np.isnan(p) & np.isnan(q)
        with np.errstate(invalid="ignore"):
            dlt = np.where(both, 0.0, np.abs(p - q))
        g = max(g, float(np.max(dlt)) if dlt.size else 0.0)
    return g


def value_tol(res, e_ref):
    """susie_ref.value_tol's reasoning with K terms in a log Bayes factor: every study's residual r_kj / sqrt(d_kj) is a solve output
    off by 1e-8 max(1, |.|), each moves its term of lbf_j by at most max(1, r_max^2) 1e-8 (r_max over all studies), the sum by K times
    that, a pip by twice that; or ten times the gap between the two statements of the reference."""
    return max(10.0 * e_ref, 2.0 * res["K"] * max(1.0, res["rmax"] ** 2) * 1e-8)


def borderline(res, a, tol_v):
    """The decisions a rounding error could turn (empty: none): susie_ref.borderline on the joint quantities -- the joint null check
    lse(V'_1 .. V'_K), the stop, the members -- and every study's purity within 1e-6 of min_abs_corr (the maximum can turn on any)."""
    a = sr.args_of(**a)
    view = dict(res, V=res["xs_V"].max(axis=0), purity=res["purity"])
    out = sr.borderline(view, a, tol_v)
    for k in range(res["K"]):
        for l in range(res["alpha"].shape[0]):
            p = res["xs_purity"][k, l]
            if np.isfinite(p) and view["V"][l] > 0 and abs(p - a["min_abs_corr"]) <= 1e-6 and f"purity of set {l} " not in " ".join(out):
                out.append(f"purity of set {l} in study {k} within 1e-6 of min_abs_corr")
    return out


# ---- the groups of tests/test_gpu_xsusie.py, built here so that tests/test_xsusie_ref.py can vet them on the CPU ---------------------
def _weights(p, k):
    """Study k's ancestry weights on panel p: the panel's own, reversed, squared and renormalised, the uniform ones"""
    w = np.asarray(p["w"], dtype=np.float64)
    return [w, w[::-1].copy(), w ** 2 * (w.sum() / (w ** 2).sum()), np.full(len(w), w.sum() / len(w))][k]


def study(p, gm, gu, z1, k, mode=1):
    return dict(mode=mode, geno_m=np.ascontiguousarray(gm), geno_u=np.ascontiguousarray(gu), pop_off=p["off"],
                pop_wgt=_weights(p, k) if mode else None, z1=np.asarray(z1, dtype=np.float64))


def identity_group(M, U, K, seed, modes=None):
    """K studies on the SNPs of susie_ref.small_window(M, U): different weights (or pooled LD), the same three planted signals,
    their own noise.  maps: None each"""
    import cs_ref
    p, gm, gu = cs_ref.window(M, U)
    modes = modes or [1] * K
    return [study(p, gm, gu, cs_ref.planted(gm, seed=seed + 100 * k), k, modes[k]) for k in range(K)], [None] * K


def maps_of(ids_lead, ids_peer):
    at = {int(s): c for c, s in enumerate(ids_peer)}
    return np.array([at.get(int(s), -1) for s in ids_lead], dtype=np.int32)


def subset_group(ids, seed, n_snp=None, scale=0.02):
    """ids: per study (ids_m, ids_u), rows of one panel.  Scores: the panel's planted signals (cs_ref.planted on the study's measured
    rows would move the causal SNPs with the rows; here SNP ids[0][0][len // 2] is causal in every study that measures it)."""
    from helpers import small_panel
    from cond_ref import window_mats
    n_snp = n_snp or int(max(max(np.max(m), np.max(u)) for m, u in ids)) + 1
    p = small_panel(n_snp=n_snp + 30 + n_snp // 20, scale=scale, seed=seed)
    assert p["G"].shape[0] >= n_snp
    causal = int(ids[0][0][len(ids[0][0]) // 2])
    out, maps = [], []
    lead = np.concatenate(ids[0])
    for k, (im, iu) in enumerate(ids):
        gm, gu = p["G"][np.asarray(im)], p["G"][np.asarray(iu)]
        st = study(p, gm, gu, np.zeros(len(im)), k)
        B, C = window_mats(1, st["geno_m"], st["geno_u"], p["off"], st["pop_wgt"])
        col = B[:, list(im).index(causal)] if causal in list(im) else C[list(iu).index(causal)]
        st["z1"] = 7.0 * col + np.random.default_rng(seed + 100 * k).standard_normal(len(im))
        out.append(st)
        maps.append(None if k == 0 else maps_of(lead, np.concatenate([im, iu])))
    return out, maps


def permute_drop_ids(seed=5):
    """Leader (12, 11) against a peer (9, 20) that shares 15 of its candidates -- nine measured and six unmeasured ones of the leader --
    three of them measured in one study and imputed in the other, in a shuffled order of its own"""
    rng = np.random.default_rng(seed)
    lm, lu = np.arange(0, 12), np.arange(12, 23)
    extra = np.arange(23, 37)                                   # 14 SNPs only the peer has
    pm = np.concatenate([lm[:7], lu[:1], extra[:1]])             # lu[0]: imputed by the leader, measured by the peer
    pu = np.concatenate([lm[7:9], lu[1:6], extra[1:]])           # lm[7], lm[8]: measured by the leader, imputed by the peer
    return [(lm, lu), (rng.permutation(pm), rng.permutation(pu))]


def mats_of(st):
    from cond_ref import window_mats
    return window_mats(st["mode"], st["geno_m"], st["geno_u"], st["pop_off"], st["pop_wgt"])


# (name, builder of (studies, maps), susie arguments).  Identity maps, K = 2: T = 2; rows of M on either side of SUSIE_VR = 8; (9, 7) with
# L = 32; (63, 192); U = 1025 beyond SUSIE_CH.  K = 3 and 4 at (12, 11).  Maps that permute and drop.  Leader T = 257 against peer
# T = 255 (on either side of SUSIE_T).  A leader of 40 + 60 whose unmeasured SNPs are spread over a peer's 1025, beyond SUSIE_CH in the
# peer's own order.  One group of a pooled and a weighted window.  Each has the seed tests/test_xsusie_ref.py vets.
def _t257():
    lm, lu = np.arange(0, 100), np.arange(100, 257)
    return [(lm, lu), (lm, lu[:-2])]


def _u1025():
    pm, pu = np.arange(0, 40), np.arange(40, 1065)
    return [(pm, pu[np.linspace(0, 1024, 60).astype(int)]), (pm, pu)]


SMALL_GROUPS = [
    ("M1-U1-K2", lambda: identity_group(1, 1, 2, 3), dict(L=1, tol=0.0, max_sweeps=1)),
    ("M7-U1-K2", lambda: identity_group(7, 1, 2, 6), dict(L=3, tol=0.0, max_sweeps=2)),
    ("M8-U1-K2", lambda: identity_group(8, 1, 2, 7), dict(L=3, tol=0.0, max_sweeps=5)),
    ("M9-U7-K2-L32", lambda: identity_group(9, 7, 2, 8), dict(L=32, tol=0.0, max_sweeps=2)),
    ("M63-U192-K2", lambda: identity_group(63, 192, 2, 12), dict(L=10, tol=0.0, max_sweeps=5)),
    ("M40-U1025-K2", lambda: identity_group(40, 1025, 2, 16), dict(L=5, tol=0.0, max_sweeps=5)),
    ("M12-U11-K3", lambda: identity_group(12, 11, 3, 14), dict(L=10, tol=0.0, max_sweeps=5)),
    ("M12-U11-K4", lambda: identity_group(12, 11, 4, 14), dict(L=10, tol=0.0, max_sweeps=5)),
    ("permute-drop", lambda: subset_group(permute_drop_ids(), 31), dict(L=5, tol=0.0, max_sweeps=5)),
    ("T257-T255", lambda: subset_group(_t257(), 32), dict(L=3, tol=0.0, max_sweeps=3)),
    ("peer-U1025", lambda: subset_group(_u1025(), 33), dict(L=3, tol=0.0, max_sweeps=3)),
    ("pooled-weighted", lambda: identity_group(12, 11, 2, 14, modes=[0, 1]), dict(L=10, tol=0.0, max_sweeps=5)),
    ("measured-only", lambda: identity_group(12, 11, 2, 14), dict(L=3, tol=0.0, max_sweeps=5, measured_only=True)),
    ("converges", lambda: identity_group(63, 192, 2, 12), dict(L=5)),
]
LARGE_GROUP = (1213, 2512, dict(L=4, tol=0.0, max_sweeps=5), 1214)


def large_group():
    import cs_ref
    M, U, kw, seed = LARGE_GROUP
    p, gm, gu = cs_ref.window(M, U, scale=0.1)
    return [study(p, gm, gu, cs_ref.planted(gm, seed=seed + 100 * k), k) for k in range(2)], [None, None], kw


def planted_window():
    """The acceptance case: a causal SNP with one tag per ancestry half.  tagA copies the causal SNP's genotypes in the first 14
    populations (1 % of the samples shuffled) and is a permutation of its own genotypes in the rest; tagB is the mirror image over the
    last 15.  Study A weighs the first half uniformly, study B the second: r(causal, tagA) = 0.984 / 0.008, r(causal, tagB) = 0.046 /
    0.994.  Returns (studies, (causal, tagA, tagB))."""
    from helpers import small_panel, split_window
    from cond_ref import window_mats
    p = small_panel(n_snp=160, scale=0.02, seed=29)
    gm, gu, _ = split_window(dict(G=p["G"][:150]), 100)
    causal, tagA, tagB = 52, 97, 70
    off = np.asarray(p["off"])
    P = len(off) - 1
    cut = int(off[14])
    rng = np.random.default_rng(1)
    gm = gm.copy()

    def tag(own, lo, hi):
        t = own.copy()
        src = gm[causal, lo:hi].copy()
        pick = rng.random(src.size) < 0.01
        src[pick] = rng.permutation(src)[pick]
        t[lo:hi] = src
        rest = np.r_[0:lo, hi:own.size]
        t[rest] = rng.permutation(own[rest])
        return t

    gm[tagA] = tag(gm[tagA], 0, cut)                            # (tagA's draws come first)
    gm[tagB] = tag(gm[tagB], cut, gm.shape[1])
    zr = np.random.default_rng(3)                               # (study A's scores are drawn first)
    out = []
    for lo, hi, o in ((0, cut, off[:15]), (cut, gm.shape[1], off[14:] - cut)):
        g1, g0 = np.ascontiguousarray(gm[:, lo:hi]), np.ascontiguousarray(gu[:, lo:hi])
        w = np.full(len(o) - 1, 1.0 / (len(o) - 1))
        B, _ = window_mats(1, g1, g0, o, w)
        z = 6.0 * B[:, causal] + np.linalg.cholesky(B) @ zr.standard_normal(gm.shape[0])
        out.append(dict(mode=1, geno_m=g1, geno_u=g0, pop_off=np.ascontiguousarray(o), pop_wgt=w, z1=z))
    return out, (causal, tagA, tagB)
