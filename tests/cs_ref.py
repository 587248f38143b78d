"""Reference statements of the credible sets of the selected signals (test infrastructure, numpy only).

Definition (include/gauss_hip.h, out_cs_*): with B = B11 of a window (lambda on the diagonal, repaired if MakePosDef acted), z = z1,
S the ordered selected set, b_u row u of B21, m_u = b_u B^-1 z and info_u = |b_u B^-1 b_u^T|.  The candidates are the M measured
SNPs (0 .. M-1), then the U unmeasured ones (M .. M+U-1).  For signal a, with S' = S \\ {a}:

    measured i:    r' = z_i - B_iS' B_S'S'^-1 z_S',       v' = B_ii - B_iS' B_S'S'^-1 B_S'i,          s = v' / B_ii
    unmeasured u:  r' = m_u - b_u[S'] B_S'S'^-1 z_S',     v' = info_u - b_u[S'] B_S'S'^-1 b_u[S']^T,  s = v'
    zc = r' / sqrt(v'),   lbf = (zc^2 omega s / (1 + omega s) - log1p(omega s)) / 2

sel[a] is always a candidate of its own set, sel[b] (b != a) never; another measured SNP while v' > mvf_m B_ii and z_i is finite, an
unmeasured one while v' > mvf_u info_u, info_u > 0 and m_u / sqrt(info_u) is finite.  pip_ia = exp(lbf_ia - lse_a); SNP i is in set a
iff pip_ia > 0 and the mass ranked ahead of it (larger pip, ties: smaller index) is below rho; at rho = 1 that is every SNP with
pip_ia > 0, whatever the rounded sum says.  Two routes:

* ``cs_by_definition`` conditions on S' with np.linalg.solve for every a: no downdate, nothing shared with the kernel's arithmetic;
* ``cs_by_downdate`` states the rank-one update the kernel evaluates: with L the Cholesky factor of B_SS in order of entry,
  w = L^-1 B_S. (or L^-1 b_u[S]^T), y = L^-1 z_S, P = B_SS^-1, beta = P z_S and g = L^-T w,
      r' = r + g_a beta_a / P_aa,   v' = v + g_a^2 / P_aa     (r, v: the statistics given all of S)
  and sel[a] in its own set has zc = beta_a / sqrt(P_aa) (the joint z) and v' = 1 / P_aa.
  Checked against np.linalg.solve on S' to 2e-15 when the formulas were written down; tests/test_cs_ref.py holds the two routes to
  1e-10.

Only the tail (lbf -> pip -> sets -> the fold over the signals) is common to the two: what zc and v' are is theirs.

``borderline`` reports the decisions a rounding error could turn: SNP i is borderline in set a when rho lies within
margin + sum{pip_j : j != i, |pip_j - pip_i| <= tol} of the mass ranked ahead of i (an error of tol may reorder it with those SNPs), or
when a guard is within 1e-9 of its threshold (tests/test_gpu_cond.py's margin).  At rho = 1 the mass ahead decides nothing -- every
SNP with pip > 0 is a member -- and a membership is borderline only where exp() is about to underflow.
"""
import numpy as np

GUARD_MARGIN = 1e-9


def _impute(B, B21, z):
    Y = np.linalg.solve(B, B21.T).T
    return B21 @ np.linalg.solve(B, z), np.abs(np.einsum("um,um->u", B21, Y))


def _tail(zc, v1, den, floor, ok, S, omega, rho, M):
    """zc, v1 [n, T]: leave-one-out z and variance; den, floor [T]: the share's denominator and the guard's threshold; ok [T]: the
    candidate's own z is usable.  Everything from the Bayes factor on."""
    n, T = zc.shape
    S = [int(s) for s in S]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cand = ok[None, :] & (v1 > floor[None, :])
    for a in range(n):
        for b, j in enumerate(S):
            cand[a, j] = b == a
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = v1 / den[None, :]
        os_ = omega * s
        lbf = np.where(cand, 0.5 * (zc * zc * os_ / (1.0 + os_) - np.log1p(os_)), -np.inf)
        mx = np.max(np.where(np.isnan(lbf), -np.inf, lbf), axis=1)
        lse = mx + np.log(np.sum(np.exp(lbf - mx[:, None]), axis=1))
        pip_ia = np.exp(lbf - lse[:, None])
    idx = np.arange(T)
    member = np.zeros((n, T), dtype=bool)
    ahead = np.zeros((n, T))
    for a in range(n):
        order = np.lexsort((idx, -pip_ia[a]))                  # pip descending, ties to the smaller candidate index
        cum = np.concatenate([[0.0], np.cumsum(pip_ia[a][order])[:-1]])
        ahead[a, order] = cum
        member[a] = (pip_ia[a] > 0) & ((ahead[a] < rho) | (rho >= 1.0))      # (rho = 1: the rounded mass ahead may reach 1; the exact one cannot)
    keep = np.ones(T)
    cs_set = np.full(T, -1, dtype=np.int64)
    set_pip = np.zeros(T)
    for a in range(n):
        keep = keep * (1.0 - pip_ia[a])
        better = member[a] & ((cs_set < 0) | (pip_ia[a] > set_pip))
        cs_set[better] = a
        set_pip[better] = pip_ia[a][better]
    pip = 1.0 - keep if n else np.zeros(T)
    zmax = float(np.max(np.abs(zc[cand]))) if n else 0.0
    return dict(n=n, zc=zc, v1=v1, cand=cand, lbf=lbf, lse=lse, pip_ia=pip_ia, ahead=ahead, member=member, pip=pip, set=cs_set,
                set_pip=set_pip, size=member.sum(axis=1).astype(np.int64), mass=np.where(member, pip_ia, 0.0).sum(axis=1), zmax=zmax, M=M)


def _guards(B, info, z, zu, mvf_m, mvf_u):
    den = np.concatenate([np.diag(B), np.ones(len(info))])
    floor = np.concatenate([mvf_m * np.diag(B), mvf_u * info])
    with np.errstate(invalid="ignore"):
        ok = np.concatenate([np.isfinite(z), (info > 0) & np.isfinite(zu)])
    return den, floor, ok


def _guard_dist(res, B, info, S, mvf_m, mvf_u):
    """|share left - guard| of every candidate that is not a member of S, per set: the room a rounding error has"""
    scale = np.concatenate([np.diag(B), info])
    mvf = np.concatenate([np.full(B.shape[0], mvf_m), np.full(len(info), mvf_u)])
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(res["v1"] / scale[None, :] - mvf[None, :])
    d[:, [int(s) for s in S]] = np.inf
    d[np.isnan(d)] = np.inf
    return d


def cs_by_definition(B, B21, z, S, mvf_m, mvf_u, omega, rho):
    B, B21, z = np.asarray(B, dtype=np.float64), np.asarray(B21, dtype=np.float64), np.asarray(z, dtype=np.float64)
    S = [int(s) for s in S]
    M, U, n = len(z), B21.shape[0], len(S)
    m, info = _impute(B, B21, z)
    with np.errstate(invalid="ignore", divide="ignore"):
        zu = m / np.sqrt(info)
    base_r, base_v = np.concatenate([z, m]), np.concatenate([np.diag(B), info])
    rows = np.vstack([B, B21])                                 # row c = the candidate's covariances with the measured SNPs
    zc, v1 = np.zeros((n, M + U)), np.zeros((n, M + U))
    for a in range(n):
        Sp = np.array(S[:a] + S[a + 1:], dtype=np.int64)
        if len(Sp) == 0:
            r, v = base_r.copy(), base_v.copy()
        else:
            X = np.linalg.solve(B[np.ix_(Sp, Sp)], rows[:, Sp].T)      # [n - 1, T]: B_S'S'^-1 B_S'c
            r = base_r - z[Sp] @ X
            v = base_v - np.einsum("cn,nc->c", rows[:, Sp], X)
        with np.errstate(invalid="ignore", divide="ignore"):
            zc[a], v1[a] = r / np.sqrt(v), v
    den, floor, ok = _guards(B, info, z, zu, mvf_m, mvf_u)
    res = _tail(zc, v1, den, floor, ok, S, omega, rho, M)
    res["guard_dist"] = _guard_dist(res, B, info, S, mvf_m, mvf_u)
    return res


def cs_by_downdate(B, B21, z, S, mvf_m, mvf_u, omega, rho):
    B, B21, z = np.asarray(B, dtype=np.float64), np.asarray(B21, dtype=np.float64), np.asarray(z, dtype=np.float64)
    S = np.array([int(s) for s in S], dtype=np.int64)
    M, U, n = len(z), B21.shape[0], len(S)
    m, info = _impute(B, B21, z)
    with np.errstate(invalid="ignore", divide="ignore"):
        zu = m / np.sqrt(info)
    den, floor, ok = _guards(B, info, z, zu, mvf_m, mvf_u)
    zc, v1 = np.zeros((n, M + U)), np.zeros((n, M + U))
    if n:
        L = np.linalg.cholesky(B[np.ix_(S, S)])
        y = np.linalg.solve(L, z[S])
        P = np.linalg.inv(B[np.ix_(S, S)])
        beta = P @ z[S]
        W = np.linalg.solve(L, np.vstack([B[:, S], B21[:, S]]).T)      # [n, T]: column c = w_c
        r = np.concatenate([z, m]) - y @ W
        v = np.concatenate([np.diag(B), info]) - np.sum(W * W, axis=0)
        G = np.linalg.solve(L.T, W)                                    # [n, T]: g = L^-T w
        for a in range(n):
            with np.errstate(invalid="ignore", divide="ignore"):
                v1[a] = v + G[a] ** 2 / P[a, a]
                zc[a] = (r + G[a] * beta[a] / P[a, a]) / np.sqrt(v1[a])
            zc[a, S[a]] = beta[a] / np.sqrt(P[a, a])
            v1[a, S[a]] = 1.0 / P[a, a]
    res = _tail(zc, v1, den, floor, ok, S, omega, rho, M)
    res["guard_dist"] = _guard_dist(res, B, info, S, mvf_m, mvf_u)
    return res


def pip_tol(res, zc_tol=1e-8):
    """The absolute bound on pip, set_pip, mass and lse that follows from zc held to zc_tol as |d| / max(1, |zc|): a log Bayes factor
    moves by at most |zc| dzc <= max(1, zc^2) zc_tol, and a pip by at most twice that (its own lbf and the lse)."""
    return 2.0 * max(1.0, res["zmax"] ** 2) * zc_tol


def borderline(res, rho, margin, tol):
    """[n, T] bool: the memberships a rounding error could turn (module docstring)."""
    n, T = res["pip_ia"].shape
    out = np.zeros((n, T), dtype=bool)
    for a in range(n):
        p = res["pip_ia"][a]
        order = np.argsort(p, kind="stable")
        ps = p[order]
        csum = np.concatenate([[0.0], np.cumsum(ps)])
        lo, hi = np.searchsorted(ps, ps - tol, side="left"), np.searchsorted(ps, ps + tol, side="right")
        near = np.zeros(T)
        near[order] = csum[hi] - csum[lo] - ps                 # the mass of the other SNPs within tol of this one's pip
        live = p > 0
        if rho >= 1.0:
            # membership is pip > 0 and nothing else: only a pip at the edge of the double range (exp underflows between -745 and
            # -708) could come out on the other side of zero
            with np.errstate(invalid="ignore"):
                d = res["lbf"][a] - res["lse"][a]
            out[a] = (d > -760.0) & (d < -700.0)
        else:
            out[a] = live & (np.abs(rho - res["ahead"][a]) <= margin + near)
        out[a] |= res["guard_dist"][a] <= GUARD_MARGIN
    return out


# ---- the windows of tests/test_gpu_cs.py, built here so that tests/test_cs_ref.py can vet their seeds on the CPU --------------------
CHI2_GWS = 29.716785                       # 5e-8, two-sided
CS = dict(coverage=0.95, prior_var=25.0)


def window(M, U=40, seed=None, scale=0.02):
    from helpers import small_panel, split_window
    p = small_panel(n_snp=M + U + 30 + (M + U) // 20, scale=scale, seed=11 + M + U if seed is None else seed)
    assert p["G"].shape[0] >= M + U
    gm, gu, _ = split_window(dict(G=p["G"][: M + U]), M)
    return p, gm, gu


def planted(gm, seed, effect=(10.0, -9.0, 9.5)):
    """Z-scores with three signals spread through the window's (pooled) LD."""
    from oracle import oracle_np
    M = gm.shape[0]
    rng = np.random.default_rng(seed)
    causal = sorted({M // 7, M // 2, max(M - 9, 0)})
    B = oracle_np.pooled_cor(gm) if M > 1 else np.ones((1, 1))
    return B[:, causal] @ np.array(effect[: len(causal)]) + rng.standard_normal(M)


# (M, U, mode, slct, seed of the Z-scores): the kernel edges of test 1.  129 + 3 990 = 4 119 candidates lie beyond the 4 096 pips cs_set_kernel keeps in LDS,
# 127 + 3 969 = 4 096 on the limit; 1 213 + 2 512 is the largest window of the chr22 study
EDGE_CASES = [(M, U, mode, dict(max=32, chi2_stop=CHI2_GWS), 14 if (M, mode) == (12, 0) else M + mode) for (M, U) in ((1, 1), (2, 3), (12, 11), (127, 128), (129, 129), (513, 40))
              for mode in (0, 1)] + \
             [(129, 129, 1, dict(max=32, chi2_stop=0.0), 136), (129, 129, 0, dict(max=3, chi2_stop=CHI2_GWS, forced=[11, 2, 44]), 129),
              (127, 3969, 0, dict(max=32, chi2_stop=CHI2_GWS), 127), (129, 3990, 0, dict(max=32, chi2_stop=CHI2_GWS), 129),
              (1213, 2512, 1, dict(max=32, chi2_stop=CHI2_GWS), 1214)]
# (the Z-scores' seed is the tuple's last entry: chosen on the CPU so that no SNP of the case is borderline, tests/test_cs_ref.py)


# (cs dict, what it shows) on the weighted 127 + 128 window at the genome-wide threshold (n = 9): coverage and prior variance reach
# the kernels.  rho = 1 is the one check of "every candidate with pip > 0 is a member"
COVERAGE_CASES = [dict(coverage=0.5), dict(coverage=1.0), dict(prior_var=4.0), dict(coverage=0.99, prior_var=100.0)]
COVERAGE_WINDOW = (127, 128, 1, dict(max=32, chi2_stop=CHI2_GWS), 128)


def edge_window(M, U, mode, zseed):
    p, gm, gu = window(M, U, scale=0.1 if (mode and M > 1000) else 0.02)
    z1 = planted(gm, seed=zseed)
    return p, gm, gu, (p["w"] if mode else None), z1


def claim_window(u=19, seed=1):
    """The window of the claim the feature rests on: three planted signals of which one has an UNMEASURED causal SNP -- the measured
    SNPs carry its effect through B21 alone.  A dense window (300 SNPs in 40 kb), so that an imputed SNP has info above 0.8 without
    being the copy of a measured one (SNP u: info 0.81, largest r^2 with a measured SNP 0.62).  Returns (p, gm, gu, z1, u)."""
    from cond_ref import window_mats
    from helpers import small_panel, split_window
    p = small_panel(n_snp=300, scale=0.02, seed=23, span_bp=40_000)
    gm, gu, _ = split_window(dict(G=p["G"]), 200)
    B, B21 = window_mats(0, gm, gu, p["off"], None)
    rng = np.random.default_rng(seed)
    z1 = B[:, [200 // 7, 200 - 9]] @ np.array([10.0, 9.5]) + B21[u] * -12.0 + rng.standard_normal(200)
    return p, gm, gu, z1, u


def store_windows(seed=41, n_snp=2000, spans=((0, 131), (97, 340), (211, 560), (330, None), (400, 540))):
    """Overlapping windows over one panel, as a chromosome's (tests/test_gpu_cond.py's construction): per window the measured and
    unmeasured row indices into G, the Z-scores and the slct dict."""
    from helpers import small_panel
    p = small_panel(n_snp=n_snp, scale=0.05, seed=seed)
    G = p["G"]
    rng = np.random.default_rng(5)
    n = G.shape[0]
    measured = np.sort(rng.choice(n, size=n // 3, replace=False))
    unmeasured = np.setdiff1d(np.arange(n), measured)
    wins = []
    for k, (a, b) in enumerate(spans):
        mi = measured[a:b]
        lo, hi = mi[len(mi) // 4], mi[3 * len(mi) // 4]
        ui = unmeasured[(unmeasured > lo) & (unmeasured < hi)]
        slct = dict(max=32, chi2_stop=(CHI2_GWS, 20.0, CHI2_GWS, 20.0, CHI2_GWS)[k], forced=[len(mi) // 2, len(mi) // 7] if k == 1 else [], unmeasured=True, cs=dict(CS))
        wins.append(dict(mi=mi.astype(np.int32), ui=ui.astype(np.int32), z1=planted(G[mi], seed=70 + k), slct=slct))
    return p, wins


def clamped_window():
    """Duplicated measured SNPs at lambda = 0 (tests/test_gpu_cond.py's construction): a B11 MakePosDef repairs.  (p, gm, gu, z1)"""
    from helpers import small_panel, split_window
    p = small_panel(n_snp=70, scale=0.02, n_pops=6, seed=21)
    gm, gu, _ = split_window(p, 30)
    gm = np.ascontiguousarray(np.vstack([gm, gm[:3]]))
    z1 = planted(gm, seed=2)
    z1[30:] = z1[:3] + 0.3
    return p, gm, gu, z1


def copy_of_the_lead_window():
    """50 measured SNPs and, as the last unmeasured one, an exact copy of the measured SNP with the largest z^2.  (p, gm, gu, z1, j)"""
    from helpers import small_panel, split_window
    p = small_panel(n_snp=120, scale=0.02, seed=31)
    gm, gu, _ = split_window(dict(G=p["G"][:110]), 50)
    z1 = planted(gm, seed=4)
    j = int(np.argmax(z1 * z1))
    return p, gm, np.ascontiguousarray(np.vstack([gu, gm[j]])), z1, j


# ---- the study of the end-to-end test: files -> table ------------------------------------------------------------------------
POPS = [("AAA", 160, "EUR"), ("BBB", 145, "EUR"), ("CCC", 170, "ASN"), ("DDD", 133, "AFR"), ("EEE", 152, "EUR"), ("FFF", 90, "ASN")]
WGT = (["aaa", "CCC", "eee", "FFF", "zzz"], [0.45, 0.2, 0.25, 0.161, 0.3])
STUDY_WINDOW = (22, 1_500_000, 2_000_000, 300_000)
STUDY_P_CUT = 1e-4          # 23 / 24 signals in the window; at 0.05 all 32 steps are taken and two weak sets have a borderline SNP


def study_files(d):
    """(gwas, index, data, description) of the synthetic study, written into directory d"""
    from gauss_amd import panel as panel_mod
    st = panel_mod.make_synthetic_study(str(d), POPS, n_snp=700, bp_lo=1_000_000, bp_hi=2_400_000, n_genes=40, frac_measured=0.3, seed=17)
    q = st["paths"]
    return q["gwas.txt"], q["index.gz"], q["data.gz"], q["desc.txt"]


def study_cases(M):
    """(forced measured indices, max_signals, cs arguments) of the two calls the end-to-end test makes"""
    return (((), None, {}), ((4, M - 2), 2, dict(coverage=0.5, prior_var=4.0)))


def feeder_window(mix, files):
    """The study's window as oracle/feeder_py.py's dist / distmix build it: measured and unmeasured SNPs (reference order), their
    matrices, the selected populations' offsets and weights, the af1 cutoff and the population argument of the call."""
    from oracle import feeder_py as fp
    chr_, start_bp, end_bp, wing = STUDY_WINDOW
    who, cutoff = (WGT, 0.02) if mix else ("EUR", 0.01)
    inp, index, data, desc = files
    pops = fp.read_ref_desc(desc)
    flags, w = fp.pop_flags_wgt(pops, *who) if mix else (fp.pop_flags(pops, who), None)
    lo, hi = start_bp - wing, end_bp + wing
    m = fp.read_input_z(inp, chr_, lo, hi, False)
    fp.read_reference_index(m, index, chr_, lo, hi, False)
    vec = fp.make_snp_vec(m, data, flags, cutoff, w)
    meas = [s for s in vec if s.type == 1]
    unme = [s for s in vec if s.type == 0 and start_bp <= s.bp <= end_bp]
    return dict(meas=meas, unme=unme, gm=fp._matrix(meas), gu=fp._matrix(unme), off=fp._selected_off(pops, flags),
                w=None if w is None else np.asarray(w, dtype=np.float64), who=who, cutoff=cutoff)
