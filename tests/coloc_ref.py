"""Reference statements of the multi-trait fit and the colocalisation of its traits (test infrastructure, numpy only).

Definition (include/gauss_hip.h, coloc_*): every fitted trait is susie_ref.fit_w on the window's B, C and the
trait's own scores.  For traits a < b, a kept effect la of a and a kept effect lb of b, with l1 = lbf row la of a, l2 = lbf row lb of b
and J the candidates admissible in both fits: coloc's bf_bf (Wallace 2021) on (l1, l2) over J.  Two statements:

* ``coloc`` states what the kernel evaluates: three sums shifted by their maxima, S1 S2 - S12 formed in logs;
* ``coloc_direct`` sums the H3 terms one by one over j != k in O(n^2), shifted once by max l1 + max l2, and shares no line with it.

``borderline`` is susie_ref.borderline of every fit plus the pairs of kept effects whose two largest l1 + l2 are within the value
tolerance of one another: there a rounding error could move ``hit``.
"""
import numpy as np

import susie_ref as sr

PRIORS = dict(p1=1e-4, p2=1e-4, p12=1e-5)


def pair_list(k):
    """The pairs of 1 + k fitted traits in the order of the outputs"""
    return [(a, b) for a in range(k + 1) for b in range(a + 1, k + 1)]


def fit_traits(B, C, z1, z_more, k, **kw):
    return [sr.fit_w(B, C, z1, **kw)] + [sr.fit_w(B, C, z_more[t], **kw) for t in range(k)]


def coloc(l1, l2, J, p1, p2, p12):
    idx = np.flatnonzero(J)
    n = len(idx)
    if n == 0:
        return dict(pp=np.full(5, np.nan), hit=-1, hit_pp=np.nan, n=0)
    x, y = l1[idx], l2[idx]
    s = x + y
    m1, m2, m12 = x.max(), y.max(), s.max()
    t12 = np.exp(s - m12).sum()
    ls1, ls2, ls12 = m1 + np.log(np.exp(x - m1).sum()), m2 + np.log(np.exp(y - m2).sum()), m12 + np.log(t12)
    both = ls1 + ls2
    ratio = ls12 - both
    lh = np.array([0.0, np.log(p1) + ls1, np.log(p2) + ls2,
                   -np.inf if ratio >= 0.0 else (np.log(p1) + np.log(p2)) + (both + np.log1p(-np.exp(ratio))), np.log(p12) + ls12])
    w = np.exp(lh - lh.max())
    return dict(pp=w / w.sum(), hit=int(idx[int(np.argmax(s))]), hit_pp=float(1.0 / t12), n=n, s=s)


def coloc_direct(l1, l2, J, p1, p2, p12):
    """The hypotheses' sums term by term: H1 = p1 sum_j e^l1_j, H2 = p2 sum_k e^l2_k, H3 = p1 p2 sum_{j != k} e^(l1_j + l2_k),
    H4 = p12 sum_j e^(l1_j + l2_j), all divided by e^(max l1 + max l2) (H0 with them)."""
    idx = [int(j) for j in np.flatnonzero(J)]
    if not idx:
        return dict(pp=np.full(5, np.nan), hit=-1, hit_pp=np.nan, n=0)
    c1, c2 = max(l1[j] for j in idx), max(l2[j] for j in idx)
    e1, e2 = {j: np.exp(l1[j] - c1) for j in idx}, {j: np.exp(l2[j] - c2) for j in idx}
    h3 = 0.0
    for j in idx:
        h3 += e1[j] * sum(e2[k] for k in idx if k != j)
    h4 = sum(e1[j] * e2[j] for j in idx)
    h = np.array([np.exp(-c1 - c2), p1 * sum(e1.values()) * np.exp(-c2), p2 * sum(e2.values()) * np.exp(-c1), p1 * p2 * h3, p12 * h4])
    best = max(idx, key=lambda j: (l1[j] + l2[j], -j))
    return dict(pp=h / h.sum(), hit=best, hit_pp=float(e1[best] * e2[best] / h4), n=len(idx))


def pairs(fits, statement=coloc, **priors):
    """coloc_pp [pairs, L, L, 5], coloc_hit, coloc_hit_pp [pairs, L, L], coloc_n [pairs] as the library returns them"""
    pr = dict(PRIORS)
    pr.update(priors)
    pl = pair_list(len(fits) - 1)
    L = len(fits[0]["V"])
    pp, hit, hit_pp = np.full((len(pl), L, L, 5), np.nan), np.full((len(pl), L, L), -1, dtype=np.int64), np.full((len(pl), L, L), np.nan)
    n = np.zeros(len(pl), dtype=np.int64)
    for q, (a, b) in enumerate(pl):
        J = fits[a]["adm"] & fits[b]["adm"]
        n[q] = int(J.sum())
        for la in np.flatnonzero(fits[a]["kept"]):
            for lb in np.flatnonzero(fits[b]["kept"]):
                r = statement(fits[a]["lbf"][la], fits[b]["lbf"][lb], J, pr["p1"], pr["p2"], pr["p12"])
                pp[q, la, lb], hit[q, la, lb], hit_pp[q, la, lb] = r["pp"], r["hit"], r["hit_pp"]
    return dict(pp=pp, hit=hit, hit_pp=hit_pp, n=n)


def pair_tol(fits, tols, a, b):
    """PP and hit_pp of a pair: lH4 adds one lbf of each fit, and the softmax does not amplify"""
    return tols[a] + tols[b]


def borderline(fits, kw, tols):
    out = []
    for t, (f, tol) in enumerate(zip(fits, tols)):
        out += [f"trait {t}: {s}" for s in sr.borderline(f, kw, tol)]
    for a, b in pair_list(len(fits) - 1):
        J = fits[a]["adm"] & fits[b]["adm"]
        if J.sum() < 2:
            continue
        for la in np.flatnonzero(fits[a]["kept"]):
            for lb in np.flatnonzero(fits[b]["kept"]):
                s = np.sort((fits[a]["lbf"][la] + fits[b]["lbf"][lb])[J])
                if s[-1] - s[-2] <= pair_tol(fits, tols, a, b):
                    out.append(f"pair ({a}, {b}) effects ({la}, {lb}): the two largest l1 + l2 within the tolerance")
    return out


# ---- the windows of tests/test_gpu_coloc.py, built here so that tests/test_coloc_ref.py can vet them on the CPU -----------------------
# the further traits' planted effects at cs_ref.planted's three causal SNPs: shared signals, a signal of its own, a trait without any
EFFECTS = [(9.0, -8.0, 0.0), (0.0, 9.5, -9.0), (-10.0, 0.0, 0.0), (0.0, 0.0, 0.0), (8.5, 9.0, 9.5), (0.0, -9.0, 0.0), (9.0, 0.0, -8.5)]


def traits_z(gm, k, seed):
    """z_more [k, M]: cs_ref.planted with the effects above, every trait with its own noise"""
    import cs_ref
    return np.array([cs_ref.planted(gm, seed=1000 * (t + 1) + seed, effect=EFFECTS[t % len(EFFECTS)]) for t in range(k)]).reshape(k, gm.shape[0])


def case_window(M, U, k, seed):
    """(p, gm, gu, z1, z_more) of a case"""
    p, gm, gu, z1 = sr.small_window(M, U, seed)
    return p, gm, gu, z1, traits_z(gm, k, seed)


# (M, U, susie arguments, further traits k, (seed under pooled LD, under weighted LD)).  (1, 1) with measured_only: n = 1 and PP.H3 is an
# exact 0; 63 / 65 on either side of the wave's 64 columns; 250 + 30: candidate blocks of 256 that straddle M; U = 1025: past the
# SUSIE_CH = 1024 candidates in LDS; 64 + 4040 = 4104 candidates: past the CS_LDS_T = 4096 of cs_set_row.  Two, three and eight fitted
# traits; L = 1, 10, 32.  The seeds are those tests/test_coloc_ref.py vets: no fit and no pair of them is borderline.
CASES = [
    (1, 1, dict(L=1, tol=0.0, max_sweeps=1, measured_only=True), 1, (3, 3)),
    (12, 11, dict(L=10, tol=0.0, max_sweeps=5), 7, (14, 14)),
    (9, 7, dict(L=32, tol=0.0, max_sweeps=2), 1, (8, 8)),
    (63, 192, dict(L=10, tol=0.0, max_sweeps=5), 1, (10, 10)),
    (65, 192, dict(L=10, tol=0.0, max_sweeps=5), 2, (10, 48)),
    (250, 30, dict(L=3, tol=0.0, max_sweeps=5), 2, (11, 19)),
    (40, 1025, dict(L=5, tol=0.0, max_sweeps=5), 1, (16, 23)),
    (64, 4040, dict(L=2, tol=0.0, max_sweeps=1), 1, (23, 21)),
]
CASE_MODES = [(c[0], c[1], c[2], c[3], c[4][mode], mode) for c in CASES for mode in (0, 1)]
# the traits stop at different sweeps: three planted signals beside pure noise, default tol
SWEEPS_CASE = (129, 129, dict(L=10), 13)


def sweeps_window():
    M, U, kw, seed = SWEEPS_CASE
    p, gm, gu, z1 = sr.small_window(M, U, seed)
    from cond_ref import window_mats
    B, _ = window_mats(0, gm, gu, p["off"], None)
    z_more = (np.random.default_rng(5).multivariate_normal(np.zeros(M), B) * 0.7).reshape(1, M)
    return p, gm, gu, z1, z_more, kw


def planted_window(which, seed=3):
    """The planted claims, on the window of susie_ref.tag_window's panel (M = 100, U = 50, pooled), z = column . effect + 0.5 noise:
    "shared": two traits driven by measured SNP 52 (effects 9 and -7); "distinct": by SNPs 52 and 70 (r = 0.029); "unmeasured": both by
    UNMEASURED SNP 7; "null": the first by SNP 52, the second pure noise.  Returns (p, gm, gu, z1, z_more [1, M])."""
    from cond_ref import window_mats
    p, gm, gu, _, _ = sr.tag_window()
    B, C = window_mats(0, gm, gu, p["off"], None)
    rng = np.random.default_rng(seed)
    e1, e2 = 0.5 * rng.standard_normal(100), 0.5 * rng.standard_normal(100)
    if which == "shared":
        z = B[:, 52] * 9.0 + e1, B[:, 52] * -7.0 + e2
    elif which == "distinct":
        z = B[:, 52] * 9.0 + e1, B[:, 70] * 9.0 + e2
    elif which == "unmeasured":
        z = C[7] * 12.0 + e1, C[7] * -11.0 + e2
    else:
        z = B[:, 52] * 9.0 + e1, e2
    return p, gm, gu, z[0], z[1].reshape(1, 100)


# ---- the study of the end-to-end test: three files -> table ---------------------------------------------------------------------
STUDY_ARGS = dict(L=6, coverage=0.9, max_sweeps=40)
STUDY_P12 = 2e-5
STUDY_SEED = 10            # of the further files' noise: the one tests/test_coloc_ref.py vets under pooled and weighted LD


def study(d, seed=None):
    """cs_ref's study in directory d and two further files.  Trait 2 = -0.8 x trait 1's Z-scores plus noise, a tenth of its rows
    allele-swapped and the rows shuffled (it shares trait 1's signals); trait 3 = noise, file order reversed; `lacking` = trait 3
    without the rows of the prediction window's first two SNPs."""
    import os
    import cs_ref
    files = cs_ref.study_files(d)
    rows = [l.split() for l in open(files[0]).read().splitlines()[1:]]
    rng = np.random.default_rng(STUDY_SEED if seed is None else seed)
    z2 = -0.8 * np.array([float(r[5]) for r in rows]) + 0.5 * rng.standard_normal(len(rows))
    z3 = rng.standard_normal(len(rows))
    swap = rng.random(len(rows)) < 0.1

    def write(name, recs):
        path = os.path.join(str(d), name)
        with open(path, "w") as f:
            f.write("rsid chr bp a1 a2 z\n")
            for r in recs:
                f.write(f"{r[0]} {r[1]} {r[2]} {r[3]} {r[4]} {float(r[5])!r}\n")
        return path
    t2 = [(r[0], r[1], r[2], r[4], r[3], -z) if s else (r[0], r[1], r[2], r[3], r[4], z) for r, z, s in zip(rows, z2, swap)]
    t3 = [tuple(r[:5]) + (z,) for r, z in zip(rows, z3)][::-1]
    inside = [r[0] for r in rows if cs_ref.STUDY_WINDOW[1] <= int(r[2]) <= cs_ref.STUDY_WINDOW[2]]
    return dict(files=files, more=[write("trait2.txt", [t2[k] for k in rng.permutation(len(t2))]), write("trait3.txt", t3)],
                lacking=write("trait3_lacking.txt", [r for r in t3 if r[0] not in inside[:2]]))


def study_z_more(meas, more):
    """The further files' Z-scores at the measured SNPs `meas` of a window (oracle SNP records), in the window's allele orientation"""
    out = []
    for path in more:
        by = {}
        for l in open(path).read().splitlines()[1:]:
            r = l.split()
            by[r[0]] = (r[3], r[4], float(r[5]))
        out.append([by[s.rsid][2] if (by[s.rsid][0], by[s.rsid][1]) == (s.a1, s.a2) else -by[s.rsid][2] for s in meas])
    return np.array(out)
