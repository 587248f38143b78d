"""numpy restatement of afmix() / cpw2() (afmix.cpp:30-215, cpw2.cpp:31-211) and the synthetic panels their tests share.

Steps 1-4 (study file, index merge, measured list, intervals) are restated on plain Python containers; steps 5-6 (per-interval
covariance, MakePosDef, inverse, accumulation, rounding) with numpy's eigh / inv."""
import math
import os

import numpy as np

from gauss_amd import panel

ST_CLAMPED, ST_NONFINITE = 1, 2


# ---- steps 1-4 -------------------------------------------------------------------------------------------------------------
def read_study(path):
    """ReadInputAf: {(chr, bp, a1, a2): [rsid, af1]}, a repeated key keeps its last row."""
    rows = {}
    with open(path) as f:
        f.readline()
        for line in f:
            t = line.split()
            rows[(int(t[1]), int(t[2]), t[3], t[4])] = [t[0], float(t[5])]
    return rows


def measured_list(study, panel_snps):
    """ReadReferenceIndexAll + the type-1 filter.  panel_snps: [(rsid, chr, bp, a1, a2)] in panel order (row = fpos).
    Returns [(rsid, chr, bp, a1, a2, af1study, panel_row)] in map order; raises ValueError on both orientations."""
    m = {k: dict(rsid=v[0], af=v[1], row=None) for k, v in study.items()}
    for row, (rsid, chr_, bp, a1, a2) in enumerate(panel_snps):
        k1, k2 = (chr_, bp, a1, a2), (chr_, bp, a2, a1)
        h1, h2 = k1 in m, k2 in m
        if h1 and h2:
            raise ValueError("ERROR: input file contains duplicates")
        if h1:
            m[k1].update(rsid=rsid, row=row)
        elif h2:
            e = m.pop(k2)
            e.update(rsid=rsid, row=row, af=1 - e["af"])
            m[k1] = e
    return [(e["rsid"], k[0], k[1], k[2], k[3], e["af"], e["row"]) for k, e in sorted(m.items()) if e["row"] is not None]


def interval_layout(S, interval):
    """interval i holds measured SNPs i, i + interval, ...: (interval_off, row of each measured SNP)."""
    sizes = [(S - i + interval - 1) // interval for i in range(interval)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = np.array([off[j % interval] + j // interval for j in range(S)], dtype=np.int64)
    return off, rows


def build_x(measured, panel_af, interval, cpw2=False):
    """The interval-major matrix [S, P + 1] (cpw2: asin(sqrt(.)) of every value, math.asin / math.sqrt)."""
    S, P = len(measured), panel_af.shape[1]
    off, rows = interval_layout(S, interval)
    x = np.zeros((S, P + 1))
    f = (lambda v: math.asin(math.sqrt(v))) if cpw2 else (lambda v: v)
    for j, m in enumerate(measured):
        x[rows[j], 0] = f(m[5])
        x[rows[j], 1:] = [f(float(v)) for v in panel_af[m[6]]]
    return x, off


# ---- steps 5-6 -------------------------------------------------------------------------------------------------------------
def interval_weights(x, off, eps=1e-5):
    """Per interval: (W_i [n_int, P], status [n_int], lambda_min of Cxx [n_int] (NaN where not finite))."""
    n_int, P = len(off) - 1, x.shape[1] - 1
    W = np.full((n_int, P), np.nan)
    st = np.zeros(n_int, dtype=np.int32)
    lmin = np.full(n_int, np.nan)
    for i in range(n_int):
        r = x[off[i]:off[i + 1]]
        n = r.shape[0]
        with np.errstate(all="ignore"):
            d = r - (r.sum(0) / n if n else np.nan)
            C = (d.T @ d) / (n - 1) if n else np.full((P + 1, P + 1), np.nan)
        if not np.all(np.isfinite(C[1:, :])):
            st[i] = ST_NONFINITE
            continue
        cxx, cxy = C[1:, 1:], C[1:, 0]
        lam, V = np.linalg.eigh(cxx)
        lmin[i] = lam.min()
        if lam.min() < eps:
            st[i] = ST_CLAMPED
            cxx = V @ np.diag(np.where(lam < eps, eps, lam)) @ V.T
        W[i] = np.linalg.inv(cxx) @ cxy
    return W, st, lmin


def finish(w_int):
    """W = sum_i W_i / interval in interval order; (raw W, rounded: < 0 -> 0, else floor(w * 1000 + 0.5) / 1000)."""
    n_int = w_int.shape[0]
    W = np.zeros(w_int.shape[1])
    for i in range(n_int):
        W = W + w_int[i] / n_int
    with np.errstate(invalid="ignore"):
        rounded = np.where(W < 0, 0.0, np.floor(W * 1000 + 0.5) / 1000)
    return W, rounded


# ---- synthetic panels ------------------------------------------------------------------------------------------------------
def make_panel(outdir, n_snp, pops, af=None, seed=5, prefix="pw", bp0=10_000):
    """BGZF text panel (index + data + description) with arbitrary per-population AF columns (the genotype strings are small
    and random: afmix reads only the AF).  pops: [(name, size, super)].  Returns dict(paths, snps [(rsid, chr, bp, a1, a2)], af)."""
    rng = np.random.default_rng(seed)
    P = len(pops)
    bp = bp0 + np.arange(n_snp) * 37 + rng.integers(0, 20, n_snp)
    alle = np.array(list("ACGT"))
    a1 = alle[rng.integers(0, 4, n_snp)]
    a2 = alle[(np.searchsorted(alle, a1) + rng.integers(1, 4, n_snp)) % 4]
    rsid = np.array([f"rs{500000 + i}" for i in range(n_snp)])
    chrs = np.full(n_snp, 7)
    if af is None:
        af = rng.uniform(0.02, 0.98, (n_snp, P))
    N = sum(p[1] for p in pops)
    G = rng.integers(0, 3, (n_snp, N)).astype(np.uint8)
    paths = {k: os.path.join(outdir, f"{prefix}_{k}") for k in ("desc.txt", "index.gz", "data.gz")}
    panel.write_pop_desc(paths["desc.txt"], pops)
    panel.write_panel(paths["index.gz"], paths["data.gz"], rsid, chrs, bp, a1, a2, G, af, [p[1] for p in pops])
    snps = [(str(rsid[i]), int(chrs[i]), int(bp[i]), str(a1[i]), str(a2[i])) for i in range(n_snp)]
    return dict(paths=paths, snps=snps, af=np.asarray(af, dtype=np.float64), pops=pops)


def pops_table(P, size=4):
    sup = ["AFR", "EUR", "EAS", "SAS", "AMR"]
    return [(f"P{k:02d}", size, sup[k % len(sup)]) for k in range(P)]
