"""Times zmix()'s GPU step against the route it replaces, and a whole zmix() call.

  (a) gauss_zmix_normal_eq at S selected SNPs (default 10 000, P = 26, ~100 samples per population): wall time of the blocking
      call (pack + Gram + the two k_zmix.hip kernels, a few kilobytes back), best of --reps.  The kernels alone come from one
      `rocprofv3 --kernel-trace --stats -- python tools/zmix_probe.py ...` run (zm_partial_kernel, zm_final_kernel beside
      the Gram and pack kernels).
  (b) the existing route at --old-snps (default 5 000): gauss_ld_per_pop's per-pair correlations copied out, then the numpy
      cross-products, on the same genotypes; the largest relative difference of X^T X between the two.
  (c) api.zmix on a packed synthetic panel (26 populations of 40 samples, no SNP monomorphic in the whole panel), population
      level, percentile 0.5, interval 1; the second call finds the study in the library's parsed-file cache.

    python tools/zmix_probe.py [--snps 10000] [--old-snps 5000] [--pops 26] [--reps 3] [--panel-snps 20000] [--skip-call]
                               [--json out.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gauss_amd import api, hotpath, panel, synth  # noqa: E402


def _geno(S, P, seed):
    rng = np.random.default_rng(seed)
    pops = [(f"P{k:02d}", int(rng.integers(90, 111)), f"S{k // 5}") for k in range(P)]
    bp = np.sort(rng.choice(np.arange(1, 300 * S), size=S, replace=False))
    G, _ = synth.synth_genotypes(bp, pops, seed=seed + 1)
    off = np.concatenate([[0], np.cumsum([p[1] for p in pops])]).astype(np.int32)
    return np.ascontiguousarray(G, dtype=np.uint8), off, rng.standard_normal(S) * 2.0


def kernel_probe(S, P, reps, ctx):
    G, off, z = _geno(S, P, 2026)
    hotpath.zmix_normal_eq(G[:300], off, z[:300], ctx=ctx)          # warm-up: code objects, attributes
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        xtx, xty, yty, n = hotpath.zmix_normal_eq(G, off, z, ctx=ctx)
        ts.append(time.perf_counter() - t0)
    return dict(S=S, P=P, N=int(off[-1]), pairs=S * (S - 1) // 2, n_rows=n, call_ms=[round(t * 1e3, 2) for t in ts],
                call_best_ms=round(min(ts) * 1e3, 2))


def old_route_probe(S, P, ctx):
    G, off, z = _geno(S, P, 2027)
    t0 = time.perf_counter()
    xtx, xty, _, n = hotpath.zmix_normal_eq(G, off, z, ctx=ctx)
    t_new = time.perf_counter() - t0
    t0 = time.perf_counter()
    r = hotpath.ld_per_pop(G, off, ctx=ctx)                         # [P, pairs], copied to the host
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    iu, ju = np.triu_indices(S, 1)
    y = z[iu] * z[ju]
    keep = np.isfinite(y) & np.isfinite(r).all(axis=0)
    rk, yk = r[:, keep], y[keep]
    D, d = rk @ rk.T, rk @ yk
    t_np = time.perf_counter() - t0
    return dict(S=S, P=P, pairs=len(y), bytes_copied=int(r.nbytes), new_call_ms=round(t_new * 1e3, 1),
                ld_per_pop_ms=round(t_copy * 1e3, 1), numpy_crossprod_ms=round(t_np * 1e3, 1),
                old_route_ms=round((t_copy + t_np) * 1e3, 1), n_rows_equal=int(keep.sum()) == n,
                max_rel_diff_xtx=float(np.max(np.abs(xtx - D)) / np.max(np.abs(D))),
                max_rel_diff_xty=float(np.max(np.abs(xty - d)) / max(1.0, np.max(np.abs(d)))))


def call_probe(n_snp, ctx):
    d = tempfile.mkdtemp(prefix="zmix_probe_")
    pops = [(a, 40, s) for a, _, s in synth.POPS_33KG[:26]]
    rng = np.random.default_rng(5)
    t0 = time.perf_counter()
    bp = np.sort(rng.choice(np.arange(1_000_000, 1_000_000 + 200 * n_snp), size=n_snp, replace=False))
    G, _ = synth.synth_genotypes(bp, pops, seed=6)
    keep = G.min(1) != G.max(1)                  # a SNP monomorphic in the whole panel has norm_var 0 / 0 (an error, as in R)
    G, bp = np.ascontiguousarray(G[keep]), bp[keep]
    S = len(bp)
    off = np.concatenate([[0], np.cumsum([p[1] for p in pops])])
    af = np.column_stack([G[:, off[k]:off[k + 1]].mean(1) / 2 for k in range(len(pops))])
    rsid = np.char.add("rs", np.arange(S).astype(str))
    chrs = np.full(S, 22)
    a1, a2 = np.full(S, "A"), np.full(S, "G")
    paths = {k: os.path.join(d, k) for k in ("desc.txt", "index.gz", "data.gz", "gwas.txt")}
    panel.write_pop_desc(paths["desc.txt"], pops)
    panel.write_panel(paths["index.gz"], paths["data.gz"], rsid, chrs, bp, a1, a2, G, af, [p[1] for p in pops])
    meas = np.sort(rng.choice(S, size=S // 2, replace=False))
    panel.write_gwas(paths["gwas.txt"], rsid[meas], chrs[meas], bp[meas], a1[meas], a2[meas], rng.standard_normal(len(meas)) * 2)
    packed = os.path.join(d, "panel.gpk")
    api.pack_panel(paths["index.gz"], paths["data.gz"], paths["desc.txt"], packed)
    t_write = time.perf_counter() - t0
    ts = []
    for _ in range(2):
        t0 = time.perf_counter()
        df, det = api.zmix(paths["gwas.txt"], paths["index.gz"], packed, paths["desc.txt"], percentile=0.5, interval=1, ctx=ctx,
                           detail=True)
        ts.append(time.perf_counter() - t0)
    shutil.rmtree(d, ignore_errors=True)
    return dict(panel_snps=S, P=len(pops), files_written_s=round(t_write, 1), n_snp=det["n_snp"], n_pairs=det["n_pairs"],
                n_rows=det["n_rows"], zmix_call_s=[round(t, 3) for t in ts], weight_sum=float(df["Weight"].sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, default=10_000)
    ap.add_argument("--old-snps", type=int, default=5_000)
    ap.add_argument("--pops", type=int, default=26)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--panel-snps", type=int, default=20_000)
    ap.add_argument("--skip-call", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = hotpath.default_context()
    out = dict(kernel=kernel_probe(a.snps, a.pops, a.reps, ctx))
    print(json.dumps(out["kernel"]), flush=True)
    out["old_route"] = old_route_probe(a.old_snps, a.pops, ctx)
    print(json.dumps(out["old_route"]), flush=True)
    if not a.skip_call:
        out["call"] = call_probe(a.panel_snps, ctx)
        print(json.dumps(out["call"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
