"""Times simulateLD()'s GPU step: gauss_ld_resampled_rows on a resident 2-bit store shaped like the 33KG panel (26 populations,
~33 000 samples), at the (M, sim_size) pairs of --shapes, every weight summed to 1 (n_drawn = sim_size).

  (a) the blocking call (upload of the draw table, resample-pack, Gram, pooled LD epilogue, the M x M copy-out), best of --reps;
  (b) the numpy restatement on the same inputs (gather into the reference's geno_mat, then oracle_np.pooled_cor), where the
      gathered matrix stays below --numpy-max-cells;
  (c) the bytes the resample-pack kernel writes (M x Kp operand bytes) and the Gram's useful flop (M^2 x n_drawn), to be set
      against the kernel times of one `rocprofv3 --kernel-trace --stats -- python tools/simld_probe.py ...` run
      (resample_pack_kernel, the Gram kernel, the LD epilogue).

    python tools/simld_probe.py [--shapes 1213x10000,1213x100000,4000x100000] [--reps 3] [--numpy-max-cells 2e8] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gauss_amd import _lib, hotpath, panel  # noqa: E402


def _store(M, sizes, seed):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    af = rng.uniform(0.02, 0.6, size=(M, 1))
    G = (rng.random((M, off[-1])) < af).astype(np.uint8) + (rng.random((M, off[-1])) < af).astype(np.uint8)
    rows2, src = panel.pack2bit(G, off)
    return G, off, rows2, src


def probe(M, sim_size, reps, numpy_max, ctx):
    import simld_ref
    from oracle import oracle_np
    sizes = [1270 + 7 * k for k in range(26)]
    G, off, rows2, src = _store(M, sizes, 2026 + M)
    rng = np.random.default_rng(sim_size)
    q = rng.integers(0, 26, sim_size).astype(np.int32)
    s = (rng.random(sim_size) * np.array(sizes)[q]).astype(np.int32)
    rs = hotpath.RowStore(rows2, ctx=ctx)
    rows = np.arange(M, dtype=np.int32)
    try:
        hotpath.ld_resampled(rs, rows[:200], off, q, s, sim_size, fmt=_lib.GENO_2BIT, pop_src_off=src, ctx=ctx)     # warm-up
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = hotpath.ld_resampled(rs, rows, off, q, s, sim_size, fmt=_lib.GENO_2BIT, pop_src_off=src, ctx=ctx)
            ts.append(time.perf_counter() - t0)
    finally:
        rs.close()
    kp = (sim_size + 63) // 64 * 64
    out = dict(M=M, sim_size=sim_size, n_drawn=sim_size, call_ms=[round(t * 1e3, 2) for t in ts], call_best_ms=round(min(ts) * 1e3, 2),
               pack_bytes_written=int(M * kp), gram_useful_flop=float(M) * M * sim_size)
    if M * sim_size <= numpy_max:
        t0 = time.perf_counter()
        X = simld_ref.gathered(G, off, np.stack([q, s], 1).astype(np.int64), sim_size)
        want = oracle_np.pooled_cor(X)
        np.fill_diagonal(want, 1.0)
        out["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        ok = ~np.isnan(want)
        out["max_abs_diff_vs_numpy"] = float(np.max(np.abs(got[ok] - want[ok])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1213x10000,1213x100000,4000x100000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-max-cells", type=float, default=2e8)
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = hotpath.default_context()
    res = []
    for sh in a.shapes.split(","):
        M, n = (int(x) for x in sh.split("x"))
        r = probe(M, n, a.reps, a.numpy_max_cells, ctx)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
