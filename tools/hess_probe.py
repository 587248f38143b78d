"""Times hess (k_hess.hip, gauss_ld_hess_rows) where it matters.

  (a) gauss_ld_hess_rows, 3 traits, k_max 256, at three sizes: M = 520 (the first 520 measured SNPs of chr22's largest window), M = the
      measured set of that window (tools/slct_probe.py's store; about 1 200) and M = 4 096 (the chromosome's first 4 096 SNPs): the
      whole call, its sweeps and its launches of hess_block_round_kernel;
  (b) baseline (i), the LD build the call rides on: gauss_ld_clump_rows on the same rows (its kernel is some 0.1 ms of the call);
  (c) baseline (ii), what a user does today: gauss_ld_rows with the matrix back, then np.linalg.eigh on the host;
  (d) every timed form is run twice, interleaved with the others: the spread between identical runs is the margin of any comparison;
  (e) from a `rocprofv3 --kernel-trace` run of its own: per size the time in hess_block_round_kernel, hess_lambda_kernel and
      hess_proj_kernel per call, and the round kernel's time per launch.

Whole calls are timed by the host clock around the blocking call; the kernels' own times come from the trace, not from events placed in
the library.  Every GPU step is a child process under its own time limit; this process never opens the GPU.  A child that fails ends
the probe.

    python tools/hess_probe.py [--steps 5] [--warmup 1] [--json out.json] [--skip-trace] [--sizes 520,0,4096]      (0: the window's measured set)
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import susie_probe      # noqa: E402  (its child runner)

KERNELS = ("hess_block_round_kernel", "hess_lambda_kernel", "hess_proj_kernel")
T, K_MAX = 3, 256


def _calls(a):
    """{size: {form: a function that makes the call once and returns a figure that says what it did}}"""
    import slct_probe
    from gauss_amd import hotpath, workload
    _hp, ctx, jobs, keep = slct_probe._jobs(a.snps, 29.716785)
    big = jobs["largest"]["plain"][0]
    ch = workload.make_chromosome(a.snps, "distmix")       # (the chromosome slct_probe's store was made from: the same seed)
    measured = np.sort(big["packed"]["rows_m"]).astype(np.int32)
    store = (big["dev"][0], big["dev"][4])
    common = dict(pop_wgt=ch["w"], mode=hotpath.MODE_WEIGHTED, ctx=ctx)
    out = {}
    for size in a.sizes:
        rows = measured if size == 0 else (measured[:size] if size <= len(measured) else np.arange(size, dtype=np.int32))
        M = len(rows)
        z = np.random.default_rng(M).standard_normal((T, M)) * 2
        bp = ch["bp"][rows].astype(np.int32)

        def hess(rows=rows, z=z, M=M):
            r = hotpath.ld_hess_rows(store, rows, ch["off"], z, k_max=K_MAX, **common)
            return [r["sweeps"], r["n_pos"], r["status"], (((M + 31) // 32 * 2) - 1) * r["sweeps"]]

        def clump(rows=rows, z=z, bp=bp):
            return int(len(hotpath.ld_clump_rows(store, rows, ch["off"], bp, z[0] ** 2, **common)))

        def eigh(rows=rows):
            R = hotpath.ld_matrix_rows(store, rows, ch["off"], ch["w"], hotpath.MODE_WEIGHTED, 1.0, ctx=ctx)
            R = np.where(np.isfinite(R), R, 0.0)
            return float(np.linalg.eigh(R)[0][-1])

        out[M] = dict(hess=hess, clump=clump, eigh=eigh)
    return out, keep


def child_time(a):
    calls, _keep = _calls(a)
    res = {}
    for M, forms in calls.items():
        rounds, what = {k: [] for k in forms}, {}
        for _ in range(2):                                   # every form twice, interleaved: two identical runs of each
            for key, fn in forms.items():
                once = key == "eigh" and M > 2000            # (seconds of LAPACK a call: one timed call a round, no warm-up)
                for _ in range(0 if once else a.warmup):
                    fn()
                ts = []
                for _ in range(1 if once else a.steps):
                    t0 = time.perf_counter()
                    what[key] = fn()
                    ts.append(time.perf_counter() - t0)
                rounds[key].append(round(float(np.median(ts)) * 1e3, 3))
        sweeps, n_pos, status, launches = what["hess"]
        res[str(M)] = dict(call_ms=rounds, sweeps=sweeps, n_pos=n_pos, status=status, round_launches=launches,
                           spread_ms=round(max(abs(v[0] - v[1]) for v in rounds.values()), 3))
    print(json.dumps(res), flush=True)


def child_trace(a):
    calls, _keep = _calls(a)
    for M, forms in calls.items():                           # in this order: the trace's launches are read in it
        for _ in range(a.steps):
            forms["hess"]()
    print(json.dumps(dict(steps=a.steps)), flush=True)


def _kernel_times(rows, n, timed):
    """per size and kernel the time per call (summed over the kernel's launches in a call), and the round kernel's time per launch.  A
    size's launches of the round kernel are told by their grid (one workgroup of 256 threads per block pair); lambda and proj by order"""
    out = {}
    sizes = list(timed)
    for name in KERNELS:
        hits = sorted((r for r in rows if re.search(r"\b%s\b" % name, r.get("Kernel_Name", ""))), key=lambda r: int(r["Start_Timestamp"]))
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in hits]
        for i, m in enumerate(sizes):
            if name == "hess_block_round_kernel":
                grid = (int(m) + 31) // 32 * 256
                mine = [u for u, r in zip(us, hits) if int(r.get("Grid_Size", r.get("Grid_Size_X", -1))) == grid]
                k = timed[m]["round_launches"]
                if len(mine) != n * k:
                    raise SystemExit(f"hess_probe: the trace holds {len(mine)} launches of {name} at M = {m}, expected {n * k}")
                out.setdefault(m, {})["round_us_per_launch"] = round(sum(mine) / len(mine), 1)
            else:
                if len(us) != n * len(sizes):
                    raise SystemExit(f"hess_probe: the trace holds {len(us)} launches of {name}, expected {n * len(sizes)}")
                mine = us[i * n:(i + 1) * n]
            out.setdefault(m, {})[name + "_ms"] = round(sum(mine) / n / 1e3, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--sizes", default="520,0,4096")
    ap.add_argument("--json")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--child", choices=["time", "trace"])
    a = ap.parse_args()
    a.sizes = [int(x) for x in a.sizes.split(",")]
    if a.child:
        return (child_time if a.child == "time" else child_trace)(a)
    common = ["--snps", str(a.snps), "--sizes", ",".join(str(x) for x in a.sizes)]
    run = lambda args, limit, prefix=(): susie_probe._child(args, limit, prefix=prefix, script=__file__)
    out = dict(time=run(["--child", "time", "--steps", str(a.steps), "--warmup", str(a.warmup)] + common, 500))
    print(json.dumps(out["time"]), flush=True)
    if not a.skip_trace and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="hess_probe_")
        try:
            # a kernel trace on its own: no counters, no other tracing beside it; 2 calls of each size
            tr = run(["--child", "trace", "--steps", "2"] + common, 400, prefix=["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"])
            rows = []
            for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                with open(f) as fh:
                    rows += list(csv.DictReader(fh))
            out["trace"] = _kernel_times(rows, tr["steps"], out["time"])
        finally:
            shutil.rmtree(d, ignore_errors=True)
        print(json.dumps(out["trace"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
