"""Times the multi-trait fit (k_susie.hip's trait dimension) and the colocalisation of its traits (k_coloc.hip) on chr22's largest
window (tools/susie_probe.py's window: M = 1 213, U = 2 512, distmix, resident 2-bit store; L = 10, defaults).

  (a) one job with 1, 2, 4 and 8 fitted traits (k = 0, 1, 3, 7 further traits; the pairs asked where there are any), and the further
      traits imputed without being fitted (plain_traits): what the fit adds is the difference;
  (b) the yardstick: T one-trait jobs, each trait fitted alone as z1 of its own job (alone1 .. alone8; trait 1's is the one-trait
      job of tools/susie_probe.py, "default") -- the sum of the first T of them.  A trait that needs more sweeps costs more alone too.
      `--one-trait-ms X`: trait 1's one-trait job on another build (the parent commit's), reported beside this build's;
  (c) every form is run twice, interleaved with the others: the spread between identical runs is the margin of any comparison;
  (d) from a `rocprofv3 --kernel-trace` run of its own: the time of every kernel of the eight-trait fit.

Every GPU step is a child process under its own time limit; this process never opens the GPU.  A child that fails ends the probe.

    python tools/coloc_probe.py [--steps 15] [--warmup 3] [--one-trait-ms X] [--json out.json] [--skip-trace]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import susie_probe  # noqa: E402

KERNELS = susie_probe.KERNELS + ("coloc_kernel",)
TRAITS = (1, 2, 4, 8)
# the further traits' bumps at the three planted SNPs of susie_probe._planted: shared signals, signals of their own, one null trait
EFFECTS = [(8.0, -9.0, 0.0), (0.0, 9.0, -8.5), (-9.5, 0.0, 0.0), (0.0, 0.0, 0.0), (8.5, 8.0, 9.0), (0.0, -9.0, 0.0), (9.0, 0.0, -8.0)]


def _window(jobs):
    """susie_probe's planted window and seven further traits on it"""
    big = susie_probe._planted(jobs)
    M = big["dev"][2]
    rng = np.random.default_rng(7)
    Z = rng.standard_normal((7, M))
    for t, eff in enumerate(EFFECTS):
        for c, b in zip((M // 7, M // 2, M - 9), eff):
            lo, hi = max(c - 3, 0), min(c + 4, M)
            Z[t, lo:hi] += b * np.exp(-0.5 * (np.arange(lo, hi) - c) ** 2)
    return big, Z


def _forms(big, Z):
    forms = dict(plain=[big], plain_traits=[dict(big, z_more=Z)])
    for T in TRAITS:
        s = dict(traits=T - 1, coloc={}) if T > 1 else dict()
        forms[f"traits{T}"] = [dict(big, z_more=Z[: T - 1] if T > 1 else None, susie=s)]
    for t in range(1, 8):                                    # every further trait alone, as z1 of a one-trait job
        forms[f"alone{t + 1}"] = [dict(big, z1=Z[t - 1], susie=dict())]
    return forms


def child_time(a):
    import slct_probe
    hotpath, ctx, jobs, _keep = slct_probe._jobs(a.snps, 29.716785)
    big, Z = _window(jobs)
    forms = _forms(big, Z)
    made = {k: hotpath.Job(v, ctx=ctx, on_device=True) for k, v in forms.items()}
    rounds, info = {k: [] for k in forms}, {}
    for _ in range(2):                                       # every form twice, interleaved: two identical runs of each
        for key, job in made.items():
            ms, res = susie_probe._median_ms(job, a.steps, a.warmup)
            rounds[key].append(ms)
            r = res[0]
            if "susie_more_sweeps" in r:
                info[key] = dict(sweeps=[int(r["susie_sweeps"])] + [int(x) for x in r["susie_more_sweeps"]],
                                 kept=[int(r["susie_kept"].sum())] + [int(x.sum()) for x in r["susie_more_kept"]],
                                 pairs_of_kept_effects=int((r["coloc_hit"] >= 0).sum()), status=int(r["status"]))
            elif "susie_sweeps" in r:
                info[key] = dict(sweeps=[int(r["susie_sweeps"])], kept=[int(r["susie_kept"].sum())], status=int(r["status"]))
    for job in made.values():
        job.close()
    best = {k: min(v) for k, v in rounds.items()}
    alone = [best["traits1"]] + [best[f"alone{t}"] for t in range(2, 9)]
    out = dict(M=big["dev"][2], U=big["dev"][3], step_ms=rounds, spread_ms=round(max(abs(v[0] - v[1]) for v in rounds.values()), 4),
               alone_ms=alone, one_trait_ms_elsewhere=a.one_trait_ms if a.one_trait_ms > 0 else None, fit=info,
               yardstick_ms={T: round(sum(alone[:T]), 4) for T in TRAITS},
               ratio={T: round(best[f"traits{T}"] / sum(alone[:T]), 4) for T in TRAITS},
               added_by_the_fit_ms={T: round(best[f"traits{T}"] - (best["plain_traits"] if T > 1 else best["plain"]), 4) for T in TRAITS})
    print(json.dumps(out), flush=True)


def child_trace(a):
    import slct_probe
    hotpath, ctx, jobs, _keep = slct_probe._jobs(a.snps, 29.716785)
    big, Z = _window(jobs)
    job = hotpath.Job(_forms(big, Z)["traits8"], ctx=ctx, on_device=True)      # one job a traced process
    for _ in range(a.steps):
        job.run()
        job.fetch()
    job.close()
    print(json.dumps(dict(steps=a.steps)), flush=True)


def trace_times(rows, steps):
    res = {}
    for key in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if key in r.get("Kernel_Name", "")]
        if len(us) < steps:
            raise SystemExit(f"coloc_probe: the trace holds {len(us)} launches of {key} for {steps} steps")
        res[key] = dict(launches_per_step=round(len(us) / steps, 1), us_per_step=round(sum(us) / steps, 2), median_us=round(float(np.median(us)), 2),
                        max_us=round(max(us), 2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--one-trait-ms", type=float, default=0.0)
    ap.add_argument("--json")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--child", choices=["time", "trace"])
    a = ap.parse_args()
    if a.child:
        return (child_time if a.child == "time" else child_trace)(a)
    common = ["--snps", str(a.snps)]
    out = dict(time=susie_probe._child(["--child", "time", "--steps", str(a.steps), "--warmup", str(a.warmup), "--one-trait-ms",
                                        str(a.one_trait_ms)] + common, 400, script=__file__))
    print(json.dumps(out["time"]), flush=True)
    if not a.skip_trace and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="coloc_probe_")
        try:
            # a kernel trace on its own: no counters, no other tracing beside it; one job a process, 3 steps
            tr = susie_probe._child(["--child", "trace", "--steps", "3"] + common, 300,
                                    prefix=["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"], script=__file__)
            rows = []
            for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                with open(f) as fh:
                    rows += list(csv.DictReader(fh))
            out["trace"] = trace_times(rows, tr["steps"])
        finally:
            shutil.rmtree(d, ignore_errors=True)
        print(json.dumps(out["trace"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
