"""Times the joint fine-mapping across studies (k_xsusie.hip) on chr22's largest window (tools/susie_probe.py's window: M = 1 213,
U = 2 512, distmix, resident 2-bit store; L = 10, defaults): two studies of one trait on the same SNPs, study 2 with the ancestry
weights reversed and scores of its own around the same three planted signals.

  (a) one job of the two windows as a group (K = 2), against the same two windows fitted separately in one job (which shares every
      launch between them), against the two windows without a fit: what the coupling costs is the first difference;
  (b) every form is run twice, interleaved with the others: the spread between identical runs is the margin of any comparison;
  (c) from a `rocprofv3 --kernel-trace` run of its own: the time of every kernel of the group's fit and of the separate fits.

Every GPU step is a child process under its own time limit; this process never opens the GPU.  A child that fails ends the probe.

    python tools/xsusie_probe.py [--steps 15] [--warmup 3] [--json out.json] [--skip-trace]
"""
import argparse
import re
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

KERNELS = susie_probe.KERNELS + ("xsusie_ser_v_kernel", "xsusie_purity_kernel", "xsusie_kept_kernel")


def _studies(jobs):
    big = susie_probe._planted(jobs)
    M = big["dev"][2]
    rng = np.random.default_rng(11)
    z2 = rng.standard_normal(M)
    for c, b in ((M // 7, 7.0), (M // 2, -9.0), (M - 9, 7.5)):
        lo, hi = max(c - 3, 0), min(c + 4, M)
        z2[lo:hi] += b * np.exp(-0.5 * (np.arange(lo, hi) - c) ** 2)
    other = dict(big, z1=z2, pop_wgt=np.ascontiguousarray(np.asarray(big["pop_wgt"], dtype=np.float64)[::-1]))
    return big, other


def _forms(a, b):
    return dict(plain=[a, b], separate=[dict(a, susie=dict()), dict(b, susie=dict())],
                group=[dict(a, susie=dict(group=1)), dict(b, susie=dict(group=1))])


def child_time(args):
    import slct_probe
    hotpath, ctx, jobs, _keep = slct_probe._jobs(args.snps, 29.716785)
    forms = _forms(*_studies(jobs))
    made = {k: hotpath.Job(v, ctx=ctx, on_device=True) for k, v in forms.items()}
    rounds, info = {k: [] for k in forms}, {}
    for _ in range(2):
        for key, job in made.items():
            ms, res = susie_probe._median_ms(job, args.steps, args.warmup)
            rounds[key].append(ms)
            info[key] = [dict(sweeps=int(r["susie_sweeps"]), kept=int(r["susie_kept"].sum()), status=int(r["status"])) for r in res if "susie_sweeps" in r]
    for job in made.values():
        job.close()
    best = {k: min(v) for k, v in rounds.items()}
    out = dict(M=forms["plain"][0]["dev"][2], U=forms["plain"][0]["dev"][3], step_ms=rounds,
               spread_ms=round(max(abs(v[0] - v[1]) for v in rounds.values()), 4), fit=info,
               added_by_the_fit_ms=dict(separate=round(best["separate"] - best["plain"], 4), group=round(best["group"] - best["plain"], 4)),
               group_over_separate=round((best["group"] - best["plain"]) / (best["separate"] - best["plain"]), 4))
    print(json.dumps(out), flush=True)


def child_trace(args):
    import slct_probe
    hotpath, ctx, jobs, _keep = slct_probe._jobs(args.snps, 29.716785)
    job = hotpath.Job(_forms(*_studies(jobs))[args.form], ctx=ctx, on_device=True)      # one job a traced process
    for _ in range(args.steps):
        job.run()
        res = job.fetch()
    job.close()
    print(json.dumps(dict(steps=args.steps, sweeps=[int(r["susie_sweeps"]) for r in res if "susie_sweeps" in r])), flush=True)


def trace_times(rows, steps):
    res = {}
    for key in KERNELS:
        # (whole names: susie_ser_v_kernel is not xsusie_ser_v_kernel)
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if re.search(r"(?<![a-z_])" + key, r.get("Kernel_Name", ""))]
        if us:
            res[key] = dict(launches_per_step=round(len(us) / steps, 1), us_per_step=round(sum(us) / steps, 2), median_us=round(float(np.median(us)), 2),
                            max_us=round(max(us), 2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--json")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--child", choices=["time", "trace"])
    ap.add_argument("--form", default="group")
    a = ap.parse_args()
    if a.child:
        return (child_time if a.child == "time" else child_trace)(a)
    common = ["--snps", str(a.snps)]
    out = dict(time=susie_probe._child(["--child", "time", "--steps", str(a.steps), "--warmup", str(a.warmup)] + common, 400, script=__file__))
    print(json.dumps(out["time"]), flush=True)
    if not a.skip_trace and shutil.which("rocprofv3"):
        for form in ("group", "separate"):
            d = tempfile.mkdtemp(prefix="xsusie_probe_")
            try:
                # a kernel trace on its own: no counters, no other tracing beside it; one job a process, 3 steps
                tr = susie_probe._child(["--child", "trace", "--steps", "3", "--form", form] + common, 300,
                                        prefix=["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"], script=__file__)
                rows = []
                for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                    with open(f) as fh:
                        rows += list(csv.DictReader(fh))
                out["trace_" + form] = dict(trace_times(rows, tr["steps"]), sweeps=tr["sweeps"])
            finally:
                shutil.rmtree(d, ignore_errors=True)
            print(json.dumps({form: out["trace_" + form]}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
