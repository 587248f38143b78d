"""Times the multi-causal fine-mapping (k_susie.hip) on the chr22 study's jobs (tools/slct_probe.py's jobs: distmix, resident 2-bit
store).

  (a) the largest window alone (M = 1 213, U = 2 512): plain; the fit held to exactly S sweeps (tol = 0) for S = 1, 5, 20 -- the slope
      is the cost of one sweep, i.e. of L x 2 dependent launches -- ; the default fit (tol = 1e-4, max_sweeps = 100): its sweeps,
      its time, and what the launches queued behind convergence cost (its time minus the 5-sweep fit's minus the slope times the
      sweeps beyond 5; the 1-sweep fit is no anchor: its sets are still spread over the window and their purity costs milliseconds);
  (b) the 36-window chr22 job: plain, and with its three largest windows asking;
  (b2) the planted tag window of the tests (tests/susie_ref.py:tag_window, M = 100, U = 50, byte rows uploaded once): plain and the
      default fit -- time and sweeps of a small converged fit, where the launches queued behind convergence dominate;
  (c) every form is run twice, interleaved with the others: the spread between identical runs is the margin of any comparison;
  (d) from a `rocprofv3 --kernel-trace` run of its own: the time of every susie kernel of the largest window's default fit.

Every GPU step is a child process under its own time limit; this process never opens the GPU.  A child that fails ends the probe.

    python tools/susie_probe.py [--steps 20] [--warmup 3] [--json out.json] [--skip-trace]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
KERNELS = ("susie_w_kernel", "susie_prep_kernel", "susie_ser_v_kernel", "susie_rb_kernel", "susie_set_kernel", "susie_rank_kernel",
           "susie_purity_kernel", "susie_kept_kernel", "susie_fold_kernel")


def _planted(jobs):
    """The jobs of slct_probe with three planted signals in the z of the largest window (its own z is noise: nothing to fine-map)"""
    big = jobs["largest"]["plain"][0]
    M = big["dev"][2]
    z = np.array(big["z1"], dtype=np.float64)
    for c, b in ((M // 7, 9.0), (M // 2, -8.0), (M - 9, 8.5)):
        lo, hi = max(c - 3, 0), min(c + 4, M)
        z[lo:hi] += b * np.exp(-0.5 * (np.arange(lo, hi) - c) ** 2)      # a short bump: neighbours in LD share the signal
    return dict(big, z1=z)


def _median_ms(job, steps, warmup):
    for _ in range(warmup):
        job.run()
        res = job.fetch()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        job.run()
        res = job.fetch()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e3, 4), res


def child_time(a):
    import slct_probe
    hotpath, ctx, jobs, _keep = slct_probe._jobs(a.snps, 29.716785)
    big = _planted(jobs)
    chr22 = jobs["chr22"]["plain"]
    order = sorted(range(len(chr22)), key=lambda k: -chr22[k]["dev"][2])[:3]
    forms = dict(plain=[big], default=[dict(big, susie=dict())])
    for s in (1, 5, 20):
        forms[f"sweeps{s}"] = [dict(big, susie=dict(tol=0.0, max_sweeps=s))]
    import susie_ref
    tp, tgm, tgu, tz1, _ = susie_ref.tag_window()
    tag = dict(mode=0, geno_m=tgm, geno_u=tgu, pop_off=tp["off"], pop_wgt=None, z1=tz1)
    forms["tag"] = [tag]
    forms["tag_default"] = [dict(tag, susie=dict())]
    forms["chr22"] = chr22
    forms["chr22_3ask"] = [dict(w, susie=dict()) if k in order else w for k, w in enumerate(chr22)]
    made = {k: hotpath.Job(v, ctx=ctx, on_device=not k.startswith("tag")) for k, v in forms.items()}
    rounds = {k: [] for k in forms}
    info = {}
    for _ in range(2):                                       # every form twice, interleaved: two identical runs of each
        for key, job in made.items():
            ms, res = _median_ms(job, a.steps, a.warmup)
            rounds[key].append(ms)
            if key == "default":
                info = dict(sweeps=int(res[0]["susie_sweeps"]), kept=int(res[0]["susie_kept"].sum()), status=int(res[0]["status"]))
            if key == "tag_default":
                info["tag"] = dict(sweeps=int(res[0]["susie_sweeps"]), kept=int(res[0]["susie_kept"].sum()), status=int(res[0]["status"]))
            if key == "chr22_3ask":
                info["chr22_sweeps"] = [int(res[k]["susie_sweeps"]) for k in order]
    for job in made.values():
        job.close()
    best = {k: min(v) for k, v in rounds.items()}
    sweep_ms = (best["sweeps20"] - best["sweeps5"]) / 15.0
    out = dict(M=big["dev"][2], U=big["dev"][3], step_ms=rounds, spread_ms=round(max(abs(v[0] - v[1]) for v in rounds.values()), 4),
               one_sweep_ms=round(sweep_ms, 4), one_step_us=round(sweep_ms * 1e3 / 10, 2), fit=info,
               default_added_ms=round(best["default"] - best["plain"], 4),
               empty_launches_ms=round(best["default"] - best["sweeps5"] - (info["sweeps"] - 5) * sweep_ms, 4),
               tag_added_ms=round(best["tag_default"] - best["tag"], 4), chr22_added_ms=round(best["chr22_3ask"] - best["chr22"], 4))
    print(json.dumps(out), flush=True)


def child_trace(a):
    import slct_probe
    hotpath, ctx, jobs, _keep = slct_probe._jobs(a.snps, 29.716785)
    job = hotpath.Job([dict(_planted(jobs), susie=dict())], ctx=ctx, on_device=True)      # one job a traced process
    for _ in range(a.steps):
        job.run()
        job.fetch()
    job.close()
    print(json.dumps(dict(steps=a.steps)), flush=True)


def trace_times(rows, steps):
    """Per kernel name: launches a step, the time of all of them a step, and the median of one launch, in microseconds"""
    res = {}
    for key in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if key in r.get("Kernel_Name", "")]
        if len(us) < steps:
            raise SystemExit(f"susie_probe: the trace holds {len(us)} launches of {key} for {steps} steps")
        res[key] = dict(launches_per_step=round(len(us) / steps, 1), us_per_step=round(sum(us) / steps, 2), median_us=round(float(np.median(us)), 2),
                        max_us=round(max(us), 2))
    return res


def _child(args, limit, prefix=(), script=None):
    """script: the probe whose child this is (tools/coloc_probe.py starts its own through here)"""
    cmd = list(prefix) + [sys.executable, os.path.abspath(script or __file__)] + args
    # a session of its own: under the profiler the process that holds the GPU is a grandchild, and the time limit ends the whole group
    pr = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, start_new_session=True)
    try:
        so, se = pr.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(pr.pid, signal.SIGKILL)
        pr.communicate()
        raise SystemExit(f"susie_probe: child {args[0]} passed its time limit of {limit} s; nothing more is run")
    if pr.returncode != 0:
        sys.stderr.write(se.decode()[-2000:])
        raise SystemExit(f"susie_probe: child {args[0]} ended with status {pr.returncode}; nothing more is run")
    lines = [l for l in so.decode().splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--json")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--child", choices=["time", "trace"])
    a = ap.parse_args()
    if a.child:
        return (child_time if a.child == "time" else child_trace)(a)
    common = ["--snps", str(a.snps)]
    out = dict(time=_child(["--child", "time", "--steps", str(a.steps), "--warmup", str(a.warmup)] + common, 400))
    print(json.dumps(out["time"]), flush=True)
    if not a.skip_trace and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="susie_probe_")
        try:
            # a kernel trace on its own: no counters, no other tracing beside it; one job a process, 3 steps
            tr = _child(["--child", "trace", "--steps", "3"] + common, 300,
                        prefix=["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"])
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
