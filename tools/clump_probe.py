"""Times LD clumping (k_clump.hip, gauss_ld_clump_rows) where it matters.

  (a) the SNPs of chr22's largest window (tools/slct_probe.py's store: measured and unmeasured rows together, about 3 700) as one
      region, PLINK's defaults (p1 1e-4, p2 1e-2, r2 0.5, 250 kb) on the benchmark's z;
  (b) the same region with key_index = key_member = 0 and r2_min = 1: almost every SNP leads its own clump, the step loop's worst case;
  (c) the same region as gauss_ld_rows with the matrix back (what a caller who clumps in Python pays before the first comparison);
  (d) (b) on the first 8 192 SNPs of the chromosome: the stated worst case of a call;
  (e) every form is run twice, interleaved with the others: the spread between identical runs is the margin of any comparison;
  (f) from a `rocprofv3 --kernel-trace` run of its own: the times of clump_kernel in (a), (b) and (d).

Every GPU step is a child process under its own time limit; this process never opens the GPU.  A child that fails ends the probe.

    python tools/clump_probe.py [--steps 10] [--warmup 2] [--json out.json] [--skip-trace]
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

FORMS = ("defaults", "worst", "matrix", "worst8192")


def _calls(a):
    """{form: a function that makes the call once and returns a figure that says what it did}"""
    import slct_probe
    from gauss_amd import hotpath, workload
    _hp, ctx, jobs, keep = slct_probe._jobs(a.snps, 29.716785)
    big = jobs["largest"]["plain"][0]
    ch = workload.make_chromosome(a.snps, "distmix")       # (the chromosome slct_probe's store was made from: the same seed)
    rows = np.sort(np.concatenate([big["packed"]["rows_m"], big["packed"]["rows_u"]])).astype(np.int32)
    store = (big["dev"][0], big["dev"][4])
    z = np.asarray(ch["z"], dtype=np.float64)
    common = dict(pop_wgt=ch["w"], mode=hotpath.MODE_WEIGHTED, ctx=ctx)

    def clump(r, **kw):
        return hotpath.ld_clump_rows(store, r, ch["off"], ch["bp"][r].astype(np.int32), z[r] * z[r], **common, **kw)

    first = np.arange(min(8192, len(ch["bp"])), dtype=np.int32)
    worst = dict(radius=250_000, r2_min=1.0, key_index=0.0, key_member=0.0)
    calls = dict(defaults=lambda: int(clump(rows)["n_clumps"]), worst=lambda: int(clump(rows, **worst)["n_clumps"]),
                 matrix=lambda: int(hotpath.ld_matrix_rows(store, rows, ch["off"], ch["w"], hotpath.MODE_WEIGHTED, 1.0, ctx=ctx).shape[0]),
                 worst8192=lambda: int(clump(first, **worst)["n_clumps"]))
    return calls, dict(M=int(len(rows)), M_first=int(len(first)), N=int(ch["off"][-1])), keep


def child_time(a):
    calls, info, _keep = _calls(a)
    rounds, what = {k: [] for k in FORMS}, {}
    for _ in range(2):                                       # every form twice, interleaved: two identical runs of each
        for key in FORMS:
            for _ in range(a.warmup):
                calls[key]()
            ts = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                what[key] = calls[key]()
                ts.append(time.perf_counter() - t0)
            rounds[key].append(round(float(np.median(ts)) * 1e3, 3))
    out = dict(info, call_ms=rounds, clumps={k: what[k] for k in FORMS if k != "matrix"}, matrix_MB=round(info["M"] ** 2 * 8 / 1e6, 1),
               spread_ms=round(max(abs(v[0] - v[1]) for v in rounds.values()), 3))
    print(json.dumps(out), flush=True)


def child_trace(a):
    calls, _info, _keep = _calls(a)
    for key in ("defaults", "worst", "worst8192"):           # in this order: the trace's launches of clump_kernel are read in it
        for _ in range(a.steps):
            calls[key]()
    print(json.dumps(dict(steps=a.steps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--json")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--child", choices=["time", "trace"])
    a = ap.parse_args()
    if a.child:
        return (child_time if a.child == "time" else child_trace)(a)
    common = ["--snps", str(a.snps)]
    run = lambda args, limit, prefix=(): susie_probe._child(args, limit, prefix=prefix, script=__file__)
    out = dict(time=run(["--child", "time", "--steps", str(a.steps), "--warmup", str(a.warmup)] + common, 400))
    print(json.dumps(out["time"]), flush=True)
    if not a.skip_trace and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="clump_probe_")
        try:
            # a kernel trace on its own: no counters, no other tracing beside it; 3 calls of each form
            tr = run(["--child", "trace", "--steps", "3"] + common, 300, prefix=["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"])
            rows = []
            for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                with open(f) as fh:
                    rows += list(csv.DictReader(fh))
            hits = sorted((r for r in rows if re.search(r"\bclump_kernel\b", r.get("Kernel_Name", ""))), key=lambda r: int(r["Start_Timestamp"]))
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in hits]
            n = tr["steps"]
            if len(us) != 3 * n:
                raise SystemExit(f"clump_probe: the trace holds {len(us)} launches of clump_kernel for {3 * n} calls")
            out["trace"] = {key: dict(median_us=round(float(np.median(us[k * n:(k + 1) * n])), 1), max_us=round(max(us[k * n:(k + 1) * n]), 1))
                            for k, key in enumerate(("defaults", "worst", "worst8192"))}
        finally:
            shutil.rmtree(d, ignore_errors=True)
        print(json.dumps(out["trace"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
