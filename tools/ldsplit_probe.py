"""Times LD splitting (k_ldsplit.hip, gauss_ld_split_rows) where it matters.

  (a) the SNPs of chr22's largest window (tools/slct_probe.py's store: measured and unmeasured rows together, about 3 700) as one
      region, the defaults (thr_r2 0.02, blocks of 50 .. 1 000 SNPs, max_K 128, max_r2 0.3): the whole call;
  (b) the same region as gauss_ld_rows with the matrix back, and tests/ldsplit_ref.py's replay() on it on the host, once: what a caller
      who splits in Python pays;
  (c) the stated worst case of a call: the first 8 192 SNPs of the chromosome, max_size 4 096, max_K 128 (min_size 1, max_r2 1);
  (d) every timed form is run twice, interleaved with the others: the spread between identical runs is the margin of any comparison;
  (e) from a `rocprofv3 --kernel-trace` run of its own: the times of ldsplit_band_kernel, ldsplit_cost_kernel and the sum over
      ldsplit_dp_kernel's launches in (a) and (c), the band kernel's share of HBM bandwidth and the DP's candidates per second.

Whole calls are timed by the host clock around the blocking call (the call is what a caller pays; its kernels run on the library's own
stream); the kernels' own times come from the trace, not from events placed in the library.

Every GPU step is a child process under its own time limit; this process never opens the GPU.  A child that fails ends the probe.

    python tools/ldsplit_probe.py [--steps 10] [--warmup 2] [--json out.json] [--skip-trace] [--skip-host]
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

FORMS = ("defaults", "matrix", "worst8192")
KERNELS = ("ldsplit_band_kernel", "ldsplit_cost_kernel", "ldsplit_dp_kernel")
DEFAULTS = dict(thr_r2=0.02, min_size=50, max_size=1000, max_K=128, max_r2=0.3)
WORST = dict(thr_r2=0.02, min_size=1, max_size=4096, max_K=128, max_r2=1.0)
HBM_BYTES_PER_S = 8.0e12        # MI355X's stated HBM3E bandwidth: the yardstick of the band kernel's share


def _calls(a):
    """{form: a function that makes the call once and returns a figure that says what it did}"""
    import slct_probe
    from gauss_amd import hotpath, workload
    _hp, ctx, jobs, keep = slct_probe._jobs(a.snps, 29.716785)
    big = jobs["largest"]["plain"][0]
    ch = workload.make_chromosome(a.snps, "distmix")       # (the chromosome slct_probe's store was made from: the same seed)
    rows = np.sort(np.concatenate([big["packed"]["rows_m"], big["packed"]["rows_u"]])).astype(np.int32)
    store = (big["dev"][0], big["dev"][4])
    common = dict(pop_wgt=ch["w"], mode=hotpath.MODE_WEIGHTED, ctx=ctx)

    def split(r, **kw):
        return hotpath.ld_split_rows(store, r, ch["off"], ch["bp"][r].astype(np.int32), **common, **kw)

    def matrix():
        return hotpath.ld_matrix_rows(store, rows, ch["off"], ch["w"], hotpath.MODE_WEIGHTED, 1.0, ctx=ctx)

    first = np.arange(min(8192, len(ch["bp"])), dtype=np.int32)
    calls = dict(defaults=lambda: int(np.isfinite(split(rows, **DEFAULTS)["cost"]).sum()), matrix=lambda: int(matrix().shape[0]),
                 worst8192=lambda: int(np.isfinite(split(first, **WORST)["cost"]).sum()))
    return calls, dict(M=int(len(rows)), M_first=int(len(first)), N=int(ch["off"][-1])), keep, (matrix, ch["bp"][rows].astype(np.int32))


def child_time(a):
    calls, info, _keep, (matrix, bp) = _calls(a)
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
    out = dict(info, call_ms=rounds, feasible_K={k: what[k] for k in FORMS if k != "matrix"}, matrix_MB=round(info["M"] ** 2 * 8 / 1e6, 1),
               spread_ms=round(max(abs(v[0] - v[1]) for v in rounds.values()), 3))
    if not a.skip_host:                                      # the host's side of (b), once: numpy, one thread
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import ldsplit_ref
        R = matrix()
        t0 = time.perf_counter()
        ref = ldsplit_ref.replay(R, bp, 1 << 32, **DEFAULTS)
        out["host_replay_s"] = round(time.perf_counter() - t0, 2)
        out["host_replay_feasible_K"] = int(np.isfinite(ref["cost"]).sum())
    print(json.dumps(out), flush=True)


def child_trace(a):
    calls, _info, _keep, _ = _calls(a)
    for key in ("defaults", "worst8192"):                    # in this order: the trace's launches are read in it
        for _ in range(a.steps):
            calls[key]()
    print(json.dumps(dict(steps=a.steps)), flush=True)


def _kernel_times(rows, n, info):
    """per form and kernel the median over the n calls of the kernel's time in a call (the DP: summed over its max_K launches)"""
    out = {}
    forms = (("defaults", info["M"], DEFAULTS), ("worst8192", info["M_first"], WORST))
    for name in KERNELS:
        hits = sorted((r for r in rows if re.search(r"\b%s\b" % name, r.get("Kernel_Name", ""))), key=lambda r: int(r["Start_Timestamp"]))
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in hits]
        per_call = [p["max_K"] if name == "ldsplit_dp_kernel" else 1 for _, _, p in forms]
        if len(us) != n * sum(per_call):
            raise SystemExit(f"ldsplit_probe: the trace holds {len(us)} launches of {name} for {n} calls of each form")
        at = 0
        for (form, _M, _p), k in zip(forms, per_call):
            calls = [sum(us[at + c * k: at + (c + 1) * k]) for c in range(n)]
            at += n * k
            out.setdefault(form, {})[name + "_us"] = round(float(np.median(calls)), 1)
    for form, M, p in forms:
        W = min(p["max_size"], M)
        band_bytes = 8.0 * (M * (W - 1) - (W - 1) * W / 2) + 16.0 * W * M          # the band read once, Sd and SMd written
        sizes = sum(max(0, min(W, b) - p["min_size"] + 1) for b in range(1, M + 1))
        o = out[form]
        o["band_share_of_hbm"] = round(band_bytes / (o["ldsplit_band_kernel_us"] * 1e-6) / HBM_BYTES_PER_S, 4)
        o["dp_candidates_per_s"] = float("%.3g" % (p["max_K"] * sizes / (o["ldsplit_dp_kernel_us"] * 1e-6)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--json")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--child", choices=["time", "trace"])
    a = ap.parse_args()
    if a.child:
        return (child_time if a.child == "time" else child_trace)(a)
    common = ["--snps", str(a.snps)]
    run = lambda args, limit, prefix=(): susie_probe._child(args, limit, prefix=prefix, script=__file__)
    out = dict(time=run(["--child", "time", "--steps", str(a.steps), "--warmup", str(a.warmup)] + common + (["--skip-host"] if a.skip_host else []), 500))
    print(json.dumps(out["time"]), flush=True)
    if not a.skip_trace and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="ldsplit_probe_")
        try:
            # a kernel trace on its own: no counters, no other tracing beside it; 3 calls of each form
            tr = run(["--child", "trace", "--steps", "3"] + common, 300, prefix=["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"])
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
