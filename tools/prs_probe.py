"""Times the polygenic score weights (k_prs.hip) on the chr22 study's jobs (tools/slct_probe.py's jobs: distmix, resident 2-bit store;
the largest window with tools/susie_probe.py's three planted signals).

  (a) the largest window alone (M = 1 213): plain, and with the default grid (4 chains x 20 penalties) as a workgroup per chain and,
      under GAUSS_PRS_T=64, as a wave per chain: the added step time is the kernel's time, since it is the last launch of the tail;
      sweeps per chain and the largest nnz from the result; with --split the coordinate steps and the row updates of every chain
      from tests/prs_ref.py:fit_cov on the exported B11 (some ten seconds of numpy);
  (b) the 36-window chr22 job: plain, and with every window asking (144 chains);
  (c) every form is run twice, interleaved with the others: the spread between identical runs is the margin of any comparison;
  (d) from a `rocprofv3 --kernel-trace` run of its own: the time of prs_kernel in the largest window's job.

Every GPU step is a child process under its own time limit; this process never opens the GPU.  A child that fails ends the probe.

    python tools/prs_probe.py [--steps 20] [--prs-steps 3] [--warmup 2] [--n 5000] [--split] [--json out.json] [--skip-trace]
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
import susie_probe      # noqa: E402  (its planted window, its timing loop, its child runner)


def _chains(res):
    """Per window: sweeps per chain, the largest nnz, cells that ran their sweeps out"""
    return [dict(sweeps=[int(v) for v in r["prs_sweeps"].sum(axis=1)], nnz=int(r["prs_nnz"].max()), noconv=int(bool(r["status"] & 64)))
            for r in res]


def child_time(a):
    import slct_probe
    hotpath, ctx, jobs, _keep = slct_probe._jobs(a.snps, 29.716785)
    big = susie_probe._planted(jobs)
    chr22 = jobs["chr22"]["plain"]
    prs = dict(n=a.n)
    forms = dict(plain=[big], wg=[dict(big, prs=prs)], wave=[dict(big, prs=prs)], chr22=chr22, chr22_all=[dict(w, prs=prs) for w in chr22])
    made = {k: hotpath.Job(v, ctx=ctx, on_device=True, want_mats=a.split and k == "wg") for k, v in forms.items()}
    rounds = {k: [] for k in forms}
    info = {}
    for _ in range(2):                                       # every form twice, interleaved: two identical runs of each
        for key, job in made.items():
            asking = key in ("wg", "wave", "chr22_all")
            if key == "wave":
                os.environ["GAUSS_PRS_T"] = "64"             # read per launch
            try:
                ms, res = susie_probe._median_ms(job, a.prs_steps if asking else a.steps, 1 if asking else a.warmup)
            finally:
                os.environ.pop("GAUSS_PRS_T", None)
            rounds[key].append(ms)
            if asking:
                info[key] = _chains(res)
            if key == "wave":
                assert all(np.array_equal(res[0][k], keep[k]) for k in ("prs_beta", "prs_delta", "prs_br", "prs_bg", "prs_kkt")), "wave != workgroup"
            if key == "wg":
                keep = res[0]
    if a.split:
        import prs_ref
        want = prs_ref.fit_cov(keep["b11"], np.asarray(forms["wg"][0]["z1"]), a.n)
        info["split"] = dict(coord_steps=want["coord_steps"], row_updates=want["row_updates"], same_bits=bool(np.array_equal(want["beta"], keep["prs_beta"])))
    for job in made.values():
        job.close()
    best = {k: min(v) for k, v in rounds.items()}
    allw = info["chr22_all"]
    out = dict(M=big["dev"][2], step_ms=rounds, spread_ms=round(max(abs(v[0] - v[1]) for v in rounds.values()), 4),
               wg_added_ms=round(best["wg"] - best["plain"], 3), wave_added_ms=round(best["wave"] - best["plain"], 3),
               chr22_all_added_ms=round(best["chr22_all"] - best["chr22"], 3), largest=info["wg"][0], split=info.get("split"),
               chr22_chains=sum(len(w["sweeps"]) for w in allw), chr22_sweeps_per_chain=[min(min(w["sweeps"]) for w in allw), max(max(w["sweeps"]) for w in allw)],
               chr22_noconv_windows=sum(w["noconv"] for w in allw))
    print(json.dumps(out), flush=True)


def child_trace(a):
    import slct_probe
    hotpath, ctx, jobs, _keep = slct_probe._jobs(a.snps, 29.716785)
    job = hotpath.Job([dict(susie_probe._planted(jobs), prs=dict(n=a.n))], ctx=ctx, on_device=True)      # one job a traced process
    for _ in range(a.steps):
        job.run()
        job.fetch()
    job.close()
    print(json.dumps(dict(steps=a.steps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--prs-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--n", type=float, default=5000.0)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--child", choices=["time", "trace"])
    a = ap.parse_args()
    if a.child:
        return (child_time if a.child == "time" else child_trace)(a)
    common = ["--snps", str(a.snps), "--n", str(a.n)]
    run = lambda args, limit, prefix=(): susie_probe._child(args, limit, prefix=prefix, script=__file__)
    out = dict(time=run(["--child", "time", "--steps", str(a.steps), "--prs-steps", str(a.prs_steps), "--warmup", str(a.warmup)] + common +
                        (["--split"] if a.split else []), 500))
    print(json.dumps(out["time"]), flush=True)
    if not a.skip_trace and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="prs_probe_")
        try:
            # a kernel trace on its own: no counters, no other tracing beside it; one job a process, 2 steps
            tr = run(["--child", "trace", "--steps", "2"] + common, 300, prefix=["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"])
            rows = []
            for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                with open(f) as fh:
                    rows += list(csv.DictReader(fh))
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "prs_kernel" in r.get("Kernel_Name", "")]
            if len(us) < tr["steps"]:
                raise SystemExit(f"prs_probe: the trace holds {len(us)} launches of prs_kernel for {tr['steps']} steps")
            out["trace"] = dict(launches_per_step=round(len(us) / tr["steps"], 1), median_us=round(float(np.median(us)), 1), max_us=round(max(us), 1))
        finally:
            shutil.rmtree(d, ignore_errors=True)
        print(json.dumps(out["trace"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
