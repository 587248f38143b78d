"""Times the signal selection (k_slct.hip), the imputed SNPs conditioned on it (k_cond.hip) and the credible sets of the selected
signals (k_cs.hip) on the chr22 study's jobs.

  (a) step time of the 36-window chr22 job (distmix, resident 2-bit store, the headline's job) and of its largest window alone
      (M = 1 213, U = 2 512), in four forms: plain, every window selecting (32 steps at the genome-wide threshold, and with
      `--stop 0` all 32 taken, so that all 32 sets are built), every window selecting and conditioning its imputed SNPs, and every
      window asking for credible sets on top.  The forms alternate on the same build and the same box, two rounds each: the spread
      between two identical runs is the margin of the comparison;
  (b) from a `rocprofv3 --kernel-trace --stats` run of its own for each job: the time of slct_kernel, of cond_kernel and of the
      three cs kernels per step, grouped by kernel name (one launch each a step; a clamped window's re-launches inside the fetch
      are counted with their step).

Every GPU step is a child process under its own time limit; this process never opens the GPU.  A child that fails ends the probe.

    python tools/slct_probe.py [--steps 30] [--warmup 5] [--snps 100000] [--stop 29.716785] [--json out.json] [--skip-trace]
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
FORMS = ("plain", "slct", "cond", "cs")


def _jobs(snps, stop):
    """(hotpath, ctx, {name: {form: windows}}, keep-alive) of the chr22 study on a synthetic resident store."""
    import ctypes as C

    import torch

    from gauss_amd import _lib, hotpath, workload
    ctx = hotpath.default_context()
    ch = workload.make_chromosome(snps, "distmix")
    N, S = int(ch["off"][-1]), len(ch["bp"])
    ld = (N + 63) // 64 * 64
    ip = C.POINTER(C.c_int32)
    raw = torch.empty((S, ld), dtype=torch.uint8, device="cuda")
    _lib.check(ctx.lib.gauss_synth_device(ctx.handle, raw.data_ptr(), S, ld, ch["off"].ctypes.data_as(ip), len(ch["pops"]),
                                          np.ascontiguousarray(ch["thr"]).ctypes.data_as(C.POINTER(C.c_float)),
                                          ch["rho"].ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(20260216)))
    ld2 = int(sum((int(m) + 63) // 64 * 16 for m in np.diff(ch["off"])))
    store = torch.empty((S, ld2), dtype=torch.uint8, device="cuda")
    _lib.check(ctx.lib.gauss_pack2bit_device(ctx.handle, raw.data_ptr(), ld, store.data_ptr(), ld2, S, ch["off"].ctypes.data_as(ip),
                                             len(ch["pops"])))
    del raw
    torch.cuda.synchronize()
    wins = workload.windows_of(ch)
    descs = [dict(mode=hotpath.MODE_WEIGHTED, pop_off=ch["off"], pop_wgt=ch["w"], z1=ch["z"][mi],
                  dev=(store.data_ptr(), store.data_ptr(), len(mi), len(ui), ld2),
                  packed=dict(fmt=1, rows_m=mi.astype(np.int32), rows_u=ui.astype(np.int32))) for _, mi, ui in wins]
    big = max(range(len(descs)), key=lambda k: descs[k]["dev"][2])
    slct = dict(max=32, chi2_stop=stop)
    forms = lambda ds: dict(plain=ds, slct=[dict(d, slct=slct) for d in ds], cond=[dict(d, slct=dict(slct, unmeasured=True)) for d in ds],
                            cs=[dict(d, slct=dict(slct, unmeasured=True, cs=dict(coverage=0.95, prior_var=25.0))) for d in ds])
    return hotpath, ctx, dict(chr22=forms(descs), largest=forms([descs[big]])), store


def child_time(a):
    hotpath, ctx, jobs, _keep = _jobs(a.snps, a.stop)
    out = {}
    for name, forms in jobs.items():
        made = {k: hotpath.Job(forms[k], ctx=ctx, on_device=True) for k in FORMS}
        rounds = {k: [] for k in FORMS}
        n_sel = []
        set_sizes = []
        for _ in range(2):                                   # plain, slct, cond, cs, plain, slct, cond, cs: two identical runs of each form
            for key, job in made.items():
                for _ in range(a.warmup):
                    job.run()
                    res = job.fetch()
                ts = []
                for _ in range(a.steps):
                    t0 = time.perf_counter()
                    job.run()
                    res = job.fetch()
                    ts.append(time.perf_counter() - t0)
                rounds[key].append(round(float(np.median(ts)) * 1e3, 4))
                if key == "cond":
                    n_sel = [int(r["slct_n"]) for r in res]
                if key == "cs":
                    set_sizes = [int(r["cs_size"].sum()) for r in res]
        for job in made.values():
            job.close()
        ms, us = [d["dev"][2] for d in forms["plain"]], [d["dev"][3] for d in forms["plain"]]
        out[name] = dict(windows=len(ms), M_max=max(ms), U_max=max(us), U_sum=sum(us), selected=n_sel,
                         gathers=int(sum(u * n for u, n in zip(us, n_sel))),      # the uncoalesced 8-byte reads of B21 a step
                         step_ms={k: rounds[k] for k in FORMS},
                         spread_ms=round(max(abs(rounds[k][0] - rounds[k][1]) for k in FORMS), 4),
                         slct_added_ms=round(min(rounds["slct"]) - min(rounds["plain"]), 4),
                         cond_added_ms=round(min(rounds["cond"]) - min(rounds["slct"]), 4),
                         cs_added_ms=round(min(rounds["cs"]) - min(rounds["cond"]), 4), set_members=set_sizes)
    print(json.dumps(out), flush=True)


def child_trace(a):
    hotpath, ctx, jobs, _keep = _jobs(a.snps, a.stop)
    job = hotpath.Job(jobs[a.job]["cs"], ctx=ctx, on_device=True)       # one job a traced process: every kernel row is this job's
    for _ in range(a.steps):
        job.run()
        job.fetch()
    job.close()
    print(json.dumps(dict(job=a.job, steps=a.steps)), flush=True)


def trace_times(rows, steps):
    """Time of slct_kernel, cond_kernel and the cs kernels per step from the kernel-trace rows of ONE job's process, grouped by kernel name.  A step
    launches each kernel once; a clamped window launches them again inside the fetch, which belongs to the step and is counted in
    `launches`.  Fewer launches than steps means the trace is not the one expected: an error, not a missing figure."""
    res = {}
    for key in ("slct_kernel", "cond_kernel", "cs_lbf_kernel", "cs_set_kernel", "cs_fold_kernel"):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if key in r.get("Kernel_Name", "")]
        if len(us) < steps:
            raise SystemExit(f"slct_probe: the trace holds {len(us)} launches of {key} for {steps} steps")
        res[key] = dict(launches=len(us), us_per_step=round(sum(us) / steps, 2), us_min=round(min(us), 2), us_max=round(max(us), 2))
    return res


def _child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    # a session of its own: under the profiler the process that holds the GPU is a grandchild, and the time limit ends the whole group
    pr = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, start_new_session=True)
    try:
        so, se = pr.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(pr.pid, signal.SIGKILL)
        pr.communicate()
        raise SystemExit(f"slct_probe: child {args[0]} passed its time limit of {limit} s; nothing more is run")
    if pr.returncode != 0:
        sys.stderr.write(se.decode()[-2000:])
        raise SystemExit(f"slct_probe: child {args[0]} ended with status {pr.returncode}; nothing more is run")
    lines = [l for l in so.decode().splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--stop", type=float, default=29.716785, help="chi^2 at which the selection stops (0: all 32 steps are taken)")
    ap.add_argument("--json")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--child", choices=["time", "trace"])
    ap.add_argument("--job", choices=["chr22", "largest"], default="chr22", help="--child trace: the job to run")
    a = ap.parse_args()
    if a.child:
        return (child_time if a.child == "time" else child_trace)(a)
    common = ["--snps", str(a.snps), "--stop", str(a.stop)]
    out = dict(time=_child(["--child", "time", "--steps", str(a.steps), "--warmup", str(a.warmup)] + common, 420))
    print(json.dumps(out["time"]), flush=True)
    if not a.skip_trace and shutil.which("rocprofv3"):
        res = {}
        for name in ("chr22", "largest"):
            d = tempfile.mkdtemp(prefix="slct_probe_")
            try:
                # a kernel trace on its own: no counters, no other tracing beside it; one job a process, 5 steps
                tr = _child(["--child", "trace", "--job", name, "--steps", "5"] + common, 420,
                            prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"])
                rows = []
                for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                    with open(f) as fh:
                        rows += list(csv.DictReader(fh))
                res[name] = trace_times(rows, tr["steps"])
            finally:
                shutil.rmtree(d, ignore_errors=True)
        out["trace"] = res
        print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
