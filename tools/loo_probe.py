"""Times the leave-one-out step (k_loo.hip) on the chr22 study's jobs: what it adds to a step, and the kernel alone.

  (a) step time of the 36-window chr22 job (distmix, resident 2-bit store, the headline's job) and of its largest window alone
      (M = 1 213), each with and without leave-one-out, the two forms alternating on the same build and the same box, two
      rounds each: the spread between two identical runs is the margin of the comparison;
  (b) from a `rocprofv3 --kernel-trace --stats` run of its own: loo_kernel's time per launch in both jobs, and the bytes / s it
      reaches on the lower block triangle of X it reads (sum over panels of (M - 64 p) rows x 512 bytes, plus y).

Every GPU step is a child process under its own time limit; this process never opens the GPU.  A child that fails ends the probe.

    python tools/loo_probe.py [--steps 30] [--warmup 5] [--snps 100000] [--json out.json] [--skip-trace]
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


def _jobs(snps):
    """(hotpath, ctx, {name: (plain windows, asking windows)}, keep-alive) of the chr22 study on a synthetic resident store."""
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
    ask = lambda ds: [dict(d, loo=True) for d in ds]
    return hotpath, ctx, dict(chr22=(descs, ask(descs)), largest=([descs[big]], ask([descs[big]]))), store


def _x_bytes(ms):
    """bytes loo_kernel reads for windows of `ms` measured SNPs: column panel p walks rows 64 p .. M - 1 of X (512 bytes a row) and of y"""
    return int(sum(sum((m - 64 * p) * (512 + 8) for p in range((m + 63) // 64)) for m in ms))


def child_time(a):
    hotpath, ctx, jobs, _keep = _jobs(a.snps)
    out = {}
    for name, (plain, asking) in jobs.items():
        ms = [d["dev"][2] for d in plain]
        pair = [hotpath.Job(plain, ctx=ctx, on_device=True), hotpath.Job(asking, ctx=ctx, on_device=True)]
        rounds = {"plain": [], "loo": []}
        for _ in range(2):                                   # plain, loo, plain, loo: two identical runs of each form
            for key, job in zip(("plain", "loo"), pair):
                for _ in range(a.warmup):
                    job.run()
                    job.fetch()
                ts = []
                for _ in range(a.steps):
                    t0 = time.perf_counter()
                    job.run()
                    job.fetch()
                    ts.append(time.perf_counter() - t0)
                rounds[key].append(round(float(np.median(ts)) * 1e3, 4))
        for job in pair:
            job.close()
        out[name] = dict(windows=len(plain), M_max=max(ms), x_bytes=_x_bytes(ms), step_ms_plain=rounds["plain"], step_ms_loo=rounds["loo"],
                         spread_ms=round(max(abs(rounds[k][0] - rounds[k][1]) for k in rounds), 4),
                         added_ms=round(min(rounds["loo"]) - min(rounds["plain"]), 4))
    print(json.dumps(out), flush=True)


def child_trace(a):
    hotpath, ctx, jobs, _keep = _jobs(a.snps)
    out = {}
    for name, (plain, asking) in jobs.items():
        job = hotpath.Job(asking, ctx=ctx, on_device=True)
        for _ in range(a.steps):
            job.run()
            job.fetch()
        job.close()
        ms = [d["dev"][2] for d in plain]
        out[name] = dict(x_bytes=_x_bytes(ms), steps=a.steps, grid=256 * sum((m + 63) // 64 for m in ms))      # loo_kernel's work-items
    print(json.dumps(out), flush=True)


def _child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    # a session of its own: under the profiler the process that holds the GPU is a grandchild, and the time limit ends the whole group
    pr = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, start_new_session=True)
    try:
        so, se = pr.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(pr.pid, signal.SIGKILL)
        pr.communicate()
        raise SystemExit(f"loo_probe: child {args[0]} passed its time limit of {limit} s; nothing more is run")
    if pr.returncode != 0:
        sys.stderr.write(se.decode()[-2000:])
        raise SystemExit(f"loo_probe: child {args[0]} ended with status {pr.returncode}; nothing more is run")
    lines = [l for l in so.decode().splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--json")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--child", choices=["time", "trace"])
    a = ap.parse_args()
    if a.child:
        return (child_time if a.child == "time" else child_trace)(a)
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--snps", str(a.snps)]
    out = dict(time=_child(["--child", "time"] + common, 420))
    print(json.dumps(out["time"]), flush=True)
    if not a.skip_trace and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="loo_probe_")
        try:
            # a kernel trace on its own: no counters, no other tracing beside it; each job runs 5 steps
            tr = _child(["--child", "trace", "--steps", "5", "--snps", str(a.snps)], 420,
                        prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"])
            traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            rows = []
            for f in traces:
                rows += [r for r in csv.DictReader(open(f)) if "loo_kernel" in r.get("Kernel_Name", "")]
            by_grid = {}
            for r in rows:
                dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                by_grid.setdefault(int(r.get("Grid_Size") or r.get("Grid_Size_X") or 0), []).append(dur)
            res = {}
            for name, info in tr.items():
                us = by_grid.get(info["grid"])               # a job's launches by their exact grid: (panels of X of its windows) x 256
                if us:
                    med = float(np.median(us))
                    res[name] = dict(launches=len(us), kernel_us_median=round(med, 2), kernel_us_min=round(min(us), 2),
                                     x_bytes=info["x_bytes"], gb_per_s=round(info["x_bytes"] / med / 1e3, 1))
            out["trace"] = res
            out["trace_grids_seen"] = {str(g): len(v) for g, v in sorted(by_grid.items())}
            print(json.dumps(res), flush=True)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
