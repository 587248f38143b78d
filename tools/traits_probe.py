"""Times further traits on one LD build (k_traits.hip) on the 36-window chr22 job of workload.make_chromosome().

  (a) step time of the job (distmix, resident 2-bit store, the headline's job) with 0, 7 and 63 further traits in every window, the
      forms alternating on the same build and the same box, two rounds each: the spread between two identical runs is the margin
      of the comparison.  The bytes of results a fetch brings back are recorded beside each;
  (b) from a `rocprofv3 --kernel-trace --stats` run of its own: the time of traits_weights_kernel (two launches a step) and
      traits_impute_kernel per step, at 7 and at 63 traits.

`--miss K` adds a masked form of the largest T (key "<T>m"): every further trait lacks K random SNPs of every window, drawn from a pool
of 128 of the window's measured SNPs (the limit on distinct missing SNPs, include/gauss_hip.h miss_more); its five further launches
(k_traits_miss.hip) are timed in (b) beside the three of k_traits.hip.

`--traits 0` runs the plain job alone and touches nothing this feature added: the same file times the parent commit's library
(the yardstick of DESIGN.md section 4, measured in the same session).

GAUSS_PROBE_ROOT names the checkout whose gauss_amd package is timed (default: the one this file lies in).

Every GPU step is a child process under its own time limit; this process never opens the GPU.  A child that fails ends the probe.

    python tools/traits_probe.py [--steps 30] [--warmup 5] [--snps 100000] [--traits 0,7,63] [--miss 8] [--json out.json] [--skip-trace]
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

ROOT = os.environ.get("GAUSS_PROBE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _forms(ts, miss):
    """[(key, T, K)]: every T plain, and with --miss K the largest T once more with a mask"""
    forms = [(str(T), T, 0) for T in ts]
    if miss and any(ts):
        forms.append((f"{max(ts)}m", max(ts), miss))
    return forms


def _mask(rng, T, M, K):
    pool = rng.choice(M, size=min(128, M), replace=False)
    mask = np.zeros((T, M), dtype=np.uint8)
    for t in range(T):
        mask[t, rng.choice(pool, size=K, replace=False)] = 1
    return mask


def _jobs(snps, forms):
    """(hotpath, ctx, {key: windows}, keep-alive) of the chr22 study on a synthetic resident store."""
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
    rng = np.random.default_rng(7)
    def ask(T, K):
        if not T:
            return descs
        more = lambda d: dict(miss_more=_mask(rng, T, d["dev"][2], K)) if K else {}
        return [dict(d, z_more=rng.standard_normal((T, d["dev"][2])) * 2.0, **more(d)) for d in descs]
    return hotpath, ctx, {key: ask(T, K) for key, T, K in forms}, store


def _shape(ws, T, K=0):
    ms, us = [d["dev"][2] for d in ws], [d["dev"][3] for d in ws]
    return dict(windows=len(ws), M_max=max(ms), U_sum=sum(us), result_bytes=8 * sum((2 + T + (T if K else 0)) * u + 2 * T * K for u in us),
                flop=sum(2 * m * m * T + 2 * u * m * T for m, u in zip(ms, us)))


def child_time(a):
    hotpath, ctx, jobs, _keep = _jobs(a.snps, a.forms)
    made = {T: hotpath.Job(ws, ctx=ctx, on_device=True) for T, ws in jobs.items()}
    rounds = {T: [] for T in jobs}
    for _ in range(2):                                       # 0, 7, 63, 0, 7, 63: two identical runs of each form
        for T, job in made.items():
            for _ in range(a.warmup):
                job.run()
                job.fetch()
            ts = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                job.run()
                job.fetch()
                ts.append(time.perf_counter() - t0)
            rounds[T].append(round(float(np.median(ts)) * 1e3, 4))
    for job in made.values():
        job.close()
    out = {}
    for key, T, K in a.forms:
        out[key] = dict(_shape(jobs[key], T, K), step_ms=rounds[key], spread_ms=round(abs(rounds[key][0] - rounds[key][1]), 4))
    print(json.dumps(out), flush=True)


def child_trace(a):
    hotpath, ctx, jobs, _keep = _jobs(a.snps, a.forms)
    out = {}
    for key, T, K in a.forms:
        if not T:
            continue
        job = hotpath.Job(jobs[key], ctx=ctx, on_device=True)
        for _ in range(a.steps):
            job.run()
            job.fetch()
        job.close()
        out[key] = dict(steps=a.steps)
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
        raise SystemExit(f"traits_probe: child {args[0]} passed its time limit of {limit} s; nothing more is run")
    if pr.returncode != 0:
        sys.stderr.write(se.decode()[-2000:])
        raise SystemExit(f"traits_probe: child {args[0]} ended with status {pr.returncode}; nothing more is run")
    lines = [l for l in so.decode().splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--traits", default="0,7,63")
    ap.add_argument("--miss", type=int, default=0, help="SNPs every further trait lacks in every window, in a masked form of the largest T")
    ap.add_argument("--json")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--child", choices=["time", "trace"])
    a = ap.parse_args()
    a.ts = [int(t) for t in a.traits.split(",")]
    a.forms = _forms(a.ts, a.miss)
    if a.child:
        return (child_time if a.child == "time" else child_trace)(a)
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--snps", str(a.snps), "--traits", a.traits, "--miss", str(a.miss)]
    out = dict(time=_child(["--child", "time"] + common, 420))
    print(json.dumps(out["time"]), flush=True)
    if not a.skip_trace and any(a.ts) and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="traits_probe_")
        try:
            # a kernel trace on its own: no counters, no other tracing beside it; each job runs 5 steps, in the order of --traits
            tr = _child(["--child", "trace", "--steps", "5", "--snps", str(a.snps), "--traits", a.traits, "--miss", str(a.miss)], 420,
                        prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"])
            rows = []
            for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                rows += [r for r in csv.DictReader(open(f)) if "traits_" in r.get("Kernel_Name", "")]
            rows.sort(key=lambda r: int(r["Start_Timestamp"]))
            res, at = {}, 0
            for key, T, K in [f for f in a.forms if f[1]]:   # per step: two launches of the weights kernel, one of the product;
                n = (8 if K else 3) * tr[key]["steps"]        # with a mask five more (columns x 2, solve, product, apply)
                mine, at = rows[at:at + n], at + n
                us = lambda key: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine if key in r["Kernel_Name"]]
                w, p, m = us("traits_weights_kernel"), us("traits_impute_kernel"), us("traits_miss_")
                if len(w) == 2 * len(p) and p:
                    res[key] = dict(launches=len(mine), weights_us_per_step=round(sum(w) / len(p), 2),      # both passes
                                    impute_us_per_step=round(sum(p) / len(p), 2))
                    if K:
                        res[key]["miss_us_per_step"] = round(sum(m) / len(p), 2)
                        for name in ("cols", "solve", "product", "apply"):
                            res[key][f"miss_{name}_us_per_step"] = round(sum(us(f"traits_miss_{name}_kernel")) / len(p), 2)
            out["trace"] = res
            print(json.dumps(res), flush=True)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
