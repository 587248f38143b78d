"""Times the LD scores (k_ldscore.hip) where they matter.

  (a) the 32-window batched computeLD job of bench.py's other_configs (gauss_amd/benchmodes.py: run_computeld -- the chr10 104-107 Mb
      window of tests/golden/PGC2_3Mb.txt on a 33KG-shaped resident 2-bit store, 32 copies, measured rows not shared), every window
      asking for its LD scores (radius 1 Mb) and for no matrix;
  (b) the same job as it is today: no scores, the matrices exported;
  (c) chr22's largest window (tools/slct_probe.py's jobs) as an LD window: with scores and no matrices against the window as it is
      today, its matrices exported; the kernels' own time is (e)'s;
  (d) every form is run twice, interleaved with the others: the spread between identical runs is the margin of any comparison;
  (e) from a `rocprofv3 --kernel-trace` run of its own: the times of ldscore_kernel and ldscore_finish_kernel in (c)'s job.

Every GPU step is a child process under its own time limit; this process never opens the GPU.  A child that fails ends the probe.

    python tools/ldscore_probe.py [--steps 20] [--warmup 3] [--radius 1000000] [--json out.json] [--skip-trace]
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import susie_probe      # noqa: E402  (its timing loop, its child runner)


def _batch(a):
    """(hotpath, ctx, the computeLD window's descriptor maker, keep-alive): run_computeld's window on a store made on the device"""
    import ctypes as C

    import torch

    from gauss_amd import _lib, hotpath, workload
    ctx = hotpath.default_context()
    study = os.path.join(ROOT, "tests", "golden", "PGC2_3Mb.txt")
    ch = workload.make_chromosome(100_000, "distmix", seed=20260214, study=study)
    keep = np.nonzero(ch["measured"])[0]                    # only the study's SNPs matter for computeLD
    bp = ch["bp"][keep]
    thr = np.ascontiguousarray(ch["thr"][keep])
    rho = np.ones(len(keep), dtype=np.float32)
    rho[1:] = np.exp(-np.diff(bp) / 50e3)
    N, S = int(ch["off"][-1]), len(keep)
    ld = (N + 63) // 64 * 64
    ip = C.POINTER(C.c_int32)
    raw = torch.empty((S, ld), dtype=torch.uint8, device="cuda")
    _lib.check(ctx.lib.gauss_synth_device(ctx.handle, raw.data_ptr(), S, ld, ch["off"].ctypes.data_as(ip), len(ch["pops"]),
                                          thr.ctypes.data_as(C.POINTER(C.c_float)), rho.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(20260214)))
    ld2 = int(sum((int(m) + 63) // 64 * 16 for m in np.diff(ch["off"])))
    store = torch.empty((S, ld2), dtype=torch.uint8, device="cuda")
    _lib.check(ctx.lib.gauss_pack2bit_device(ctx.handle, raw.data_ptr(), ld, store.data_ptr(), ld2, S, ch["off"].ctypes.data_as(ip), len(ch["pops"])))
    del raw
    torch.cuda.synchronize()
    rows = np.nonzero((bp >= 104_000_001) & (bp <= 107_000_000))[0].astype(np.int32)
    M = len(rows)

    def desc(scores):
        d = dict(mode=hotpath.MODE_WEIGHTED, pop_off=ch["off"], pop_wgt=ch["w"], z1=np.zeros(M), lam=0.0,
                 dev=(store.data_ptr(), store.data_ptr(), M, 0, ld2), packed=dict(fmt=1, rows_m=rows, rows_u=np.zeros(0, np.int32)))
        if scores:
            return dict(d, ldscore=dict(radius=a.radius, bp_m=bp[rows], bp_u=None, n=float(N)), want_matrices=False)
        return dict(d, ld_codings=_lib.CODE_ADDITIVE)
    return hotpath, ctx, desc, M, N, store


def child_time(a):
    hotpath, ctx, desc, M, N, _keep = _batch(a)
    B = 32
    os.environ["GAUSS_SHARE_MEASURED"] = "0"                 # 32 different computeLD() windows share nothing (run_computeld)
    made = dict(scores=hotpath.Job([desc(True) for _ in range(B)], ctx=ctx, on_device=True),
                matrices=hotpath.Job([desc(False) for _ in range(B)], ctx=ctx, on_device=True))
    os.environ.pop("GAUSS_SHARE_MEASURED", None)
    rounds = {k: [] for k in made}
    for _ in range(2):                                       # every form twice, interleaved: two identical runs of each
        for key, job in made.items():
            ms, res = susie_probe._median_ms(job, a.steps, a.warmup)
            rounds[key].append(ms)
            if key == "scores":
                l2 = res[0]["lds_raw"][0]
                assert res[0]["b11"] is None and np.all(np.isfinite(l2)) and all(np.array_equal(r["lds_raw"], res[0]["lds_raw"]) for r in res)
    for job in made.values():
        job.close()
    best = {k: min(v) for k, v in rounds.items()}
    out = dict(batch=dict(windows=B, M=M, N=N, radius=a.radius, step_ms=rounds, export_MB=round(B * M * M * 8 / 1e6, 1),
                          saved_ms=round(best["matrices"] - best["scores"], 3), mean_l2_raw=round(float(l2.mean()), 3)))
    # chr22's largest window as an LD window
    import slct_probe
    from gauss_amd import workload
    _hp, _ctx, jobs, _keep2 = slct_probe._jobs(a.snps, 29.716785)
    big = jobs["largest"]["plain"][0]
    bp = workload.make_chromosome(a.snps, "distmix")["bp"]   # (the positions slct_probe's store was made from: the same seed)
    mi, ui = big["packed"]["rows_m"], big["packed"]["rows_u"]
    ld_win = dict(big, z1=np.zeros(len(mi)), lam=0.0)
    lds = dict(radius=a.radius, bp_m=bp[mi], bp_u=bp[ui], n=float(big["pop_off"][-1]))
    forms = dict(matrices=[dict(ld_win, ld_codings=1)], scores=[dict(ld_win, ldscore=lds, want_matrices=False)])
    made = {k: hotpath.Job(v, ctx=ctx, on_device=True) for k, v in forms.items()}
    rounds = {k: [] for k in made}
    for _ in range(2):
        for key, job in made.items():
            ms, res = susie_probe._median_ms(job, a.steps, a.warmup)
            rounds[key].append(ms)
            if key == "scores":
                band = res[0]["lds_mass"][0]
    for job in made.values():
        job.close()
    best = {k: min(v) for k, v in rounds.items()}
    out["largest"] = dict(M=len(mi), U=len(ui), step_ms=rounds, saved_ms=round(best["matrices"] - best["scores"], 3),
                          rows_in_band=[int(band.min()), int(band.max())])
    out["spread_ms"] = round(max(abs(v[0] - v[1]) for blk in (out["batch"], out["largest"]) for v in blk["step_ms"].values()), 4)
    print(json.dumps(out), flush=True)


def child_trace(a):
    import slct_probe
    from gauss_amd import workload
    hotpath, ctx, jobs, _keep = slct_probe._jobs(a.snps, 29.716785)
    big = jobs["largest"]["plain"][0]
    bp = workload.make_chromosome(a.snps, "distmix")["bp"]
    mi, ui = big["packed"]["rows_m"], big["packed"]["rows_u"]
    job = hotpath.Job([dict(big, z1=np.zeros(len(mi)), lam=0.0, want_matrices=False,
                            ldscore=dict(radius=a.radius, bp_m=bp[mi], bp_u=bp[ui], n=float(big["pop_off"][-1])))], ctx=ctx, on_device=True)
    for _ in range(a.steps):
        job.run()
        job.fetch()
    job.close()
    print(json.dumps(dict(steps=a.steps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--radius", type=int, default=1_000_000)
    ap.add_argument("--json")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--child", choices=["time", "trace"])
    a = ap.parse_args()
    if a.child:
        return (child_time if a.child == "time" else child_trace)(a)
    common = ["--snps", str(a.snps), "--radius", str(a.radius)]
    run = lambda args, limit, prefix=(): susie_probe._child(args, limit, prefix=prefix, script=__file__)
    out = dict(time=run(["--child", "time", "--steps", str(a.steps), "--warmup", str(a.warmup)] + common, 400))
    print(json.dumps(out["time"]), flush=True)
    if not a.skip_trace and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="ldscore_probe_")
        try:
            # a kernel trace on its own: no counters, no other tracing beside it; one job a process, 3 steps
            tr = run(["--child", "trace", "--steps", "3"] + common, 300, prefix=["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"])
            rows = []
            for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                with open(f) as fh:
                    rows += list(csv.DictReader(fh))
            out["trace"] = {}
            for name in ("ldscore_kernel", "ldscore_finish_kernel"):
                us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if re.search(r"\b" + name + r"\b", r.get("Kernel_Name", ""))]
                if len(us) < tr["steps"]:
                    raise SystemExit(f"ldscore_probe: the trace holds {len(us)} launches of {name} for {tr['steps']} steps")
                out["trace"][name] = dict(launches_per_step=round(len(us) / tr["steps"], 1), median_us=round(float(np.median(us)), 1), max_us=round(max(us), 1))
        finally:
            shutil.rmtree(d, ignore_errors=True)
        print(json.dumps(out["trace"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
