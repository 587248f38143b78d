"""Times the gene-based sum-of-chi2 test (k_sumchi2.hip, gauss_gene_sumchi2_rows) where it matters.

  (a) the benchmark's jepegmix configuration (bench.py --mode jepegmix: ~350 synthetic genes of 1 - 20 SNPs of the chr22 study on the
      resident packed panel, PGC2 weights): the call, pruning at 0.9, one trait;
  (b) the same genes as gauss_gene_ld_batch_rows (diag 1) with the blocks back plus numpy.linalg.eigvalsh per gene: what a caller pays
      today before the first p-value;
  (c) one synthetic call of 256 genes of 128 independent SNPs each (n = k = 128, 512 samples, host bytes): the solve at its limit;
  (d) every form is run twice, interleaved with the others: the spread between identical runs is the margin of any comparison;
  (e) from a `rocprofv3 --kernel-trace` run of its own: the times of sumchi2_kernel in (a) and (c).

Every GPU step is a child process under its own time limit; this process never opens the GPU.  A child that fails ends the probe.

    python tools/sumchi2_probe.py [--steps 10] [--warmup 2] [--json out.json] [--skip-trace]
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

FORMS = ("sumchi2", "blocks_eigvalsh", "synthetic")


def _calls(a):
    """{form: a function that makes the call once and returns a figure that says what it did}, facts, what must stay alive"""
    import bench
    from gauss_amd import _lib, api, benchmodes, hotpath, synth, workload
    args = bench.parse_args(["--no-cpu-baseline", "--snps", str(a.snps)])
    rig = bench.Rig(args)
    ctx = rig.ctx
    ch = workload.make_chromosome(args.snps, "distmix", seed=20260216, sample_scale=1.0)
    tmp = tempfile.mkdtemp(prefix="gauss_sumchi2_")
    files = benchmodes.write_study_files(rig, ch, tmp)
    annot, n_genes, _ = benchmodes.make_annotation(ch, files, tmp)
    wgt = (list(synth.PGC2_WEIGHTS.keys()), list(synth.PGC2_WEIGHTS.values()))
    pr = api.Prepared(api.KIND_JEPEGMIX, pop_wgt_df=wgt, input_file=files["gwas"], annotation_file=annot, reference_index_file="(packed)",
                      reference_data_file=files["panel"], reference_pop_desc_file=files["desc"])
    api.panel_resident(files["panel"], ctx=ctx)
    d = pr.window_rows(files["panel"], ctx)
    go = np.ascontiguousarray(pr.gene_off(), dtype=np.int32)
    po, w = np.ascontiguousarray(pr.pop_off(), np.int32), np.ascontiguousarray(pr.pop_wgt(), np.float64)
    rows = np.ascontiguousarray(d["rows_m"], dtype=np.int32)[:pr.M]
    store = (d["store"], d["ld"])
    rng = np.random.default_rng(7)
    z = rng.normal(size=pr.M)
    common = dict(pop_wgt=w, mode=hotpath.MODE_WEIGHTED, pop_src_off=d["pop_src_off"], ctx=ctx)

    def blocks():
        bl = hotpath.gene_ld_batch_rows(store, rows, po, go, diag=1.0, **common)
        return int(sum(len(np.linalg.eigvalsh(b)) for b in bl if len(b)))

    G = rng.integers(0, 3, size=(256 * 128, 512), dtype=np.uint8)
    G[:, 0], G[:, 1] = 0, 2
    go_s = np.arange(0, 256 * 128 + 1, 128, dtype=np.int32)
    z_s = rng.normal(size=len(G))
    calls = dict(sumchi2=lambda: int(hotpath.gene_sumchi2_rows(store, rows, po, go, z, prune_r2=0.9, **common)["n_kept"].sum()),
                 blocks_eigvalsh=blocks,
                 synthetic=lambda: int(hotpath.gene_sumchi2(G, [0, 512], go_s, z_s, None, hotpath.MODE_POOLED, 0.9, ctx=ctx)["sweeps"].max()))
    sizes = np.diff(go)
    return calls, dict(genes=int(len(sizes)), snps=int(pr.M), largest_gene=int(sizes.max()), N=int(po[-1])), (rig, pr, tmp)


def child_time(a):
    calls, info, keep = _calls(a)
    rounds, what = {k: [] for k in FORMS}, {}
    try:
        for _ in range(2):                                   # every form twice, interleaved: two identical runs of each
            for key in FORMS:
                for _ in range(a.warmup):
                    calls[key]()
                ts = []
                for _ in range(a.steps if key != "synthetic" else max(2, a.steps // 3)):
                    t0 = time.perf_counter()
                    what[key] = calls[key]()
                    ts.append(time.perf_counter() - t0)
                rounds[key].append(round(float(np.median(ts)) * 1e3, 3))
    finally:
        shutil.rmtree(keep[2], ignore_errors=True)
    out = dict(info, call_ms=rounds, figure=what, spread_ms=round(max(abs(v[0] - v[1]) for v in rounds.values()), 3))
    print(json.dumps(out), flush=True)


def child_trace(a):
    calls, _info, keep = _calls(a)
    try:
        for key in ("sumchi2", "synthetic"):                 # in this order: the trace's launches of sumchi2_kernel are read in it
            for _ in range(a.steps):
                calls[key]()
    finally:
        shutil.rmtree(keep[2], ignore_errors=True)
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
        d = tempfile.mkdtemp(prefix="sumchi2_probe_")
        try:
            # a kernel trace on its own: no counters, no other tracing beside it; 3 calls of each form
            tr = run(["--child", "trace", "--steps", "3"] + common, 300, prefix=["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"])
            rows = []
            for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                with open(f) as fh:
                    rows += list(csv.DictReader(fh))
            hits = sorted((r for r in rows if re.search(r"\bsumchi2_kernel\b", r.get("Kernel_Name", ""))), key=lambda r: int(r["Start_Timestamp"]))
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in hits]
            n = tr["steps"]
            if len(us) != 2 * n:
                raise SystemExit(f"sumchi2_probe: the trace holds {len(us)} launches of sumchi2_kernel for {2 * n} calls")
            out["trace"] = {key: dict(median_us=round(float(np.median(us[k * n:(k + 1) * n])), 1), max_us=round(max(us[k * n:(k + 1) * n]), 1))
                            for k, key in enumerate(("sumchi2", "synthetic"))}
        finally:
            shutil.rmtree(d, ignore_errors=True)
        print(json.dumps(out["trace"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
