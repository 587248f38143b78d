"""Times afmix()'s GPU step and the whole call at genome scale (S = 10^6 measured SNPs, P = 29, interval = 1000).

  (a) gauss_pop_weights on a seeded interval-major matrix: wall time of the blocking call (allele frequencies uploaded, four
      launches, weights back), best of --reps; the kernels alone come from one `rocprofv3 --kernel-trace --stats` run of this
      script (pw_*_kernel rows).  Beside it: the numpy restatement (tests/popwgt_ref.py: eigh, the clamp rule, inv) on the same
      matrix, and the largest difference between the two.
  (b) api.afmix on a packed panel of S SNPs with 4 samples per population (afmix reads allele frequencies only, so the panel
      stays small) and a study file listing every one of them; the study's parsing and the index merge are timed apart
      (api.popwgt_inputs, no GPU).

    python tools/popwgt_probe.py [--snps 1000000] [--interval 1000] [--reps 3] [--skip-call] [--json out.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gauss_amd import api, hotpath, panel, synth  # noqa: E402
from popwgt_ref import finish, interval_layout, interval_weights  # noqa: E402


def kernel_probe(S, P, interval, reps, ctx):
    rng = np.random.default_rng(2026)
    x = rng.uniform(0.02, 0.98, (S, P + 1))
    x[:, 0] = np.clip(x[:, 1:] @ rng.dirichlet(np.ones(P)) + rng.normal(0, 0.02, S), 0, 1)
    off, _ = interval_layout(S, interval)
    hotpath.pop_weights(x[:off[2]], off[:3], ctx=ctx)             # warm-up: code objects, attributes
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        w, st = hotpath.pop_weights(x, off, ctx=ctx)
        ts.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    wn, stn, _ = interval_weights(x, off)
    t_np = time.perf_counter() - t0
    return dict(S=S, P=P, interval=interval, gpu_call_ms=[round(t * 1e3, 3) for t in ts], gpu_call_best_ms=round(min(ts) * 1e3, 3),
                numpy_ms=round(t_np * 1e3, 1), max_abs_diff=float(np.nanmax(np.abs(w - wn))), clamped=int(np.count_nonzero(st & 1)),
                W_max_abs_diff=float(np.nanmax(np.abs(finish(w)[0] - finish(wn)[0]))))


def call_probe(S, P, interval, ctx):
    d = tempfile.mkdtemp(prefix="popwgt_probe_")
    pops = [(a, 4, s) for a, _, s in synth.POPS_33KG[:P]]
    rng = np.random.default_rng(7)
    bp = np.arange(S, dtype=np.int64) * 3 + 10_000
    alle = np.array(list("ACGT"))
    a1 = alle[rng.integers(0, 4, S)]
    a2 = alle[(np.searchsorted(alle, a1) + rng.integers(1, 4, S)) % 4]
    rsid = np.char.add("rs", np.arange(S).astype(str))
    chrs = np.full(S, 1)
    af = rng.uniform(0.02, 0.98, (S, P))
    src_off, ld = panel.pack2bit_layout([p[1] for p in pops])
    packed = os.path.join(d, "panel.pk")
    t0 = time.perf_counter()
    panel.write_packed_panel(packed, pops, rsid, chrs, bp, a1, a2, np.zeros((S, ld), np.uint8), af, np.zeros((S, P), np.int32),
                             sorted_flag=True)
    desc = os.path.join(d, "desc.txt")
    panel.write_pop_desc(desc, pops)
    study = os.path.join(d, "study_af.txt")
    saf = np.clip(af @ rng.dirichlet(np.ones(P)) + rng.normal(0, 0.02, S), 0.001, 0.999)
    order = rng.permutation(S)
    with open(study, "w") as f:
        f.write("rsid chr bp a1 a2 af1\n")
        f.writelines(f"{rsid[i]} 1 {bp[i]} {a1[i]} {a2[i]} {float(saf[i])!r}\n" for i in order)
    t_write = time.perf_counter() - t0
    t0 = time.perf_counter()
    _, x, off = api.popwgt_inputs(api.KIND_AFMIX, study, None, packed, desc, interval=interval)
    t_inputs = time.perf_counter() - t0
    ts = []
    for _ in range(2):               # the first call parses the study; the second finds it in the library's parsed-file cache
        t0 = time.perf_counter()
        df = api.afmix(study, None, packed, desc, interval=interval, ctx=ctx)
        ts.append(time.perf_counter() - t0)
    study_mb = round(os.path.getsize(study) / 1e6, 1)
    shutil.rmtree(d, ignore_errors=True)
    return dict(S=S, P=P, interval=interval, files_written_s=round(t_write, 2), popwgt_inputs_s=round(t_inputs, 3),
                afmix_call_s=[round(t, 3) for t in ts], n_pops_returned=len(df), study_mb=study_mb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, default=1_000_000)
    ap.add_argument("--pops", type=int, default=29)
    ap.add_argument("--interval", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-call", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = hotpath.default_context()
    out = dict(kernel=kernel_probe(a.snps, a.pops, a.interval, a.reps, ctx))
    print(json.dumps(out["kernel"]), flush=True)
    if not a.skip_call:
        out["call"] = call_probe(a.snps, a.pops, a.interval, ctx)
        print(json.dumps(out["call"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
