#!/usr/bin/env python3
"""Regenerates tests/golden/*.npz: seeded inputs + the CPU oracle's outputs, frozen.

The reference ships no golden vectors for this path and cannot be run here (no R/Rcpp/RcppEigen), so
these vectors pin the *oracle* (cross-validated against numpy/scipy in tests/test_oracle.py), not the
reference binary: "parity unpinned" in the sense of the task statement.  They guard against silent
drift of either the oracle or the HIP path between rounds.  Run from the repo root:
    python tests/golden/make_golden.py
    python tests/golden/make_golden.py --bgzf      (ref_bgzf.*: needs oracle/_ref/libref_bgzf.so)
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
from gauss_amd import synth  # noqa: E402


def main():
    pops = [("CEU", 151, "EUR"), ("FIN", 97, "EUR"), ("CCE", 130, "ASN"), ("ASW", 41, "AFR"), ("GBR", 88, "EUR"),
            ("JPT", 64, "ASN"), ("YRI", 29, "AFR")]
    rng = np.random.default_rng(20260213)
    bp = np.sort(rng.choice(np.arange(1, 250_000), size=110, replace=False))
    G, _ = synth.synth_genotypes(bp, pops, seed=20260213)
    G = G[G.min(1) != G.max(1)][:96]
    off = synth.pop_offsets([p[1] for p in pops])
    w = np.array([0.165, 0.138, 0.008, 0.036, 0.165, 0.011, 0.538])        # sums to 1.061 like PGC2
    idx = rng.permutation(G.shape[0])
    gm = np.ascontiguousarray(G[np.sort(idx[:42])])
    gu = np.ascontiguousarray(G[np.sort(idx[42:])])
    z1 = np.round(rng.standard_normal(gm.shape[0]) * 2, 6)
    out = dict(gm=gm, gu=gu, off=off, w=w, zin=z1)
    for mode in (0, 1):
        r = oracle.run_impute(mode, gm, gu, off, w, z1, want_mats=True)
        out[f"z{mode}"], out[f"info{mode}"], out[f"b11_{mode}"], out[f"b21_{mode}"] = r["z"], r["info"], r["b11"], r["b21"]
    out["ld_weighted"] = oracle.compute_ld(gm, off, w)
    out["ld_pooled"] = oracle.ld_pooled(gm, off, 1.1)
    out["counts"] = oracle.gram_counts(gm)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "window_small.npz"), **out)
    print("wrote tests/golden/window_small.npz", {k: v.shape for k, v in out.items()})

    # the widened rows: QCAT, raw LD export with recoded rows, per-population LD
    ext = dict(n_head=np.int32(6), n_pred=np.int32(25))
    for mode in (0, 1):
        q = oracle.run_qcat(mode, gm, gu, off, w, z1, 6, 25)
        ext[f"qcat_r{mode}"], ext[f"qcat_num_eig{mode}"] = q["r"], np.int32(q["num_eig"])
        b = oracle.ld_blocks(mode, gm, gu, off, w, 1.0, (0, 1, 2))
        ext[f"ldx_b11_{mode}"], ext[f"ldx_b21_{mode}"] = b["b11"], b["b21"]
    ext["ld_per_pop"] = oracle.ld_per_pop(gm[:24], off)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "window_small_ext.npz"), **ext)
    print("wrote tests/golden/window_small_ext.npz", {k: np.shape(v) for k, v in ext.items()})


class _RefBgzf(ctypes.Structure):
    """The leading fields of the reference's BGZF handle (bgzf.h, built without _USE_KNETFILE): bgzf_tell is a macro over them."""
    _fields_ = [("file_descriptor", ctypes.c_int), ("open_mode", ctypes.c_char), ("owned_file", ctypes.c_int16),
                ("compress_level", ctypes.c_int16), ("file", ctypes.c_void_p), ("uncompressed_block_size", ctypes.c_int),
                ("compressed_block_size", ctypes.c_int), ("uncompressed_block", ctypes.c_void_p), ("compressed_block", ctypes.c_void_p),
                ("block_address", ctypes.c_int64), ("block_length", ctypes.c_int), ("block_offset", ctypes.c_int)]


def bgzf():
    """tests/golden/ref_bgzf.gz + ref_bgzf.json: a panel-shaped text written by the reference's OWN BGZF writer (oracle/_ref/libref_bgzf.so,
    built by oracle/Makefile where the reference tree exists), with the virtual offset bgzf_tell gave at the start of every 40th line.
    tests/test_feeder.py reads it with the project's readers, so the codec stays pinned where the reference cannot be built."""
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_bgzf.so"))
    lib.bgzf_open.restype = ctypes.POINTER(_RefBgzf)
    lib.bgzf_open.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.bgzf_write.argtypes = [ctypes.POINTER(_RefBgzf), ctypes.c_void_p, ctypes.c_int]
    lib.bgzf_close.argtypes = [ctypes.POINTER(_RefBgzf)]
    rng = np.random.default_rng(20261016)
    lines = []
    for i in range(1500):
        g = "".join(map(str, rng.choice(3, size=int(rng.integers(60, 240)), p=[0.6, 0.3, 0.1])))
        lines.append(f"rs{1000 + 7 * i}\t22\t{16_050_000 + 211 * i}\t{'ACGT'[i % 4]}\t{'GTAC'[i % 4]}\t{g}")
    path = os.path.join(ROOT, "tests", "golden", "ref_bgzf.gz")
    h = lib.bgzf_open(path.encode(), b"w")
    assert h
    voff = []
    for i, line in enumerate(lines):
        if i % 40 == 0:
            voff.append([i, (h.contents.block_address << 16) | (h.contents.block_offset & 0xFFFF)])
        b = (line + "\n").encode()
        assert lib.bgzf_write(h, b, len(b)) == len(b)
    assert lib.bgzf_close(h) == 0
    text = ("\n".join(lines) + "\n").encode()
    meta = {"lines": len(lines), "text_bytes": len(text), "text_sha256": hashlib.sha256(text).hexdigest(), "line_voffsets": voff,
            "made_by": "the reference's bgzf_open / bgzf_write / bgzf_close (src/bgzf.c); voffsets from its bgzf_tell"}
    with open(os.path.join(ROOT, "tests", "golden", "ref_bgzf.json"), "w") as fh:
        json.dump(meta, fh, indent=0)
    print("wrote tests/golden/ref_bgzf.gz", os.path.getsize(path), "bytes,", len(text), "bytes of text")


if __name__ == "__main__":
    if "--bgzf" in sys.argv:
        bgzf()
    else:
        main()
