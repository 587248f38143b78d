"""Driver of tools/wave_simd_probe.hip: which wave indices of co-resident workgroups share a SIMD.

    hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o /tmp/libwavesimd.so tools/wave_simd_probe.hip
    python3 tools/wave_simd_probe.py [--lib /tmp/libwavesimd.so] [--wgs 4096] [--iters 40]

Prints
* how a workgroup's wave index maps to a SIMD: the histogram of (SIMD of wave 0, 1, 2, 3);
* per CU, for every moment a workgroup starts: the workgroups resident beside it, which of their wave indices sit on the
  SIMD of ITS wave 0, and how many different "rotations" (SIMD of wave 0) the residents have between them;
* how the block indices of co-resident workgroups relate: their differences, and block index mod 8 against the XCC id
  (the XCD interleave of gauss_plan.cpp assumes workgroup b runs on XCD b % 8);
* what a rotation of the wave roles keyed on the block index would do: for keys (b >> s) & 3, the share of resident groups
  of four whose workgroups put four different roles (wave + key) & 3 on one SIMD.
"""
import argparse
import collections
import ctypes as C

import numpy as np


def decode(rec):
    hw = rec[:, 0]
    return {
        "simd": (hw >> 4) & 3, "cu": (hw >> 8) & 15, "sh": (hw >> 12) & 1, "se": (hw >> 13) & 7, "xcc": rec[:, 1] & 15,
        "block": rec[:, 2], "wave": rec[:, 3],
        "t0": rec[:, 4].astype(np.uint64) | (rec[:, 5].astype(np.uint64) << np.uint64(32)),
        "t1": rec[:, 6].astype(np.uint64) | (rec[:, 7].astype(np.uint64) << np.uint64(32)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="/tmp/libwavesimd.so")
    ap.add_argument("--wgs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--show-cus", type=int, default=2)
    a = ap.parse_args()
    lib = C.CDLL(a.lib)
    lib.wave_simd_probe.argtypes = [C.c_int, C.c_int, C.c_void_p]
    rec = np.zeros((a.wgs * 4, 8), dtype=np.uint32)
    per_cu = lib.wave_simd_probe(a.wgs, a.iters, rec.ctypes.data)
    if per_cu < 0:
        raise SystemExit("probe failed")
    d = decode(rec)
    assert (d["block"] == np.repeat(np.arange(a.wgs), 4)).all() and (d["wave"] == np.tile(np.arange(4), a.wgs)).all(), "records missing"
    print("workgroups %d, occupancy calculator: %d workgroups a CU" % (a.wgs, per_cu))

    simd = d["simd"].reshape(a.wgs, 4)
    cu_key = (d["xcc"].astype(np.int64) * 8 + d["se"]) * 32 + d["sh"] * 16 + d["cu"]
    cu_key = cu_key.reshape(a.wgs, 4)
    assert (cu_key == cu_key[:, :1]).all(), "a workgroup's waves report different CUs"
    cu_key = cu_key[:, 0]
    t0 = d["t0"].reshape(a.wgs, 4).min(axis=1).astype(np.int64)
    t1 = d["t1"].reshape(a.wgs, 4).max(axis=1).astype(np.int64)
    xcc = d["xcc"].reshape(a.wgs, 4)[:, 0]
    print("distinct CUs seen: %d; workgroup duration (100 MHz ticks): median %d, max %d" % (len(set(cu_key.tolist())), np.median(t1 - t0), (t1 - t0).max()))

    # 1. wave index -> SIMD
    pat = collections.Counter(tuple(int(x) for x in row) for row in simd)
    print("\n(SIMD of wave 0, 1, 2, 3): workgroups")
    for p, n in sorted(pat.items(), key=lambda kv: -kv[1]):
        print("   %s: %d%s" % (p, n, "" if len(set(p)) == 4 else "   <- two waves of one workgroup on one SIMD"))
    start = simd[:, 0]
    print("SIMD of wave 0: %s" % dict(sorted(collections.Counter(int(s) for s in start).items())))

    # 2. block index mod 8 against the XCC id
    tab = collections.Counter((int(b) % 8, int(x)) for b, x in zip(range(a.wgs), xcc))
    one_to_one = all(len([1 for (m, x) in tab if m == mm]) == 1 for mm in range(8))
    print("\nblock %% 8 -> XCC id: %s (%s)" % (sorted(tab.keys()), "one XCC per residue" if one_to_one else "NOT one XCC per residue"))

    # 3. residents per CU at every workgroup start
    by_cu = collections.defaultdict(list)
    for b in range(a.wgs):
        by_cu[int(cu_key[b])].append(b)
    n_res = collections.Counter()
    distinct_rot = collections.Counter()
    share = collections.Counter()           # how many residents' wave w sits on the newcomer's wave-0 SIMD, by w
    diffs = collections.Counter()
    groups = []                             # full groups of per_cu residents (block indices)
    shown = 0
    for cu, blocks in sorted(by_cu.items()):
        blocks.sort(key=lambda b: t0[b])
        lines = []
        for b in blocks:
            res = [o for o in blocks if o != b and t0[o] <= t0[b] < t1[o]]
            n_res[len(res) + 1] += 1
            if len(res) + 1 == per_cu:
                grp = sorted(res + [b])
                groups.append(grp)
                distinct_rot[len(set(int(start[o]) for o in grp))] += 1
                for o in res:
                    w = [k for k in range(4) if simd[o, k] == simd[b, 0]]
                    share[tuple(w)] += 1
                    diffs[abs(o - b)] += 1
            lines.append("      block %5d  SIMDs %s  beside %s" % (b, tuple(int(x) for x in simd[b]), [(o, tuple(int(x) for x in simd[o])) for o in res]))
        if shown < a.show_cus:
            shown += 1
            print("\n   CU key %d (XCC %d): %d workgroups in start order" % (cu, cu // 256, len(blocks)))
            print("\n".join(lines[:12]))
    print("\nresidents on the CU when a workgroup starts (itself included): %s" % dict(sorted(n_res.items())))
    print("full groups: different SIMDs of wave 0 among the %d residents: %s" % (per_cu, dict(sorted(distinct_rot.items()))))
    print("a resident's wave indices on the SIMD of the newcomer's wave 0: %s" % dict(sorted(share.items(), key=lambda kv: -kv[1])))
    top = sorted(diffs.items(), key=lambda kv: -kv[1])[:12]
    print("block-index differences between co-residents (most frequent): %s" % top)

    # 4. a rotation keyed on the block index
    print("\nrotation key -> share of full resident groups whose workgroups put four different roles (wave + key) & 3 on SIMD 0 / all the same role")
    for name, key in [("none", lambda b: 0)] + [("(b >> %d) & 3" % s, (lambda s_: lambda b: (b >> s_) & 3)(s)) for s in range(0, 12)]:
        alld = alleq = 0
        for grp in groups:
            # the role (wave + key) & 3 that each resident puts on SIMD 0 (the other SIMDs follow when every workgroup
            # walks the SIMDs in the same cyclic order)
            v = [[(w + key(o)) & 3 for w in range(4) if simd[o, w] == 0] for o in grp]
            v = set(x[0] for x in v if len(x) == 1)
            alld += len(v) == len(grp)
            alleq += len(v) == 1
        print("   %-14s %.3f / %.3f" % (name, alld / max(1, len(groups)), alleq / max(1, len(groups))))


if __name__ == "__main__":
    main()
