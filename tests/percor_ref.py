"""Exact reference for the per-population correlation kernels (pop_cor_kernel, pair_cor_kernel in k_pack_epilogue.hip,
zm_partial_kernel / zm_final_kernel in k_zmix.hip) and the inputs of tests/test_gpu_percor_segments.py.  No GPU, no oracle.

Every sum these kernels read is an integer: per group g of populations n, Sx, Sy, Sxx, Syy, Sxy.  They are formed here with
int64 matmuls per population and pooled as Python ints; the correlation

    r = (n Sxy - Sx Sy) / sqrt((n Sxx - Sx^2) (n Syy - Sy^2))

is then evaluated from those integers beyond any doubt about rounding -- math.isqrt of the denominator's square scaled by 2^256
(relative error below 2^-128), and Python's correctly rounded int / int division -- i.e. rounded once to float64.  exact_r_decimal
is the same value through `decimal` at 60 digits (tests/test_percor_ref.py holds the two against each other).  A variance
integer of 0 gives NaN: that is exactly where the kernels' tail is 0 / 0 (a monomorphic SNP has n Sxy = Sx Sy as well).

The inputs: population tables whose sizes sit on the planner's segment cuts (see TABLES below), SNP counts on the tile edges,
genotypes from synth.synth_genotypes with a few SNPs made monomorphic inside ONE SEGMENT of a multi-segment population (finite
result: only the population's total counts), in a whole population (NaN there) and in a whole group (NaN in the grouped runs too).
"""
import decimal
import functools
import math
import zlib

import numpy as np

from gauss_amd import synth

TILE = 128          # Gram tile (gauss_internal.h)
KC = 64             # K chunk: a population is zero padded to a multiple of it
SHIFT = 128

# ---- the planner's cut, restated (gauss_plan.cpp: seg_max_for, plan_problem) ----
#
# A population of m samples takes chunks = ceil(m / 64) K chunks.  With max_chunks = seg_max / 64 it is cut into
# ns = ceil(chunks / max_chunks) segments of per = ceil(chunks / ns) chunks (the last one shorter), one Gram partial slab each.
# seg_max is 2 048 for a listed-pair job (gauss_ld_per_pop_pairs).  For a one-window every-pair job (gauss_ld_per_pop,
# gauss_zmix_normal_eq) it is min(2048, max(384, floor(want / 64) * 64)) with want = tile_pairs * (N + 32 P) / 1300: at
# n_snp <= 300 (<= 6 tile pairs) and N <= 10^4 samples want stays below 50, so seg_max = 384 = six chunks.  Hence
#   every-pair: 384 -> one segment (6 chunks), 385 -> two (4 + 3), 1 000 -> three (6 + 6 + 4); 17, 64, 130 -> one
#   listed:     2 048 -> one (32 chunks), 2 049 -> two (17 + 16), 4 200 -> three (22 + 22 + 22)
# and the listed tables are cut into 6 / 6 / 11 segments when the every-pair calls run on them.
SEG_EVERY_PAIR = 384
SEG_LISTED = 2048


def segment_chunks(m, seg_max):
    """Chunks per segment of a population of m samples."""
    chunks = -(-m // KC)
    if chunks == 0:
        return []
    max_chunks = seg_max // KC
    ns = -(-chunks // max_chunks)
    per = -(-chunks // ns)
    return [min(per, chunks - c) for c in range(0, chunks, per)]


def segment_ranges(m, seg_max):
    """[a, b) sample ranges (inside the population) of its segments."""
    out, c = [], 0
    for k in segment_chunks(m, seg_max):
        out.append((c * KC, min(m, (c + k) * KC)))
        c += k
    return out


def seg_max_every_pair(n_snp, sizes):
    mt = -(-n_snp // TILE)
    want = (mt * (mt + 1) / 2) * (sum(sizes) + 32.0 * len(sizes)) / 1300.0
    return int(min(2048.0, max(384.0, math.floor(want / KC) * KC)))


# name -> (population sizes, population -> group, the cut the table is placed on).  A multi-segment population is first, in the
# middle and last; groups are not contiguous; every grouped table has a group mixing a multi-segment population with
# single-segment ones, and "mid_last" / "big_first_mid" have a group holding two multi-segment populations.
TABLES = {
    "first_mid": ([385, 17, 1000, 64, 384, 130], [0, 0, 1, 2, 1, 2], SEG_EVERY_PAIR),
    "mid_last": ([130, 1000, 64, 17, 384, 385], [1, 0, 1, 0, 2, 0], SEG_EVERY_PAIR),
    "lead_1000": ([1000, 17, 385, 130, 64, 384], [0, 1, 1, 0, 2, 2], SEG_EVERY_PAIR),
    "big_first_mid": ([2049, 17, 4200, 130, 2048, 64], [0, 1, 0, 0, 2, 1], SEG_LISTED),
    "big_last": ([64, 4200, 2048, 17, 130, 2049], [0, 0, 1, 2, 2, 2], SEG_LISTED),
}
SNP_COUNTS = (2, 129, 300)          # one ragged tile; two tiles, the second of one row; three tiles = all six tile pairs
CASES = {f"{t}-S{S}": (t, S) for t in TABLES for S in SNP_COUNTS}
EVERY_PAIR_CASES = [c for c, (t, _) in CASES.items() if TABLES[t][2] == SEG_EVERY_PAIR]
LISTED_CASES = [c for c, (t, _) in CASES.items() if TABLES[t][2] == SEG_LISTED]

# SNPs that are edited, by SNP count.  S = 2 is one pair in one ragged tile: it cannot both keep and drop a row.  In the tables of
# S2_POP_MONO its SNP 0 is monomorphic in the first single-segment population -- NaN in that population's entry, the only row of
# the ungrouped normal equations dropped (kept rows 0, every sum 0), finite once the population is pooled into its group --;
# in the other tables both SNPs stay polymorphic and the row is kept.
S2_POP_MONO = ("mid_last", "big_last")
SEG_MONO = {2: [1], 129: [3, 128], 300: [3, 128, 255, 299]}       # monomorphic inside one segment only: finite
POP_MONO = {2: [], 129: [9, 77], 300: [9, 77, 130, 222, 290]}     # monomorphic in a whole population: NaN there
GRP_MONO = {2: [], 129: [50], 300: [50, 180]}                     # one value over a whole group: NaN in the grouped runs too


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one case (read-only arrays): G uint8 [S, N], off, grp, z, and what was edited where."""
    table, S = CASES[name]
    sizes, grp, seg_max = TABLES[table]
    seed = zlib.crc32(name.encode()) % 1_000_000
    rng = np.random.default_rng(seed)
    pops = [(f"P{k:02d}", m, f"S{grp[k]}") for k, m in enumerate(sizes)]
    bp = np.sort(rng.choice(np.arange(1, 2000 * S + 100), size=S, replace=False))
    # maf_lo: a 17-sample population must not lose a third of the SNPs to chance monomorphism (at most half of the rows may drop)
    G, _ = synth.synth_genotypes(bp, pops, seed=seed + 1, maf_lo=0.15)
    off = synth.pop_offsets(sizes)
    multis = [p for p, m in enumerate(sizes) if len(segment_chunks(m, seg_max)) > 1]
    singles = [p for p, m in enumerate(sizes) if len(segment_chunks(m, seg_max)) == 1]
    seg_mono, pop_mono, grp_mono = [], [], []
    for t, s in enumerate(SEG_MONO[S]):
        p = multis[t % len(multis)]
        rngs = segment_ranges(sizes[p], seg_max)
        k = (t + 1) % len(rngs)                                   # (the last, ragged segment among them)
        a, b = rngs[k]
        c = t % 3
        G[s, off[p] + a:off[p] + b] = c
        o = rngs[(k + 1) % len(rngs)][0]                          # one carrier in another segment: polymorphic overall
        G[s, off[p] + o] = (c + 1) % 3
        seg_mono.append((s, p, a, b))
    if S == 2 and table in S2_POP_MONO:
        G[0, off[singles[0]]:off[singles[0] + 1]] = 1
        pop_mono.append((0, singles[0]))
    for t, s in enumerate(POP_MONO[S]):
        cand = multis + singles[:1]
        p = cand[t % len(cand)]
        G[s, off[p]:off[p + 1]] = t % 3
        pop_mono.append((s, p))
    for t, s in enumerate(GRP_MONO[S]):
        g = grp[multis[t % len(multis)]]
        for p in range(len(sizes)):
            if grp[p] == g:
                G[s, off[p]:off[p + 1]] = (t + 1) % 3
        grp_mono.append((s, g))
    z = rng.standard_normal(S) * 2.0
    G = np.ascontiguousarray(G, dtype=np.uint8)
    grp = np.array(grp, dtype=np.int32)
    for a in (G, off, grp, z):
        a.setflags(write=False)
    return dict(name=name, G=G, off=off, grp=grp, z=z, sizes=list(sizes), S=S, seg_max=seg_max, multis=multis, singles=singles,
                seg_mono=seg_mono, pop_mono=pop_mono, grp_mono=grp_mono)


def pair_list(S):
    """The listed pairs of a case (int32 i, j; i < j), in no particular order: the first and last row, both sides of a tile
    edge -- (127, 128), (0, S - 1), (128, 129) --, about forty pairs from every tile pair but (1, 2), which stays untouched."""
    if S == 2:
        return np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    rng = np.random.default_rng(1000 + S)
    pairs = {(0, 1), (0, S - 1), (S - 2, S - 1), (126, 127), (127, 128)}
    if S > 129:
        pairs |= {(128, 129), (127, 129)}
    nT = -(-S // TILE)
    for ti in range(nT):
        for tj in range(ti, nT):
            if (ti, tj) == (1, 2):
                continue
            i = rng.integers(ti * TILE, min(S, (ti + 1) * TILE), size=40)
            j = rng.integers(tj * TILE, min(S, (tj + 1) * TILE), size=40)
            pairs |= {(int(a), int(b)) for a, b in zip(i, j) if a < b}
    pairs = sorted(pairs)
    order = rng.permutation(len(pairs))
    pi = np.array([pairs[k][0] for k in order], dtype=np.int32)
    pj = np.array([pairs[k][1] for k in order], dtype=np.int32)
    return pi, pj


def pair_row_index(S, pi, pj):
    """Row of pair (i, j) in the every-pair order (i ascending, then j)."""
    pi, pj = np.asarray(pi, dtype=np.int64), np.asarray(pj, dtype=np.int64)
    return pi * S - pi * (pi + 1) // 2 + (pj - pi - 1)


# ---- exact integer sums ----

def group_sums(G, off, grp=None):
    """Per group g (every population its own group when grp is None): n[g] (Python int), Sx[g], Sxx[g] ([S] Python ints) and
    Sxy[g] ([S, S] Python ints), from int64 matmuls per population."""
    G = np.asarray(G)
    assert G.dtype == np.uint8 and G.ndim == 2
    P = len(off) - 1
    grp = list(range(P)) if grp is None else [int(g) for g in grp]
    ng = max(grp) + 1
    S = G.shape[0]
    n = [0] * ng
    Sx = [np.zeros(S, dtype=object) for _ in range(ng)]
    Sxx = [np.zeros(S, dtype=object) for _ in range(ng)]
    Sxy = [np.zeros((S, S), dtype=object) for _ in range(ng)]
    for p in range(P):
        X = G[:, int(off[p]):int(off[p + 1])].astype(np.int64)
        g = grp[p]
        n[g] += int(X.shape[1])
        Sx[g] = Sx[g] + X.sum(axis=1).astype(object)
        Sxx[g] = Sxx[g] + (X * X).sum(axis=1).astype(object)
        Sxy[g] = Sxy[g] + (X @ X.T).astype(object)
    return dict(n=n, Sx=Sx, Sxx=Sxx, Sxy=Sxy, S=S, n_group=ng)


def exact_r(n, sx, sy, sxx, syy, sxy):
    """The correlation from exact Python ints, rounded once to float64; NaN when a variance integer is 0."""
    vx, vy = n * sxx - sx * sx, n * syy - sy * sy
    assert vx >= 0 and vy >= 0
    if vx == 0 or vy == 0:
        return math.nan
    num = n * sxy - sx * sy
    return (num << SHIFT) / math.isqrt((vx * vy) << (2 * SHIFT))       # int / int: correctly rounded


def exact_r_decimal(n, sx, sy, sxx, syy, sxy, prec=60):
    """exact_r through `decimal` at `prec` digits."""
    vx, vy = n * sxx - sx * sx, n * syy - sy * sy
    if vx == 0 or vy == 0:
        return math.nan
    with decimal.localcontext() as c:
        c.prec = prec
        return float(decimal.Decimal(n * sxy - sx * sy) / (decimal.Decimal(vx) * decimal.Decimal(vy)).sqrt())


def cor_pairs(sums, pi, pj):
    """float64 [n_group, n_pairs]: exact_r of the listed pairs inside every group."""
    pi, pj = np.asarray(pi, dtype=np.int64), np.asarray(pj, dtype=np.int64)
    out = np.empty((sums["n_group"], len(pi)))
    for g in range(sums["n_group"]):
        n, Sx, Sxx = sums["n"][g], sums["Sx"][g], sums["Sxx"][g]
        cols = (Sx[pi].tolist(), Sx[pj].tolist(), Sxx[pi].tolist(), Sxx[pj].tolist(), sums["Sxy"][g][pi, pj].tolist())
        out[g] = [exact_r(n, *v) for v in zip(*cols)]
    return out


def pair_rows(G, off, z, grp=None):
    """[y | r_1 .. r_G] of every pair i < j in the reference's order (i ascending, then j), y = z_i z_j in float64."""
    G = np.asarray(G)
    iu, ju = np.triu_indices(G.shape[0], 1)
    z = np.asarray(z, dtype=np.float64)
    return np.column_stack([z[iu] * z[ju], cor_pairs(group_sums(G, off, grp), iu, ju).T])


def normal_eq_exact(rows):
    """Rows with a non-finite entry dropped; X^T X, X^T y, y^T y with every entry summed by math.fsum, the kept-row count, and
    A = sum_k |x_a(k) x_b(k)| for every entry of the [y | X] cross-product (A[0, 0]: y^T y, A[0, 1:]: X^T y, A[1:, 1:]: X^T X)."""
    rows = np.asarray(rows, dtype=np.float64)
    keep = np.isfinite(rows).all(axis=1)
    m = rows[keep]
    nc = rows.shape[1]
    M, A = np.zeros((nc, nc)), np.zeros((nc, nc))
    for a in range(nc):
        for b in range(a, nc):
            prod = m[:, a] * m[:, b]
            M[a, b] = M[b, a] = math.fsum(prod)
            A[a, b] = A[b, a] = math.fsum(np.abs(prod))
    return dict(xtx=M[1:, 1:], xty=M[0, 1:], yty=float(M[0, 0]), n_rows=int(keep.sum()), A=A)


def normal_eq_bound(n_rows, A, factor=1.0):
    """factor * (n_rows 2^-53 + 2^-49) * A: any-order summation of n_rows products (gamma_n sum |x_a x_b|) on inputs that each
    carry at most 2^-50 relative error; the device tests take factor 2 for the second-order terms."""
    return factor * (n_rows * 2.0 ** -53 + 2.0 ** -49) * np.asarray(A)


@functools.lru_cache(maxsize=None)
def case_rows(name, grouped):
    """pair_rows of a case, computed once (read-only)."""
    c = case(name)
    rows = pair_rows(c["G"], c["off"], c["z"], c["grp"] if grouped else None)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def case_normal_eq(name, grouped):
    return normal_eq_exact(case_rows(name, grouped))
