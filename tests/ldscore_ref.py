"""LD scores of a window's measured SNPs (include/gauss_hip.h, lds_*), stated twice in numpy from given B11 [M, M], B21 [U, M], the rows'
positions, the radius, n and the annotation weights:

  replay()  the order of ldscore_kernel as DESIGN.md section 4 writes it down: rows in chunks of CHUNK (the measured rows from row 0, the
            others from row M, never both in a chunk); a chunk's partial starts at 0 and takes its contributing rows in ascending order
            (t = r r, raw += a t, mass += a); the totals start at 0 and take the partials in ascending chunk order;
  plain()   a masked np.sum over the concatenated rows.

Both return dict(raw, l2, mass), each [1 + C, M]: row 0 the plain score, row 1 + c the score stratified by category c.  Row k of the
concatenated row space (measured rows first) contributes to target j iff |bp(k) - bp_m(j)| <= radius; a row outside the band is never
read into the sum, so a NaN there does not reach the target; inside it the arithmetic is plain.
l2 = raw (1 + 1 / (n - 2)) - mass / (n - 2)."""
import numpy as np

CHUNK = 64          # GAUSS_LDS_CHUNK


def _inputs(b11, b21, bp_m, bp_u, annot):
    b11 = np.asarray(b11, dtype=np.float64)
    M = b11.shape[0]
    b21 = np.zeros((0, M)) if b21 is None or len(b21) == 0 else np.asarray(b21, dtype=np.float64)
    U = b21.shape[0]
    R = np.vstack([b11, b21])                       # [M + U, M]: row k, target j
    bp = np.concatenate([np.asarray(bp_m, dtype=np.int64), np.asarray(bp_u if bp_u is not None else (), dtype=np.int64)])
    assert len(bp) == M + U
    A = np.ones((1, M + U))
    if annot is not None:
        A = np.vstack([A, np.asarray(annot, dtype=np.float64).reshape(-1, M + U)])
    return R, bp, A, M, U


def _band(bp, M, radius):
    return np.abs(bp[:, None] - bp[None, :M]) <= int(radius)          # [M + U, M]


def _l2(raw, mass, n):
    nm2 = float(n) - 2.0
    return raw * (1.0 + 1.0 / nm2) - mass / nm2


def chunks(M, U, chunk=CHUNK):
    """[(k0, k1)] in the concatenated row space, in the order the totals take them"""
    out = [(k, min(k + chunk, M)) for k in range(0, M, chunk)]
    return out + [(M + k, M + min(k + chunk, U)) for k in range(0, U, chunk)]


def replay(b11, b21, bp_m, bp_u, radius, n, annot=None, chunk=CHUNK):
    R, bp, A, M, U = _inputs(b11, b21, bp_m, bp_u, annot)
    band = _band(bp, M, radius)
    C1 = A.shape[0]
    raw, mass = np.zeros((C1, M)), np.zeros((C1, M))
    with np.errstate(invalid="ignore", over="ignore"):
        for k0, k1 in chunks(M, U, chunk):
            p_raw, p_mass = np.zeros((C1, M)), np.zeros((C1, M))
            for k in range(k0, k1):                     # one row at a time: every target's sum takes its rows in ascending order
                on = band[k]
                if not on.any():
                    continue
                t = R[k, on] * R[k, on]
                for c in range(C1):
                    p_raw[c, on] += A[c, k] * t
                    p_mass[c, on] += A[c, k]
            raw += p_raw
            mass += p_mass
        return dict(raw=raw, l2=_l2(raw, mass, n), mass=mass)


def plain(b11, b21, bp_m, bp_u, radius, n, annot=None):
    R, bp, A, M, U = _inputs(b11, b21, bp_m, bp_u, annot)
    band = _band(bp, M, radius)
    C1 = A.shape[0]
    raw, mass = np.zeros((C1, M)), np.zeros((C1, M))
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(M):
            on = band[:, j]
            r2 = R[on, j] ** 2
            for c in range(C1):
                raw[c, j] = np.sum(A[c, on] * r2)
                mass[c, j] = np.sum(A[c, on])
        return dict(raw=raw, l2=_l2(raw, mass, n), mass=mass)


def count(bp_m, bp_u, radius):
    """mass[0] by brute force: the rows within the radius of every target"""
    bp = [int(v) for v in bp_m] + [int(v) for v in (bp_u if bp_u is not None else ())]
    return np.array([sum(1 for b in bp if abs(b - int(t)) <= int(radius)) for t in bp_m], dtype=np.float64)
