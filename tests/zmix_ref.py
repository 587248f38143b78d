"""An independent numpy statement of zmix() (zmix.R) for the tests: the pair matrix from the oracle's prep_zmix5 /
prep_zmix5_sup, the finite-row filter, the two cross-products, a KKT certificate of the QP's optimum and the reduced solve on
the free set, the normalisation and rounding."""
import numpy as np

from oracle import feeder_py as fp


def normal_eq(mat):
    """[y | X] -> (D = X^T X, d = X^T y, y^T y, kept rows), rows with a non-finite entry dropped (is.finite(rowSums(mat)))."""
    mat = np.asarray(mat, dtype=np.float64)
    if mat.ndim == 1:
        mat = mat.reshape(0, -1) if mat.size == 0 else mat.reshape(1, -1)
    keep = np.isfinite(mat.sum(axis=1))
    m = mat[keep]
    y, X = m[:, 0], m[:, 1:]
    return X.T @ X, X.T @ y, float(y @ y), int(keep.sum())


def matrix(input_file, index, data, desc, percentile=0.9, interval=10, level="population"):
    """prep_zmix5 / prep_zmix5_sup's matrix [n_pairs x (1 + G)] from the oracle (pure Python)."""
    if level == "superpopulation":
        return np.asarray(fp.prep_zmix_variant("zmix5_sup", input_file, index, data, desc, percentile=percentile,
                                               interval=interval)["data_mat"], dtype=np.float64)
    return np.asarray(fp.prep_zmix5(input_file, index, data, desc, percentile=percentile, interval=interval)["data_mat"],
                      dtype=np.float64)


def kkt(D, d, w, tol=1e-9):
    """KKT certificate of w for min 1/2 w'Dw - d'w, sum w = 1, w >= 0 (w <= 1 is implied).  D positive definite makes the
    problem strictly convex, so a certified w is THE optimum whatever algorithm produced it.  Returns the violations."""
    D, d, w = (np.asarray(a, dtype=np.float64) for a in (D, d, w))
    g = D @ w - d
    scale = max(1.0, float(np.max(np.abs(D))) * max(1.0, float(np.max(np.abs(w)))), float(np.max(np.abs(d))))
    F = w > 1e-10
    nu = float(np.mean(g[F])) if F.any() else 0.0
    bad = []
    if F.any() and np.max(np.abs(g[F] - nu)) > tol * scale:
        bad.append(("stationarity on F", float(np.max(np.abs(g[F] - nu))), tol * scale))
    if (~F).any() and np.min(g[~F] - nu) < -tol * scale:
        bad.append(("dual feasibility off F", float(np.min(g[~F] - nu)), -tol * scale))
    if np.min(w) < -1e-12:
        bad.append(("w >= 0", float(np.min(w))))
    if abs(float(np.sum(w)) - 1.0) > 1e-12:
        bad.append(("sum w = 1", float(np.sum(w))))
    return bad


def reduced_solve(D, d, F):
    """The equality-constrained QP on the free set F (others 0): [D_FF 1; 1' 0] [w_F; -nu] = [d_F; 1]."""
    D, d = np.asarray(D, dtype=np.float64), np.asarray(d, dtype=np.float64)
    idx = np.nonzero(F)[0]
    k = len(idx)
    A = np.zeros((k + 1, k + 1))
    A[:k, :k] = D[np.ix_(idx, idx)]
    A[:k, k] = 1.0
    A[k, :k] = 1.0
    rhs = np.concatenate([d[idx], [1.0]])
    sol = np.linalg.solve(A, rhs)
    w = np.zeros(len(d))
    w[idx] = sol[:k]
    return w


def finish(w):
    """w / sum w; round to 5 decimals (half-even: numpy's rounding); / sum again.  Returns (unrounded, final)."""
    w = np.asarray(w, dtype=np.float64)
    u = w / np.sum(w)
    r = np.round(u, 5)
    return u, r / np.sum(r)


def near_rounding_boundary(u, tol=1e-9):
    """Entries whose value is within tol of a half-way point of the 5-decimal grid."""
    x = np.asarray(u) * 1e5
    return np.abs(x - np.floor(x) - 0.5) <= tol * 1e5
