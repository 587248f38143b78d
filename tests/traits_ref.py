"""Reference statements of the further traits of a window (test infrastructure, numpy only).

Definition (include/gauss_hip.h, n_traits_more): row t of the output is what run_dist / run_distmix (dist.cpp:129-227,
distmix.cpp:138-253) return as z when the same window is run with z1 = z_more[t].  Two routes to it:

* ``traits_by_oracle`` does exactly that, one oracle call per trait (the primary reference);
* ``traits_closed_form`` is the algebra the GPU kernels evaluate -- G = B^-1 Z, B21 G, divided by sqrt(info) -- in LAPACK,
  on the b11 / b21 of ``oracle.run_impute(..., want_mats=True)`` (b11 as repaired by MakePosDef when it acted).
"""
import numpy as np


def traits_closed_form(b11, b21, Z, info=None):
    """b11 [M, M] with lambda on the diagonal (repaired if MakePosDef acted), b21 [U, M], Z [T, M].
    Returns mean [T, U] = (b21 B^-1 Z^T)^T, info [U] = |b21 B^-1 b12| (or the one passed) and z = mean / sqrt(info)."""
    b11 = np.asarray(b11, dtype=np.float64)
    b21 = np.asarray(b21, dtype=np.float64)
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    G = np.linalg.solve(b11, Z.T)                                   # [M, T]
    mean = (b21 @ G).T                                              # [T, U]
    if info is None:
        info = np.abs(np.einsum("um,mu->u", b21, np.linalg.solve(b11, b21.T)))      # dist.cpp:198
    with np.errstate(invalid="ignore", divide="ignore"):
        z = mean / np.sqrt(info)[None, :]                           # dist.cpp:200
    return dict(z=z, mean=mean, info=np.asarray(info, dtype=np.float64))


def traits_by_oracle(mode, geno_m, geno_u, pop_off, pop_wgt, Z, lam=0.1, min_abs_eig=1e-5, run_impute=None):
    """One run of the oracle per trait with z1 = Z[t] (default: the loop-literal C oracle).  Returns z [T, U], info [U] and
    `mpd`, the number of runs in which MakePosDef acted (0 or T: the LD does not depend on the trait)."""
    if run_impute is None:
        import oracle
        run_impute = oracle.run_impute
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    z, info, mpd = [], None, 0
    for t in range(Z.shape[0]):
        r = run_impute(mode, geno_m, geno_u, pop_off, pop_wgt, Z[t], lam=lam, min_abs_eig=min_abs_eig)
        z.append(r["z"])
        info = r["info"] if info is None else info
        assert np.array_equal(info, r["info"])                     # the information depends on the LD only
        mpd += int(r["mpd"])
    return dict(z=np.array(z), info=info, mpd=mpd)
