"""numpy-level front end of the C ABI (include/gauss_hip.h) -- the numeric hot path on the GPU.

Each function is a thin marshalling layer over one C entry point; all arithmetic happens in
libgauss_hip.so on the device.  Names follow the reference functions they replace.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import MODE_POOLED, MODE_WEIGHTED, WindowDesc, check  # noqa: F401

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class Context:
    """One HIP device context (gauss_hip_init / gauss_hip_destroy)."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.gauss_hip_init(int(device), C.byref(h)))
        self.handle = h
        self.device = device

    def set_gram_dtype(self, dtype):
        """'f32' (default, v_mfma_f32_32x32x2_f32) or 'i8' (v_mfma_i32_32x32x32_i8); same exact integers."""
        code = {"f32": _lib.GRAM_F32, "i8": _lib.GRAM_I8}[dtype] if isinstance(dtype, str) else int(dtype)
        check(self.lib.gauss_hip_set_gram_dtype(self.handle, code))

    @property
    def id(self):
        """Process-unique id of the context (gauss_hip_context_id); 0 once closed."""
        return int(self.lib.gauss_hip_context_id(self.handle)) if self.handle else 0

    def trim_cache(self):
        """Give the context's cached job workspaces back to the device; returns the bytes freed."""
        n = C.c_int64()
        check(self.lib.gauss_hip_trim_cache(self.handle, C.byref(n)))
        return n.value

    def counters(self):
        """gauss_hip_counters: runs queued merged / demoted to two launches, merged runs that gave up (re-run inside the
        fetch), re-runs that failed too."""
        out = (C.c_int64 * 4)()
        check(self.lib.gauss_hip_counters(self.handle, out))
        return dict(merged=int(out[0]), demoted=int(out[1]), giveups=int(out[2]), rerun_failed=int(out[3]))

    def queues(self):
        """gauss_hip_queues: the library's priority streams on this device, the runtime's hardware queues per class, and whether
        this context's chain / low-priority / main queues were SEEN to run side by side when it was made."""
        out = (C.c_int32 * 4)()
        check(self.lib.gauss_hip_queues(self.handle, out))
        return dict(hi_streams=int(out[0]), lo_streams=int(out[1]), hw_queues_per_class=int(out[2]), probed_distinct=bool(out[3]))

    def close(self):
        if self.handle:
            # jobs and row stores that are still alive are released here (gauss_hip.h, lifetime rule)
            self.lib.gauss_hip_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None


def device_count():
    """HIP devices visible to this process (gauss_hip_device_count; does not create a context)."""
    n = C.c_int()
    check(_lib.load().gauss_hip_device_count(C.byref(n)))
    return n.value


def rank_device(local_rank=None, n_devices=None):
    """The device a rank of a one-process-per-GPU job owns: LOCAL_RANK modulo the visible devices.
    GAUSS_SHARED_DEVICE=1 (a rehearsal of several ranks on one card) maps every rank to device 0."""
    import os
    if os.environ.get("GAUSS_SHARED_DEVICE") == "1" or os.environ.get("GAUSS_BENCH_SHARED_DEVICE") == "1":
        return 0
    if local_rank is None:
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if n_devices is None:
        n_devices = device_count()
    if n_devices < 1:
        raise _lib.GaussHipError("no HIP device is visible: the hot path has no CPU fallback")
    return int(local_rank) % int(n_devices)


def default_context():
    """One context per process, on the device this rank owns (LOCAL_RANK under torchrun, else 0)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(rank_device())
    return _default_ctx


def _pops(pop_off, pop_wgt):
    po = np.ascontiguousarray(pop_off, dtype=np.int32)
    w = None if pop_wgt is None else np.ascontiguousarray(pop_wgt, dtype=np.float64)
    return po, w


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


class _Source:
    """The SNP rows of an LD-only call and the populations of their samples: the converted arrays (kept alive here), the number of
    rows S, and the head of the arguments of a C entry point.  on_dev stands apart: its place differs between the entry points."""

    def __init__(self, store, rows, pop_off, pop_wgt, mode, fmt, pop_src_off):
        """The rows `rows` of a row store: a numpy matrix (host rows; rows None: all of them), a RowStore (resident rows) or a raw
        (device pointer, row stride) pair."""
        self.store, self.rows, self.so = store, _i32(rows), _i32(pop_src_off)
        if isinstance(store, RowStore):
            self.ptr, self.ld, self.on_dev = store.ptr, store.ld, 1
        elif isinstance(store, np.ndarray):
            self.ptr, self.ld, self.on_dev = store.ctypes.data, store.strides[0], 0
        else:
            (self.ptr, self.ld), self.on_dev = store, 1
        self.S = len(self.rows) if self.rows is not None else store.shape[0]
        self.po, self.w = _pops(pop_off, pop_wgt)
        self.mode, self.fmt = int(mode), int(fmt)

    @classmethod
    def matrix(cls, geno, pop_off, pop_wgt, mode):
        """Every row of a byte matrix."""
        return cls(_lib.as_u8(geno), None, pop_off, pop_wgt, mode, _lib.GENO_U8, None)

    def geno_head(self):
        """mode, geno, n_snp, ld, pop_off, pop_wgt, n_pop: the head of an entry point on a byte matrix"""
        return self.mode, self.ptr, self.S, self.ld, self.po.ctypes.data_as(_ip), _lib.ptr(self.w, _dp), len(self.po) - 1

    def rows_head(self):
        """mode, store, ld, geno_format, rows, n_snp, pop_off, pop_src_off, pop_wgt, n_pop: the head of a `_rows` entry point"""
        return (self.mode, self.ptr, self.ld, self.fmt, _lib.ptr(self.rows, _ip), self.S, self.po.ctypes.data_as(_ip), _lib.ptr(self.so, _ip),
                _lib.ptr(self.w, _dp), len(self.po) - 1)


def gram_counts(geno, ctx=None):
    """Exact integer sum_n x_i[n] x_j[n] (util.cpp:62,114 `sumxy`), int64 (S, S)."""
    ctx = ctx or default_context()
    g = _lib.as_u8(geno)
    S, N = g.shape
    out = np.zeros((S, S), dtype=np.int64)
    check(ctx.lib.gauss_gram_counts(ctx.handle, g.ctypes.data, S, N, g.strides[0],
                                    out.ctypes.data_as(C.POINTER(C.c_int64))))
    return out


def ld_matrix(geno, pop_off, pop_wgt=None, mode=MODE_WEIGHTED, diag=1.0, ctx=None):
    """LD matrix among the rows of `geno`.

    mode=MODE_WEIGHTED, diag=1.0  -> computeLD core (computeLD.cpp:95-116)
    mode=MODE_POOLED, diag=1+lambda -> CorG of jepeg (gene.cpp:305-315)
    """
    ctx = ctx or default_context()
    src = _Source.matrix(geno, pop_off, pop_wgt, mode)
    out = np.zeros((src.S, src.S), dtype=np.float64)
    check(ctx.lib.gauss_ld(ctx.handle, *src.geno_head(), float(diag), out.ctypes.data_as(_dp)))
    return out


def ld_per_pop(geno, pop_off, ctx=None):
    """Per-population Pearson r of every SNP pair i < j (prep_zmix5, zmix.cpp:158-176): (P, S(S-1)/2)."""
    ctx = ctx or default_context()
    g = _lib.as_u8(geno)
    po, _ = _pops(pop_off, None)
    S, P = g.shape[0], len(po) - 1
    out = np.zeros((P, S * (S - 1) // 2))
    check(ctx.lib.gauss_ld_per_pop(ctx.handle, g.ctypes.data, S, g.strides[0], po.ctypes.data_as(_ip), P,
                                   out.ctypes.data_as(_dp)))
    return out


def zmix_normal_eq(geno, pop_off, z, pop_group=None, ctx=None):
    """gauss_zmix_normal_eq: normal equations of the zmix regression over every pair i < j of the S genotype rows, row
    [z_i z_j, r_1(i, j) .. r_G(i, j)] (r_g: correlation inside population g, or inside group g of populations pooled when
    pop_group [P] is given), non-finite rows dropped.  Returns (XtX [G, G], Xty [G], yty, n_rows)."""
    ctx = ctx or default_context()
    g = _lib.as_u8(geno)
    po, _ = _pops(pop_off, None)
    S, P = g.shape[0], len(po) - 1
    za = np.ascontiguousarray(z, dtype=np.float64)
    if za.shape != (S,):
        raise ValueError(f"z has shape {za.shape}, expected ({S},)")
    grp = None if pop_group is None else np.ascontiguousarray(pop_group, dtype=np.int32)
    G = P if grp is None else (int(grp.max()) + 1 if grp.size else 0)
    xtx = np.zeros((max(G, 0), max(G, 0)))
    xty = np.zeros(max(G, 0))
    yty = C.c_double()
    n_rows = C.c_int64()
    check(ctx.lib.gauss_zmix_normal_eq(ctx.handle, g.ctypes.data, S, g.strides[0], po.ctypes.data_as(_ip), P,
                                       None if grp is None else grp.ctypes.data_as(_ip), G, za.ctypes.data_as(_dp),
                                       xtx.ctypes.data_as(_dp), xty.ctypes.data_as(_dp), C.byref(yty), C.byref(n_rows)))
    return xtx, xty, yty.value, int(n_rows.value)


def pop_weights(x, interval_off, min_abs_eig=1e-5, ctx=None):
    """gauss_pop_weights: per-interval population weights W_i = MakePosDef(Cxx)^-1 Cxy of an interval-major matrix
    x [S, P + 1] (rows [af1study, AF_0 .. AF_(P-1)]; interval i = rows interval_off[i] .. interval_off[i+1]).
    Returns (w [n_interval, P], status [n_interval] of GAUSS_ST_* bits)."""
    ctx = ctx or default_context()
    xa = np.ascontiguousarray(x, dtype=np.float64)
    off = np.ascontiguousarray(interval_off, dtype=np.int64)
    n_int, P = len(off) - 1, xa.shape[1] - 1
    w = np.zeros((max(n_int, 0), max(P, 0)))
    st = np.zeros(max(n_int, 0), dtype=np.int32)
    check(ctx.lib.gauss_pop_weights(ctx.handle, xa.ctypes.data_as(_dp), off.ctypes.data_as(C.POINTER(C.c_int64)), n_int, P,
                                    float(min_abs_eig), w.ctypes.data_as(_dp), st.ctypes.data_as(_ip)))
    return w, st


def gene_ld_batch(geno, pop_off, gene_off, pop_wgt=None, mode=MODE_POOLED, diag=1.1, ctx=None):
    """LD blocks of all genes in one launch; returns a list of (n_g, n_g) arrays."""
    ctx = ctx or default_context()
    src = _Source.matrix(geno, pop_off, pop_wgt, mode)
    go, out, blocks = _gene_blocks(gene_off)
    check(ctx.lib.gauss_gene_ld_batch(ctx.handle, *src.geno_head(), go.ctypes.data_as(_ip), len(go) - 1, float(diag), out.ctypes.data_as(_dp)))
    return blocks


def _gene_blocks(gene_off):
    """(the int32 gene offsets, the flat output of a gene_ld_batch call, its (n_g, n_g) block of every gene)"""
    go = np.ascontiguousarray(gene_off, dtype=np.int32)
    sizes = np.diff(go).astype(np.int64)
    out = np.zeros(int((sizes * sizes).sum()), dtype=np.float64)
    blocks, o = [], 0
    for n in sizes:
        blocks.append(out[o:o + n * n].reshape(n, n))
        o += n * n
    return go, out, blocks


def ld_matrix_rows(store, rows, pop_off, pop_wgt=None, mode=MODE_WEIGHTED, diag=1.0, fmt=_lib.GENO_2BIT, pop_src_off=None,
                   ctx=None):
    """gauss_ld_rows: the LD matrix of the store rows `rows` (computeLD on a packed / resident panel)."""
    ctx = ctx or default_context()
    len(rows)                                              # (this call names its rows: None raises here, as it always did)
    src = _Source(store, rows, pop_off, pop_wgt, mode, fmt, pop_src_off)
    out = np.zeros((src.S, src.S))
    check(ctx.lib.gauss_ld_rows(ctx.handle, *src.rows_head(), float(diag), src.on_dev, out.ctypes.data_as(_dp)))
    return out


# chi^2 (1 df) of PLINK's --clump-p1 1e-4 and --clump-p2 1e-2 (api.slct_chi2 of them): the default thresholds of a key that is z^2
CLUMP_KEY_INDEX, CLUMP_KEY_MEMBER = 15.136705226623402, 6.634896601021217


def _clump(ctx, src, bp, key, radius, r2_min, key_index, key_member):
    S = src.S
    b = np.ascontiguousarray(bp, dtype=np.int32).reshape(-1)
    k = np.ascontiguousarray(key, dtype=np.float64)
    one = k.ndim == 1
    k = k.reshape(1, -1) if one else k
    if k.ndim != 2 or k.shape[1] != S or b.shape != (S,):
        raise ValueError(f"bp has shape {b.shape} and key {np.shape(key)}: expected ({S},) and ({S},) or (T, {S})")
    T = k.shape[0]
    owner, rank = np.full((T, S), -2, dtype=np.int32), np.full((T, S), -2, dtype=np.int32)
    r2, n = np.zeros((T, S)), np.full(T, -2, dtype=np.int32)
    check(ctx.lib.gauss_ld_clump_rows(ctx.handle, *src.rows_head(), src.on_dev, b.ctypes.data_as(_ip), k.ctypes.data_as(_dp), T, int(radius),
                                      float(r2_min), float(key_index), float(key_member), owner.ctypes.data_as(_ip),
                                      rank.ctypes.data_as(_ip), r2.ctypes.data_as(_dp), n.ctypes.data_as(_ip)))
    if one:
        return dict(owner=owner[0], rank=rank[0], r2=r2[0], n_clumps=int(n[0]))
    return dict(owner=owner, rank=rank, r2=r2, n_clumps=n)


def ld_clump(geno, pop_off, bp, key, pop_wgt=None, mode=MODE_WEIGHTED, radius=250_000, r2_min=0.5, key_index=CLUMP_KEY_INDEX,
             key_member=CLUMP_KEY_MEMBER, ctx=None):
    """gauss_ld_clump_rows on the rows of a byte matrix: LD clumping (PLINK's --clump rule) on the LD that ld_matrix would return,
    which stays on the device.  bp [S] never decreases; key [S] or [T, S], the larger the more significant (z^2: clumping; minor-allele
    frequency with key_index = key_member = 0: LD pruning).  Returns dict(owner, rank, r2, n_clumps): owner[i] the row that leads
    SNP i's clump (-1: none), rank[i] = k where row i leads the k-th clump (else 0), r2[i] the squared LD to the lead (1 for a lead,
    NaN for none).  A 1-D key gives 1-D outputs."""
    return _clump(ctx or default_context(), _Source.matrix(geno, pop_off, pop_wgt, mode), bp, key, radius, r2_min, key_index, key_member)


def ld_clump_rows(store, rows, pop_off, bp, key, pop_wgt=None, mode=MODE_WEIGHTED, radius=250_000, r2_min=0.5,
                  key_index=CLUMP_KEY_INDEX, key_member=CLUMP_KEY_MEMBER, fmt=_lib.GENO_2BIT, pop_src_off=None, ctx=None):
    """ld_clump on the store rows `rows` (a numpy matrix of host rows, a RowStore or a raw device pointer, as ld_matrix_rows)."""
    return _clump(ctx or default_context(), _Source(store, rows, pop_off, pop_wgt, mode, fmt, pop_src_off), bp, key, radius, r2_min,
                  key_index, key_member)


def ldsplit_backtrack(cost, prev, K):
    """The boundaries b_1 < ... < b_K = M of the best K-block split (block k is rows b_{k-1} .. b_k - 1, b_0 = 0), read backwards from
    prev [max_K, M + 1]; None where cost[K - 1] is +inf."""
    if not np.isfinite(cost[K - 1]):
        return None
    b = prev.shape[1] - 1
    ends = np.empty(K, dtype=np.int64)
    for k in range(K, 0, -1):
        ends[k - 1] = b
        b = int(prev[k - 1, b])
    assert b == 0
    return ends


def _split(ctx, src, bp, radius, thr_r2, min_size, max_size, max_K, max_r2):
    S = src.S
    b = np.ascontiguousarray(bp, dtype=np.int32).reshape(-1)
    if b.shape != (S,):
        raise ValueError(f"bp has shape {b.shape}: expected ({S},)")
    K = int(max_K)
    cost, prev = np.full(max(K, 0), np.nan), np.full((max(K, 0), S + 1), -2, dtype=np.int32)
    mx, n = np.full(S + 1, np.nan), np.full(1, -1, dtype=np.int64)
    check(ctx.lib.gauss_ld_split_rows(ctx.handle, *src.rows_head(), src.on_dev, b.ctypes.data_as(_ip), int(radius), float(thr_r2), int(min_size),
                                      int(max_size), K, float(max_r2), cost.ctypes.data_as(_dp), prev.ctypes.data_as(_ip),
                                      mx.ctypes.data_as(_dp), n.ctypes.data_as(C.POINTER(C.c_int64))))
    return dict(cost=cost, prev=prev, max_r2=mx, n_nonfinite=int(n[0]),
                splits={k: ldsplit_backtrack(cost, prev, k) for k in range(1, K + 1)})


def ld_split(geno, pop_off, bp, pop_wgt=None, mode=MODE_WEIGHTED, radius=1 << 32, thr_r2=0.02, min_size=50, max_size=1000,
             max_K=_lib.LDSPLIT_MAX_K, max_r2=0.3, ctx=None):
    """gauss_ld_split_rows on the rows of a byte matrix: the splits of the rows (in position order; bp [S] never decreases) into
    K = 1 .. max_K contiguous blocks of min_size .. max_size rows that minimise the sum of r^2 between blocks, on the LD that
    ld_matrix would return, which stays on the device.  The defaults: a pair below thr_r2 costs nothing, blocks of 50 .. 1 000 rows,
    up to GAUSS_LDSPLIT_MAX_K of them, no pair above max_r2 across a boundary, no distance limit beside max_size.  Returns
    dict(cost [max_K] (+inf: no such split), prev [max_K, S + 1], max_r2 [S + 1], n_nonfinite, splits): splits[K] is the array of
    the K blocks' end rows (exclusive, the last is S), or None.  Which K to use is the caller's choice."""
    return _split(ctx or default_context(), _Source.matrix(geno, pop_off, pop_wgt, mode), bp, radius, thr_r2, min_size, max_size, max_K, max_r2)


def ld_split_rows(store, rows, pop_off, bp, pop_wgt=None, mode=MODE_WEIGHTED, radius=1 << 32, thr_r2=0.02, min_size=50, max_size=1000,
                  max_K=_lib.LDSPLIT_MAX_K, max_r2=0.3, fmt=_lib.GENO_2BIT, pop_src_off=None, ctx=None):
    """ld_split on the store rows `rows` (a numpy matrix of host rows, a RowStore or a raw device pointer, as ld_matrix_rows)."""
    return _split(ctx or default_context(), _Source(store, rows, pop_off, pop_wgt, mode, fmt, pop_src_off), bp, radius, thr_r2, min_size,
                  max_size, max_K, max_r2)


def _hess(ctx, src, z_traits, k_max, eig_min, want_vectors):
    S = src.S
    z = np.ascontiguousarray(z_traits, dtype=np.float64)
    if z.ndim == 1:
        z = z.reshape(1, -1)
    if z.ndim != 2 or z.shape[1] != S:
        raise ValueError(f"z_traits has shape {z.shape}: expected (n_trait, {S})")
    T, K = z.shape[0], int(k_max)
    lam, proj = np.full(S, np.nan), np.full((T, max(K, 0)), np.nan)
    out = np.full(3, -1, dtype=np.int32)                   # n_pos, sweeps, status
    n = np.full(1, -1, dtype=np.int64)
    vec = np.full((S, S), np.nan) if want_vectors else None
    order = np.full(S, -1, dtype=np.int32) if want_vectors else None
    o = out.ctypes.data
    check(ctx.lib.gauss_ld_hess_rows(ctx.handle, *src.rows_head(), src.on_dev, z.ctypes.data_as(_dp), T, K, float(eig_min),
                                     lam.ctypes.data_as(_dp), proj.ctypes.data_as(_dp), C.cast(o, _ip), C.cast(o + 4, _ip),
                                     n.ctypes.data_as(C.POINTER(C.c_int64)), C.cast(o + 8, _ip), _lib.ptr(vec, _dp), _lib.ptr(order, _ip)))
    res = dict(lam=lam, proj=proj, n_pos=int(out[0]), sweeps=int(out[1]), status=int(out[2]), n_nonfinite=int(n[0]))
    if want_vectors:
        res.update(vectors=vec, order=order)
    return res


def ld_hess(geno, pop_off, z_traits, pop_wgt=None, mode=MODE_WEIGHTED, k_max=256, eig_min=1e-6, want_vectors=False, ctx=None):
    """gauss_ld_hess_rows on the rows of a byte matrix: every eigenvalue of the LD that ld_matrix would return (repaired as the header
    states; the matrix stays on the device) and the projections of the traits z_traits [T, S] on its leading eigenvectors.  Returns
    dict(lam [S] descending, proj [T, k_max] = (v_i . z_t) / sqrt(lam_i) for i < min(k_max, n_pos) and NaN beyond, n_pos, sweeps,
    status, n_nonfinite); api.hess_estimates turns lam and proj into h2, covariances and correlations on the host.
    want_vectors=True (for the tests) adds vectors [S, S] (row i = v_i) and order [S] (the solver's column of lam_i)."""
    return _hess(ctx or default_context(), _Source.matrix(geno, pop_off, pop_wgt, mode), z_traits, k_max, eig_min, want_vectors)


def ld_hess_rows(store, rows, pop_off, z_traits, pop_wgt=None, mode=MODE_WEIGHTED, k_max=256, eig_min=1e-6, want_vectors=False,
                 fmt=_lib.GENO_2BIT, pop_src_off=None, ctx=None):
    """ld_hess on the store rows `rows` (a numpy matrix of host rows, a RowStore or a raw device pointer, as ld_matrix_rows)."""
    return _hess(ctx or default_context(), _Source(store, rows, pop_off, pop_wgt, mode, fmt, pop_src_off), z_traits, k_max, eig_min,
                 want_vectors)


def ld_resampled(store, rows, pop_off, draw_pop, draw_sample, n_cols, diag=1.0, fmt=_lib.GENO_2BIT, pop_src_off=None, ctx=None):
    """gauss_ld_resampled_rows: pooled LD (CalCor, n = n_cols) of the store rows `rows` (None: rows 0 .. S-1 of a numpy matrix)
    over the drawn samples -- draw k is sample draw_sample[k] of population draw_pop[k] -- and n_cols - len(draws) zero columns
    (simulateLD)."""
    ctx = ctx or default_context()
    src = _Source(store, rows, pop_off, None, MODE_POOLED, fmt, pop_src_off)
    dp = np.ascontiguousarray(draw_pop, dtype=np.int32).reshape(-1)
    ds = np.ascontiguousarray(draw_sample, dtype=np.int32).reshape(-1)
    if dp.shape != ds.shape:
        raise ValueError(f"draw_pop has {dp.size} entries, draw_sample {ds.size}")
    out = np.zeros((src.S, src.S))
    # (pooled: the entry point takes neither a mode nor weights, so its head is spelled out)
    check(ctx.lib.gauss_ld_resampled_rows(ctx.handle, src.ptr, src.ld, src.fmt, _lib.ptr(src.rows, _ip), src.S, src.po.ctypes.data_as(_ip),
                                          _lib.ptr(src.so, _ip), len(src.po) - 1, dp.ctypes.data_as(_ip), ds.ctypes.data_as(_ip), int(dp.size),
                                          int(n_cols), float(diag), src.on_dev, out.ctypes.data_as(_dp)))
    return out


def gene_ld_batch_rows(store, rows, pop_off, gene_off, pop_wgt=None, mode=MODE_POOLED, diag=1.1, fmt=_lib.GENO_2BIT,
                       pop_src_off=None, ctx=None):
    """gauss_gene_ld_batch_rows: LD blocks of all genes whose SNPs are the store rows `rows`."""
    ctx = ctx or default_context()
    len(rows)                                              # (this call names its rows: None raises here, as it always did)
    src = _Source(store, rows, pop_off, pop_wgt, mode, fmt, pop_src_off)
    go, out, blocks = _gene_blocks(gene_off)
    check(ctx.lib.gauss_gene_ld_batch_rows(ctx.handle, *src.rows_head(), go.ctypes.data_as(_ip), len(go) - 1, float(diag), src.on_dev,
                                           out.ctypes.data_as(_dp)))
    return blocks


def _sumchi2(ctx, src, by_rows, gene_off, z, prune_r2):
    """gauss_gene_sumchi2_rows (by_rows) or gauss_gene_sumchi2 on the rows of src, and the returned dict."""
    S = src.S
    go = np.ascontiguousarray(gene_off, dtype=np.int32)
    za = np.ascontiguousarray(z, dtype=np.float64)
    one = za.ndim == 1
    za = za.reshape(1, -1) if one else za
    if za.ndim != 2 or za.shape[1] != S:
        raise ValueError(f"z has shape {np.shape(z)}: expected ({S},) or (T, {S})")
    T, G = za.shape[0], len(go) - 1
    kept, n_kept = np.full(S, -2, dtype=np.int32), np.full(max(G, 0), -2, dtype=np.int32)
    lam, q = np.zeros((max(G, 0), _lib.SUMCHI2_MAX_KEPT)), np.zeros((T, max(G, 0)))
    top, status, sweeps = np.full((T, max(G, 0)), -2, dtype=np.int32), np.full(max(G, 0), -2, dtype=np.int32), np.full(max(G, 0), -2, dtype=np.int32)
    genes = (go.ctypes.data_as(_ip), G)
    tail = (za.ctypes.data_as(_dp), T, float(prune_r2), kept.ctypes.data_as(_ip), n_kept.ctypes.data_as(_ip), lam.ctypes.data_as(_dp),
            q.ctypes.data_as(_dp), top.ctypes.data_as(_ip), status.ctypes.data_as(_ip), sweeps.ctypes.data_as(_ip))
    if by_rows:
        check(ctx.lib.gauss_gene_sumchi2_rows(ctx.handle, *src.rows_head(), *genes, src.on_dev, *tail))
    else:
        check(ctx.lib.gauss_gene_sumchi2(ctx.handle, *src.geno_head(), *genes, *tail))
    from . import api       # (the p-value is the host library's: gauss_host_sumchi2_pval)
    pval = np.array([[api.sumchi2_pval(lam[g], q[t, g]) if status[g] == 0 else np.nan for g in range(G)] for t in range(T)]).reshape(T, max(G, 0))
    if one:
        q, top, pval = q[0], top[0], pval[0]
    return dict(kept=kept, n_kept=n_kept, lam=lam, q=q, top=top, status=status, sweeps=sweeps, pval=pval)


def gene_sumchi2(geno, pop_off, gene_off, z, pop_wgt=None, mode=MODE_WEIGHTED, prune_r2=0.9, ctx=None):
    """gauss_gene_sumchi2 on the rows of a byte matrix: the gene-based sum-of-chi2 test of every gene (rows gene_off[g] ..
    gene_off[g+1]) on the LD blocks gene_ld_batch(diag=1) would return, which stay on the device.  z [S] or [T, S].  Returns
    dict(kept [S] 0/1, n_kept [G], lam [G, 128] descending with NaN beyond n_kept, q [T, G], top [T, G] (row inside the gene, -1:
    none), status [G], sweeps [G], pval [T, G] from gauss_host_sumchi2_pval; NaN where status is not 0).  A 1-D z gives 1-D q, top
    and pval."""
    return _sumchi2(ctx or default_context(), _Source.matrix(geno, pop_off, pop_wgt, mode), False, gene_off, z, prune_r2)


def gene_sumchi2_rows(store, rows, pop_off, gene_off, z, pop_wgt=None, mode=MODE_WEIGHTED, prune_r2=0.9, fmt=_lib.GENO_2BIT,
                      pop_src_off=None, ctx=None):
    """gene_sumchi2 on the store rows `rows` (a numpy matrix of host rows, a RowStore or a raw device pointer, as
    gene_ld_batch_rows; rows None: rows 0 .. S-1 of a numpy matrix)."""
    return _sumchi2(ctx or default_context(), _Source(store, rows, pop_off, pop_wgt, mode, fmt, pop_src_off), True, gene_off, z, prune_r2)


# lassosum's grid: the default of prs=dict(...)
PRS_S = (0.2, 0.5, 0.9, 1.0)
PRS_LAM = tuple(float(v) for v in np.exp(np.linspace(np.log(0.1), np.log(0.001), 20)))


_F, _I, _NAN = np.float64, np.int32, np.nan
# The riders' output buffers: key -> (dtype, shape, fill of what is not fitted).  A shape names sizes of the window (_Win.sz): M, U,
# T = M + U; k: slct's max; L: susie's effects, t: the further traits fitted, p: their pairs, K: the group's studies; s, l: the prs
# grid; c: 1 + the annotation categories -- each as capped by its rider.  _Win._alloc() makes a table's buffers and binds each to
# out_<prefix>_<key> (_field()); result() returns them as <prefix>_<key>
_OUT = dict(
    slct=dict(n=(_I, "1", 0), idx=(_I, "k", -1), zin=(_F, "k", _NAN), joint=(_F, "k", _NAN), zc=(_F, "M", _NAN), var=(_F, "M", _NAN)),
    cond=dict(z=(_F, "U", _NAN), var=(_F, "U", _NAN)),
    cs=dict(pip=(_F, "T", _NAN), set=(_I, "T", -1), set_pip=(_F, "T", _NAN), size=(_I, "k", 0), mass=(_F, "k", _NAN), lse=(_F, "k", _NAN)),
    susie=dict(pip=(_F, "T", _NAN), set=(_I, "T", -1), set_pip=(_F, "T", _NAN), V=(_F, "L", _NAN), lse=(_F, "L", _NAN), mass=(_F, "L", _NAN),
               purity=(_F, "L", _NAN), size=(_I, "L", 0), kept=(_I, "L", 0), sweeps=(_F, "2", _NAN),
               alpha=(_F, "L T", _NAN), mu=(_F, "L T", _NAN), lbf=(_F, "L T", _NAN)),                  # (want_alpha, want_lbf)
    coloc=dict(pp=(_F, "p L L 5", _NAN), hit=(_I, "p L L", -1), hit_pp=(_F, "p L L", _NAN), n=(_I, "p", 0)),
    xs=dict(V=(_F, "K L", _NAN), purity=(_F, "K L", _NAN), n=(_I, "1", 0), mu=(_F, "K L T", _NAN)),     # (mu: want_mu)
    prs=dict(beta=(_F, "s l M", _NAN), nnz=(_I, "s l", 0), sweeps=(_I, "s l", 0), delta=(_F, "s l", _NAN), br=(_F, "s l", _NAN),
             bg=(_F, "s l", _NAN), kkt=(_F, "s l", _NAN)),
    lds=dict(raw=(_F, "c M", _NAN), l2=(_F, "c M", _NAN), mass=(_F, "c M", _NAN)),
)
# the further traits' fits: susie's buffers with a leading [t], and their status bits
_OUT["susie_more"] = dict({key: (dtype, "t " + shape, fill) for key, (dtype, shape, fill) in _OUT["susie"].items()}, status=(_I, "t", 0))


def _field(prefix, key):
    """The descriptor's name of a buffer: out_<prefix>_<key>, but the further traits' fits and the lbf belong to coloc_* there."""
    if prefix == "susie_more":
        return "out_coloc_more_" + key
    return "out_coloc_lbf" if (prefix, key) == ("susie", "lbf") else f"out_{prefix}_{key}"


def _xs_roles(windows):
    """Per window of a job: None, or (role, K) of a window whose susie dict names a group -- the job's first window of a group is
    its "leader", a later one a "peer"; K is the number of the group's windows (the leader's buffers are sized by it)."""
    groups = [(w.get("susie") or {}).get("group") for w in windows]
    size = {}
    for g in groups:
        if g:
            size[g] = size.get(g, 0) + 1
    roles, led = [], set()
    for g in groups:
        roles.append(("peer" if g in led else "leader", size[g]) if g else None)
        led.add(g)
    return roles


class _Win:
    """Fills the C descriptor of one window and keeps the numpy buffers behind its pointers alive.  `window` is the dict Job
    documents (unknown keys are ignored); xs is the window's (role, K) in a group across studies (_xs_roles)."""

    def __init__(self, desc, window, want_mats=False, xs=None):
        w = window
        self.po, self.w = _pops(w["pop_off"], w.get("pop_wgt"))
        self.z1 = np.ascontiguousarray(w["z1"], dtype=np.float64)
        lam, ldscore = w.get("lam", 0.1), w.get("ldscore")
        M, U = self._geno(desc, w.get("geno_m"), w.get("geno_u"), w.get("dev"), w.get("packed"))
        self.sz = dict(M=M, U=U, T=M + U)
        self.ld_codings = w.get("ld_codings")
        if ldscore is not None and self.ld_codings is None:
            self.ld_codings = _lib.CODE_ADDITIVE            # LD scores ride on an LD window
        if not w.get("want_matrices", True) and ldscore is None:        # (such a window would run and return nothing)
            raise ValueError("want_matrices=False is for an LD window that asks for its LD scores (ldscore=dict(...))")
        ncode = 1
        if self.ld_codings is not None:                     # B21 has one block of rows per coding
            ncode = max(1, bin(int(self.ld_codings)).count("1"))
            want_mats = bool(w.get("want_matrices", True))  # (False: out_b11 = out_b21 = NULL, nothing of the matrices comes back)
        self.z, self.info, self.status = np.zeros(U), np.zeros(U), np.zeros(1, dtype=np.int32)
        self.b11 = np.zeros((M, M)) if want_mats else None
        self.b21 = np.zeros((ncode * U, M)) if want_mats else None
        desc.mode = int(w["mode"])
        desc.n_pop = len(self.po) - 1
        desc.pop_off, desc.pop_wgt = self.po.ctypes.data_as(_ip), _lib.ptr(self.w, _dp)
        desc.z1 = self.z1.ctypes.data_as(_dp)
        desc.lambda_, desc.min_abs_eig = float(lam), float(w.get("min_abs_eig", 1e-5))
        desc.out_z, desc.out_info, desc.out_status = self.z.ctypes.data_as(_dp), self.info.ctypes.data_as(_dp), self.status.ctypes.data_as(_ip)
        desc.out_b11, desc.out_b21 = _lib.ptr(self.b11, _dp), _lib.ptr(self.b21, _dp)
        self.out = {}                                       # prefix -> key -> buffer of the riders asked for (_OUT)
        self.traits = self.miss = self.qcat = None
        if w.get("loo"):
            self._loo(desc)
        if w.get("slct") is not None:
            self._slct(desc, w["slct"], lam)
        if w.get("susie") is not None:
            self._susie(desc, w["susie"], xs)
        if w.get("z_more") is not None or w.get("miss_more") is not None:
            self._traits(desc, w.get("z_more"), w.get("miss_more"))
        if w.get("prs") is not None:
            self._prs(desc, w["prs"])
        if ldscore is not None:
            self._ldscore(desc, ldscore)
        if self.ld_codings is not None:                     # an LD window has no Z-scores, in or out
            desc.kind, desc.u_codings = _lib.WIN_LD, int(self.ld_codings)
            desc.z1 = desc.out_z = desc.out_info = None
        if w.get("qcat") is not None:
            self._qcat(desc, *w["qcat"])

    def _geno(self, desc, geno_m, geno_u, dev, packed):
        """The genotype rows: host matrices, or dev=(ptr_m, ptr_u, M, U, ld); packed=dict(fmt=GENO_*, rows_m=, rows_u=, pop_src_off=)
        makes either the base and stride of a row store whose rows the window names.  Returns M, U."""
        if dev is None:
            self.gm = _lib.as_u8(geno_m)
            self.gu = _lib.as_u8(geno_u) if geno_u is not None and len(geno_u) else np.zeros((0, 1), np.uint8)
            M, U = self.gm.shape[0], self.gu.shape[0]
            desc.geno_m, desc.geno_u, desc.ld = self.gm.ctypes.data, self.gu.ctypes.data, self.gm.strides[0]
            if U and self.gu.strides[0] != desc.ld:
                raise ValueError("geno_m and geno_u must share a row stride")
        else:
            desc.geno_m, desc.geno_u, M, U, desc.ld = dev
        if packed is not None:
            desc.geno_format = int(packed.get("fmt", _lib.GENO_U8))
            self.rows = {key: _i32(packed[key]) for key in ("rows_m", "rows_u", "pop_src_off") if packed.get(key) is not None}
            for key, a in self.rows.items():
                setattr(desc, key, a.ctypes.data_as(_ip))
            if "rows_m" in self.rows:                       # the matrices are row lists into the store
                M, U = len(self.rows["rows_m"]), len(self.rows.get("rows_u", ()))
        desc.n_measured, desc.n_unmeasured = M, U
        return M, U

    def _alloc(self, desc, prefix, skip=(), bind=True):
        """The buffers of _OUT[prefix] but `skip`, each bound to its descriptor field with the pointer type of its dtype."""
        bufs = self.out[prefix] = {}
        for key, (dtype, shape, fill) in _OUT[prefix].items():
            if key not in skip:
                a = bufs[key] = np.full([int(c) if c.isdigit() else self.sz[c] for c in shape.split()], fill, dtype)
                if bind:
                    setattr(desc, _field(prefix, key), a.ctypes.data_as(_ip if dtype is _I else _dp))
        return bufs

    def _loo(self, desc):
        """loo=True: out_loo_* are the rows of one [3, M] block."""
        blk = np.zeros((3, self.sz["M"]))
        self.out["loo"] = dict(z=blk[0], info=blk[1], t=blk[2])
        desc.out_loo_z, desc.out_loo_info, desc.out_loo_t = (blk[k].ctypes.data_as(_dp) for k in range(3))

    def _slct(self, desc, slct, lam):
        """slct=dict(...): slct_*, with unmeasured=True out_cond_*, with cs=dict(...) cs_*; either reads cond_min_var_frac."""
        K, collin = int(slct.get("max", _lib.SLCT_MAX)), float(slct.get("collin", 0.9))
        self.sz["k"] = max(K, 0)
        forced = self.forced = np.ascontiguousarray(slct.get("forced", ()), dtype=np.int32)
        desc.slct_max, desc.slct_chi2_stop = K, float(slct.get("chi2_stop", 0.0))
        desc.slct_min_var_frac = float(slct["min_var_frac"]) if "min_var_frac" in slct else 1.0 - collin / (1.0 + float(lam)) ** 2
        desc.slct_forced, desc.n_slct_forced = _lib.ptr(forced if len(forced) else None, _ip), len(forced)
        self._alloc(desc, "slct")
        cs = slct.get("cs")
        if slct.get("unmeasured") or cs is not None:
            desc.cond_min_var_frac = float(slct["min_var_frac_u"]) if "min_var_frac_u" in slct else 1.0 - collin
        if slct.get("unmeasured"):
            self._alloc(desc, "cond")
        if cs is not None:
            desc.cs_coverage, desc.cs_prior_var = float(cs.get("coverage", 0.95)), float(cs.get("prior_var", 25.0))
            self._alloc(desc, "cs")

    def _susie(self, desc, susie, xs):
        """susie=dict(...): susie_*, with traits=k coloc_traits_more / out_coloc_more_*, with coloc=dict(...) coloc_*; in a group
        xs_*: a leader (a grouped window nobody gave a role leads a group of 2) also fills out_xs_*, a peer has no buffers."""
        role, K = (xs or ("leader", 2)) if susie.get("group") else (None, 0)
        L, k = int(susie.get("L", 10)), int(susie.get("traits", 0))
        desc.susie_L, desc.coloc_traits_more = L, k         # (uncapped: the library does the refusing, only the buffers are capped)
        desc.susie_coverage, desc.susie_prior_var = float(susie.get("coverage", 0.95)), float(susie.get("prior_var", 25.0))
        desc.susie_tol, desc.susie_max_sweeps = float(susie.get("tol", 1e-4)), int(susie.get("max_sweeps", 100))
        desc.susie_min_abs_corr = float(susie.get("min_abs_corr", 0.5))
        desc.susie_estimate_var = 1 if susie.get("estimate_var", True) else 0
        desc.susie_measured_only = 1 if susie.get("measured_only", False) else 0
        if role:
            desc.xs_group = int(susie["group"])
            if susie.get("from_lead") is not None:          # (from a leader it is refused by the library: a leader has no map)
                self.xs_map = _i32(susie["from_lead"])
                desc.xs_from_lead = self.xs_map.ctypes.data_as(_ip)
        if role == "peer":
            return
        t = min(max(k, 0), _lib.SUSIE_TRAITS_MORE_MAX)
        self.sz.update(L=min(max(L, 0), _lib.SUSIE_MAX_L), t=t, p=(t + 1) * t // 2, K=min(max(int(K), 1), _lib.XS_MAX))
        skip = [key for key, want in (("alpha", "want_alpha"), ("mu", "want_alpha"), ("lbf", "want_lbf")) if not susie.get(want)]
        self._alloc(desc, "susie", skip)
        if t:
            self._alloc(desc, "susie_more", skip)
        if susie.get("coloc") is not None:
            co = susie["coloc"]
            desc.coloc_p1, desc.coloc_p2, desc.coloc_p12 = float(co.get("p1", 1e-4)), float(co.get("p2", 1e-4)), float(co.get("p12", 1e-5))
            self._alloc(desc, "coloc", bind=self.sz["p"] > 0)
        if role == "leader":
            self._alloc(desc, "xs", () if susie.get("want_mu") else ("mu",))

    def _traits(self, desc, z_more, miss_more):
        """z_more [T, M]: n_traits_more / z_more / out_z_more [T, U]; miss_more [T, M] beside it: miss_more / out_info_more [T, U] and
        the compact out_z_miss / out_info_miss, one entry per set mask bit."""
        M, U, T = self.sz["M"], self.sz["U"], 0
        if z_more is not None:
            zm = np.ascontiguousarray(z_more, dtype=np.float64)
            if zm.ndim != 2 or zm.shape[1] != M:
                raise ValueError(f"z_more must be [T, {M}] (one row per further trait), got {zm.shape}")
            T = zm.shape[0]
            self.traits = dict(z_more=zm, out=np.zeros((T, U)))
            desc.n_traits_more = T
            desc.z_more, desc.out_z_more = _lib.ptr(zm if T else None, _dp), _lib.ptr(self.traits["out"] if T else None, _dp)
        if miss_more is not None:
            mask = np.ascontiguousarray(np.asarray(miss_more) != 0, dtype=np.uint8)
            if T == 0 or mask.shape != (T, M):
                raise ValueError(f"miss_more must be [{T}, {M}] like z_more, got {mask.shape}")
            n = int(mask.sum())
            self.miss = dict(mask=mask, info_more=np.zeros((T, U)), z=np.zeros(max(n, 1)), info=np.zeros(max(n, 1)))
            desc.miss_more = mask.ctypes.data
            desc.out_info_more = self.miss["info_more"].ctypes.data_as(_dp)
            desc.out_z_miss, desc.out_info_miss = self.miss["z"].ctypes.data_as(_dp), self.miss["info"].ctypes.data_as(_dp)

    def _prs(self, desc, prs):
        """prs=dict(...): prs_*; the whole grid goes into the descriptor, the buffers hold what the library accepts at the most."""
        s = np.ascontiguousarray(PRS_S if prs.get("s") is None else prs["s"], dtype=np.float64).reshape(-1)
        lm = np.ascontiguousarray(PRS_LAM if prs.get("lam") is None else prs["lam"], dtype=np.float64).reshape(-1)
        if len(s) == 0:                                     # (prs_n_s = 0 is the descriptor's "off": the library could not refuse it)
            raise ValueError("prs_n_s = 0: the score takes 1 .. %d shrinkage values" % _lib.PRS_MAX_S)
        self.prs_grid = (s, lm)
        self.sz.update(s=min(len(s), _lib.PRS_MAX_S), l=min(len(lm), _lib.PRS_MAX_LAM))
        desc.prs_n_s, desc.prs_n_lam = len(s), len(lm)
        desc.prs_s, desc.prs_lam = _lib.ptr(s if len(s) else None, _dp), _lib.ptr(lm if len(lm) else None, _dp)
        desc.prs_n, desc.prs_tol, desc.prs_max_sweeps = float(prs.get("n", 0.0)), float(prs.get("tol", 1e-4)), int(prs.get("max_sweeps", 100))
        self._alloc(desc, "prs")

    def _ldscore(self, desc, q):
        """ldscore=dict(...): lds_*; a count of categories outside 0 .. LDS_MAX_ANNOT is the library's to refuse."""
        bm, bu = (None if q.get(key) is None else _i32(q[key]).reshape(-1) for key in ("bp_m", "bp_u"))
        an = np.ascontiguousarray(q["annot"], dtype=np.float64) if q.get("annot") is not None else None
        nc = 0 if an is None else (an.shape[0] if an.ndim == 2 else 1)
        self.lds_in = (bm, bu, an)
        self.sz["c"] = 1 + min(max(nc, 0), _lib.LDS_MAX_ANNOT)
        desc.lds_on, desc.lds_n_annot, desc.lds_radius, desc.lds_n = 1, nc, int(q.get("radius", 0)), float(q.get("n", 0.0))
        desc.lds_bp_m = _lib.ptr(bm if bm is not None and len(bm) else None, _ip)
        desc.lds_bp_u = _lib.ptr(bu if bu is not None and len(bu) else None, _ip)
        desc.lds_annot = _lib.ptr(an if an is not None and an.size else None, _dp)
        self._alloc(desc, "lds")

    def _qcat(self, desc, n_head, n_pred, eig_cutoff):
        """qcat=(n_head, n_pred, eig_cutoff): a QCAT window returns r and num_eig, no Z-scores."""
        self.qcat = (n_head, n_pred, eig_cutoff)
        self.r, self.num_eig = np.zeros(n_pred + self.sz["U"]), np.zeros(1, dtype=np.int32)
        desc.kind = _lib.WIN_QCAT
        desc.n_head_measured, desc.n_pred_measured, desc.eig_cutoff = int(n_head), int(n_pred), float(eig_cutoff)
        desc.out_r, desc.out_num_eig = self.r.ctypes.data_as(_dp), self.num_eig.ctypes.data_as(_ip)
        desc.out_z = desc.out_info = None

    def result(self):
        st = int(self.status[0])
        if self.ld_codings is not None:
            out = dict(b11=self.b11, b21=self.b21, status=st)
            out.update(("lds_" + key, a) for key, a in self.out.get("lds", {}).items())
            return out
        out = dict(z=self.z, info=self.info, status=st) if self.qcat is None else dict(r=self.r, num_eig=int(self.num_eig[0]), status=st)
        if self.b11 is not None:
            out["b11"], out["b21"] = self.b11, self.b21
        if self.qcat is None:
            if self.out:
                self._riders(out)
            if self.traits is not None:
                self._traits_result(out)
        return out

    def _riders(self, out):
        """Every buffer as <prefix>_<key>, then what is not the buffer as it stands."""
        for prefix, bufs in self.out.items():
            for key, a in bufs.items():
                out[f"{prefix}_{key}"] = a
        if "slct" in self.out:                              # per signal: cut to the n found (copies), the buffers under *_raw
            n = out["slct_n"] = int(self.out["slct"]["n"][0])
            for prefix, keys in (("slct", ("idx", "zin", "joint")), ("cs", ("size", "mass", "lse"))):
                bufs = self.out.get(prefix)
                if bufs is not None:
                    out[prefix + "_raw"] = {key: bufs[key] for key in keys}
                    out.update((f"{prefix}_{key}", bufs[key][:n].copy()) for key in keys)
        if "susie" in self.out:                             # sweeps = [sweeps run (NaN: not fitted), last change]
            sw = self.out["susie"]["sweeps"]
            out.update(susie_sweeps=int(sw[0]) if np.isfinite(sw[0]) else 0, susie_delta=float(sw[1]))
            if "susie_more" in self.out:
                sw = self.out["susie_more"]["sweeps"]
                out.update(susie_more_sweeps=np.where(np.isfinite(sw[:, 0]), sw[:, 0], 0).astype(np.int64), susie_more_delta=sw[:, 1].copy())
            if "xs" in self.out:
                out["xs_n"] = int(self.out["xs"]["n"][0])

    def _traits_result(self, out):
        out["z_more"] = self.traits["out"]
        if self.miss is not None:
            # the compact arrays hold one entry per set mask bit in mask order: scattered here, NaN where nothing is missing
            m = self.miss
            at = m["mask"] != 0
            n = int(at.sum())
            out["info_more"] = m["info_more"]
            out["z_miss"], out["info_miss"] = np.full(at.shape, np.nan), np.full(at.shape, np.nan)
            out["z_miss"][at], out["info_miss"][at] = m["z"][:n], m["info"][:n]


def _one_window(ctx, window, want_mats=False):
    """One window on its own: descriptor, buffers, gauss_impute_window, result()."""
    ctx = ctx or default_context()
    desc = WindowDesc()
    win = _Win(desc, window, want_mats)
    check(ctx.lib.gauss_impute_window(ctx.handle, C.byref(desc)))
    return win.result()


def impute_window(mode, geno_m, geno_u, pop_off, pop_wgt, z1, lam=0.1, min_abs_eig=1e-5,
                  want_mats=False, ctx=None, loo=False, slct=None, z_more=None, miss_more=None, susie=None, prs=None):
    """run_dist (mode 0, dist.cpp:129-227) / run_distmix (mode 1, distmix.cpp:138-253).
    loo=True adds loo_z, loo_info, loo_t [M]: every measured SNP re-imputed from the other measured SNPs, and its
    standardised residual (include/gauss_hip.h, out_loo_*).
    slct=dict(max=K, chi2_stop=, collin=0.9, forced=[...]) adds the stepwise conditional signal selection among the measured SNPs
    (include/gauss_hip.h, slct_*): slct_n, slct_idx / slct_zin / slct_joint [n] in order of entry, slct_zc / slct_var [M]; status bit
    8 when a forced SNP failed the collinearity guard.  The guard is "un-ridged r^2 >= collin"; min_var_frac= passes it as it is.
    unmeasured=True in that dict (with min_var_frac_u= to pass their guard as it
    is) adds cond_z / cond_var [U]: the imputed SNPs conditioned on the selected ones (include/gauss_hip.h, out_cond_*).  The ridge
    does not cap what the signals explain of an imputed SNP: their "r^2 >= collin" is 1 - collin, without (1 + lambda)^2.
    cs=dict(coverage=0.95, prior_var=25.0) in that dict adds a credible set for each selected signal (include/gauss_hip.h, out_cs_*):
    cs_pip / cs_set / cs_set_pip [M + U] per candidate, the measured SNPs first, and cs_size / cs_mass / cs_lse [n] per signal.  The
    unmeasured candidates' guard is that of unmeasured=True, whether or not it asks for the conditional columns.
    z_more [T, M] (T <= 63) adds z_more [T, U]: the Z-scores of T further traits measured at the same SNPs, imputed from the same LD
    and the same factorisation (include/gauss_hip.h, n_traits_more); row t is what z would be with z1 = z_more[t].
    miss_more [T, M] (non-zero: further trait t has no score at measured SNP m; at most 32 per trait, 128 distinct per window) makes row t
    what the window returns for trait t alone with those SNPs unmeasured (include/gauss_hip.h, miss_more) and adds info_more [T, U], the
    info per trait, and z_miss / info_miss [T, M]: the imputed Z-scores and the info of the SNPs a trait lacks, NaN elsewhere.
    susie=dict(L=10, coverage=0.95, prior_var=25.0, tol=1e-4, max_sweeps=100, min_abs_corr=0.5, estimate_var=True, measured_only=False)
    adds the multi-causal fine-mapping of the window (include/gauss_hip.h, susie_*): susie_pip / susie_set / susie_set_pip [M + U] per
    candidate, the measured SNPs first, susie_V / susie_lse / susie_size / susie_mass / susie_purity / susie_kept [L] per effect,
    susie_sweeps and susie_delta; want_alpha=True in that dict adds susie_alpha / susie_mu [L, M + U], want_lbf=True susie_lbf.  Status
    bit 16: the sweeps ran out; bit 32: MakePosDef repaired the window, which is then not fitted.
    traits=k in that dict (k <= 7, with z_more of at least k rows and no miss_more) fits the first k rows of z_more in the same launches
    (include/gauss_hip.h, coloc_traits_more): susie_more_* are the susie_* of the further traits with a leading [k], susie_more_status [k]
    their bits 16 / 32.  coloc=dict(p1=1e-4, p2=1e-4, p12=1e-5) beside it colocalises every pair of fitted traits (coloc_*): coloc_pp
    [pairs, L, L, 5] = the posteriors of H0 .. H4 for effect la of the pair's first trait and lb of its second (NaN unless both are
    kept), coloc_hit / coloc_hit_pp [pairs, L, L] the most likely shared candidate (measured first; -1: none) and its share of H4,
    coloc_n [pairs]; pairs in the order (0, 1), (0, 2), .., (k - 1, k), trait 0 being z1.
    prs=dict(n=study sample size, s=[...], lam=[...], tol=1e-4, max_sweeps=100) adds the polygenic score weights of the measured SNPs
    (include/gauss_hip.h, prs_*): lassosum's elastic net on the window's own LD, one warm-started chain over lam per s (defaults: PRS_S,
    PRS_LAM, lassosum's grid).  prs_beta [n_s, n_lam, M], prs_nnz / prs_sweeps / prs_delta / prs_br / prs_bg / prs_kkt [n_s, n_lam]; the
    in-sample predicted R^2 of a cell is prs_br^2 / prs_bg.  Status bit 64: some cell ran its sweeps out."""
    return _one_window(ctx, dict(mode=mode, geno_m=geno_m, geno_u=geno_u, pop_off=pop_off, pop_wgt=pop_wgt, z1=z1, lam=lam,
                                 min_abs_eig=min_abs_eig, loo=loo, slct=slct, z_more=z_more, miss_more=miss_more, susie=susie, prs=prs),
                       want_mats)


def qcat_window(mode, geno_m, geno_u, pop_off, pop_wgt, z1, n_head, n_pred, lam=0.1, eig_cutoff=0.01,
                want_mats=False, ctx=None):
    """run_qcat (mode 0, qcat.cpp:134-262) / run_qcatmix (mode 1, qcatmix.cpp): correlation r between the
    whitened measured Z-scores and the whitened LD column of every tested SNP -- first the n_pred measured
    SNPs that follow the n_head left-wing ones, then the unmeasured SNPs -- plus CountPC's num_eig."""
    return _one_window(ctx, dict(mode=mode, geno_m=geno_m, geno_u=geno_u, pop_off=pop_off, pop_wgt=pop_wgt, z1=z1, lam=lam,
                                 qcat=(n_head, n_pred, eig_cutoff)), want_mats)


def ld_window(mode, geno_m, geno_u, pop_off, pop_wgt, lam=0.0, codings=_lib.CODE_ADDITIVE, ctx=None, ldscore=None, want_matrices=True):
    """Raw LD export (prep_qcat.cpp:104-132, prep_qcatmix.cpp:136-221): B11 among the measured rows
    (diagonal 1 + lam) and B21 of the geno_u rows against them, one block of rows per coding in
    `codings` (additive, dominant, recessive).
    ldscore=dict(radius=bp, bp_m=[M], bp_u=[U], n=sample size, annot=None or [C, M + U]) adds the LD scores of the measured SNPs
    (include/gauss_hip.h, lds_*), reduced on the device: lds_raw / lds_l2 / lds_mass [1 + C, M], row 0 the plain score, row 1 + c
    the score stratified by category c; annot holds the weights of the C annotation categories, the measured SNPs' columns first.
    want_matrices=False passes out_b11 = out_b21 = NULL: b11 / b21 are None and nothing of
    the matrices comes back; without ldscore it is refused (the window would return nothing)."""
    return _one_window(ctx, dict(mode=mode, geno_m=geno_m, geno_u=geno_u, pop_off=pop_off, pop_wgt=pop_wgt, z1=np.zeros(len(geno_m)),
                                 lam=lam, ld_codings=codings, ldscore=ldscore, want_matrices=want_matrices), True)


class PinnedArray:
    """A numpy uint8 matrix in page-locked host memory (gauss_pinned_alloc): uploads from it run at PCIe speed."""

    def __init__(self, shape, ctx=None):
        self.ctx = ctx or default_context()
        n = int(np.prod(shape))
        p = C.c_void_p()
        check(self.ctx.lib.gauss_pinned_alloc(self.ctx.handle, max(n, 1), C.byref(p)))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(n, 1),))[:n].reshape(shape)

    def close(self):
        if self.ptr:
            self.array = None
            self.ctx.lib.gauss_pinned_free(self.ctx.handle, C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RowStore:
    """Genotype rows resident in HBM (gauss_store_upload): a whole packed chromosome is uploaded once and
    windows name their rows by index."""

    @classmethod
    def from_file(cls, path, file_offset, n_rows, ld, ctx=None, reserve_only=False):
        """The rows are a section of a FILE (a packed panel's genotype section): gauss_store_upload_fd, or with reserve_only
        gauss_store_alloc + fill() through gauss_store_fill_fd -- pread straight into the pinned staging buffers."""
        import os
        self = cls.__new__(cls)
        self.ctx = ctx or default_context()
        self.n_rows, self.ld = int(n_rows), int(ld)
        self._host = None
        self._fd, self._file_off = os.open(path, os.O_RDONLY), int(file_offset)
        p = C.c_void_p()
        try:
            if reserve_only:
                check(self.ctx.lib.gauss_store_alloc(self.ctx.handle, self.n_rows * self.ld, C.byref(p)))
            else:
                check(self.ctx.lib.gauss_store_upload_fd(self.ctx.handle, self._fd, C.c_int64(self._file_off), C.c_int64(self.n_rows * self.ld), C.byref(p)))
        except Exception:
            os.close(self._fd)
            raise
        self.ptr = p.value
        return self

    def __init__(self, rows, ctx=None, asynchronous=False, reserve_only=False):
        """asynchronous: gauss_store_upload_async -- the rows travel in the background (keep `rows` alive until
        wait() has returned); wait(n_rows) makes the context's stream wait for the first n_rows rows.
        reserve_only: gauss_store_alloc -- the store is only reserved; fill(r0, r1) brings rows [r0, r1) up (gauss_store_fill)."""
        self.ctx = ctx or default_context()
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        self.n_rows, self.ld = rows.shape
        self._fd = None
        p = C.c_void_p()
        if reserve_only:
            self._host = rows
            check(self.ctx.lib.gauss_store_alloc(self.ctx.handle, rows.nbytes, C.byref(p)))
        elif asynchronous:
            self._host = rows
            check(self.ctx.lib.gauss_store_upload_async(self.ctx.handle, rows.ctypes.data_as(C.c_void_p), rows.nbytes, C.byref(p)))
        else:
            check(self.ctx.lib.gauss_store_upload(self.ctx.handle, rows.ctypes.data_as(C.c_void_p), rows.nbytes, C.byref(p)))
        self.ptr = p.value

    def fill(self, r0, r1):
        """Rows [r0, r1) of a reserve_only store travel now (on a queue of their own); returns when they have landed."""
        if self._fd is not None:
            check(self.ctx.lib.gauss_store_fill_fd(self.ctx.handle, C.c_void_p(self.ptr), self._fd, C.c_int64(self._file_off),
                                                   C.c_int64(int(r0) * self.ld), C.c_int64((int(r1) - int(r0)) * self.ld)))
            return
        check(self.ctx.lib.gauss_store_fill(self.ctx.handle, C.c_void_p(self.ptr), self._host.ctypes.data_as(C.c_void_p),
                                            int(r0) * self.ld, (int(r1) - int(r0)) * self.ld))

    def wait(self, n_rows=0):
        """Rows [0, n_rows) have landed for everything queued on the context afterwards (0: all rows, host waits)."""
        check(self.ctx.lib.gauss_store_wait(self.ctx.handle, C.c_void_p(self.ptr), int(n_rows) * self.ld))

    def close(self):
        if self.ptr:
            self.ctx.lib.gauss_store_free(self.ctx.handle, C.c_void_p(self.ptr))
            self.ptr = None
        if getattr(self, "_fd", None) is not None:
            import os
            os.close(self._fd)
            self._fd = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Job:
    """A batch of windows sharing every launch (gauss_job_*)."""

    def __init__(self, windows, ctx=None, on_device=False, want_mats=False):
        """windows: list of dicts(mode, geno_m, geno_u, pop_off, pop_wgt, z1[, lam, min_abs_eig]) or, with on_device=True, dicts
        carrying dev=(ptr_m, ptr_u, M, U, ld) instead of arrays.  Further keys of a window's dict:
        loo, slct, z_more, miss_more, susie, prs: the riders of impute_window, with the same meaning and the same result keys.
        qcat=(n_head, n_pred, eig_cutoff): a QCAT window (qcat_window).
        ld_codings=mask: an LD window; ldscore=dict(...) makes a window one too and adds its LD scores; want_matrices=False beside
        ldscore (and only beside it): no b11 / b21 come back (ld_window).
        packed=dict(fmt=GENO_*, rows_m=, rows_u=, pop_src_off=): the rows are taken from a row store, optionally 2-bit packed
        (include/gauss_hip.h); dev or geno_m / geno_u give its base pointer and stride.
        susie=dict(L=, ..., group=g[, from_lead=idx]) (g > 0) in two to four windows' dicts: one joint fit across those studies
        (include/gauss_hip.h, xs_group).  The job's first window of a group is its leader: its result carries the joint susie_* in its
        candidate order and xs_V / xs_purity [K, L], xs_n, K being the group's windows (want_mu=True: xs_mu [K, L, T]).  A later one is
        a peer: it passes from_lead=[T_lead] (leader candidate -> its own, -1: absent; None: the same index) and returns z / info
        and no susie_*."""
        self.ctx = ctx or default_context()
        n = len(windows)
        roles = _xs_roles(windows)
        self.descs = (WindowDesc * n)()
        self.wins = [_Win(self.descs[i], w, want_mats, roles[i]) for i, w in enumerate(windows)]
        h = C.c_void_p()
        check(self.ctx.lib.gauss_job_create(self.ctx.handle, self.descs, n, 1 if on_device else 0,
                                            C.byref(h)))
        self.handle = h

    def run(self):
        check(self.ctx.lib.gauss_job_run(self.handle))

    def fetch(self):
        check(self.ctx.lib.gauss_job_fetch(self.handle))
        return [w.result() for w in self.wins]

    def counters(self):
        """gauss_job_counters: this job's own runs -- queued merged / demoted, give-ups repaired inside a fetch, re-runs that failed."""
        out = (C.c_int64 * 4)()
        check(self.ctx.lib.gauss_job_counters(self.handle, out))
        return dict(merged=int(out[0]), demoted=int(out[1]), giveups=int(out[2]), rerun_failed=int(out[3]))

    def profile(self, enable=True):
        check(self.ctx.lib.gauss_job_profile(self.handle, 1 if enable else 0))

    def profile_get(self, kernel=0):
        ms, n = C.c_double(), C.c_int64()
        check(self.ctx.lib.gauss_job_profile_get(self.handle, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def work(self):
        a, b, c, d = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        check(self.ctx.lib.gauss_job_work(self.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(ld_flops=a.value, solve_flops=b.value, bytes=c.value, imputed_snps=d.value)

    def stats(self):
        out = (C.c_double * 4)()
        check(self.ctx.lib.gauss_job_stats(self.handle, out))
        return dict(items=int(out[0]), executed_flops=out[1], slab_bytes=out[2], workspace_bytes=out[3])

    def close(self):
        if self.handle:
            # safe in any order with the context (interpreter shutdown destroys objects in no particular order):
            # gauss_hip_destroy leaves the jobs that outlive it as empty shells, which gauss_job_destroy frees
            self.ctx.lib.gauss_job_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def xs_maps(ids_lead, ids_peer):
    """Leader candidate -> peer candidate for the joint fit across studies: ids_* are the integer SNP ids of a study's candidates in
    its own order (measured first, then unmeasured), each id at most once; -1 where the peer does not have the leader's SNP."""
    ids_lead, ids_peer = np.asarray(ids_lead, dtype=np.int64), np.asarray(ids_peer, dtype=np.int64)
    if len(np.unique(ids_peer)) != len(ids_peer) or len(np.unique(ids_lead)) != len(ids_lead):
        raise ValueError("a study names a SNP id twice")
    order = np.argsort(ids_peer, kind="stable")
    pos = np.searchsorted(ids_peer[order], ids_lead)
    pos = np.minimum(pos, len(ids_peer) - 1)
    hit = ids_peer[order][pos] == ids_lead
    return np.where(hit, order[pos], -1).astype(np.int32)


def fine_map_studies(studies, susie=None, ctx=None, want_mats=False):
    """One joint fit across 2 .. 4 studies of one trait (include/gauss_hip.h, xs_group): every study is a dict of a window's arguments
    (mode, geno_m, geno_u, pop_off, pop_wgt, z1[, lam, min_abs_eig]) plus ids_m / ids_u, the integer SNP ids of its measured and
    unmeasured SNPs.  The first study leads.  Builds the maps from the ids, runs one job and returns the leader's result -- the joint
    susie_* in the leader's candidate order, xs_V / xs_purity [K, L], xs_n -- with ids (the leader's candidates' ids), joint (True
    where the SNP is a candidate of every study) and peers (the other windows' results)."""
    if not 2 <= len(studies) <= _lib.XS_MAX:
        raise ValueError(f"fine_map_studies takes 2 .. {_lib.XS_MAX} studies, got {len(studies)}")
    ids = [np.concatenate([np.asarray(s["ids_m"], dtype=np.int64), np.asarray(s["ids_u"], dtype=np.int64)]) for s in studies]
    wins, joint = [], np.ones(len(ids[0]), dtype=bool)
    for k, s in enumerate(studies):
        w = {key: v for key, v in s.items() if key not in ("ids_m", "ids_u")}
        q = dict(susie or {}, group=1)
        if k:
            q["from_lead"] = xs_maps(ids[0], ids[k])
            joint &= q["from_lead"] >= 0
        w["susie"] = q
        wins.append(w)
    job = Job(wins, ctx=ctx, want_mats=want_mats)
    try:
        job.run()
        res = job.fetch()
    finally:
        job.close()
    out = dict(res[0], ids=ids[0], joint=joint, peers=res[1:])
    return out
