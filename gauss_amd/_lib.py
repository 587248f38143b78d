"""ctypes binding of libgauss_hip.so (include/gauss_hip.h).

There is deliberately no fallback: if the HIP library is missing or fails to load, importing the
numeric entry points raises.  The CPU oracle under ``oracle/`` is test infrastructure and is never
imported from here.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgauss_hip.so")

MODE_POOLED = 0
MODE_WEIGHTED = 1
ST_CLAMPED = 1
ST_NONFINITE = 2
ST_NOCONV = 4
WIN_IMPUTE = 0
WIN_QCAT = 1
WIN_LD = 2
GENO_U8, GENO_2BIT = 0, 1
SLCT_MAX = 32            # GAUSS_SLCT_MAX
TRAITS_MORE_MAX = 63     # GAUSS_TRAITS_MORE_MAX
TRAITS_MISS_MAX = 32     # GAUSS_TRAITS_MISS_MAX
TRAITS_MISS_UNION_MAX = 128   # GAUSS_TRAITS_MISS_UNION_MAX
ST_SLCT_SKIPPED = 8      # GAUSS_ST_SLCT_SKIPPED
ST_SUSIE_NOCONV = 16     # GAUSS_ST_SUSIE_NOCONV
ST_SUSIE_NOFIT = 32      # GAUSS_ST_SUSIE_NOFIT
SUSIE_MAX_L = 32         # GAUSS_SUSIE_MAX_L
SUSIE_MAX_SWEEPS = 1000  # GAUSS_SUSIE_MAX_SWEEPS
SUSIE_TRAITS_MORE_MAX = 7  # GAUSS_SUSIE_TRAITS_MORE_MAX
XS_MAX = 4               # GAUSS_XS_MAX
ST_PRS_NOCONV = 64       # GAUSS_ST_PRS_NOCONV
PRS_MAX_S, PRS_MAX_LAM, PRS_MAX_SWEEPS, PRS_MAX_M = 8, 32, 1000, 4096      # GAUSS_PRS_MAX_*
LDS_MAX_ANNOT, LDS_CHUNK = 32, 64      # GAUSS_LDS_MAX_ANNOT, GAUSS_LDS_CHUNK
CLUMP_MAX_M, CLUMP_MAX_KEYS = 8192, 64  # GAUSS_CLUMP_MAX_M, GAUSS_CLUMP_MAX_KEYS
LDSPLIT_MAX_M, LDSPLIT_MAX_SIZE, LDSPLIT_MAX_K = 8192, 4096, 128      # GAUSS_LDSPLIT_MAX_*
HESS_MAX_M, HESS_MAX_TRAITS, HESS_MAX_K = 4096, 64, 1024      # GAUSS_HESS_MAX_*
ST_HESS_NOCONV = 512     # GAUSS_ST_HESS_NOCONV
SUMCHI2_MAX_N, SUMCHI2_MAX_KEPT, SUMCHI2_MAX_TRAITS = 1024, 128, 64      # GAUSS_SUMCHI2_MAX_*
ST_SUMCHI2_TOOLARGE, ST_SUMCHI2_EMPTY = 128, 256       # GAUSS_ST_SUMCHI2_*
CODE_ADDITIVE, CODE_DOMINANT, CODE_RECESSIVE = 1, 2, 4
GRAM_F32 = 0
GRAM_I8 = 1

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_u8p = C.c_void_p


class WindowDesc(C.Structure):
    _fields_ = [
        ("mode", C.c_int), ("n_pop", C.c_int), ("pop_off", _ip), ("pop_wgt", _dp),
        ("n_measured", C.c_int), ("n_unmeasured", C.c_int),
        ("geno_m", _u8p), ("geno_u", _u8p), ("ld", C.c_int64), ("z1", _dp),
        ("lambda_", C.c_double), ("min_abs_eig", C.c_double),
        ("prs_n_s", C.c_int), ("prs_n_lam", C.c_int), ("prs_s", _dp), ("prs_lam", _dp), ("prs_n", C.c_double), ("prs_tol", C.c_double),
        ("prs_max_sweeps", C.c_int), ("out_prs_beta", _dp), ("out_prs_nnz", _ip), ("out_prs_sweeps", _ip), ("out_prs_delta", _dp),
        ("out_prs_br", _dp), ("out_prs_bg", _dp), ("out_prs_kkt", _dp),
        ("out_z", _dp), ("out_info", _dp), ("out_status", _ip),
        ("lds_on", C.c_int), ("lds_n_annot", C.c_int), ("lds_radius", C.c_int64), ("lds_bp_m", _ip), ("lds_bp_u", _ip), ("lds_n", C.c_double),
        ("lds_annot", _dp), ("out_lds_raw", _dp), ("out_lds_l2", _dp), ("out_lds_mass", _dp),
        ("out_b11", _dp), ("out_b21", _dp),
        ("xs_group", C.c_int), ("xs_from_lead", _ip), ("out_xs_V", _dp), ("out_xs_purity", _dp), ("out_xs_mu", _dp), ("out_xs_n", _ip),
        ("kind", C.c_int), ("n_head_measured", C.c_int), ("n_pred_measured", C.c_int), ("eig_cutoff", C.c_double),
        ("out_r", _dp), ("out_num_eig", _ip),
        ("coloc_traits_more", C.c_int), ("coloc_p1", C.c_double), ("coloc_p2", C.c_double), ("coloc_p12", C.c_double),
        ("out_coloc_lbf", _dp), ("out_coloc_more_pip", _dp), ("out_coloc_more_set", _ip), ("out_coloc_more_set_pip", _dp),
        ("out_coloc_more_V", _dp), ("out_coloc_more_lse", _dp), ("out_coloc_more_mass", _dp), ("out_coloc_more_purity", _dp),
        ("out_coloc_more_size", _ip), ("out_coloc_more_kept", _ip), ("out_coloc_more_alpha", _dp), ("out_coloc_more_mu", _dp),
        ("out_coloc_more_lbf", _dp), ("out_coloc_more_sweeps", _dp), ("out_coloc_more_status", _ip),
        ("out_coloc_pp", _dp), ("out_coloc_hit", _ip), ("out_coloc_hit_pp", _dp), ("out_coloc_n", _ip),
        ("u_codings", C.c_int),
        ("susie_L", C.c_int), ("susie_coverage", C.c_double), ("susie_prior_var", C.c_double), ("susie_tol", C.c_double),
        ("susie_min_abs_corr", C.c_double), ("out_susie_pip", _dp), ("out_susie_set", _ip), ("out_susie_set_pip", _dp),
        ("out_susie_V", _dp), ("out_susie_lse", _dp), ("out_susie_mass", _dp), ("out_susie_purity", _dp),
        ("out_susie_size", _ip), ("out_susie_kept", _ip), ("out_susie_alpha", _dp), ("out_susie_mu", _dp), ("out_susie_sweeps", _dp),
        ("susie_max_sweeps", C.c_int), ("susie_estimate_var", C.c_int), ("susie_measured_only", C.c_int),
        ("geno_format", C.c_int), ("rows_m", _ip), ("rows_u", _ip), ("pop_src_off", _ip),
        ("cs_coverage", C.c_double), ("cs_prior_var", C.c_double), ("out_cs_pip", _dp), ("out_cs_set", _ip), ("out_cs_set_pip", _dp),
        ("out_cs_size", _ip), ("out_cs_mass", _dp), ("out_cs_lse", _dp),
        ("slct_max", C.c_int), ("slct_chi2_stop", C.c_double), ("slct_min_var_frac", C.c_double),
        ("slct_forced", _ip), ("n_slct_forced", C.c_int), ("out_slct_n", _ip), ("out_slct_idx", _ip),
        ("out_slct_zin", _dp), ("out_slct_joint", _dp), ("out_slct_zc", _dp), ("out_slct_var", _dp),
        ("cond_min_var_frac", C.c_double), ("out_cond_z", _dp), ("out_cond_var", _dp),
        ("miss_more", _u8p), ("out_info_more", _dp), ("out_z_miss", _dp), ("out_info_miss", _dp),
        ("n_traits_more", C.c_int), ("z_more", _dp), ("out_z_more", _dp),
        ("out_loo_z", _dp), ("out_loo_info", _dp), ("out_loo_t", _dp),
    ]


class GaussHipError(RuntimeError):
    pass


_lib = None

# every symbol include/gauss_hip.h declares
SYMBOLS = [
    "gauss_hip_init", "gauss_hip_device_count", "gauss_hip_device_of", "gauss_hip_destroy", "gauss_last_error", "gauss_hip_version", "gauss_hip_set_gram_dtype", "gauss_pinned_alloc", "gauss_pinned_free", "gauss_store_upload", "gauss_store_free", "gauss_pack2bit_device", "gauss_ld", "gauss_ld_per_pop", "gauss_ld_per_pop_pairs",
    "gauss_impute_window", "gauss_gene_ld_batch", "gauss_gram_counts", "gauss_job_create",
    "gauss_ld_rows", "gauss_gene_ld_batch_rows", "gauss_job_run", "gauss_job_fetch", "gauss_job_destroy", "gauss_job_span_ms", "gauss_job_profile",
    "gauss_job_profile_get", "gauss_job_work", "gauss_job_stats", "gauss_synth_device",
    "gauss_store_upload_async", "gauss_store_upload_fd_async", "gauss_store_wait", "gauss_store_alloc", "gauss_store_fill", "gauss_store_fill_fd", "gauss_store_upload_fd", "gauss_hip_context_id", "gauss_hip_add_destroy_hook", "gauss_hip_trim_cache", "gauss_hip_source_hash", "gauss_hip_counters", "gauss_job_counters", "gauss_hip_queues",
    "gauss_pop_weights", "gauss_zmix_normal_eq", "gauss_ld_resampled_rows", "gauss_ld_clump_rows", "gauss_ld_split_rows", "gauss_ld_hess_rows",
    "gauss_gene_sumchi2", "gauss_gene_sumchi2_rows",
]


def load():
    """Load libgauss_hip.so; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GaussHipError(
            f"{LIB_PATH} not found: build it with `python -m gauss_amd.build` "
            "(gauss_amd has no CPU fallback by design)")
    lib = C.CDLL(LIB_PATH)
    for name in SYMBOLS:
        if not hasattr(lib, name):
            raise GaussHipError(f"libgauss_hip.so does not export {name}")
    lib.gauss_last_error.restype = C.c_char_p
    lib.gauss_hip_version.restype = C.c_char_p
    lib.gauss_hip_source_hash.restype = C.c_char_p
    lib.gauss_hip_init.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.gauss_hip_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.gauss_hip_device_of.argtypes = [C.c_void_p]
    lib.gauss_hip_destroy.argtypes = [C.c_void_p]
    lib.gauss_hip_destroy.restype = None
    lib.gauss_hip_set_gram_dtype.argtypes = [C.c_void_p, C.c_int]
    lib.gauss_pinned_alloc.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
    lib.gauss_pinned_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.gauss_store_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
    lib.gauss_store_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.gauss_store_upload_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
    lib.gauss_store_wait.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.gauss_store_alloc.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
    lib.gauss_store_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
    lib.gauss_store_fill_fd.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64]
    lib.gauss_store_upload_fd.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]
    lib.gauss_ld.argtypes = [C.c_void_p, C.c_int, _u8p, C.c_int, C.c_int64, _ip, _dp, C.c_int,
                             C.c_double, _dp]
    lib.gauss_pack2bit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, _ip, C.c_int]
    lib.gauss_ld_per_pop.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int64, _ip, C.c_int, _dp]
    lib.gauss_ld_per_pop_pairs.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int64, _ip, C.c_int, _ip, C.c_int, _ip, _ip, C.c_int64, _dp]
    lib.gauss_impute_window.argtypes = [C.c_void_p, C.POINTER(WindowDesc)]
    lib.gauss_gene_ld_batch.argtypes = [C.c_void_p, C.c_int, _u8p, C.c_int, C.c_int64, _ip, _dp,
                                        C.c_int, _ip, C.c_int, C.c_double, _dp]
    lib.gauss_ld_rows.argtypes = [C.c_void_p, C.c_int, _u8p, C.c_int64, C.c_int, _ip, C.c_int, _ip, _ip, _dp, C.c_int, C.c_double,
                                  C.c_int, _dp]
    lib.gauss_gene_ld_batch_rows.argtypes = [C.c_void_p, C.c_int, _u8p, C.c_int64, C.c_int, _ip, C.c_int, _ip, _ip, _dp, C.c_int,
                                             _ip, C.c_int, C.c_double, C.c_int, _dp]
    lib.gauss_gram_counts.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int64,
                                      C.POINTER(C.c_int64)]
    lib.gauss_job_create.argtypes = [C.c_void_p, C.POINTER(WindowDesc), C.c_int, C.c_int,
                                     C.POINTER(C.c_void_p)]
    lib.gauss_job_run.argtypes = [C.c_void_p]
    lib.gauss_job_fetch.argtypes = [C.c_void_p]
    lib.gauss_job_destroy.argtypes = [C.c_void_p]
    lib.gauss_job_destroy.restype = None
    lib.gauss_job_span_ms.argtypes = [C.c_void_p, C.c_void_p, _dp]
    lib.gauss_job_profile.argtypes = [C.c_void_p, C.c_int]
    lib.gauss_job_profile_get.argtypes = [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_int64)]
    lib.gauss_job_counters.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.gauss_job_work.argtypes = [C.c_void_p, _dp, _dp, _dp, C.POINTER(C.c_int64)]
    lib.gauss_job_stats.argtypes = [C.c_void_p, _dp]
    lib.gauss_hip_context_id.argtypes = [C.c_void_p]
    lib.gauss_hip_context_id.restype = C.c_uint64
    lib.gauss_hip_trim_cache.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.gauss_hip_counters.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.gauss_hip_queues.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.gauss_synth_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, _ip, C.c_int,
                                       C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint64]
    lib.gauss_pop_weights.argtypes = [C.c_void_p, _dp, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_double, _dp, _ip]
    lib.gauss_zmix_normal_eq.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int64, _ip, C.c_int, _ip, C.c_int, _dp, _dp, _dp, _dp,
                                         C.POINTER(C.c_int64)]
    lib.gauss_ld_resampled_rows.argtypes = [C.c_void_p, _u8p, C.c_int64, C.c_int, _ip, C.c_int, _ip, _ip, C.c_int, _ip, _ip, C.c_int64,
                                            C.c_int64, C.c_double, C.c_int, _dp]
    lib.gauss_ld_clump_rows.argtypes = [C.c_void_p, C.c_int, _u8p, C.c_int64, C.c_int, _ip, C.c_int, _ip, _ip, _dp, C.c_int, C.c_int, _ip, _dp,
                                        C.c_int, C.c_int64, C.c_double, C.c_double, C.c_double, _ip, _ip, _dp, _ip]
    lib.gauss_ld_split_rows.argtypes = [C.c_void_p, C.c_int, _u8p, C.c_int64, C.c_int, _ip, C.c_int, _ip, _ip, _dp, C.c_int, C.c_int, _ip,
                                        C.c_int64, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, _dp, _ip, _dp, C.POINTER(C.c_int64)]
    lib.gauss_ld_hess_rows.argtypes = [C.c_void_p, C.c_int, _u8p, C.c_int64, C.c_int, _ip, C.c_int, _ip, _ip, _dp, C.c_int, C.c_int, _dp,
                                       C.c_int, C.c_int, C.c_double, _dp, _dp, _ip, _ip, C.POINTER(C.c_int64), _ip, _dp, _ip]
    sc2_tail = [_dp, C.c_int, C.c_double, _ip, _ip, _dp, _dp, _ip, _ip, _ip]      # z, n_trait, prune_r2, then the seven outputs
    lib.gauss_gene_sumchi2.argtypes = lib.gauss_gene_ld_batch.argtypes[:-2] + sc2_tail
    lib.gauss_gene_sumchi2_rows.argtypes = lib.gauss_gene_ld_batch_rows.argtypes[:-3] + [C.c_int] + sc2_tail
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise GaussHipError(f"gauss_hip error {rc}: {load().gauss_last_error().decode()}")


def as_u8(g):
    g = np.ascontiguousarray(g)
    if g.dtype != np.uint8:
        g = g.astype(np.uint8)
    return g


def ptr(a, t):
    return a.ctypes.data_as(t) if a is not None else None
