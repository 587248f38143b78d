"""The reference's R-level entry points, same names and argument lists (R/RcppExports.R:28-104).

    computeLD(chr, start_bp, end_bp, pop_wgt_df, input_file, reference_index_file,
              reference_data_file, reference_pop_desc_file, af1_cutoff=None)
    dist(chr, start_bp, end_bp, wing_size, study_pop, input_file, ...)
    distmix(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_file, ...)
    jepeg(study_pop, input_file, annotation_file, ...)
    jepegmix(pop_wgt_df, input_file, annotation_file, ...)
    afmix(input_file, reference_index_file, ...) / cpw2(...)   population weights from allele frequencies
    simulateLD(chr, start_bp, end_bp, pop_wgt_df, sim_size, input_file, ..., seed=None)   LD of a simulated mixed cohort

Each is a thin ctypes call into libgauss_host.so (C++ host data layer) which delegates the numeric
hot path to libgauss_hip.so (HIP).  A ``pop_wgt_df`` is anything with two columns (population
names, weights): a pandas DataFrame, a dict, or a (names, weights) pair.  Results come back as
pandas DataFrames with the reference's column names; computeLD returns
``{"snplist": DataFrame, "cormat": ndarray}`` like the reference's R list.  Errors the reference
raises with Rcpp::stop surface as ``GaussError`` with the same text.
"""
import ctypes as C
import os

import numpy as np

from . import _lib, hotpath

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "lib", "libgauss_host.so")

KIND_COMPUTELD, KIND_DIST, KIND_DISTMIX, KIND_JEPEG, KIND_JEPEGMIX, KIND_QCAT, KIND_QCATMIX, \
    KIND_PREP_QCAT, KIND_PREP_RECESSIVE, KIND_AFMIX, KIND_CPW2 = range(11)

HOST_SYMBOLS = [
    "gauss_host_last_error", "gauss_table_nrow", "gauss_table_ncol", "gauss_table_colname",
    "gauss_table_coltype", "gauss_table_str", "gauss_table_int", "gauss_table_dbl", "gauss_table_matrix",
    "gauss_table_free", "gauss_table_strcol", "gauss_host_computeLD", "gauss_host_dist", "gauss_host_distmix", "gauss_host_jepeg",
    "gauss_host_jepegmix", "gauss_host_qcat", "gauss_host_qcatmix", "gauss_prepared_qcat_counts",
    "gauss_host_prep_qcat", "gauss_host_prep_recessive_impute", "gauss_host_pack_panel", "gauss_prepared_packed_store", "gauss_host_prep_zmix5", "gauss_host_prep_zmix", "gauss_host_prep_zmix2", "gauss_host_prep_zmix3", "gauss_host_prep_zmix4", "gauss_host_prep_zmix5_sup", "gauss_table_n_named", "gauss_table_named_name",
    "gauss_table_named", "gauss_host_prepare", "gauss_prepared_snps", "gauss_prepared_counts",
    "gauss_prepared_measured_rows", "gauss_prepared_unmeasured_rows", "gauss_prepared_geno_m",
    "gauss_prepared_geno_u", "gauss_prepared_pop_off", "gauss_prepared_pop_wgt", "gauss_prepared_z1",
    "gauss_prepared_gene_off", "gauss_prepared_window_desc", "gauss_prepared_finish", "gauss_prepared_free",
    "gauss_host_bgzf_copy", "gauss_host_set_threads",
    "gauss_host_panel_resident", "gauss_host_panel_evict", "gauss_host_impute_chromosome", "gauss_host_impute_genome", "gauss_host_chrom_window_view", "gauss_host_panel_cache", "gauss_table_n_messages",
    "gauss_table_message", "gauss_table_strcol_fixed", "gauss_host_panel_device_rows", "gauss_prepared_store_rows",
    "gauss_host_jepeg_gene_tail", "gauss_host_plan_cost",
    "gauss_host_jepeg_rank", "gauss_host_jepeg_genome", "gauss_prepared_jepeg_plan", "gauss_prepared_jepeg_finish",
    "gauss_host_afmix", "gauss_host_cpw2", "gauss_host_popwgt_inputs", "gauss_host_zmix", "gauss_host_zmix_qp",
    "gauss_host_simulateLD", "gauss_host_simulate_draws", "gauss_host_clump", "gauss_host_ldsplit", "gauss_host_hess",
    "gauss_host_sumchi2", "gauss_host_sumchi2mix", "gauss_host_sumchi2_pval",
    "gauss_host_dist_loo", "gauss_host_distmix_loo",
    "gauss_host_dist_slct", "gauss_host_distmix_slct", "gauss_host_slct_chi2", "gauss_host_dist_cond", "gauss_host_distmix_cond",
    "gauss_host_dist_cs", "gauss_host_distmix_cs", "gauss_host_dist_susie", "gauss_host_distmix_susie", "gauss_host_dist_prs", "gauss_host_distmix_prs", "gauss_host_dist_ldscore", "gauss_host_distmix_ldscore", "gauss_host_dist_xsusie", "gauss_host_distmix_xsusie", "gauss_host_dist_coloc", "gauss_host_distmix_coloc",
    "gauss_host_dist_traits", "gauss_host_distmix_traits", "gauss_host_dist_traits_miss", "gauss_host_distmix_traits_miss",
]


class ChromStats(C.Structure):
    """gauss_chrom_stats (include/gauss_host.h)"""
    _fields_ = [("n_windows", C.c_int32), ("n_windows_mine", C.c_int32), ("n_skipped", C.c_int32), ("n_failed", C.c_int32),
                ("n_batches", C.c_int32), ("n_merged_giveups", C.c_int32), ("imputed", C.c_int64), ("panel_bytes_uploaded", C.c_int64),
                ("t_total", C.c_double), ("t_plan", C.c_double), ("t_panel_upload", C.c_double), ("t_feeder_wait", C.c_double),
                ("t_job_create", C.c_double), ("t_gpu_wait", C.c_double), ("t_tables", C.c_double), ("gpu_span_ms", C.c_double),
                ("t_tables_tail", C.c_double)]


class GaussError(RuntimeError):
    pass


_host = None
_vp, _cp, _i64, _dbl = C.c_void_p, C.c_char_p, C.c_int64, C.c_double
_strs = C.POINTER(C.c_char_p)
_dp = C.POINTER(C.c_double)


def load_host():
    global _host
    if _host is not None:
        return _host
    _lib.load()       # libgauss_host.so links against libgauss_hip.so: fail loudly if that is missing
    if not os.path.exists(HOST_LIB_PATH):
        raise GaussError(f"{HOST_LIB_PATH} not found: build it with `python -m gauss_amd.build`")
    h = C.CDLL(HOST_LIB_PATH)
    for s in HOST_SYMBOLS:
        if not hasattr(h, s):
            raise GaussError(f"libgauss_host.so does not export {s}")
    h.gauss_host_last_error.restype = _cp
    h.gauss_table_colname.restype = _cp
    h.gauss_table_colname.argtypes = [_vp, C.c_int]
    h.gauss_table_str.restype = _cp
    h.gauss_table_str.argtypes = [_vp, C.c_int, C.c_int]
    h.gauss_table_strcol.restype = C.c_void_p
    h.gauss_table_strcol.argtypes = [_vp, C.c_int, C.POINTER(_i64)]
    h.gauss_table_int.restype = C.POINTER(C.c_int32)
    h.gauss_table_int.argtypes = [_vp, C.c_int]
    h.gauss_table_dbl.restype = _dp
    h.gauss_table_dbl.argtypes = [_vp, C.c_int]
    h.gauss_table_matrix.restype = _dp
    h.gauss_table_matrix.argtypes = [_vp, C.POINTER(C.c_int)]
    for f in ("gauss_table_nrow", "gauss_table_ncol"):
        getattr(h, f).argtypes = [_vp]
    h.gauss_table_coltype.argtypes = [_vp, C.c_int]
    h.gauss_table_free.argtypes = [_vp]
    h.gauss_table_free.restype = None
    files4 = [_cp, _cp, _cp, _cp]
    h.gauss_host_computeLD.argtypes = [_vp, C.c_int, _i64, _i64, _strs, _dp, C.c_int] + files4 + [_dbl, C.POINTER(_vp)]
    h.gauss_host_dist.argtypes = [_vp, C.c_int, _i64, _i64, _i64, _cp] + files4 + [_dbl, C.POINTER(_vp)]
    h.gauss_host_distmix.argtypes = [_vp, C.c_int, _i64, _i64, _i64, _strs, _dp, C.c_int] + files4 + [_dbl, C.POINTER(_vp)]
    h.gauss_host_jepeg.argtypes = [_vp, _cp, _cp] + files4 + [_dbl, C.POINTER(_vp)]
    h.gauss_host_jepegmix.argtypes = [_vp, _strs, _dp, C.c_int, _cp] + files4 + [_dbl, C.POINTER(_vp)]
    h.gauss_host_sumchi2.argtypes = h.gauss_host_jepeg.argtypes[:-1] + [_dbl, C.POINTER(_vp)]            # ..., prune_r2, out
    h.gauss_host_sumchi2mix.argtypes = h.gauss_host_jepegmix.argtypes[:-1] + [_dbl, C.POINTER(_vp)]
    h.gauss_host_sumchi2_pval.argtypes = [_dp, C.c_int, _dbl, _dp, C.POINTER(C.c_int)]
    h.gauss_host_jepeg_rank.argtypes = [_vp, C.c_int, _cp, _strs, _dp, C.c_int, _cp] + files4 + [_dbl, C.c_int, C.c_int, C.POINTER(_vp)]
    h.gauss_host_jepeg_genome.argtypes = [_vp, C.c_int, C.c_int, _cp, _strs, _dp, C.c_int, _strs, _strs, _strs, _strs, _cp, _dbl, C.c_int, C.c_int,
                                          C.POINTER(_vp), C.POINTER(C.c_int32)]
    h.gauss_prepared_jepeg_plan.argtypes = [_vp, C.c_int, C.POINTER(C.c_int32)]
    h.gauss_prepared_jepeg_finish.argtypes = [_vp, C.c_int, C.c_int, _dp, C.POINTER(_vp)]
    h.gauss_host_prep_zmix5.argtypes = [_vp, _cp, _cp, _cp, _cp, _dbl, C.c_int, C.POINTER(_vp)]
    h.gauss_host_prep_zmix5_sup.argtypes = [_vp, _cp, _cp, _cp, _cp, _dbl, C.c_int, C.POINTER(_vp)]
    h.gauss_host_prep_zmix.argtypes = [_vp, _cp, _cp, _cp, _cp, C.c_int, C.POINTER(_vp)]
    for f in (h.gauss_host_prep_zmix2, h.gauss_host_prep_zmix3, h.gauss_host_prep_zmix4):
        f.argtypes = [_vp, _cp, _cp, _cp, _cp, C.c_int, C.c_int, C.POINTER(_vp)]
    h.gauss_host_afmix.argtypes = [_vp, _cp, _cp, _cp, _cp, C.c_int, C.POINTER(_vp)]
    h.gauss_host_cpw2.argtypes = [_vp, _cp, _cp, _cp, _cp, C.c_int, C.POINTER(_vp)]
    h.gauss_host_popwgt_inputs.argtypes = [C.c_int, _cp, _cp, _cp, _cp, C.c_int, C.POINTER(_vp)]
    h.gauss_host_zmix.argtypes = [_vp, _cp, _cp, _cp, _cp, _dbl, C.c_int, C.c_int, C.POINTER(_vp)]
    h.gauss_host_zmix_qp.argtypes = [_dp, _dp, C.c_int, _dp, _dp]
    h.gauss_host_simulateLD.argtypes = [_vp, C.c_int, _i64, _i64, _strs, _dp, C.c_int, _i64] + files4 + [_dbl, _i64, C.POINTER(_vp)]
    h.gauss_host_simulate_draws.argtypes = [_cp, _strs, _dp, C.c_int, _i64, _i64, C.POINTER(_vp)]
    h.gauss_host_pack_panel.restype = _i64
    h.gauss_host_pack_panel.argtypes = [_cp, _cp, _cp, _cp]
    h.gauss_prepared_packed_store.argtypes = [_vp, C.POINTER(C.c_void_p), C.POINTER(_i64), C.POINTER(_i64)]
    h.gauss_host_prep_qcat.argtypes = h.gauss_host_dist.argtypes
    h.gauss_host_prep_recessive_impute.argtypes = h.gauss_host_distmix.argtypes
    h.gauss_table_n_named.argtypes = [_vp]
    h.gauss_table_named_name.restype = _cp
    h.gauss_table_named_name.argtypes = [_vp, C.c_int]
    h.gauss_table_named.restype = _dp
    h.gauss_table_named.argtypes = [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    h.gauss_host_qcat.argtypes = h.gauss_host_dist.argtypes
    h.gauss_host_dist_loo.argtypes = h.gauss_host_dist.argtypes
    h.gauss_host_distmix_loo.argtypes = h.gauss_host_distmix.argtypes
    slct_tail = [_dbl, _dbl, C.c_int, _strs, C.c_int, C.POINTER(_vp)]      # p_cutoff, collin, max_signals, cond_rsids, n_cond, out
    h.gauss_host_dist_slct.argtypes = h.gauss_host_dist.argtypes[:-1] + slct_tail
    h.gauss_host_distmix_slct.argtypes = h.gauss_host_distmix.argtypes[:-1] + slct_tail
    h.gauss_host_slct_chi2.argtypes = [_dbl, _dp]
    h.gauss_host_clump.argtypes = [_vp, C.c_int, _i64, _i64, _strs, _dp, C.c_int] + files4 + [_dbl, _dbl, _dbl, _dbl, _dbl, C.POINTER(_vp)]
    h.gauss_host_ldsplit.argtypes = [_vp, C.c_int, _i64, _i64, _strs, _dp, C.c_int] + files4 + [_dbl, _dbl, C.c_int, C.c_int, C.c_int, _dbl, _dbl,
                                                                                                 C.POINTER(_vp)]
    h.gauss_host_hess.argtypes = [_vp, C.c_int, _i64, _i64, _strs, _dp, C.c_int, _strs, C.c_int, _cp, _cp, _cp, _dbl, C.c_int, _dbl, C.POINTER(_vp)]
    h.gauss_host_dist_cond.argtypes = h.gauss_host_dist_slct.argtypes
    h.gauss_host_distmix_cond.argtypes = h.gauss_host_distmix_slct.argtypes
    h.gauss_host_dist_cs.argtypes = h.gauss_host_dist_slct.argtypes[:-1] + [_dbl, _dbl, C.POINTER(_vp)]      # ..., coverage, prior_var, out
    h.gauss_host_distmix_cs.argtypes = h.gauss_host_distmix_slct.argtypes[:-1] + [_dbl, _dbl, C.POINTER(_vp)]
    susie_tail = [C.c_int, _dbl, _dbl, _dbl, C.c_int, _dbl, C.c_int, C.c_int, C.POINTER(_vp)]      # L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only, out
    h.gauss_host_dist_susie.argtypes = h.gauss_host_dist.argtypes[:-1] + susie_tail
    h.gauss_host_distmix_susie.argtypes = h.gauss_host_distmix.argtypes[:-1] + susie_tail
    prs_tail = [_dbl, C.POINTER(_dbl), C.c_int, C.POINTER(_dbl), C.c_int, _dbl, C.c_int, C.POINTER(_vp)]      # n, s, n_s, lam, n_lam, tol, max_sweeps, out
    h.gauss_host_dist_prs.argtypes = h.gauss_host_dist.argtypes[:-1] + prs_tail
    h.gauss_host_distmix_prs.argtypes = h.gauss_host_distmix.argtypes[:-1] + prs_tail
    h.gauss_host_dist_ldscore.argtypes = h.gauss_host_dist.argtypes[:-1] + [_dbl, C.POINTER(_vp)]      # n, out
    h.gauss_host_distmix_ldscore.argtypes = h.gauss_host_distmix.argtypes[:-1] + [_dbl, C.POINTER(_vp)]
    files_tail = [C.c_char_p, C.c_char_p, C.c_char_p, _dbl]                  # index, data, description, af1_cutoff
    h.gauss_host_dist_xsusie.argtypes = h.gauss_host_dist.argtypes[:5] + [_strs, _strs, C.c_int] + files_tail + susie_tail
    h.gauss_host_distmix_xsusie.argtypes = h.gauss_host_distmix.argtypes[:8] + [_strs, C.c_int] + files_tail + susie_tail
    traits_tail = [_strs, C.c_int, C.POINTER(_vp)]                           # more_input_files, n_more, out
    h.gauss_host_dist_traits.argtypes = h.gauss_host_dist.argtypes[:-1] + traits_tail
    h.gauss_host_distmix_traits.argtypes = h.gauss_host_distmix.argtypes[:-1] + traits_tail
    h.gauss_host_dist_traits_miss.argtypes = h.gauss_host_dist_traits.argtypes
    coloc_tail = traits_tail[:-1] + susie_tail[:-1] + [_dbl, _dbl, _dbl, C.POINTER(_vp)]      # the files, the fit's arguments, p1, p2, p12, out
    h.gauss_host_dist_coloc.argtypes = h.gauss_host_dist.argtypes[:-1] + coloc_tail
    h.gauss_host_distmix_coloc.argtypes = h.gauss_host_distmix.argtypes[:-1] + coloc_tail
    h.gauss_host_distmix_traits_miss.argtypes = h.gauss_host_distmix_traits.argtypes
    h.gauss_host_qcatmix.argtypes = h.gauss_host_distmix.argtypes
    h.gauss_prepared_qcat_counts.argtypes = [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    h.gauss_host_prepare.argtypes = [C.c_int, C.c_int, _i64, _i64, _i64, _cp, _strs, _dp, C.c_int, _cp, _cp, _cp, _cp, _cp,
                                     _dbl, C.POINTER(_vp)]
    h.gauss_prepared_snps.restype = _vp
    h.gauss_prepared_snps.argtypes = [_vp]
    h.gauss_prepared_counts.argtypes = [_vp] + [C.POINTER(C.c_int)] * 5
    for f in ("gauss_prepared_measured_rows", "gauss_prepared_unmeasured_rows", "gauss_prepared_pop_off",
              "gauss_prepared_gene_off"):
        getattr(h, f).restype = C.POINTER(C.c_int32)
        getattr(h, f).argtypes = [_vp]
    for f in ("gauss_prepared_pop_wgt", "gauss_prepared_z1"):
        getattr(h, f).restype = _dp
        getattr(h, f).argtypes = [_vp]
    for f in ("gauss_prepared_geno_m", "gauss_prepared_geno_u"):
        getattr(h, f).restype = C.POINTER(C.c_uint8)
        getattr(h, f).argtypes = [_vp, C.POINTER(_i64)]
    h.gauss_prepared_window_desc.argtypes = [_vp, C.POINTER(_lib.WindowDesc)]
    h.gauss_prepared_finish.argtypes = [_vp, C.POINTER(_vp)]
    h.gauss_prepared_free.argtypes = [_vp]
    h.gauss_prepared_free.restype = None
    h.gauss_host_set_threads.argtypes = [C.c_int]
    h.gauss_host_set_threads.restype = None
    h.gauss_host_bgzf_copy.restype = _i64
    h.gauss_host_bgzf_copy.argtypes = [_cp, _cp]
    h.gauss_host_panel_resident.argtypes = [_vp, _cp, C.POINTER(_i64)]
    h.gauss_host_panel_evict.argtypes = [_vp, _cp]
    h.gauss_host_panel_device_rows.argtypes = [_vp, _cp, C.POINTER(C.c_void_p)]
    ipp = C.POINTER(C.POINTER(C.c_int32))
    h.gauss_prepared_store_rows.argtypes = [_vp, ipp, ipp, ipp, C.POINTER(C.c_int)]
    h.gauss_host_impute_chromosome.argtypes = [_vp, C.c_int, C.c_int, _i64, _i64, _i64, _i64, _cp, _strs, _dp, C.c_int, _cp, _cp, _cp, _cp,
                                               _dbl, C.c_int, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(ChromStats)]
    h.gauss_host_impute_genome.argtypes = [_vp, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(_i64), C.POINTER(_i64), _i64, _i64, _cp, _strs, _dp,
                                           C.c_int, _cp, _cp, _cp, _cp, _dbl, C.c_int, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(ChromStats)]
    h.gauss_host_chrom_window_view.argtypes = [C.c_int, C.c_int, _i64, _i64, _i64, _cp, _strs, _dp, C.c_int, _cp, _cp, _cp, _dbl, C.POINTER(_vp)]
    h.gauss_host_panel_cache.argtypes = [_cp, _cp, _cp, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64)]
    h.gauss_table_n_messages.argtypes = [_vp]
    h.gauss_table_message.restype = _cp
    h.gauss_table_message.argtypes = [_vp, C.c_int]
    h.gauss_table_strcol_fixed.restype = C.c_void_p
    h.gauss_table_strcol_fixed.argtypes = [_vp, C.c_int, C.POINTER(C.c_int)]
    _host = h
    return h


def pack_panel(reference_index_file, reference_data_file, reference_pop_desc_file, out_file):
    """BGZF text panel -> packed panel (gauss_host_pack_panel); returns the number of SNPs.  The packed file is
    then passed as reference_data_file to any entry point."""
    n = load_host().gauss_host_pack_panel(_enc(reference_index_file), _enc(reference_data_file),
                                          _enc(reference_pop_desc_file), _enc(out_file))
    if n < 0:
        raise GaussError(load_host().gauss_host_last_error().decode())
    return int(n)


def set_host_threads(n):
    """Threads used inside one prepare call to inflate/split panel lines (gauss_host_set_threads)."""
    load_host().gauss_host_set_threads(int(n))


def _hcheck(rc):
    if rc != 0:
        raise GaussError(load_host().gauss_host_last_error().decode())


def _enc(s):
    return None if s is None else os.fspath(s).encode()


def _pop_wgt(pop_wgt_df):
    """(names, weights) from a DataFrame / dict / pair; first column names, second weights."""
    if hasattr(pop_wgt_df, "iloc"):
        names, w = list(pop_wgt_df.iloc[:, 0]), list(pop_wgt_df.iloc[:, 1])
    elif isinstance(pop_wgt_df, dict):
        names, w = list(pop_wgt_df.keys()), list(pop_wgt_df.values())
    else:
        names, w = list(pop_wgt_df[0]), list(pop_wgt_df[1])
    arr = (C.c_char_p * len(names))(*[str(n).encode() for n in names])
    wv = np.ascontiguousarray(w, dtype=np.float64)
    return arr, wv, len(names)


def _table(h, t, free=True):
    """gauss_table -> pandas DataFrame (or dict of columns when pandas is unavailable)."""
    cols = {}
    n = h.gauss_table_nrow(t)
    for c in range(h.gauss_table_ncol(t)):
        name = h.gauss_table_colname(t, c).decode()
        ty = h.gauss_table_coltype(t, c)
        if ty == 0:
            nb = _i64()
            buf = h.gauss_table_strcol(t, c, C.byref(nb))       # one call per column, not one per cell
            cols[name] = C.string_at(buf, nb.value).decode().split("\0")[:n] if (n and buf) else []
        elif ty == 1:
            cols[name] = np.ctypeslib.as_array(h.gauss_table_int(t, c), shape=(n,)).copy() if n else np.zeros(0, np.int32)
        else:
            cols[name] = np.ctypeslib.as_array(h.gauss_table_dbl(t, c), shape=(n,)).copy() if n else np.zeros(0)
    nn = C.c_int()
    mp = h.gauss_table_matrix(t, C.byref(nn))
    mat = np.ctypeslib.as_array(mp, shape=(nn.value, nn.value)).copy() if mp else None
    if free:
        h.gauss_table_free(t)
    try:
        import pandas as pd
        df = pd.DataFrame(cols)
    except ImportError:       # pragma: no cover
        df = cols
    return df, mat


def _af(af1_cutoff):
    return float("nan") if af1_cutoff is None else float(af1_cutoff)


def _ctx(ctx):
    return (ctx or hotpath.default_context()).handle


def computeLD(chr, start_bp, end_bp, pop_wgt_df, input_file, reference_index_file, reference_data_file,
              reference_pop_desc_file, af1_cutoff=None, ctx=None):
    h = load_host()
    names, w, n = _pop_wgt(pop_wgt_df)
    out = _vp()
    _hcheck(h.gauss_host_computeLD(_ctx(ctx), int(chr), int(start_bp), int(end_bp), names, w.ctypes.data_as(_dp), n,
                                   _enc(input_file), _enc(reference_index_file), _enc(reference_data_file),
                                   _enc(reference_pop_desc_file), _af(af1_cutoff), C.byref(out)))
    df, mat = _table(h, out)
    return {"snplist": df, "cormat": mat}


def _seed(seed):
    return -1 if seed is None else int(seed)


def _draws(named):
    d = np.asarray(named["draws"]).reshape(-1, 2) if named["draws"].size else np.zeros((0, 2))
    counts = named["counts"].reshape(-1).astype(np.int64)
    return dict(draws=d.astype(np.int64), counts=counts, seed=int(named["seed"].reshape(-1)[0]), n_drawn=int(counts.sum()))


def simulateLD(chr, start_bp, end_bp, pop_wgt_df, sim_size, input_file, reference_index_file, reference_data_file,
               reference_pop_desc_file, af1_cutoff=None, seed=None, ctx=None, detail=False):
    """simulateLD() of the reference (simulateLD.cpp:34-252): the LD of sim_size subjects drawn with replacement from the panel's
    populations, (int)(weight * sim_size) from each population of pop_wgt_df (panel order), the rest of the columns zero.  The SNPs
    and ``snplist`` are computeLD's.  seed: an integer in [0, 2**32) replays a call exactly; None (or -1) draws one from
    std::random_device as the reference does, and the seed used is in the detail.  Returns ``{"snplist", "cormat"}``; with
    detail=True also ``draws`` [n_drawn, 2] (index into the weighted populations in panel order, sample), ``counts``, ``seed`` and
    ``n_drawn``."""
    h = load_host()
    names, w, n = _pop_wgt(pop_wgt_df)
    out = _vp()
    _hcheck(h.gauss_host_simulateLD(_ctx(ctx), int(chr), int(start_bp), int(end_bp), names, w.ctypes.data_as(_dp), n, int(sim_size),
                                    _enc(input_file), _enc(reference_index_file), _enc(reference_data_file),
                                    _enc(reference_pop_desc_file), _af(af1_cutoff), _seed(seed), C.byref(out)))
    named = _named(h, out)
    df, mat = _table(h, out)
    res = {"snplist": df, "cormat": mat}
    if detail:
        res.update(_draws(named))
    return res


def clump(chr, start_bp, end_bp, pop_wgt_df, input_file, reference_index_file, reference_data_file, reference_pop_desc_file,
          p1=1e-4, p2=1e-2, r2=0.5, kb=250, af1_cutoff=None, ctx=None):
    """LD clumping (PLINK's --clump, whose defaults these are) of a region of a mixed-ancestry study on the ancestry-weighted LD of
    computeLD, on the GPU (gauss_host_clump): the SNPs are computeLD's for the same arguments; a SNP with p < p1 that no more
    significant index has claimed leads a clump and takes every unclaimed SNP within kb with p < p2 and squared LD >= r2.  Returns the
    frame rsid chr bp a1 a2 af1mix z pval clump index_rsid r2 (clump: rank of the SNP's clump, 0 for none); ``attrs["clumps"]`` is a
    frame with one row per clump: index_row, size, bp_first, bp_last.  One region of at most 8 192 SNPs per call; clumps are cut at
    the region's edges.  To clump imputed SNPs, write the imputed table out as the study file; pval takes its z at face value."""
    h = load_host()
    names, w, n = _pop_wgt(pop_wgt_df)
    out = _vp()
    _hcheck(h.gauss_host_clump(_ctx(ctx), int(chr), int(start_bp), int(end_bp), names, w.ctypes.data_as(_dp), n, _enc(input_file),
                               _enc(reference_index_file), _enc(reference_data_file), _enc(reference_pop_desc_file), _af(af1_cutoff),
                               float(p1), float(p2), float(r2), float(kb), C.byref(out)))
    named = _named(h, out)
    df, _ = _table(h, out)
    cm = np.asarray(named["clumps"]).reshape(-1, 4).astype(np.int64)
    import pandas as pd       # (the frame's attrs carry the clumps: this call needs pandas)
    df.attrs["clumps"] = pd.DataFrame(dict(index_row=cm[:, 0], size=cm[:, 1], bp_first=cm[:, 2], bp_last=cm[:, 3]))
    return df


def ldsplit(chr, start_bp, end_bp, pop_wgt_df, input_file, reference_index_file, reference_data_file, reference_pop_desc_file,
            thr_r2=0.02, min_size=50, max_size=1000, max_K=128, max_r2=0.3, kb=None, af1_cutoff=None, ctx=None):
    """Approximately independent LD blocks of a region of a mixed-ancestry study, on the ancestry-weighted LD of computeLD, on the GPU
    (gauss_host_ldsplit): the splits of the region's SNPs (computeLD's for the same arguments, in position order) into K = 1 .. max_K
    contiguous blocks of min_size .. max_size SNPs that minimise the sum of r^2 over the pairs in different blocks.  A pair with r^2
    below thr_r2, or further apart than kb (None: no limit), costs nothing; no pair with r^2 above max_r2 ends in two blocks (1: off).
    Returns a frame with one row per K that has a split: n_block, cost, perc_kept (sum of size^2 / M^2: the share of the LD matrix
    that the blocks keep), cost2 (sum of size^2), max_size_used.  ``attrs["snps"]``: computeLD's snplist frame; ``attrs["last"]``:
    per row, the snplist row of every block's last SNP; ``attrs["max_r2_at"]`` [M + 1]: the largest r^2 cut by a boundary before SNP b;
    ``attrs["n_nonfinite"]``: LD entries in the band that are not finite (counted as 0).  Which K to use is the caller's choice (a
    small cost at a small cost2; bigsnpr's guide plots one against the other); ldsplit_blocks() turns a row into blocks.  One region
    of at most 8 192 SNPs per call, blocks of at most 4 096, at most 128 of them; sizes in SNPs.  The result is held to the rule of
    include/gauss_hip.h and its numpy statement (tests/ldsplit_ref.py), not to bigsnpr's snp_ldsplit output.  min_size, max_size and
    max_K are taken as given: 0 is refused here (the C call reads 0 as "not given")."""
    for name, v in (("min_size", min_size), ("max_size", max_size), ("max_K", max_K)):
        if int(v) < 1:
            raise GaussError(f"ldsplit: {name} = {int(v)}; it must be at least 1")
    h = load_host()
    names, w, n = _pop_wgt(pop_wgt_df)
    out = _vp()
    _hcheck(h.gauss_host_ldsplit(_ctx(ctx), int(chr), int(start_bp), int(end_bp), names, w.ctypes.data_as(_dp), n, _enc(input_file),
                                 _enc(reference_index_file), _enc(reference_data_file), _enc(reference_pop_desc_file), _af(af1_cutoff),
                                 float(thr_r2), int(min_size), int(max_size), int(max_K), float(max_r2),
                                 float("nan") if kb is None else float(kb), C.byref(out)))
    named = _named(h, out)
    snps, _ = _table(h, out)
    import pandas as pd       # (the frame's attrs carry the SNPs and the splits: this call needs pandas)
    sp = np.asarray(named["splits"]).reshape(-1, 5)
    last = np.asarray(named["last"]).reshape(len(sp), -1).astype(np.int64) if len(sp) else np.zeros((0, 0), dtype=np.int64)
    df = pd.DataFrame(dict(n_block=sp[:, 0].astype(np.int64), cost=sp[:, 1], perc_kept=sp[:, 2], cost2=sp[:, 3].astype(np.int64),
                           max_size_used=sp[:, 4].astype(np.int64)))
    df.attrs["snps"] = snps
    df.attrs["last"] = [last[r, :int(sp[r, 0])].copy() for r in range(len(sp))]
    df.attrs["max_r2_at"] = np.asarray(named["max_r2_at"]).reshape(-1)
    df.attrs["n_nonfinite"] = int(np.asarray(named["n_nonfinite"]).reshape(-1)[0])
    return df


def ldsplit_blocks(res, K):
    """The K blocks of an ldsplit() result as a frame, one row per block: block (from 1), first_row, last_row (snplist rows, inclusive),
    size, first_rsid, last_rsid, start_bp, end_bp.  Consecutive blocks tile the region with no gap and no overlap: a block ends at
    the midpoint between its last SNP and the next block's first (end_bp, inclusive; the next block's start_bp is end_bp + 1); the
    first block starts at the first SNP, the last ends at the last SNP.  Loop a per-window call (distmix_susie, distmix_prs, clump)
    over the rows' start_bp .. end_bp.  K must be one of res.n_block.  Refused: a split with a boundary between two SNPs at one
    position -- no bp range can tell them apart, and a call over start_bp .. end_bp would hand the second SNP to the earlier block;
    take another K, or work by first_row .. last_row of ``res.attrs["last"]``."""
    import pandas as pd
    rows = np.flatnonzero(res["n_block"].to_numpy() == int(K))
    if len(rows) != 1:
        raise GaussError(f"ldsplit_blocks: the result holds no split into {K} blocks (it has {list(res['n_block'])})")
    snps = res.attrs["snps"]
    last = np.asarray(res.attrs["last"][int(rows[0])], dtype=np.int64)
    first = np.concatenate([[0], last[:-1] + 1])
    bp = snps["bp"].to_numpy().astype(np.int64)
    rsid = list(snps["rsid"])
    tied = np.flatnonzero(bp[last[:-1]] == bp[first[1:]])
    if len(tied):
        k = int(tied[0])
        raise GaussError(f"ldsplit_blocks: the boundary between blocks {k + 1} and {k + 2} of the split into {K} lies between two SNPs at bp "
                         f"{int(bp[last[k]])} ({rsid[last[k]]}, {rsid[first[k + 1]]}): no bp range separates them")
    end_bp = np.concatenate([(bp[last[:-1]] + bp[first[1:]]) // 2, bp[-1:]])
    start_bp = np.concatenate([bp[:1], end_bp[:-1] + 1])
    return pd.DataFrame(dict(block=np.arange(1, len(last) + 1), first_row=first, last_row=last, size=last - first + 1,
                             first_rsid=[rsid[i] for i in first], last_rsid=[rsid[i] for i in last], start_bp=start_bp, end_bp=end_bp))


def hess(chr, start_bp, end_bp, pop_wgt_df, input_files, reference_index_file, reference_data_file, reference_pop_desc_file, n,
         k=None, var_frac=0.99, k_max=256, eig_min=1e-6, overlap=None, af1_cutoff=None, ctx=None):
    """Local heritability of one or more traits in an LD block of a mixed-ancestry study, and the local genetic covariance and
    correlation of every pair of them (the statistics of HESS, rho-HESS and LAVA), on the ancestry-weighted LD of computeLD, which
    stays on the GPU (gauss_host_hess): input_files names one study file per trait; the SNPs are computeLD's for the first file and
    the same arguments, every further file must hold them all (swapped alleles flip the sign).  n: the traits' sample sizes (one
    number, or one per file).  The block's LD is decomposed on the GPU (gauss_ld_hess_rows: all eigenvalues, the projections of every
    trait on the first k_max eigenvectors); the estimators are hess_estimates' at the caller's k -- an integer, or the smallest k whose
    eigenvalues hold var_frac of the trace (LAVA's 0.99) -- capped at min(k_max, n_pos); eig_min and overlap as hess_estimates.
    Returns a frame with one row per trait: trait n k H h2 se n_snp n_pos var_kept.  attrs: pairs (a frame, one row per a < b: a b C
    cov rg s), lam [M], curve [T, k_max] (H_t at every k: how the estimate moves with k), var_curve [k_max], snps (computeLD's snplist
    frame), z [M, T], n_nonfinite, sweeps, status.  One block of at most 4 096 SNPs, 64 traits and k_max <= 1 024 per call: cut a
    region with ldsplit() and ldsplit_blocks() first.  h2 is not bounded to [0, 1] and se is HESS's approximation; the values are held
    to the rule of include/gauss_hip.h and the numpy statements of tests/hess_ref.py, not to the output of HESS, rho-HESS or LAVA."""
    files = [os.fsencode(f) for f in input_files]
    if not files:
        raise ValueError("input_files: at least one study file")
    if int(k_max) < 1:
        raise GaussError(f"hess: k_max = {int(k_max)}; it must be at least 1")
    h = load_host()
    names, w, n_w = _pop_wgt(pop_wgt_df)
    out = _vp()
    _hcheck(h.gauss_host_hess(_ctx(ctx), int(chr), int(start_bp), int(end_bp), names, w.ctypes.data_as(_dp), n_w, (C.c_char_p * len(files))(*files),
                              len(files), _enc(reference_index_file), _enc(reference_data_file), _enc(reference_pop_desc_file), _af(af1_cutoff),
                              int(k_max), float(eig_min), C.byref(out)))
    named = _named(h, out)
    snps, _ = _table(h, out)
    import pandas as pd       # (the frame's attrs carry the pairs and the SNPs: this call needs pandas)
    T = len(files)
    lam = np.asarray(named["lam"]).reshape(-1)
    proj = np.asarray(named["proj"]).reshape(T, -1)
    solve = np.asarray(named["solve"]).reshape(-1)
    est = hess_estimates(lam, proj, n, k=k, var_frac=var_frac, overlap=overlap, eig_min=eig_min)
    nn = np.broadcast_to(np.asarray(n, dtype=np.float64).reshape(-1), (T,))
    df = pd.DataFrame(dict(trait=np.arange(1, T + 1), n=nn, k=est["k"], H=est["H"], h2=est["h2"], se=est["se"], n_snp=len(lam),
                           n_pos=int(solve[0]), var_kept=est["var_kept"]))
    pr = est["pairs"]
    df.attrs.update(pairs=pd.DataFrame(dict(a=pr["a"] + 1, b=pr["b"] + 1, C=pr["C"], cov=pr["cov"], rg=pr["rg"], s=pr["s"])), lam=lam,
                    curve=est["curve"], var_curve=est["var_curve"], snps=snps, z=np.asarray(named["z"]).reshape(len(lam), T),
                    n_nonfinite=int(solve[2]), sweeps=int(solve[1]), status=int(solve[3]))
    return df


def hess_n_pos(lam, eig_min=1e-6):
    """The number of eigenvalues a hess call projects on: lam_i > eig_min * lam_0 and lam_i > 0 (lam descending; 0 if one is not finite)."""
    l = np.asarray(lam, dtype=np.float64).reshape(-1)
    if not len(l) or not np.all(np.isfinite(l)):
        return 0
    return int(np.sum((l > float(eig_min) * l[0]) & (l > 0.0)))


def hess_estimates(lam, proj, n, k=None, var_frac=0.99, overlap=None, eig_min=1e-6):
    """The host arithmetic of hess() alone (no GPU): local heritability of each trait and genetic covariance / correlation of each pair
    of traits from the eigenvalues lam [M] (descending) and the projections proj [T, k_max] that hotpath.ld_hess returns.  With p = proj,
        H_t(k) = sum_{i<k} p[t,i]^2,  C_ab(k) = sum_{i<k} p[a,i] p[b,i]      (ascending i, plain fp64 adds)
        h2_t   = (H_t(k) - k) / (n_t - k)
        se_t^2 = (n_t / (n_t - k))^2 (2 k (1 - h2_t) / n_t + 4 h2_t) (1 - h2_t) / n_t
        cov_ab = (C_ab(k) - k s_ab) / sqrt(n_a n_b),  rg_ab = cov_ab / sqrt(h2_a h2_b) (NaN unless both h2 > 0)
    n: the traits' sample sizes (one number for all, or one per trait).  k: an integer, or (k=None) the smallest k whose share
    sum_{i<k} lam / sum lam of the variance reaches var_frac (LAVA's 0.99); both are capped at min(k_max, n_pos), n_pos counted as
    hess_n_pos does.  overlap: s_ab, the pair's intercept n_s rho_pheno / sqrt(n_a n_b) (None: 0; one number, or a [T, T] matrix).
    Every product is of two projections on the same eigenvector, so no value depends on the eigenvectors' signs.  Returns dict(k, H, h2,
    se [T], var_kept, n_pos, curve [T, k_max] (H_t at every k; NaN beyond the cap), var_curve [k_max], pairs: dict(a, b, C, s, cov, rg)
    with one entry per a < b).  k = 0 (no positive eigenvalue): H = 0 and NaN estimates."""
    l = np.asarray(lam, dtype=np.float64)
    p = np.asarray(proj, dtype=np.float64)
    if l.ndim != 1 or not len(l):
        raise GaussError(f"hess_estimates: lam has shape {l.shape}; expected (M,) with M >= 1")
    if p.ndim != 2 or p.shape[0] < 1 or p.shape[1] < 1:
        raise GaussError(f"hess_estimates: proj has shape {p.shape}; expected (T, k_max)")
    T, k_max = p.shape
    if np.any(l[1:] > l[:-1]):
        raise GaussError("hess_estimates: lam is not in descending order")
    nn = np.asarray(n, dtype=np.float64).reshape(-1)
    if len(nn) == 1:
        nn = np.repeat(nn, T)
    if len(nn) != T:
        raise GaussError(f"hess_estimates: n has {len(nn)} entries for {T} traits")
    if not np.all(np.isfinite(nn)) or np.any(nn <= 0):
        raise GaussError("hess_estimates: every n must be positive and finite")
    if not (0.0 <= float(eig_min) < 1.0):
        raise GaussError(f"hess_estimates: eig_min = {eig_min} is outside [0, 1)")
    n_pos = hess_n_pos(l, eig_min)
    cap = min(k_max, n_pos)
    tot = np.cumsum(l)[-1]
    var_curve = np.cumsum(l[:k_max]) / tot if tot > 0 else np.full(min(k_max, len(l)), np.nan)
    if k is not None:
        if int(k) != k or int(k) < 1:
            raise GaussError(f"hess_estimates: k = {k}; it must be a whole number of at least 1")
        kk = min(int(k), cap)
    else:
        if not (0.0 < float(var_frac) <= 1.0):
            raise GaussError(f"hess_estimates: var_frac = {var_frac} is outside (0, 1]")
        hit = np.flatnonzero(var_curve[:cap] >= float(var_frac))
        kk = int(hit[0]) + 1 if len(hit) else cap
    if np.any(nn <= kk):
        raise GaussError(f"hess_estimates: n = {nn.min():g} is not above k = {kk}; the estimator needs n > k")
    if overlap is None:
        s = np.zeros((T, T))
    else:
        s = np.asarray(overlap, dtype=np.float64)
        if s.ndim == 0:
            s = np.full((T, T), float(s))
        if s.shape != (T, T) or not np.all(np.isfinite(s)):
            raise GaussError(f"hess_estimates: overlap has shape {s.shape}; expected one finite number or a finite ({T}, {T}) matrix")
    curve = np.cumsum(p * p, axis=1)
    curve[:, cap:] = np.nan
    nan = np.full(T, np.nan)
    if kk == 0:
        H, h2, se = np.zeros(T), nan.copy(), nan.copy()
    else:
        H = curve[:, kk - 1].copy()
        h2 = (H - kk) / (nn - kk)
        se2 = (nn / (nn - kk)) ** 2 * (2.0 * kk * (1.0 - h2) / nn + 4.0 * h2) * (1.0 - h2) / nn
        se = np.sqrt(np.where(se2 >= 0, se2, np.nan))
    ia, ib = np.triu_indices(T, 1)
    if kk == 0:
        Cab = np.zeros(len(ia))
        cov = rg = np.full(len(ia), np.nan)
    else:
        Cab = np.cumsum(p[ia, :kk] * p[ib, :kk], axis=1)[:, -1] if len(ia) else np.zeros(0)
        cov = (Cab - kk * s[ia, ib]) / np.sqrt(nn[ia] * nn[ib])
        ok = (h2[ia] > 0) & (h2[ib] > 0)
        rg = np.where(ok, cov / np.sqrt(np.where(ok, h2[ia] * h2[ib], 1.0)), np.nan)
    return dict(k=kk, H=H, h2=h2, se=se, var_kept=float(var_curve[kk - 1]) if kk else 0.0, n_pos=n_pos, curve=curve, var_curve=var_curve,
                pairs=dict(a=ia, b=ib, C=Cab, s=s[ia, ib], cov=cov, rg=rg))


def simulate_draws(pop_wgt_df, sim_size, reference_pop_desc_file, seed=None):
    """gauss_host_simulate_draws (no GPU): simulateLD's draws alone.  Returns (DataFrame pop n count of the weighted populations in
    panel order, dict(draws, counts, seed, n_drawn))."""
    h = load_host()
    names, w, n = _pop_wgt(pop_wgt_df)
    out = _vp()
    _hcheck(h.gauss_host_simulate_draws(_enc(reference_pop_desc_file), names, w.ctypes.data_as(_dp), n, int(sim_size), _seed(seed),
                                        C.byref(out)))
    named = _named(h, out)
    return _table(h, out)[0], _draws(named)


def _window_call(name, window, pop, files, af1_cutoff, ctx, extra=()):
    """One one-window host call, symbol `name`: window = (chr, start_bp, end_bp, wing_size); pop = study_pop, or pop_wgt_df where the
    symbol takes population weights; files = (input, index, data, description), a name or bytes each; extra = the call's own trailing
    arguments.  Returns (h, out): the library and the result table, for _table / _cond_frame / _traits_frame to read and free."""
    h = load_host()
    fn = getattr(h, name)
    if fn.argtypes[5] is _strs:
        names, w, n = _pop_wgt(pop)
        pop = (names, w.ctypes.data_as(_dp), n)
    else:
        pop = (_enc(pop),)
    out = _vp()
    _hcheck(fn(_ctx(ctx), *(int(v) for v in window), *pop, *(f if isinstance(f, bytes) else _enc(f) for f in files), _af(af1_cutoff),
               *extra, C.byref(out)))
    return h, out


def dist(chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file, reference_data_file,
         reference_pop_desc_file, af1_cutoff=None, ctx=None):
    return _table(*_window_call("gauss_host_dist", (chr, start_bp, end_bp, wing_size), study_pop,
                       (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx))[0]


def distmix(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_file, reference_index_file, reference_data_file,
            reference_pop_desc_file, af1_cutoff=None, ctx=None):
    return _table(*_window_call("gauss_host_distmix", (chr, start_bp, end_bp, wing_size), pop_wgt_df,
                       (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx))[0]


def dist_loo(chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file, reference_data_file,
             reference_pop_desc_file, af1_cutoff=None, ctx=None):
    """Leave-one-out check of a dist() window (gauss_host_dist_loo): every measured SNP inside [start_bp, end_bp] re-imputed from
    the other measured SNPs of the extended window.  Columns rsid chr bp a1 a2 af1ref z z_loo info_loo t pval; t is the
    standardised residual (N(0, 1) under the model), pval = 2 pnorm(-|t|): a flipped or misplaced study SNP has a large |t|."""
    return _table(*_window_call("gauss_host_dist_loo", (chr, start_bp, end_bp, wing_size), study_pop,
                       (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx))[0]


def distmix_loo(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_file, reference_index_file, reference_data_file,
                reference_pop_desc_file, af1_cutoff=None, ctx=None):
    """Leave-one-out check of a distmix() window (gauss_host_distmix_loo); columns as dist_loo with af1mix."""
    return _table(*_window_call("gauss_host_distmix_loo", (chr, start_bp, end_bp, wing_size), pop_wgt_df,
                       (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx))[0]


def _slct_args(p_cutoff, collin, max_signals, cond_rsids):
    cond = [os.fsencode(r) for r in (cond_rsids or ())]
    arr = (C.c_char_p * max(len(cond), 1))(*cond)
    return (0.0 if p_cutoff is None else float(p_cutoff), 0.0 if collin is None else float(collin),
            0 if max_signals is None else int(max_signals), arr, len(cond))


def dist_slct(chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file, reference_data_file,
              reference_pop_desc_file, af1_cutoff=None, p_cutoff=None, collin=None, max_signals=None, cond_rsids=None, ctx=None):
    """Stepwise conditional signal selection in a dist() window (gauss_host_dist_slct): how many independent signals the window holds.
    A SNP enters while its conditional p-value is below p_cutoff (None: 5e-8); SNPs whose un-ridged r^2 with the selected set reaches
    collin (None: 0.9) are not considered; at most max_signals (None: 32) enter; cond_rsids enter first, in their order, whatever
    their p-value.  One row per measured SNP of the extended window, wings included: rsid chr bp a1 a2 af1ref z wing order z_entry
    z_joint z_cond pval_cond var_left (include/gauss_host.h)."""
    return _table(*_window_call("gauss_host_dist_slct", (chr, start_bp, end_bp, wing_size), study_pop,
                       (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx,
                       _slct_args(p_cutoff, collin, max_signals, cond_rsids)))[0]


def distmix_slct(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_file, reference_index_file, reference_data_file,
                 reference_pop_desc_file, af1_cutoff=None, p_cutoff=None, collin=None, max_signals=None, cond_rsids=None, ctx=None):
    """Signal selection in a distmix() window (gauss_host_distmix_slct) on the ancestry-weighted LD; columns as dist_slct with af1mix."""
    return _table(*_window_call("gauss_host_distmix_slct", (chr, start_bp, end_bp, wing_size), pop_wgt_df,
                       (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx,
                       _slct_args(p_cutoff, collin, max_signals, cond_rsids)))[0]


def _cond_frame(h, out, sets=False):
    named = _named(h, out)
    df = _table(h, out)[0]                                 # (frees the table: nothing may fail between the two reads and this)
    sig = np.asarray(named["signals"], dtype=np.float64).reshape(-1, 3)
    df.attrs["signals"] = dict(row=sig[:, 0].astype(np.int64), z_entry=sig[:, 1].copy(), z_joint=sig[:, 2].copy())
    if sets:                                               # the *_cs calls: one row per credible set beside `signals`
        st = np.asarray(named["sets"], dtype=np.float64).reshape(-1, 4)
        df.attrs["sets"] = dict(row=st[:, 0].astype(np.int64), size=st[:, 1].astype(np.int64), mass=st[:, 2].copy(), lse=st[:, 3].copy())
    return df


def dist_cond(chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file, reference_data_file,
              reference_pop_desc_file, af1_cutoff=None, p_cutoff=None, collin=None, max_signals=None, cond_rsids=None, ctx=None):
    """dist() with its imputed SNPs conditioned on the signals dist_slct() selects (gauss_host_dist_cond): is an imputed hit a signal
    of its own or the shadow of the lead SNP?  Arguments as dist_slct.  The frame opens with dist()'s rows (same order, same bits:
    rsid chr bp a1 a2 af1ref z pval info type); the measured SNPs of the wings follow, so that every selected SNP has a row.  Appended
    columns: wing order z_cond pval_cond var_left -- a measured row carries dist_slct()'s values, an imputed row the z of the imputed
    SNP given the selected ones (variance info, not 1: include/gauss_hip.h), its two-sided p-value and the share of its variance they
    leave (z_cond NaN below 1 - collin).  frame.attrs["signals"] = dict(row, z_entry, z_joint) of the selected SNPs in order of entry."""
    return _cond_frame(*_window_call("gauss_host_dist_cond", (chr, start_bp, end_bp, wing_size), study_pop,
                       (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx,
                       _slct_args(p_cutoff, collin, max_signals, cond_rsids)))


def distmix_cond(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_file, reference_index_file, reference_data_file,
                 reference_pop_desc_file, af1_cutoff=None, p_cutoff=None, collin=None, max_signals=None, cond_rsids=None, ctx=None):
    """distmix() with its imputed SNPs conditioned on the selected signals (gauss_host_distmix_cond), on the ancestry-weighted LD;
    columns as dist_cond with af1mix."""
    return _cond_frame(*_window_call("gauss_host_distmix_cond", (chr, start_bp, end_bp, wing_size), pop_wgt_df,
                       (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx,
                       _slct_args(p_cutoff, collin, max_signals, cond_rsids)))


def _cs_args(coverage, prior_var):
    return (0.0 if coverage is None else float(coverage), 0.0 if prior_var is None else float(prior_var))


def dist_cs(chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file, reference_data_file,
            reference_pop_desc_file, af1_cutoff=None, p_cutoff=None, collin=None, max_signals=None, cond_rsids=None,
            coverage=None, prior_var=None, ctx=None):
    """dist_cond() with a credible set for each selected signal (gauss_host_dist_cs): which SNPs, measured or imputed, could be the
    causal one?  Arguments as dist_cond, plus coverage (None: 0.95), the share of a signal's posterior mass its set holds, and
    prior_var (None: 25.0), the prior variance of the causal SNP's non-centrality in z units.  The frame is dist_cond()'s (same rows,
    same bits in its columns) with pip, cs and cs_pip appended: the SNP's posterior inclusion probability over all signals, the
    1-based order of entry of the set that holds it (0: none; the `order` column's numbering) and its pip in that set.
    frame.attrs["signals"] as dist_cond; frame.attrs["sets"] = dict(row, size, mass, lse) per signal in order of entry.
    Limits: the candidates are the measured SNPs of the extended window and the unmeasured SNPs of the prediction window, so a signal
    near a window edge has a truncated set; one causal SNP per signal; uniform prior; z units; at most 32 signals."""
    return _cond_frame(*_window_call("gauss_host_dist_cs", (chr, start_bp, end_bp, wing_size), study_pop,
                     (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx,
                     _slct_args(p_cutoff, collin, max_signals, cond_rsids) + _cs_args(coverage, prior_var)), sets=True)


def distmix_cs(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_file, reference_index_file, reference_data_file,
               reference_pop_desc_file, af1_cutoff=None, p_cutoff=None, collin=None, max_signals=None, cond_rsids=None,
               coverage=None, prior_var=None, ctx=None):
    """distmix_cond() with a credible set for each selected signal (gauss_host_distmix_cs), on the ancestry-weighted LD; columns as
    dist_cs with af1mix."""
    return _cond_frame(*_window_call("gauss_host_distmix_cs", (chr, start_bp, end_bp, wing_size), pop_wgt_df,
                     (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx,
                     _slct_args(p_cutoff, collin, max_signals, cond_rsids) + _cs_args(coverage, prior_var)), sets=True)


def _susie_args(L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only):
    f = lambda v: 0.0 if v is None else float(v)
    return (0 if L is None else int(L), f(coverage), f(prior_var), f(min_abs_corr), 0 if max_sweeps is None else int(max_sweeps), f(tol),
            -1 if estimate_prior_var is None else int(bool(estimate_prior_var)), int(bool(measured_only)))


def _susie_frame(h, out):
    named = _named(h, out)
    df = _table(h, out)[0]                                 # (frees the table: nothing may fail between the two reads and this)
    e = np.asarray(named["effects"], dtype=np.float64).reshape(-1, 7)
    df.attrs["effects"] = dict(row=e[:, 0].astype(np.int64), V=e[:, 1].copy(), lse=e[:, 2].copy(), size=e[:, 3].astype(np.int64),
                               mass=e[:, 4].copy(), purity=e[:, 5].copy(), kept=e[:, 6] != 0)
    f = np.asarray(named["fit"], dtype=np.float64).reshape(-1)
    df.attrs["fit"] = dict(sweeps=int(f[0]), delta=float(f[1]), converged=bool(f[2]))
    return df


def dist_susie(chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file, reference_data_file,
               reference_pop_desc_file, af1_cutoff=None, L=None, coverage=None, prior_var=None, min_abs_corr=None, max_sweeps=None, tol=None,
               estimate_prior_var=None, measured_only=False, ctx=None):
    """Multi-causal fine-mapping of a dist() window (gauss_host_dist_susie): the "sum of single effects" model (SuSiE-RSS) fitted to the
    measured z, with the imputed SNPs as candidates beside the measured ones, each with the variance an imputed SNP really has.  Unlike
    dist_cs() it does not build on a stepwise selection: a measured SNP that tags two causal SNPs does not mislead it.
    L (None: 10, at most 32) effects; coverage (None: 0.95); prior_var (None: 25.0, in z units); min_abs_corr (None: 0.5), the purity a
    reported set needs; max_sweeps (None: 100, at most 1000); tol (None: 1e-4; negative: exactly max_sweeps sweeps); estimate_prior_var (None: True);
    measured_only=True: plain SuSiE-RSS on the measured SNPs.  The frame has dist()'s rows (same bits in the shared columns), then the
    measured SNPs of the wings, with wing, pip, cs (1-based effect of the reported set that holds the SNP, 0: none) and cs_pip appended.
    frame.attrs["effects"] = dict(row, V, lse, size, mass, purity, kept) per effect; frame.attrs["fit"] = dict(sweeps, delta, converged).
    Limits: the candidates are the measured SNPs of the extended window and the unmeasured SNPs of the prediction window; a window whose
    B11 MakePosDef repairs is not fitted (a message says so); z units; L <= 32; residual variance fixed at 1; uniform prior."""
    return _susie_frame(*_window_call("gauss_host_dist_susie", (chr, start_bp, end_bp, wing_size), study_pop,
                        (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx,
                        _susie_args(L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only)))


def distmix_susie(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_file, reference_index_file, reference_data_file,
                  reference_pop_desc_file, af1_cutoff=None, L=None, coverage=None, prior_var=None, min_abs_corr=None, max_sweeps=None, tol=None,
                  estimate_prior_var=None, measured_only=False, ctx=None):
    """Multi-causal fine-mapping of a distmix() window (gauss_host_distmix_susie), on the ancestry-weighted LD; columns as dist_susie
    with af1mix."""
    return _susie_frame(*_window_call("gauss_host_distmix_susie", (chr, start_bp, end_bp, wing_size), pop_wgt_df,
                        (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx,
                        _susie_args(L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only)))


def _xsusie_frame(h, out, K):
    named = _named(h, out)
    df = _table(h, out)[0]                                 # (frees the table: nothing may fail between the two reads and this)
    e = np.asarray(named["effects"], dtype=np.float64).reshape(-1, 2 * K + 5)
    df.attrs["effects"] = dict(row=e[:, 0].astype(np.int64), V=e[:, 1:1 + K].T.copy(), purity=e[:, 1 + K:1 + 2 * K].T.copy(), lse=e[:, 1 + 2 * K].copy(),
                               size=e[:, 2 + 2 * K].astype(np.int64), mass=e[:, 3 + 2 * K].copy(), kept=e[:, 4 + 2 * K] != 0)
    f = np.asarray(named["fit"], dtype=np.float64).reshape(-1)
    df.attrs["fit"] = dict(sweeps=int(f[0]), delta=float(f[1]), converged=bool(f[2]))
    return df


def dist_xsusie(chr, start_bp, end_bp, wing_size, study_pops, input_files, reference_index_file, reference_data_file,
                reference_pop_desc_file, af1_cutoff=None, L=None, coverage=None, prior_var=None, min_abs_corr=None, max_sweeps=None, tol=None,
                estimate_prior_var=None, measured_only=False, ctx=None):
    """Joint fine-mapping of one trait across 2 .. 4 studies of different populations (gauss_host_dist_xsusie): one shared causal SNP
    per effect, each study's own LD (study_pops[k]) and effect size -- a tag SNP one ancestry cannot tell from the causal SNP is often
    only loosely linked to it in another.  input_files[k] is study k's GWAS; study 1 leads.  The frame is dist_susie()'s of study 1 with
    the joint pip, cs, cs_pip and a column joint (1: the SNP is a candidate of every study) appended; frame.attrs["effects"] =
    dict(row, V [K, L], purity [K, L], lse, size, mass, kept), frame.attrs["fit"] as dist_susie.  The fit's arguments are dist_susie's.
    Limits: the candidates are an intersection over the studies; residual variance 1; uniform prior; a set is reported when it is pure
    in at least one study; a group in which MakePosDef repairs any study's window is not fitted (a message says which)."""
    h = load_host()
    K = len(input_files)
    if len(study_pops) != K:
        raise ValueError("one study population per input file")
    out = _vp()
    pops, files = (C.c_char_p * K)(*[_enc(p) for p in study_pops]), (C.c_char_p * K)(*[_enc(f) for f in input_files])
    _hcheck(h.gauss_host_dist_xsusie(_ctx(ctx), int(chr), int(start_bp), int(end_bp), int(wing_size), pops, files, K, _enc(reference_index_file),
                                     _enc(reference_data_file), _enc(reference_pop_desc_file), _af(af1_cutoff),
                                     *_susie_args(L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only), C.byref(out)))
    return _xsusie_frame(h, out, K)


def distmix_xsusie(chr, start_bp, end_bp, wing_size, pop_wgt_dfs, input_files, reference_index_file, reference_data_file,
                   reference_pop_desc_file, af1_cutoff=None, L=None, coverage=None, prior_var=None, min_abs_corr=None, max_sweeps=None, tol=None,
                   estimate_prior_var=None, measured_only=False, ctx=None):
    """Joint fine-mapping of one trait across 2 .. 4 studies of different ancestry mixes (gauss_host_distmix_xsusie): pop_wgt_dfs[k] is
    study k's weights as distmix() takes them, over the same population names in the same order; the rest as dist_xsusie with af1mix."""
    h = load_host()
    K = len(input_files)
    if len(pop_wgt_dfs) != K:
        raise ValueError("one set of ancestry weights per input file")
    parts = [_pop_wgt(p) for p in pop_wgt_dfs]
    names, n = parts[0][0], parts[0][2]
    if any(list(p[0]) != list(names) or p[2] != n for p in parts[1:]):
        raise ValueError("the studies' weights must name the same populations in the same order")
    w = np.ascontiguousarray(np.stack([np.asarray(p[1], dtype=np.float64) for p in parts]))
    out = _vp()
    files = (C.c_char_p * K)(*[_enc(f) for f in input_files])
    _hcheck(h.gauss_host_distmix_xsusie(_ctx(ctx), int(chr), int(start_bp), int(end_bp), int(wing_size), names, w.ctypes.data_as(_dp), n, files, K,
                                        _enc(reference_index_file), _enc(reference_data_file), _enc(reference_pop_desc_file), _af(af1_cutoff),
                                        *_susie_args(L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only),
                                        C.byref(out)))
    return _xsusie_frame(h, out, K)


def _prs_args(n, s, lam, tol, max_sweeps):
    """(the call's trailing arguments, the arrays they point into: keep them alive over the call)"""
    sa = None if s is None else np.ascontiguousarray(s, dtype=np.float64).reshape(-1)
    la = None if lam is None else np.ascontiguousarray(lam, dtype=np.float64).reshape(-1)
    if (sa is not None and len(sa) == 0) or (la is not None and len(la) == 0):
        raise ValueError("s and lam are None (lassosum's grid) or lists of at least one value")
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(_dbl))
    return (float(n), p(sa), 0 if sa is None else len(sa), p(la), 0 if la is None else len(la), 0.0 if tol is None else float(tol),
            0 if max_sweeps is None else int(max_sweeps)), (sa, la)


def _prs_frame(h, out, per_allele):
    named = _named(h, out)
    df = _table(h, out)[0]                                 # (frees the table: nothing may fail between the two reads and this)
    g = np.asarray(named["grid"], dtype=np.float64).reshape(-1, 9)
    beta = np.asarray(named["beta"], dtype=np.float64).reshape(g.shape[0], -1)
    if per_allele:
        af = df["af1mix" if "af1mix" in df else "af1ref"].to_numpy()
        beta = beta / np.sqrt(2.0 * af * (1.0 - af))[None, :]
    df.attrs["beta"] = beta
    df.attrs["grid"] = dict(s=g[:, 0].copy(), lam=g[:, 1].copy(), nnz=g[:, 2].astype(np.int64), sweeps=g[:, 3].astype(np.int64), delta=g[:, 4].copy(),
                            br=g[:, 5].copy(), bg=g[:, 6].copy(), kkt=g[:, 7].copy(), converged=g[:, 8] != 0)
    return df


def dist_prs(chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file, reference_data_file,
             reference_pop_desc_file, n, af1_cutoff=None, s=None, lam=None, tol=None, max_sweeps=None, per_allele=False, ctx=None):
    """Polygenic score weights of a dist() window (gauss_host_dist_prs): lassosum's elastic net on summary statistics, fitted by
    coordinate descent on the window's own LD over a grid of shrinkage values s and a path of penalties lam (lam = 0: ridge regression,
    LDpred-inf's estimator).  n: the study's sample size.  s (None: 0.2, 0.5, 0.9, 1; at most 8 values in (0, 1]); lam (None: 20 values
    log-spaced from 0.1 down to 0.001; at most 32, taken in the order given, each from the solution of the one before); tol (None: 1e-4);
    max_sweeps (None: 100, at most 1000).  The frame has one row per measured SNP of the extended window: rsid chr bp a1 a2 af1ref z r
    wing.  frame.attrs["beta"] [n_s n_lam, rows]: the weights of grid cell i_s n_lam + i_lam; frame.attrs["grid"] = dict(s, lam, nnz,
    sweeps, delta, br, bg, kkt, converged) per cell; the in-sample predicted R^2 of a cell is br^2 / bg.  per_allele=True divides the
    weights by sqrt(2 af (1 - af)).
    Limits: weights for measured SNPs only (an imputed SNP adds no information to a score); standardised-genotype units unless
    per_allele; one trait; the tuning value is the caller's choice (pseudovalidation needs genotypes of the target cohort)."""
    extra, keep = _prs_args(n, s, lam, tol, max_sweeps)
    return _prs_frame(*_window_call("gauss_host_dist_prs", (chr, start_bp, end_bp, wing_size), study_pop,
                      (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx, extra), per_allele)


def distmix_prs(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_file, reference_index_file, reference_data_file,
                reference_pop_desc_file, n, af1_cutoff=None, s=None, lam=None, tol=None, max_sweeps=None, per_allele=False, ctx=None):
    """Polygenic score weights of a distmix() window (gauss_host_distmix_prs), on the ancestry-weighted LD: the LD reference a
    mixed-ancestry cohort otherwise lacks.  Columns as dist_prs with af1mix."""
    extra, keep = _prs_args(n, s, lam, tol, max_sweeps)
    return _prs_frame(*_window_call("gauss_host_distmix_prs", (chr, start_bp, end_bp, wing_size), pop_wgt_df,
                      (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx, extra), per_allele)


def _ldscore_frame(h, out):
    named = _named(h, out)
    df = _table(h, out)[0]                                 # (frees the table: nothing may fail between the two reads and this)
    a = np.asarray(named["ldscore"], dtype=np.float64).reshape(-1)
    df.attrs.update(n_eff=float(a[0]), M=int(a[1]), M_5_50=int(a[2]), radius=int(a[3]))
    return df


def dist_ldscore(chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file, reference_data_file,
                 reference_pop_desc_file, af1_cutoff=None, n=None, ctx=None):
    """LD scores of a dist() window (gauss_host_dist_ldscore): l2_raw = sum r^2 over the panel SNPs within wing_size bp of each SNP, on
    the pooled LD of the selected populations, reduced on the GPU -- the matrices never come back.  The SNPs scored are those of
    input_file (its z column is ignored) that the panel has inside [start_bp, end_bp]; the sum runs over EVERY panel SNP of the extended
    window that passes af1_cutoff, the wings' study SNPs included.  One row per scored SNP: rsid chr bp a1 a2 af1ref l2 l2_raw n_band;
    l2 = l2_raw (1 + 1 / (n - 2)) - n_band / (n - 2) is ldsc's bias-adjusted score, n (None: the selected populations' sample count)
    the sample size in it.  frame.attrs: n_eff, M (panel SNPs of the window, scored ones included), M_5_50 (those with minor allele
    frequency above 0.05), radius.  Limits: one window per call; a bp radius, no cM; no stratified scores from files
    (hotpath.ld_window(ldscore=dict(annot=...)) has them)."""
    return _ldscore_frame(*_window_call("gauss_host_dist_ldscore", (chr, start_bp, end_bp, wing_size), study_pop,
                          (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx,
                          (0.0 if n is None else float(n),)))


def distmix_ldscore(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_file, reference_index_file, reference_data_file,
                    reference_pop_desc_file, af1_cutoff=None, n=None, ctx=None):
    """LD scores of a distmix() window (gauss_host_distmix_ldscore) on the ancestry-weighted LD: the LD scores a mixed-ancestry cohort
    has no file to download for.  Columns as dist_ldscore with af1mix.  n (None): Kish's effective size of the weighted panel,
    (sum w_p)^2 / sum (w_p^2 / n_p) over the populations of non-zero weight, the weights as passed -- a convention of this project,
    stated in frame.attrs["n_eff"], not a measurement."""
    return _ldscore_frame(*_window_call("gauss_host_distmix_ldscore", (chr, start_bp, end_bp, wing_size), pop_wgt_df,
                          (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx,
                          (0.0 if n is None else float(n),)))


def slct_chi2(p):
    """The chi^2 (1 df) threshold of a two-sided p-value in the library's own normal tail (gauss_host_slct_chi2): the smallest chi2
    with 2 pnorm(-sqrt(chi2)) < p."""
    h = load_host()
    out = C.c_double()
    _hcheck(h.gauss_host_slct_chi2(float(p), C.byref(out)))
    return out.value


def qcat(chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file, reference_data_file,
         reference_pop_desc_file, af1_cutoff=None, ctx=None):
    """qcat() of the reference (qcat.cpp:30-132); af1_cutoff None -> 0.05."""
    return _table(*_window_call("gauss_host_qcat", (chr, start_bp, end_bp, wing_size), study_pop,
                       (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx))[0]


def qcatmix(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_file, reference_index_file, reference_data_file,
            reference_pop_desc_file, af1_cutoff=None, ctx=None):
    """qcatmix() of the reference (qcatmix.cpp:30-140); af1_cutoff None -> 0.01."""
    return _table(*_window_call("gauss_host_qcatmix", (chr, start_bp, end_bp, wing_size), pop_wgt_df,
                       (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx))[0]


def _traits_files(input_files):
    files = [os.fsencode(f) for f in input_files]
    if not files:
        raise ValueError("input_files: at least the first trait's study file")
    more = files[1:]
    return files[0], (C.c_char_p * max(len(more), 1))(*more), len(more)


def _traits_frame(h, out):
    """The trait-1 frame with z_2, pval_2, ..., z_T, pval_T appended (the named matrices z_traits / pval_traits, column 0 = z / pval)."""
    named = _named(h, out)
    df = _table(h, out)[0]
    z, pv = (np.asarray(named[k]).reshape(len(df), -1) for k in ("z_traits", "pval_traits"))
    if "info_traits" in named:          # missing="impute": every trait has its own info and type (a SNP it lacks is imputed for it)
        info, typ = (np.asarray(named[k]).reshape(len(df), -1) for k in ("info_traits", "type_traits"))
        for k in range(1, z.shape[1]):
            df[f"z_{k + 1}"], df[f"pval_{k + 1}"], df[f"info_{k + 1}"], df[f"type_{k + 1}"] = z[:, k], pv[:, k], info[:, k], typ[:, k].astype(np.int64)
        df.attrs["n_missing"] = np.asarray(named["n_missing"]).reshape(-1).astype(np.int64)
        return df
    for k in range(1, z.shape[1]):
        df[f"z_{k + 1}"], df[f"pval_{k + 1}"] = z[:, k], pv[:, k]
    return df


def _traits_symbol(name, missing):
    if missing not in ("refuse", "impute"):
        raise ValueError(f"missing must be 'refuse' or 'impute', got {missing!r}")
    return name + ("_miss" if missing == "impute" else "")


def dist_traits(chr, start_bp, end_bp, wing_size, study_pop, input_files, reference_index_file, reference_data_file,
                reference_pop_desc_file, af1_cutoff=None, ctx=None, missing="refuse"):
    """dist() for many traits measured at the same SNPs, from ONE LD build and one factorisation (gauss_host_dist_traits).
    input_files: a list of study files (rsid chr bp a1 a2 z), at most 64; the first is trait 1 and defines the window, the measured
    set, the allele orientation and the AF filter exactly as dist() does.  Every measured SNP of the extended window must be in each
    further file (swapped alleles flip the sign, a key listed twice ends with its later row, other rows are ignored).  Returns dist()'s
    frame of trait 1 with columns z_2, pval_2, ..., z_T, pval_T appended: a measured SNP's own study z, an unmeasured SNP's imputed z
    (info is shared).
    missing="impute" (gauss_host_dist_traits_miss): a measured SNP that a further file lacks -- at most 32 per file, 128 distinct per window,
    more than 10 left -- is imputed for that trait as if the file had been run alone; the columns appended per trait are then
    z_k, pval_k, info_k, type_k (type 0 where trait k lacks a SNP trait 1 measures), and frame.attrs["n_missing"] counts, per trait, the
    measured SNPs of the extended window its file lacked.  Column set k equals dist() of file k alone when that file's SNPs in the
    extended window are a subset of trait 1's."""
    name = _traits_symbol("gauss_host_dist_traits", missing)
    first, more, n_more = _traits_files(input_files)
    return _traits_frame(*_window_call(name, (chr, start_bp, end_bp, wing_size), study_pop,
                       (first, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx, (more, n_more)))


def distmix_traits(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_files, reference_index_file, reference_data_file,
                   reference_pop_desc_file, af1_cutoff=None, ctx=None, missing="refuse"):
    """distmix() for many traits measured at the same SNPs (gauss_host_distmix_traits); input_files, missing and the frame as dist_traits."""
    name = _traits_symbol("gauss_host_distmix_traits", missing)
    first, more, n_more = _traits_files(input_files)
    return _traits_frame(*_window_call(name, (chr, start_bp, end_bp, wing_size), pop_wgt_df,
                       (first, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx, (more, n_more)))


COLOC_COLUMNS = ("trait_a", "trait_b", "cs_a", "cs_b", "n", "H0", "H1", "H2", "H3", "H4", "hit_row", "hit_pp")


def _coloc_frame(h, out):
    """The *_traits frame with *_susie's columns for trait 1 and pip_t, cs_t, cs_pip_t per further trait; attrs: coloc (a DataFrame, one
    row per pair of kept effects of two traits, hit_rsid resolved), effects and fit (lists, one entry per trait)."""
    import pandas as pd
    named = _named(h, out)
    df = _table(h, out)[0]
    z, pv = (np.asarray(named[k]).reshape(len(df), -1) for k in ("z_traits", "pval_traits"))
    n_traits = z.shape[1]
    at = list(df.columns).index("wing")                    # the *_traits columns stand in front of the fit's
    for k in range(1, n_traits):
        df.insert(at, f"z_{k + 1}", z[:, k])
        df.insert(at + 1, f"pval_{k + 1}", pv[:, k])
        at += 2
    effects, fits = [], []
    for t in range(1, n_traits + 1):
        e = np.asarray(named[f"effects_{t}"], dtype=np.float64).reshape(-1, 7)
        effects.append(dict(row=e[:, 0].astype(np.int64), V=e[:, 1].copy(), lse=e[:, 2].copy(), size=e[:, 3].astype(np.int64),
                            mass=e[:, 4].copy(), purity=e[:, 5].copy(), kept=e[:, 6] != 0))
        f = np.asarray(named[f"fit_{t}"], dtype=np.float64).reshape(-1)
        fits.append(dict(sweeps=int(f[0]), delta=float(f[1]), converged=bool(f[2])))
    c = np.asarray(named["coloc"], dtype=np.float64).reshape(-1, len(COLOC_COLUMNS))
    co = pd.DataFrame({k: c[:, j] for j, k in enumerate(COLOC_COLUMNS)})
    for k in ("trait_a", "trait_b", "cs_a", "cs_b", "n", "hit_row"):
        co[k] = co[k].astype(np.int64)
    rsid = df["rsid"].to_numpy()
    co["hit_rsid"] = [rsid[r] if r >= 0 else None for r in co["hit_row"]]
    df.attrs.update(coloc=co, effects=effects, fit=fits)
    return df


def _coloc_args(input_files, susie, p1, p2, p12):
    first, more, n_more = _traits_files(input_files)
    f = lambda v: 0.0 if v is None else float(v)
    return first, (more, n_more) + _susie_args(*susie) + (f(p1), f(p2), f(p12))


def dist_coloc(chr, start_bp, end_bp, wing_size, study_pop, input_files, reference_index_file, reference_data_file,
               reference_pop_desc_file, af1_cutoff=None, L=None, coverage=None, prior_var=None, min_abs_corr=None, max_sweeps=None, tol=None,
               estimate_prior_var=None, measured_only=False, p1=None, p2=None, p12=None, ctx=None):
    """Do two traits share a causal SNP in this window, or do they have two different ones in LD?  (gauss_host_dist_coloc)
    input_files: 2 .. 8 study files as for dist_traits (the first is trait 1 and defines the window; every measured SNP of the window
    must be in each further file).  Every trait is fine-mapped as dist_susie does (its arguments; all traits in the same launches), then
    every pair of reported effects of two traits is colocalised: coloc's bf_bf on the fit's Bayes factors with the priors p1, p2, p12
    (None: 1e-4, 1e-4, 1e-5), the imputed SNPs among the candidates -- the shared SNP may be one that neither study measured.
    The frame: dist_susie()'s rows; dist_traits()'s columns; wing, pip, cs, cs_pip for trait 1 (dist_susie's bits on the first file);
    pip_t, cs_t, cs_pip_t for t = 2 .. T.  frame.attrs["coloc"]: a DataFrame, one row per pair of reported effects of two traits, with
    trait_a, trait_b (1-based), cs_a, cs_b (the cs / cs_t numbering), n, H0 .. H4 (the posteriors: none, a only, b only, two different
    SNPs, one shared), hit_row, hit_rsid and hit_pp (the most likely shared SNP and its share of H4); attrs["effects"] / attrs["fit"]:
    lists with dist_susie's dicts, one per trait.  Limits: dist_susie's; eight traits; traits that lack measured SNPs are not fitted."""
    first, tail = _coloc_args(input_files, (L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only), p1, p2, p12)
    return _coloc_frame(*_window_call("gauss_host_dist_coloc", (chr, start_bp, end_bp, wing_size), study_pop,
                        (first, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx, tail))


def distmix_coloc(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_files, reference_index_file, reference_data_file,
                  reference_pop_desc_file, af1_cutoff=None, L=None, coverage=None, prior_var=None, min_abs_corr=None, max_sweeps=None, tol=None,
                  estimate_prior_var=None, measured_only=False, p1=None, p2=None, p12=None, ctx=None):
    """dist_coloc on the ancestry-weighted LD of a distmix() window (gauss_host_distmix_coloc); columns as dist_coloc with af1mix."""
    first, tail = _coloc_args(input_files, (L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only), p1, p2, p12)
    return _coloc_frame(*_window_call("gauss_host_distmix_coloc", (chr, start_bp, end_bp, wing_size), pop_wgt_df,
                        (first, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx, tail))


def _named(h, t):
    """Named numeric members of a result List (column-major in C, returned as (nrow, ncol) arrays)."""
    out = {}
    for k in range(h.gauss_table_n_named(t)):
        nr, nc = C.c_int(), C.c_int()
        p = h.gauss_table_named(t, k, C.byref(nr), C.byref(nc))
        name = h.gauss_table_named_name(t, k).decode()
        n = nr.value * nc.value
        a = np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0)
        out[name] = a if nc.value == 1 else a.reshape(nc.value, nr.value).T
    return out


def prep_qcat(chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file, reference_data_file,
              reference_pop_desc_file, af1_cutoff=None, ctx=None):
    """prep_qcat() of the reference (prep_qcat.cpp:16-205): list(snplist, z_vec, cor_mat1, cor_mat2)."""
    h, out = _window_call("gauss_host_prep_qcat", (chr, start_bp, end_bp, wing_size), study_pop,
                       (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx)
    named = _named(h, out)
    return dict(snplist=_table(h, out)[0], **named)


def prep_recessive_impute(chr, start_bp, end_bp, wing_size, pop_wgt_df, input_file, reference_index_file,
                          reference_data_file, reference_pop_desc_file, af1_cutoff=None, ctx=None):
    """prep_recessive_impute() of the reference (prep_qcatmix.cpp:36-316): list(snplist, zvec, cormat,
    cormat_add, cormat_dom, cormat_rec)."""
    h, out = _window_call("gauss_host_prep_recessive_impute", (chr, start_bp, end_bp, wing_size), pop_wgt_df,
                       (input_file, reference_index_file, reference_data_file, reference_pop_desc_file), af1_cutoff, ctx)
    named = _named(h, out)
    return dict(snplist=_table(h, out)[0], **named)


def prep_zmix5(input_file, reference_index_file, reference_data_file, reference_pop_desc_file, percentile=None,
               interval=None, ctx=None, with_snps=False):
    """prep_zmix5() of the reference (zmix.cpp:44-190): matrix [n_pairs x (1 + n_pop)], column 0 = z_i*z_j,
    column k+1 = genotype correlation of the pair inside population k."""
    h = load_host()
    out = _vp()
    _hcheck(h.gauss_host_prep_zmix5(_ctx(ctx), _enc(input_file), _enc(reference_index_file), _enc(reference_data_file),
                                    _enc(reference_pop_desc_file), _af(percentile), int(interval or 0), C.byref(out)))
    named = _named(h, out)
    df = _table(h, out)[0]
    return (named["data_mat"], df) if with_snps else named["data_mat"]


def prep_zmix_variant(variant, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, percentile=None,
                      interval=None, p2=None, ctx=None):
    """prep_zmix() / prep_zmix2() / prep_zmix3() / prep_zmix4() / prep_zmix5_sup() of the reference (zmix.cpp:201-1076;
    variant "zmix", "zmix2", "zmix3", "zmix4", "zmix5_sup"; p2 = offset or steps).  Returns dict(data_mat, snps (DataFrame),
    pairs [n_pairs x 2] rows of snps, groups: the names of the correlation columns)."""
    h = load_host()
    out = _vp()
    files = (_enc(input_file), _enc(reference_index_file), _enc(reference_data_file), _enc(reference_pop_desc_file))
    if variant == "zmix":
        _hcheck(h.gauss_host_prep_zmix(_ctx(ctx), *files, int(interval or 0), C.byref(out)))
    elif variant == "zmix5_sup":
        _hcheck(h.gauss_host_prep_zmix5_sup(_ctx(ctx), *files, _af(percentile), int(interval or 0), C.byref(out)))
    else:
        fn = {"zmix2": h.gauss_host_prep_zmix2, "zmix3": h.gauss_host_prep_zmix3, "zmix4": h.gauss_host_prep_zmix4}[variant]
        _hcheck(fn(_ctx(ctx), *files, int(interval or 0), int(p2 or 0), C.byref(out)))
    named = _named(h, out)
    groups = [h.gauss_table_message(out, k).decode() for k in range(h.gauss_table_n_messages(out))]
    df = _table(h, out)[0]
    return dict(data_mat=named["data_mat"], pairs=named["pairs"].astype(np.int64), snps=df, groups=groups)


def _popwgt(kind, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, interval, ctx, detail):
    h = load_host()
    out = _vp()
    fn = h.gauss_host_afmix if kind == KIND_AFMIX else h.gauss_host_cpw2
    _hcheck(fn(_ctx(ctx), _enc(input_file), _enc(reference_index_file), _enc(reference_data_file), _enc(reference_pop_desc_file),
               int(interval or 0), C.byref(out)))
    named = _named(h, out)
    msgs = [h.gauss_table_message(out, k).decode() for k in range(h.gauss_table_n_messages(out))]
    df = _table(h, out)[0]
    if not detail:
        return df
    return df, dict(w_raw=named["w_raw"].reshape(-1), w_interval=named["w_interval"].reshape(-1, len(named["w_raw"])),
                    status=named["status"].reshape(-1).astype(np.int32), messages=msgs)


def afmix(input_file, reference_index_file, reference_data_file, reference_pop_desc_file, interval=None, ctx=None, detail=False):
    """afmix() of the reference (afmix.cpp:30-111): ancestry proportions of a study from its allele frequencies.

    input_file: header, then ``rsid chr bp a1 a2 af1`` per line.  interval=None means 1000, as in R.  Returns a DataFrame
    with columns ``sup.pop, pop, wgt`` (populations with a positive weight, panel order).  detail=True returns
    ``(df, dict(w_raw, w_interval, status, messages))``: the weights of every population before the clamp at 0 and the
    rounding, the per-interval weights, their GAUSS_ST_* status bits and any message (e.g. interval <= S < 2 interval:
    every weight is NaN and the frame is empty, as in the reference).

    To weight distmix / qcatmix / jepegmix / computeLD with the result, pass ``df[["pop", "wgt"]]`` as pop_wgt_df (the
    entry points read the first two columns, as R does)."""
    return _popwgt(KIND_AFMIX, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, interval, ctx, detail)


def cpw2(input_file, reference_index_file, reference_data_file, reference_pop_desc_file, interval=None, ctx=None, detail=False):
    """cpw2() of the reference (cpw2.cpp:31-107): afmix on arcsine-square-root transformed allele frequencies.  Returns a
    DataFrame with columns ``pop, wgt`` -- directly usable as a pop_wgt_df; detail as in afmix."""
    return _popwgt(KIND_CPW2, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, interval, ctx, detail)


ZMIX_LEVELS = {"population": 0, "superpopulation": 1}      # GAUSS_ZMIX_POPULATION / GAUSS_ZMIX_SUPERPOPULATION


def zmix(input_file, reference_index_file, reference_data_file, reference_pop_desc_file, percentile=0.9, interval=10,
         level="population", ctx=None, detail=False):
    """zmix() of the reference (zmix.R): ancestry proportions of a study from its Z-scores.

    input_file: header, then ``rsid chr bp a1 a2 z`` per line.  percentile / interval: the selection of prep_zmix5 (None
    means zmix.R's defaults 0.9 / 10).  level: "population" (columns ``Population, SuperPopulation, Weight``, every population
    in description order) or "superpopulation" (``SuperPopulation, Weight``, order of first appearance).  The normal equations
    of the pair regression are reduced on the GPU; the constrained QP of solve.QP runs on the host.  detail=True returns
    ``(df, dict(dmat, dvec, w_unrounded, yty, n_snp, n_pairs, n_rows))``.

    To weight distmix / qcatmix / jepegmix / computeLD with a population-level result, pass ``df[["Population", "Weight"]]``
    as pop_wgt_df."""
    if level not in ZMIX_LEVELS:
        raise ValueError(f"level must be one of {sorted(ZMIX_LEVELS)}, not {level!r}")
    h = load_host()
    out = _vp()
    _hcheck(h.gauss_host_zmix(_ctx(ctx), _enc(input_file), _enc(reference_index_file), _enc(reference_data_file),
                              _enc(reference_pop_desc_file), _af(percentile), int(interval or 0), ZMIX_LEVELS[level], C.byref(out)))
    named = _named(h, out)
    df = _table(h, out)[0]
    if not detail:
        return df
    G = len(named["dvec"])
    return df, dict(dmat=np.asarray(named["dmat"]).reshape(G, G), dvec=named["dvec"].reshape(-1),
                    w_unrounded=named["w_unrounded"].reshape(-1), yty=float(named["yty"][0]),
                    n_snp=int(named["n_snp"][0]), n_pairs=int(named["n_pairs"][0]), n_rows=int(named["n_rows"][0]))


def zmix_qp(D, d):
    """gauss_host_zmix_qp (no GPU): zmix's constrained QP (quadprog::solve.QP's Goldfarb-Idnani method) on D [P, P], d [P].
    Returns (w_unrounded: solution / its sum, w_final: rounded to 5 decimals and normalised again)."""
    Da = np.ascontiguousarray(D, dtype=np.float64)
    da = np.ascontiguousarray(d, dtype=np.float64).reshape(-1)
    P = da.shape[0]
    if Da.shape != (P, P):
        raise ValueError(f"D has shape {Da.shape}, expected ({P}, {P})")
    w_unr, w_fin = np.zeros(P), np.zeros(P)
    _hcheck(load_host().gauss_host_zmix_qp(Da.ctypes.data_as(_dp), da.ctypes.data_as(_dp), P, w_unr.ctypes.data_as(_dp),
                                           w_fin.ctypes.data_as(_dp)))
    return w_unr, w_fin


def popwgt_inputs(kind,input_file, reference_index_file, reference_data_file, reference_pop_desc_file, interval=None):
    """gauss_host_popwgt_inputs (no GPU): the data layer of afmix (kind=KIND_AFMIX) / cpw2 (KIND_CPW2).  Returns
    (snps DataFrame rsid chr bp a1 a2 af1study in the reference's order, x [S, P + 1] interval-major matrix as the kernel
    receives it, interval_off [interval + 1])."""
    h = load_host()
    out = _vp()
    _hcheck(h.gauss_host_popwgt_inputs(int(kind), _enc(input_file), _enc(reference_index_file), _enc(reference_data_file),
                                       _enc(reference_pop_desc_file), int(interval or 0), C.byref(out)))
    named = _named(h, out)
    df = _table(h, out)[0]
    x = named["x"]
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    return df, np.ascontiguousarray(x), named["interval_off"].reshape(-1).astype(np.int64)


def jepeg(study_pop, input_file, annotation_file, reference_index_file, reference_data_file, reference_pop_desc_file,
          af1_cutoff=None, ctx=None):
    h = load_host()
    out = _vp()
    _hcheck(h.gauss_host_jepeg(_ctx(ctx), _enc(study_pop), _enc(input_file), _enc(annotation_file),
                               _enc(reference_index_file), _enc(reference_data_file), _enc(reference_pop_desc_file),
                               _af(af1_cutoff), C.byref(out)))
    return _table(h, out)[0]


def jepegmix(pop_wgt_df, input_file, annotation_file, reference_index_file, reference_data_file,
             reference_pop_desc_file, af1_cutoff=None, ctx=None):
    h = load_host()
    names, w, n = _pop_wgt(pop_wgt_df)
    out = _vp()
    _hcheck(h.gauss_host_jepegmix(_ctx(ctx), names, w.ctypes.data_as(_dp), n, _enc(input_file), _enc(annotation_file),
                                  _enc(reference_index_file), _enc(reference_data_file), _enc(reference_pop_desc_file),
                                  _af(af1_cutoff), C.byref(out)))
    return _table(h, out)[0]


def _sumchi2_frame(h, out):
    lam = np.asarray(_named(h, out)["lam"])
    df, _ = _table(h, out)
    df.attrs["lam"] = lam.reshape(len(df), 128)       # (the frame's attrs carry the eigenvalues: this call needs pandas)
    return df


def sumchi2(study_pop, input_file, annotation_file, reference_index_file, reference_data_file, reference_pop_desc_file,
            af1_cutoff=None, prune_r2=0.9, ctx=None):
    """The gene-based sum-of-chi2 test (fastBAT, VEGAS, MAGMA's SNP-wise mean model) of jepeg()'s genes on the pooled LD of
    study_pop, on the GPU (gauss_host_sumchi2): per gene Q = sum z^2 over the SNPs that survive LD pruning at prune_r2 in position
    order, against sum lambda_i chi2_1 with lambda the eigenvalues of the kept SNPs' LD.  Returns the frame geneid num_snp num_kept
    chisq pval lam_max n_pos status top_snp top_snp_pval message, one row per gene; ``attrs["lam"]`` [n_gene, 128] holds the
    eigenvalues.  At most 1 024 SNPs a gene and 128 after pruning (pval NaN and a message beyond); z is taken at face value (an
    imputed z has variance `info`, not 1); pval is a saddlepoint approximation."""
    h = load_host()
    out = _vp()
    _hcheck(h.gauss_host_sumchi2(_ctx(ctx), _enc(study_pop), _enc(input_file), _enc(annotation_file), _enc(reference_index_file),
                                 _enc(reference_data_file), _enc(reference_pop_desc_file), _af(af1_cutoff),
                                 float("nan") if prune_r2 is None else float(prune_r2), C.byref(out)))
    return _sumchi2_frame(h, out)


def sumchi2mix(pop_wgt_df, input_file, annotation_file, reference_index_file, reference_data_file, reference_pop_desc_file,
               af1_cutoff=None, prune_r2=0.9, ctx=None):
    """sumchi2() of a mixed-ancestry study on the ancestry-weighted LD of jepegmix() (gauss_host_sumchi2mix)."""
    h = load_host()
    names, w, n = _pop_wgt(pop_wgt_df)
    out = _vp()
    _hcheck(h.gauss_host_sumchi2mix(_ctx(ctx), names, w.ctypes.data_as(_dp), n, _enc(input_file), _enc(annotation_file),
                                    _enc(reference_index_file), _enc(reference_data_file), _enc(reference_pop_desc_file),
                                    _af(af1_cutoff), float("nan") if prune_r2 is None else float(prune_r2), C.byref(out)))
    return _sumchi2_frame(h, out)


def sumchi2_pval(lam, q, n_pos=False):
    """gauss_host_sumchi2_pval (no GPU): P(sum lam_i chi2_1 > q); lam_i <= 0 or NaN are left out.  n_pos=True: (p, how many stay)."""
    h = load_host()
    l = np.ascontiguousarray(lam, dtype=np.float64).reshape(-1)
    p, k = C.c_double(), C.c_int()
    _hcheck(h.gauss_host_sumchi2_pval(l.ctypes.data_as(_dp), len(l), float(q), C.byref(p), C.byref(k)))
    return (p.value, k.value) if n_pos else p.value


def jepeg_rank(kind, input_file, annotation_file, reference_index_file, reference_data_file, reference_pop_desc_file,
               study_pop=None, pop_wgt_df=None, af1_cutoff=None, rank=0, world=1, ctx=None):
    """gauss_host_jepeg_rank: rank `rank` of `world`'s contiguous gene range of a jepeg() (KIND_JEPEG, study_pop) or jepegmix()
    (KIND_JEPEGMIX, pop_wgt_df) call.  Returns (table of the range's genes, (first gene, one past the last, genes in all)); the
    ranks' tables concatenated in rank order are the one-rank table."""
    h = load_host()
    names, w, n = (None, None, 0) if pop_wgt_df is None else _pop_wgt(pop_wgt_df)
    out = _vp()
    _hcheck(h.gauss_host_jepeg_rank(_ctx(ctx), int(kind), _enc(study_pop), names, None if w is None else w.ctypes.data_as(_dp), n,
                                    _enc(input_file), _enc(annotation_file), _enc(reference_index_file), _enc(reference_data_file),
                                    _enc(reference_pop_desc_file), _af(af1_cutoff), int(rank), int(world), C.byref(out)))
    rng = tuple(int(v) for v in _named(h, out)["gene_range"].reshape(-1))
    return _table(h, out)[0], rng


def jepeg_genome(kind, calls, reference_pop_desc_file, study_pop=None, pop_wgt_df=None, af1_cutoff=None, rank=0, world=1, ctx=None,
                 raise_on_error=True):
    """gauss_host_jepeg_genome: `calls` = [(input_file, annotation_file, reference_index_file, reference_data_file)], one jepeg() /
    jepegmix() call each (the reference's user: one per chromosome), dealt whole to the ranks.  Returns (tables, owner): tables[c] is
    call c's gene table on the rank that ran it and None elsewhere; owner[c] that rank."""
    h = load_host()
    names, w, n = (None, None, 0) if pop_wgt_df is None else _pop_wgt(pop_wgt_df)
    nc = len(calls)
    arr = lambda k: (C.c_char_p * nc)(*[_enc(c[k]) for c in calls])
    outs = (_vp * nc)()
    owner = (C.c_int32 * nc)()
    rc = h.gauss_host_jepeg_genome(_ctx(ctx), int(kind), nc, _enc(study_pop), names, None if w is None else w.ctypes.data_as(_dp), n,
                                   arr(0), arr(1), arr(2), arr(3), _enc(reference_pop_desc_file), _af(af1_cutoff), int(rank), int(world),
                                   outs, owner)
    tabs = [(_table(h, _vp(outs[c]))[0] if outs[c] else None) for c in range(nc)]
    if rc != 0 and raise_on_error:
        _hcheck(rc)
    return tabs, [int(o) for o in owner]


class _TableOwner:
    """Keeps a gauss_table alive for the numpy views handed out over its columns; frees it when the last view is gone."""

    def __init__(self, h, t):
        self.h, self.t = h, t

    def __del__(self):
        try:
            if self.t:
                self.h.gauss_table_free(self.t)
                self.t = None
        except Exception:
            pass


def _columns(h, t, owner=None):
    """gauss_table -> {name: numpy array}; string columns come across as ONE fixed-width bytes array each
    (dtype "S<w>"), not as Python strings: a chromosome's table has ~10^5 rows.
    owner = None: the arrays are copies (the caller frees the table).  owner = a _TableOwner of `t`: the arrays are VIEWS of the
    library's columns -- no copy; every array keeps the owner, and with it the table, alive."""
    cols = {}
    n = h.gauss_table_nrow(t)

    def view(ctype, addr, count, dtype):
        buf = (ctype * count).from_address(addr)
        if owner is None:
            return np.frombuffer(buf, dtype=dtype).copy()
        buf._gauss_owner = owner                     # numpy array -> .base (this ctypes view) -> the table's owner
        return np.frombuffer(buf, dtype=dtype)

    for c in range(h.gauss_table_ncol(t)):
        name = h.gauss_table_colname(t, c).decode()
        ty = h.gauss_table_coltype(t, c)
        if ty == 0:
            w = C.c_int()
            buf = h.gauss_table_strcol_fixed(t, c, C.byref(w))
            cols[name] = view(C.c_char, buf, n * w.value, f"S{w.value}") if (n and buf) else np.zeros(0, dtype="S1")
        elif ty == 1:
            cols[name] = view(C.c_int32, C.addressof(h.gauss_table_int(t, c).contents), n, np.int32) if n else np.zeros(0, np.int32)
        else:
            cols[name] = view(C.c_double, C.addressof(h.gauss_table_dbl(t, c).contents), n, np.float64) if n else np.zeros(0)
    return cols


class ChromResult:
    """What gauss_host_impute_chromosome hands back for one rank: `columns` (the reference's output columns as numpy
    arrays plus "window"), `windows` [n_windows x 6: start_bp end_bp owner status measured unmeasured], `stats`
    (dict of gauss_chrom_stats) and `messages` (one text per failed window)."""

    def __init__(self, columns, windows, stats, messages):
        self.columns, self.windows, self.stats, self.messages = columns, windows, stats, messages

    def frame(self):
        """pandas DataFrame with the reference's column names and types (strings decoded)."""
        import pandas as pd
        return pd.DataFrame({k: (v.astype(str) if v.dtype.kind == "S" else v) for k, v in self.columns.items() if k != "window"})

    @staticmethod
    def merge(parts):
        """Tables of several ranks -> one, in window order (prediction windows are disjoint: no de-duplication)."""
        parts = [p for p in parts if p is not None]
        names = list(parts[0].columns)
        cat = {}
        for k in names:
            arrs = [p.columns[k] for p in parts]
            if arrs[0].dtype.kind == "S":
                w = max(a.dtype.itemsize for a in arrs)
                arrs = [a.astype(f"S{w}") for a in arrs]
            cat[k] = np.concatenate(arrs)
        order = np.argsort(cat["window"], kind="stable")
        cat = {k: v[order] for k, v in cat.items()}
        windows = parts[0].windows.copy()
        for p in parts[1:]:
            mine = p.windows[:, 3] >= 0
            windows[mine] = p.windows[mine]
        stats = {k: ([p.stats[k] for p in parts]) for k in parts[0].stats}
        return ChromResult(cat, windows, stats, [m for p in parts for m in p.messages])


def jepeg_gene_tail(corg, z, info, has, wgt):
    """gauss_host_jepeg_gene_tail: the host k x k tail of jepeg()/jepegmix() for one gene (no GPU involved)."""
    h = load_host()
    corg = np.ascontiguousarray(corg, dtype=np.float64)
    n = corg.shape[0]
    z, info = np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(info, dtype=np.float64)
    has = np.ascontiguousarray(has, dtype=np.int32).reshape(n, 6)
    wgt = np.ascontiguousarray(wgt, dtype=np.float64).reshape(n, 6)
    chisq, jp, tcp, tsp = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    df, tc, ts = C.c_int32(), C.c_int32(), C.c_int32()
    ip = C.POINTER(C.c_int32)
    h.gauss_host_jepeg_gene_tail.argtypes = [C.c_int, _dp, _dp, _dp, ip, _dp, _dp, ip, _dp, ip, _dp, ip, _dp]
    _hcheck(h.gauss_host_jepeg_gene_tail(n, corg.ctypes.data_as(_dp), z.ctypes.data_as(_dp), info.ctypes.data_as(_dp),
                                         has.ctypes.data_as(ip), wgt.ctypes.data_as(_dp), C.byref(chisq), C.byref(df), C.byref(jp),
                                         C.byref(tc), C.byref(tcp), C.byref(ts), C.byref(tsp)))
    return dict(chisq=chisq.value, df=df.value, jepeg_pval=jp.value, top_categ=tc.value, top_categ_pval=tcp.value,
                top_snp=ts.value, top_snp_pval=tsp.value, num_snp=n)


def panel_resident(packed_file, ctx=None):
    """Upload a packed panel's genotype rows to the GPU once (gauss_host_panel_resident); returns the bytes moved now."""
    n = _i64()
    _hcheck(load_host().gauss_host_panel_resident(_ctx(ctx), _enc(packed_file), C.byref(n)))
    return n.value


def panel_evict(packed_file=None, ctx=None):
    _hcheck(load_host().gauss_host_panel_evict(_ctx(ctx), _enc(packed_file)))


def panel_cache(reference_index_file, reference_data_file, reference_pop_desc_file, create=True):
    """The packed form of a text panel in the panel cache (gauss_host_panel_cache): (path, SNPs packed by this call),
    or (None, 0) when there is none and create is False."""
    buf = C.create_string_buffer(4096)
    n = C.c_int64()
    rc = load_host().gauss_host_panel_cache(_enc(reference_index_file), _enc(reference_data_file), _enc(reference_pop_desc_file),
                                            1 if create else 0, buf, len(buf), C.byref(n))
    if rc < 0:
        _hcheck(rc)
    return (buf.value.decode(), n.value) if rc == 0 else (None, 0)


def impute_chromosome(kind, chr, start_bp, end_bp, wing_size, input_file, reference_data_file, reference_pop_desc_file,
                      study_pop=None, pop_wgt_df=None, af1_cutoff=None, window_size=1_000_000, rank=0, world=1, n_batches=0,
                      ctx=None, reference_index_file=None):
    """dist / distmix / qcat / qcatmix over every window of [start_bp, end_bp] as ONE native call
    (gauss_host_impute_chromosome): windows sharded over `world` ranks, this rank's windows pipelined through the
    GPU in batches against the resident packed panel.  reference_data_file: a packed panel, or the reference's BGZF
    text panel together with reference_index_file (packed on first use into the panel cache).  Returns a ChromResult."""
    import time
    t0 = time.perf_counter()
    h = load_host()
    names, w, n = (None, None, 0) if pop_wgt_df is None else _pop_wgt(pop_wgt_df)
    out, st = _vp(), ChromStats()
    t1 = time.perf_counter()
    _hcheck(h.gauss_host_impute_chromosome(_ctx(ctx), int(kind), int(chr), int(start_bp), int(end_bp), int(wing_size),
                                           int(window_size), _enc(study_pop), names, None if w is None else w.ctypes.data_as(_dp), n,
                                           _enc(input_file), _enc(reference_index_file), _enc(reference_data_file),
                                           _enc(reference_pop_desc_file),
                                           _af(af1_cutoff), int(rank), int(world), int(n_batches), C.byref(out), C.byref(st)))
    t2 = time.perf_counter()
    owner = _TableOwner(h, out)                                  # frees the table when the last reference to it is gone
    cols = _columns(h, out, owner=owner)                         # views: the table lives as long as any of its columns
    t3 = time.perf_counter()
    windows = _named(h, out)["windows"]
    msgs = [h.gauss_table_message(out, k).decode() for k in range(h.gauss_table_n_messages(out))]
    stats = {k: getattr(st, k) for k, _ in ChromStats._fields_}
    # the wrapper's own time around the native call (ms): arguments in, columns out, the rest (named matrix, messages, free, stats)
    stats["py_ms"] = dict(args=(t1 - t0) * 1e3, native=(t2 - t1) * 1e3, columns=(t3 - t2) * 1e3, rest=(time.perf_counter() - t3) * 1e3)
    res = ChromResult(cols, windows, stats, msgs)
    res._owner = owner                                           # (a table without rows has no view to keep it)
    return res


def chrom_window_view(kind, chr, start_bp, end_bp, wing_size, input_file, packed_file, reference_pop_desc_file, study_pop=None,
                      pop_wgt_df=None, af1_cutoff=None):
    """gauss_host_chrom_window_view (no GPU): one window as the chromosome driver builds it on a sorted packed panel.
    Returns (snps DataFrame, dict of named vectors rows_m / rows_u / z1 / counts, guard message or None)."""
    h = load_host()
    names, w, n = (None, None, 0) if pop_wgt_df is None else _pop_wgt(pop_wgt_df)
    out = _vp()
    _hcheck(h.gauss_host_chrom_window_view(int(kind), int(chr), int(start_bp), int(end_bp), int(wing_size), _enc(study_pop), names,
                                           None if w is None else w.ctypes.data_as(_dp), n, _enc(input_file), _enc(packed_file),
                                           _enc(reference_pop_desc_file), _af(af1_cutoff), C.byref(out)))
    named = {k: v.reshape(-1) for k, v in _named(h, out).items()}
    msgs = [h.gauss_table_message(out, k).decode() for k in range(h.gauss_table_n_messages(out))]
    df = _table(h, out)[0]
    return df, named, (msgs[0] if msgs else None)


def impute_genome(kind, chromosomes, wing_size, input_file, reference_data_file, reference_pop_desc_file, study_pop=None,
                  pop_wgt_df=None, af1_cutoff=None, window_size=1_000_000, rank=0, world=1, depth=2, ctx=None, reference_index_file=None,
                  raise_on_error=True):
    """gauss_host_impute_genome: gauss_host_impute_chromosome for every (chr, start_bp, end_bp) of `chromosomes`, `depth` calls in
    flight on the context at a time (host threads of the library), so that one call's host part runs under the other's GPU work.
    Returns one ChromResult per chromosome, identical to what impute_chromosome returns for it (raise_on_error=False: None in
    the place of a chromosome that failed, and the first failure's message as a second return value)."""
    h = load_host()
    names, w, n = (None, None, 0) if pop_wgt_df is None else _pop_wgt(pop_wgt_df)
    nc = len(chromosomes)
    chrs = np.ascontiguousarray([c[0] for c in chromosomes], dtype=np.int32)
    lo = np.ascontiguousarray([c[1] for c in chromosomes], dtype=np.int64)
    hi = np.ascontiguousarray([c[2] for c in chromosomes], dtype=np.int64)
    outs = (_vp * nc)()
    sts = (ChromStats * nc)()
    rc = h.gauss_host_impute_genome(_ctx(ctx), int(kind), nc, chrs.ctypes.data_as(C.POINTER(C.c_int32)), lo.ctypes.data_as(C.POINTER(_i64)),
                                    hi.ctypes.data_as(C.POINTER(_i64)), int(wing_size), int(window_size), _enc(study_pop), names,
                                    None if w is None else w.ctypes.data_as(_dp), n, _enc(input_file), _enc(reference_index_file),
                                    _enc(reference_data_file), _enc(reference_pop_desc_file), _af(af1_cutoff), int(rank), int(world), int(depth),
                                    outs, sts)
    res = []
    for c in range(nc):
        if not outs[c]:
            res.append(None)
            continue
        out = _vp(outs[c])
        cols = _columns(h, out)
        windows = _named(h, out)["windows"]
        msgs = [h.gauss_table_message(out, k).decode() for k in range(h.gauss_table_n_messages(out))]
        h.gauss_table_free(out)
        res.append(ChromResult(cols, windows, {k: getattr(sts[c], k) for k, _ in ChromStats._fields_}, msgs))
    if not raise_on_error:
        return res, (h.gauss_host_last_error().decode() if rc != 0 else None)
    _hcheck(rc)
    return res


class Prepared:
    """Host data layer output for one window / gene set (no GPU involved): gauss_host_prepare."""

    def __init__(self, kind, chr=0, start_bp=0, end_bp=0, wing_size=0, study_pop=None, pop_wgt_df=None, input_file=None,
                 annotation_file=None, reference_index_file=None, reference_data_file=None, reference_pop_desc_file=None,
                 af1_cutoff=None):
        self.h = load_host()
        names, w, n = (None, None, 0) if pop_wgt_df is None else _pop_wgt(pop_wgt_df)
        self._keep = (names, w)
        out = _vp()
        _hcheck(self.h.gauss_host_prepare(int(kind), int(chr), int(start_bp), int(end_bp), int(wing_size), _enc(study_pop),
                                          names, None if w is None else w.ctypes.data_as(_dp), n, _enc(input_file),
                                          _enc(annotation_file), _enc(reference_index_file), _enc(reference_data_file),
                                          _enc(reference_pop_desc_file), _af(af1_cutoff), C.byref(out)))
        self.handle = out
        c = [C.c_int() for _ in range(5)]
        self.h.gauss_prepared_counts(out, *[C.byref(x) for x in c])
        self.M, self.U, self.N, self.P, self.n_gene = [x.value for x in c]
        a, b = C.c_int(), C.c_int()
        self.h.gauss_prepared_qcat_counts(out, C.byref(a), C.byref(b))
        self.n_head, self.n_pred = a.value, b.value

    def snps(self):
        return _table(self.h, self.h.gauss_prepared_snps(self.handle), free=False)[0]

    def _arr(self, fn, n, dtype):
        p = fn(self.handle)
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dtype).copy() if (n and p) else np.zeros(0, dtype)

    def measured_rows(self):
        return self._arr(self.h.gauss_prepared_measured_rows, self.M, np.int32)

    def unmeasured_rows(self):
        return self._arr(self.h.gauss_prepared_unmeasured_rows, self.U, np.int32)

    def pop_off(self):
        return self._arr(self.h.gauss_prepared_pop_off, self.P + 1, np.int32)

    def pop_wgt(self):
        return self._arr(self.h.gauss_prepared_pop_wgt, self.P, np.float64)

    def z1(self):
        return self._arr(self.h.gauss_prepared_z1, self.M, np.float64)

    def gene_off(self):
        return self._arr(self.h.gauss_prepared_gene_off, self.n_gene + 1 if self.n_gene else 0, np.int32)

    def _geno(self, fn, rows):
        ld = _i64()
        p = fn(self.handle, C.byref(ld))
        if not rows:
            return np.zeros((0, self.N), dtype=np.uint8)
        a = np.ctypeslib.as_array(p, shape=(rows, ld.value))
        return a[:, : self.N]          # a view: keep `self` alive while using it

    def geno_m(self):
        return self._geno(self.h.gauss_prepared_geno_m, self.M)

    def geno_u(self):
        return self._geno(self.h.gauss_prepared_geno_u, self.U)

    def packed_store(self):
        """(host pointer, bytes, row stride) of the packed panel's genotype section, or None for byte matrices."""
        base, nb, rb = C.c_void_p(), _i64(), _i64()
        _hcheck(self.h.gauss_prepared_packed_store(self.handle, C.byref(base), C.byref(nb), C.byref(rb)))
        return (base.value, nb.value, rb.value) if base.value else None

    def window_rows(self, packed_file=None, ctx=None):
        """For a packed-panel object: dict(rows_m, rows_u, pop_src_off, ld[, store]) -- the panel rows of its SNPs and,
        when `packed_file` is resident on `ctx`, the device pointer of the panel's row 0."""
        rm, ru, so = (C.POINTER(C.c_int32)() for _ in range(3))
        n = C.c_int()
        _hcheck(self.h.gauss_prepared_store_rows(self.handle, C.byref(rm), C.byref(ru), C.byref(so), C.byref(n)))
        arr = lambda p, k: (np.ctypeslib.as_array(p, shape=(k,)).astype(np.int32).copy() if k else np.zeros(0, np.int32))
        out = dict(rows_m=arr(rm, self.M), rows_u=arr(ru, self.U), pop_src_off=arr(so, n.value), ld=self.packed_store()[2])
        if packed_file is not None:
            dev = C.c_void_p()
            _hcheck(self.h.gauss_host_panel_device_rows(_ctx(ctx), _enc(packed_file), C.byref(dev)))
            out["store"] = dev.value
        return out

    def window_desc(self):
        d = _lib.WindowDesc()
        _hcheck(self.h.gauss_prepared_window_desc(self.handle, C.byref(d)))
        return d

    def finish(self):
        out = _vp()
        _hcheck(self.h.gauss_prepared_finish(self.handle, C.byref(out)))
        return _table(self.h, out)[0]

    def jepeg_plan(self, world):
        """gauss_prepared_jepeg_plan: first[r] = rank r's first gene (contiguous ranges of equal cost), first[world] = genes in all."""
        first = (C.c_int32 * (int(world) + 1))()
        _hcheck(self.h.gauss_prepared_jepeg_plan(self.handle, int(world), first))
        return [int(v) for v in first]

    def jepeg_finish(self, g0, g1, blocks):
        """gauss_prepared_jepeg_finish: the gene table of genes [g0, g1) from their CorG blocks (a list of n_g x n_g arrays, or
        their concatenation; diagonal 1 + lambda)."""
        flat = np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1) for b in blocks]) if len(blocks)
                                    else np.zeros(1), dtype=np.float64)
        out = _vp()
        _hcheck(self.h.gauss_prepared_jepeg_finish(self.handle, int(g0), int(g1), flat.ctypes.data_as(_dp), C.byref(out)))
        return _table(self.h, out)[0]

    def close(self):
        if self.handle:
            self.h.gauss_prepared_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
