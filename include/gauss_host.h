/*
 * gauss_host.h -- C ABI of libgauss_host.so: the host side of the hot path, i.e. the
 * reference entry points with their reference argument lists, in plain C.
 *
 *   reference (Rcpp, src/RcppExports.cpp:335-340)          here
 *   -----------------------------------------------------  ------------------------------
 *   computeLD(chr,start_bp,end_bp,pop_wgt_df,input_file,    gauss_host_computeLD
 *             reference_index_file,reference_data_file,
 *             reference_pop_desc_file,af1_cutoff)           computeLD.cpp:26-166
 *   dist(chr,start_bp,end_bp,wing_size,study_pop,...)       gauss_host_dist      dist.cpp:30-126
 *   distmix(chr,start_bp,end_bp,wing_size,pop_wgt_df,...)   gauss_host_distmix   distmix.cpp:30-135
 *   jepeg(study_pop,input_file,annotation_file,...)         gauss_host_jepeg     jepeg.cpp:28-153
 *   jepegmix(pop_wgt_df,input_file,annotation_file,...)     gauss_host_jepegmix  jepegmix.cpp:26-161
 *   qcat(chr,start_bp,end_bp,wing_size,study_pop,...)       gauss_host_qcat      qcat.cpp:30-132
 *   qcatmix(chr,start_bp,end_bp,wing_size,pop_wgt_df,...)   gauss_host_qcatmix   qcatmix.cpp:30-140
 *   prep_qcat(chr,start_bp,end_bp,wing_size,study_pop,...)  gauss_host_prep_qcat prep_qcat.cpp:16-205
 *   prep_recessive_impute(chr,...,pop_wgt_df,...)           gauss_host_prep_recessive_impute
 *                                                           prep_qcatmix.cpp:36-316
 *   prep_zmix5(input_file,...,percentile,interval)          gauss_host_prep_zmix5 zmix.cpp:44-190
 *   afmix(input_file,...,interval)                          gauss_host_afmix     afmix.cpp:30-215
 *   cpw2(input_file,...,interval)                           gauss_host_cpw2      cpw2.cpp:31-211
 *   zmix(input_file,...,percentile,interval,level)          gauss_host_zmix      zmix.R
 *
 * Same argument meaning, same defaults (af1_cutoff NaN = R's NULL -> 0.01, dist.cpp:53-57), same
 * row order (std::map order on (chr,bp,a1,a2), gauss.h:72-99), same column names and types as
 * the reference's DataFrames, same error texts (returned through gauss_host_last_error instead of
 * Rcpp::stop).  A pop_wgt_df is passed as two parallel arrays (names, weights).
 *
 * The host data layer (text + BGZF readers, allele matching, AF filters, window partition:
 * src/gauss.cpp:121-190, 293-399, 431-518, 543-604, 631-693, 720-785, 951-1117, 1275-1439) is
 * restated here in C++; the numeric part is delegated to libgauss_hip.so (include/gauss_hip.h).
 * The *_prepare functions run the host part alone (no GPU needed) and expose what would be handed
 * to the GPU; the farm harness and the CPU tests use them.
 */
#ifndef GAUSS_HOST_H
#define GAUSS_HOST_H

#include <stdint.h>

#include "gauss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gauss_table gauss_table;     /* a result DataFrame (column store)            */
typedef struct gauss_prepared gauss_prepared; /* one window/gene set after the host data layer */

#define GAUSS_COL_STR 0
#define GAUSS_COL_INT 1
#define GAUSS_COL_DBL 2

#define GAUSS_KIND_COMPUTELD 0
#define GAUSS_KIND_DIST      1
#define GAUSS_KIND_DISTMIX   2
#define GAUSS_KIND_JEPEG     3
#define GAUSS_KIND_JEPEGMIX  4
#define GAUSS_KIND_QCAT      5
#define GAUSS_KIND_QCATMIX   6
#define GAUSS_KIND_PREP_QCAT 7
#define GAUSS_KIND_PREP_RECESSIVE 8
#define GAUSS_KIND_AFMIX     9
#define GAUSS_KIND_CPW2      10
#define GAUSS_KIND_LDSCORE    11   /* gauss_host_dist_ldscore's window (pooled LD) */
#define GAUSS_KIND_LDSCOREMIX 12   /* gauss_host_distmix_ldscore's window (weighted LD) */

const char* gauss_host_last_error(void);

/* ---- result tables --------------------------------------------------------------------------- */
int gauss_table_nrow(const gauss_table* t);
int gauss_table_ncol(const gauss_table* t);
const char* gauss_table_colname(const gauss_table* t, int col);
int gauss_table_coltype(const gauss_table* t, int col);
const char* gauss_table_str(const gauss_table* t, int col, int row);
const int32_t* gauss_table_int(const gauss_table* t, int col);
const double* gauss_table_dbl(const gauss_table* t, int col);
/* A whole string column at once: NUL-separated values in one buffer (n values, *bytes long in total). */
const char* gauss_table_strcol(const gauss_table* t, int c, int64_t* bytes);
/* Named numeric members of a result List (prep_qcat's z_vec / cor_mat1 / cor_mat2, prep_recessive_impute's
 * zvec / cormat / cormat_add / cormat_dom / cormat_rec): nrow x ncol, COLUMN-major like an R NumericMatrix
 * (vectors have ncol = 1). */
int gauss_table_n_named(const gauss_table* t);
const char* gauss_table_named_name(const gauss_table* t, int k);
const double* gauss_table_named(const gauss_table* t, int k, int* nrow, int* ncol);
/* computeLD's `cormat` (n x n, symmetric); NULL for the other tables */
const double* gauss_table_matrix(const gauss_table* t, int* n);
void gauss_table_free(gauss_table* t);

/* ---- the five entry points (blocking; ctx from gauss_hip_init) -------------------------------- */
int gauss_host_computeLD(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp,
                         const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                         const char* input_file, const char* reference_index_file,
                         const char* reference_data_file, const char* reference_pop_desc_file,
                         double af1_cutoff, gauss_table** out);
int gauss_host_dist(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                    const char* study_pop, const char* input_file, const char* reference_index_file,
                    const char* reference_data_file, const char* reference_pop_desc_file,
                    double af1_cutoff, gauss_table** out);
int gauss_host_distmix(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                       const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                       const char* input_file, const char* reference_index_file,
                       const char* reference_data_file, const char* reference_pop_desc_file,
                       double af1_cutoff, gauss_table** out);
int gauss_host_jepeg(gauss_ctx* ctx, const char* study_pop, const char* input_file,
                     const char* annotation_file, const char* reference_index_file,
                     const char* reference_data_file, const char* reference_pop_desc_file,
                     double af1_cutoff, gauss_table** out);
int gauss_host_jepegmix(gauss_ctx* ctx, const char* const* pop_names, const double* pop_wgts,
                        int n_pop_wgt, const char* input_file, const char* annotation_file,
                        const char* reference_index_file, const char* reference_data_file,
                        const char* reference_pop_desc_file, double af1_cutoff, gauss_table** out);

/* jepeg() / jepegmix() on several GPUs (BASELINE.json configs[4], SURVEY.md section 8e: "genes: contiguous gene ranges or one
 * gene-batch per GPU").  Genes are independent (jepeg.cpp:114-131 builds and tests one Gene at a time; jepegmix.cpp:119-140;
 * grouping at gauss.cpp:1383-1439), so rank `rank` of `world` runs the host data layer on the same files as every other rank,
 * derives the same plan -- contiguous gene ranges of equal cost, a gene costing its SNP pairs n (n + 1) plus a constant for its
 * k x k tail -- and computes CorG (GPU) and the tails of ITS range only: no communication.  The tables of ranks 0 .. world-1,
 * concatenated in rank order, are gauss_host_jepeg(mix)'s table row for row, bit for bit.  The result carries the named matrix
 * "gene_range" [1 x 3] = first gene, one past the last gene, genes in all.  kind = GAUSS_KIND_JEPEG (study_pop) or
 * GAUSS_KIND_JEPEGMIX (pop_names / pop_wgts); rank 0 of world 1 is the reference's call. */
int gauss_host_jepeg_rank(gauss_ctx* ctx, int kind, const char* study_pop, const char* const* pop_names, const double* pop_wgts,
                          int n_pop_wgt, const char* input_file, const char* annotation_file, const char* reference_index_file,
                          const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff,
                          int rank, int world, gauss_table** out);
/* The loop over calls above that: n_calls independent jepeg() / jepegmix() calls -- the reference's user runs one per chromosome
 * file set (jepeg.cpp:28-34 takes one input / annotation / panel per call) -- dealt WHOLE to the ranks, longest first by the size of
 * the annotation file onto the least loaded rank (every rank sees the same files and derives the same deal; no communication).  A
 * call is host-bound (3.4 ms, of which 0.6 ms GPU), so whole calls per rank is the split that scales; the gene split above divides
 * only the GPU batch and the tails.  out[c] = call c's table on its owner, NULL on the other ranks; owner_out[c] (may be NULL) = the
 * rank that ran it.  reference_index_files may be NULL when every data file is a packed panel.  A call that fails leaves out[c] NULL,
 * the others still run, and the function returns -1 with the first failure's message. */
int gauss_host_jepeg_genome(gauss_ctx* ctx, int kind, int n_calls, const char* study_pop, const char* const* pop_names,
                            const double* pop_wgts, int n_pop_wgt, const char* const* input_files, const char* const* annotation_files,
                            const char* const* reference_index_files, const char* const* reference_data_files,
                            const char* reference_pop_desc_file, double af1_cutoff, int rank, int world, gauss_table** out,
                            int32_t* owner_out);
/* The two halves of gauss_host_jepeg_rank for a harness that computes CorG itself (the CPU tests put the oracle there): the plan
 * -- first[r] = rank r's first gene, first[world] = genes in all -- and the gene table of genes [g0, g1) from their CorG blocks
 * (concatenated n_g x n_g, row-major, diagonal 1 + lambda = 1.1).  No GPU needed. */
int gauss_prepared_jepeg_plan(const gauss_prepared* p, int world, int32_t* first);
int gauss_prepared_jepeg_finish(const gauss_prepared* p, int g0, int g1, const double* blocks, gauss_table** out);

/* Leave-one-out re-imputation of the measured SNPs: the input check before a dist() / distmix() result is trusted.  Same
 * arguments, same window (wings included), same data layer and the same single job as gauss_host_dist / gauss_host_distmix; the
 * job's window sets out_loo_z / out_loo_info / out_loo_t (include/gauss_hip.h).  The table lists the MEASURED SNPs inside
 * [start_bp, end_bp] in the reference's SNP order -- the wings' SNPs contribute to B11 and are not reported, as with QCAT --
 * with columns rsid chr bp a1 a2 af1ref|af1mix z z_loo info_loo t pval: z the study's Z-score, z_loo / info_loo what
 * dist() / distmix() would return for the SNP were it deleted from the study file, t = (z - mean_loo) sqrt((B11^-1)_ii) the
 * standardised residual (N(0, 1) under the model), pval = 2 pnorm(-|t|).  A flipped allele, a strand mix-up or a misplaced
 * SNP shows as a large |t|. */
int gauss_host_dist_loo(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                        const char* study_pop, const char* input_file, const char* reference_index_file,
                        const char* reference_data_file, const char* reference_pop_desc_file,
                        double af1_cutoff, gauss_table** out);
int gauss_host_distmix_loo(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                           const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                           const char* input_file, const char* reference_index_file,
                           const char* reference_data_file, const char* reference_pop_desc_file,
                           double af1_cutoff, gauss_table** out);

/* Stepwise conditional signal selection: how many independent signals a dist() / distmix() window holds.  Same arguments, same
 * window (wings included), same data layer and the same single job as gauss_host_dist / gauss_host_distmix; the job's window sets the
 * slct_* fields of gauss_window_desc (include/gauss_hip.h: the statistic, the greedy rule and the collinearity guard), so the
 * ancestry-weighted B11 of a mixed cohort serves where the usual tools need one homogeneous LD panel.
 *   p_cutoff     a SNP enters while its conditional two-sided p-value is below this (<= 0: 5e-8); the chi^2 threshold is
 *                gauss_host_slct_chi2(p_cutoff)
 *   collin       a SNP whose un-ridged r^2 with the selected set reaches this is not considered (<= 0: 0.9); passed on as
 *                slct_min_var_frac = 1 - collin / (1 + lambda)^2
 *   max_signals  at most this many SNPs are selected (<= 0: 32 = GAUSS_SLCT_MAX, the most)
 *   cond_rsids   n_cond SNPs that enter first, in this order, whatever their p-value (max_signals == n_cond: a pure conditional
 *                analysis on the list).  One that is not a measured SNP of the extended window is an error that names it.
 * The table lists EVERY measured SNP of the extended window in the reference's SNP order -- the wings take part: a signal in a wing
 * must be conditioned on, not hidden -- with columns rsid chr bp a1 a2 af1ref|af1mix z wing order z_entry z_joint z_cond pval_cond
 * var_left: wing 1 outside [start_bp, end_bp]; order 1 .. n for the selected SNPs in order of entry, else 0; z_entry the conditional z
 * at entry and z_joint the joint z of the selected SNPs (NaN unless selected); z_cond the z given all selected SNPs (NaN for the
 * selected SNPs and those the guard excludes), pval_cond = 2 pnorm(-|z_cond|); var_left the share of the SNP's variance the
 * selected SNPs leave.  A window without unmeasured SNPs is refused, as by dist() / distmix(). */
int gauss_host_dist_slct(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                         const char* study_pop, const char* input_file, const char* reference_index_file,
                         const char* reference_data_file, const char* reference_pop_desc_file,
                         double af1_cutoff, double p_cutoff, double collin, int max_signals,
                         const char* const* cond_rsids, int n_cond, gauss_table** out);
int gauss_host_distmix_slct(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                            const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                            const char* input_file, const char* reference_index_file,
                            const char* reference_data_file, const char* reference_pop_desc_file,
                            double af1_cutoff, double p_cutoff, double collin, int max_signals,
                            const char* const* cond_rsids, int n_cond, gauss_table** out);
/* The imputed SNPs conditioned on the selected signals: is an imputed hit a signal of its own or the shadow of the lead SNP?
 * Arguments, window, data layer, single job and refusals of gauss_host_dist_slct / gauss_host_distmix_slct; the job's window also sets
 * out_cond_z / out_cond_var of gauss_window_desc (include/gauss_hip.h: the statistic and why its variance is info, not 1), with
 * cond_min_var_frac = 1 - collin: the ridge does not cap what the signals explain of an imputed SNP, so the (1 + lambda)^2 of the
 * measured SNPs' guard has no place here.
 * The table opens with the rows of gauss_host_dist / gauss_host_distmix for the same call, in the same order and with the same bits
 * in their columns (rsid chr bp a1 a2 af1ref|af1mix z pval info type); below them follow the measured SNPs of the wings in
 * gauss_host_dist_slct's order (info 1, type 1), so that every selected SNP has a row.  Appended columns: wing order z_cond pval_cond
 * var_left.  A measured row carries gauss_host_dist_slct's values; an imputed row carries order 0, z_cond = the conditional z of the
 * imputed SNP (NaN where the selected SNPs leave it less than 1 - collin of its variance), pval_cond = 2 pnorm(-|z_cond|) and
 * var_left = the share of its variance they leave.  z_entry / z_joint of the n selected SNPs are the named matrix `signals`
 * [n x 3], in order of entry: table row (from 0), z_entry, z_joint. */
int gauss_host_dist_cond(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                         const char* study_pop, const char* input_file, const char* reference_index_file,
                         const char* reference_data_file, const char* reference_pop_desc_file,
                         double af1_cutoff, double p_cutoff, double collin, int max_signals,
                         const char* const* cond_rsids, int n_cond, gauss_table** out);
int gauss_host_distmix_cond(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                            const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                            const char* input_file, const char* reference_index_file,
                            const char* reference_data_file, const char* reference_pop_desc_file,
                            double af1_cutoff, double p_cutoff, double collin, int max_signals,
                            const char* const* cond_rsids, int n_cond, gauss_table** out);
/* Credible sets of the selected signals: for each signal, which SNPs -- measured or imputed -- could be the causal one?
 * Arguments, window, data layer, single job, refusals and table of gauss_host_dist_cond / gauss_host_distmix_cond (the same rows, the
 * same bits in the shared columns); the job's window also sets the cs_* fields of gauss_window_desc (include/gauss_hip.h: the
 * leave-one-signal-out statistic, the Bayes factor, the membership rule) with
 *   coverage   rho in (0, 1]: the share of a signal's posterior mass its set holds; <= 0 or NaN: 0.95
 *   prior_var  omega > 0: prior variance of the causal SNP's non-centrality, in z units; <= 0 or NaN: 25.0 (a prior s.d. of 5: a
 *              documented default of this project, not a measured value)
 * coverage > 1 and a non-finite prior_var are refused by the window (GAUSS_E_INVALID).
 * Appended columns: pip (1 - prod over the signals of 1 - pip_ia), cs (the 1-based order of entry of the set that holds the SNP, as in
 * the `order` column; 0: in none) and cs_pip (its pip in that set; 0: none).  Named matrices: `signals` as gauss_host_dist_cond has
 * it, and `sets` [n x 4] in order of entry: table row of the lead SNP (from 0), size, mass, lse.
 * Limits: the candidates are the measured SNPs of the extended window and the unmeasured SNPs of the prediction window, so a signal
 * near a window edge has a truncated set; one causal SNP per signal; uniform prior; z units; at most GAUSS_SLCT_MAX signals. */
int gauss_host_dist_cs(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                       const char* study_pop, const char* input_file, const char* reference_index_file,
                       const char* reference_data_file, const char* reference_pop_desc_file,
                       double af1_cutoff, double p_cutoff, double collin, int max_signals,
                       const char* const* cond_rsids, int n_cond, double coverage, double prior_var, gauss_table** out);
int gauss_host_distmix_cs(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                          const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                          const char* input_file, const char* reference_index_file,
                          const char* reference_data_file, const char* reference_pop_desc_file,
                          double af1_cutoff, double p_cutoff, double collin, int max_signals,
                          const char* const* cond_rsids, int n_cond, double coverage, double prior_var, gauss_table** out);
/* Multi-causal fine-mapping of the window: the "sum of single effects" model (SuSiE-RSS) fitted to the measured z with the imputed
 * SNPs as candidates beside the measured ones -- unlike the credible sets above it does not condition on one selected SNP per signal,
 * so a measured SNP that tags two causal SNPs does not mislead it.  Arguments, window, data layer, single job and refusals of
 * gauss_host_dist / gauss_host_distmix; the job's window also sets the susie_* fields of gauss_window_desc (include/gauss_hip.h: the
 * model, the fit, the sets, their purity) with
 *   L                   effects; <= 0: 10; at most GAUSS_SUSIE_MAX_L
 *   coverage            rho in (0, 1]; <= 0 or NaN: 0.95
 *   prior_var           omega > 0, prior variance of an effect in z units; <= 0 or NaN: 25.0 (this project's documented default, as above)
 *   min_abs_corr        purity a reported set needs; <= 0 or NaN: 0.5
 *   max_sweeps          <= 0: 100; at most GAUSS_SUSIE_MAX_SWEEPS (the window refuses more)
 *   tol                 the fit stops when no alpha moved by this much in a sweep; 0 or NaN: 1e-4; negative: exactly max_sweeps sweeps
 *                       (`fit` then reports converged = 0 whatever delta is, and no message is added: running them out was asked for)
 *   estimate_prior_var  0: the prior variance stays omega; otherwise (negative: the default) it is re-estimated every sweep
 *   measured_only       > 0: only the measured SNPs are candidates (plain SuSiE-RSS on z and B11)
 * Table: the call's own rows (same order, same bits in the shared columns), then the measured SNPs of the wings, so that every
 * candidate has a row (gauss_host_dist_cond's row set, without its conditional columns).  Appended columns: wing, pip, cs (the 1-based
 * effect of the kept set that holds the SNP; 0: none) and cs_pip.  Named matrices: `effects` [L x 7]: table row (from 0) of the SNP of
 * largest alpha, V, lse, size, mass, purity, kept; `fit` [1 x 3]: sweeps, the last delta, converged.  A message is added when the
 * sweeps ran out (GAUSS_ST_SUSIE_NOCONV) and when the window was not fitted (GAUSS_ST_SUSIE_NOFIT, GAUSS_ST_NONFINITE).
 * Limits: the candidates are the measured SNPs of the extended window and the unmeasured SNPs of the prediction window; a window that
 * MakePosDef repairs is not fitted; z units; L <= 32; the residual variance is fixed at 1; uniform prior. */
int gauss_host_dist_susie(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                          const char* study_pop, const char* input_file, const char* reference_index_file,
                          const char* reference_data_file, const char* reference_pop_desc_file,
                          double af1_cutoff, int L, double coverage, double prior_var, double min_abs_corr, int max_sweeps,
                          double tol, int estimate_prior_var, int measured_only, gauss_table** out);
int gauss_host_distmix_susie(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                             const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                             const char* input_file, const char* reference_index_file,
                             const char* reference_data_file, const char* reference_pop_desc_file,
                             double af1_cutoff, int L, double coverage, double prior_var, double min_abs_corr, int max_sweeps,
                             double tol, int estimate_prior_var, int measured_only, gauss_table** out);
/* Joint fine-mapping across studies (gauss_hip.h, xs_group): n_studies = 2 .. GAUSS_XS_MAX GWAS of ONE trait, each with its own study
 * population (dist_xsusie: study_pops [n_studies]) or its own ancestry weights over the same population names (distmix_xsusie:
 * pop_wgts [n_studies][n_pop_wgt], row k study k's) and its own file (input_files [n_studies]), on one panel.  Every study's window
 * is built exactly as its own dist() / distmix() call builds it; a SNP may be measured in one study and imputed in another; the
 * candidates are those of study 1 that every study has (the panel SNP decides: alleles are already oriented to the panel).  One job
 * of n_studies windows.  The table is study 1's *_susie table -- its rows, then the measured SNPs of its wings; wing pip cs cs_pip
 * from the joint fit -- with `joint` appended (1: the SNP is a candidate of every study), the named matrices `effects`
 * [L x (2 n_studies + 5)] (table row of the SNP of largest alpha, V_1 .. V_K, purity_1 .. purity_K, lse, size, mass, kept) and `fit`
 * [1 x 3], and a message when the sweeps ran out or when the group was not fitted (MakePosDef repaired some study's B11).  A set is
 * reported when it is pure in at least one study.  The fit's arguments are those of *_susie. */
int gauss_host_dist_xsusie(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                           const char* const* study_pops, const char* const* input_files, int n_studies,
                           const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                           double af1_cutoff, int L, double coverage, double prior_var, double min_abs_corr, int max_sweeps,
                           double tol, int estimate_prior_var, int measured_only, gauss_table** out);
int gauss_host_distmix_xsusie(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                              const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                              const char* const* input_files, int n_studies,
                              const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                              double af1_cutoff, int L, double coverage, double prior_var, double min_abs_corr, int max_sweeps,
                              double tol, int estimate_prior_var, int measured_only, gauss_table** out);
/* Every trait of the window in one multi-causal fit, and the colocalisation of their signals: do two traits share a causal SNP in
 * this locus, or do they have two different ones in LD?  The arguments of gauss_host_dist_traits / _distmix_traits with 1 .. 7 further
 * study files (input_file is trait 1 and defines the window; a further file that lacks a measured SNP of the window is refused, as
 * there), the arguments of gauss_host_dist_susie / _distmix_susie, and coloc's priors p1, p2, p12 (<= 0 or NaN: 1e-4, 1e-4, 1e-5; they
 * must lie in (0, 1) with p12 <= min(p1, p2)).  The window sets coloc_traits_more = n_more and the coloc_* fields of gauss_window_desc
 * (include/gauss_hip.h: the definition): all traits are fitted in the same launches, every pair of kept effects of two traits is
 * colocalised, the imputed SNPs among the candidates.
 * The table: the rows of *_susie (the call's own, then the wings' measured SNPs); its columns wing pip cs cs_pip for trait 1 with the
 * same bits as *_susie on the first file; pip_t cs_t cs_pip_t for t = 2 .. 1 + n_more.  Named matrices: z_traits and pval_traits
 * (as *_traits, on every row); effects_t [L x 7] and fit_t [1 x 3] (the `effects` and `fit` of *_susie) for t = 1 .. 1 + n_more;
 * coloc, one row per pair of kept effects of two traits: trait_a trait_b (1-based) cs_a cs_b (1-based effects) n H0 H1 H2 H3 H4
 * hit_row (the table row, from 0, of the most likely shared SNP) hit_pp.  A message per trait whose sweeps ran out or that was not
 * fitted.  Limits: those of *_susie; eight traits; traits that lack measured SNPs are not fitted. */
int gauss_host_dist_coloc(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                          const char* study_pop, const char* input_file, const char* reference_index_file,
                          const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff,
                          const char* const* more_input_files, int n_more, int L, double coverage, double prior_var,
                          double min_abs_corr, int max_sweeps, double tol, int estimate_prior_var, int measured_only,
                          double p1, double p2, double p12, gauss_table** out);
int gauss_host_distmix_coloc(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                             const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                             const char* input_file, const char* reference_index_file,
                             const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff,
                             const char* const* more_input_files, int n_more, int L, double coverage, double prior_var,
                             double min_abs_corr, int max_sweeps, double tol, int estimate_prior_var, int measured_only,
                             double p1, double p2, double p12, gauss_table** out);
/* Polygenic score weights of the window: lassosum's elastic net on summary statistics (Mak et al. 2017), fitted by coordinate descent on
 * the window's own LD -- the ancestry-weighted B11 of distmix, the pooled one of dist -- over a grid of shrinkage values s and a path of
 * penalties lam; lam = 0 is ridge regression (LDpred-inf's estimator).  Arguments, window, data layer, single job and refusals of
 * gauss_host_dist / gauss_host_distmix; the job's window also sets the prs_* fields of gauss_window_desc (include/gauss_hip.h: the
 * model, the sweep, the stopping rule, the outputs) with
 *   n           the study's sample size, finite and > 2 (z becomes the correlation r = z / sqrt(n - 2 + z^2))
 *   s, n_s      shrinkage values in (0, 1]; NULL or n_s <= 0: 0.2, 0.5, 0.9, 1; at most GAUSS_PRS_MAX_S
 *   lam, n_lam  penalties >= 0 in the order each chain takes them; NULL or n_lam <= 0: 20 values log-spaced from 0.1 down to 0.001
 *               (lassosum's grid); at most GAUSS_PRS_MAX_LAM
 *   tol         a penalty is left when no weight moved by tol r_max in a sweep; 0 or NaN: 1e-4
 *   max_sweeps  <= 0: 100; at most GAUSS_PRS_MAX_SWEEPS (the window refuses more)
 * Table: one row per measured SNP of the extended window (the wings included), in matrix order: rsid chr bp a1 a2 af1ref|af1mix z r
 * wing.  Named matrices: `beta` [n_s n_lam x rows], the weights of grid cell i_s n_lam + i_lam; `grid` [n_s n_lam x 9]: s, lam, nnz,
 * sweeps, delta, br, bg, kkt, converged (the in-sample predicted R^2 of a cell is br^2 / bg).  A message is added when a cell ran its
 * sweeps out (GAUSS_ST_PRS_NOCONV) and when the window was not fitted (GAUSS_ST_NONFINITE).
 * Limits: weights for the measured SNPs of the extended window only -- an imputed SNP adds no information to a score; standardised-
 * genotype units (divide by sqrt(2 af (1 - af)) for per-allele weights); one trait; the tuning value (s, lam) is the caller's choice:
 * pseudovalidation needs genotypes of the target cohort. */
int gauss_host_dist_prs(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                        const char* study_pop, const char* input_file, const char* reference_index_file,
                        const char* reference_data_file, const char* reference_pop_desc_file,
                        double af1_cutoff, double n, const double* s, int n_s, const double* lam, int n_lam, double tol, int max_sweeps,
                        gauss_table** out);
int gauss_host_distmix_prs(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                           const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                           const char* input_file, const char* reference_index_file,
                           const char* reference_data_file, const char* reference_pop_desc_file,
                           double af1_cutoff, double n, const double* s, int n_s, const double* lam, int n_lam, double tol, int max_sweeps,
                           gauss_table** out);
/* LD scores of the window: l_j = sum_k r_jk^2 over the panel SNPs within wing_size bp of SNP j, on the ancestry-weighted LD of distmix or
 * the pooled LD of dist -- the input of LD-score regression for a cohort that has no matching LD-score file to download.  Arguments of
 * gauss_host_dist / gauss_host_distmix, and their population selection, allele orientation and af1_cutoff; ONE window per call.
 * The window is a kind of its own (GAUSS_KIND_LDSCORE / GAUSS_KIND_LDSCOREMIX, in both data layers):
 *   targets         the SNPs that are in both the study file and the panel with bp in [start_bp, end_bp]: the study file is the list of
 *                   SNPs to score (ldsc's --print-snps); its z column is read and ignored
 *   reference rows  EVERY other panel SNP of [start_bp - wing_size, end_bp + wing_size] that passes the af1 cutoff -- the panel SNPs
 *                   the study measured in the wings included (dist()'s unmeasured rows stop at the prediction window; these do not)
 * The job's one window is a GAUSS_WIN_LD window with the lds_* fields of gauss_window_desc (include/gauss_hip.h: the band, the order
 * of summation, the bias adjustment) and out_b11 = out_b21 = NULL: the scores are reduced on the device, the matrices never come back.
 * lds_radius = wing_size, so every target sees its whole neighbourhood.
 *   n   the sample size of the bias adjustment; <= 0 or NaN: dist -- the selected populations' sample count N; distmix -- Kish's
 *       effective size (sum w_p)^2 / sum (w_p^2 / n_p) over the populations of non-zero weight, the weights un-normalised as passed.
 *       Kish's size is this project's convention for a weighted panel, not a measurement
 * Table: one row per target: rsid chr bp a1 a2 af1ref|af1mix l2 l2_raw n_band (l2_raw = sum r^2, n_band = the rows in the band, l2 =
 * l2_raw (1 + 1 / (n - 2)) - n_band / (n - 2)).  Named matrix `ldscore` [1 x 4]: n_eff, M (the window's reference rows, targets
 * included), M_5_50 (those with min(af, 1 - af) > 0.05), radius.
 * Refused with a message: a window with no target; a window of more than GAUSS_HOST_LDSCORE_MAX_TARGETS targets or
 * GAUSS_HOST_LDSCORE_MAX_ROWS rows (shorten it).  The two numbers are a budget this call sets for its one job, not a limit of the
 * kernels: at both of them the window's fp64 matrices are B11 [8 192][8 192] = 0.5 GiB and B21 [122 880][8 192] = 7.5 GiB, the
 * parked chunk partials 2 048 chunks x 2 x 8 192 doubles = 0.25 GiB -- 8.25 GiB of workspace, which a card that also holds the
 * panel's rows gives without question; 6 times chr22's largest window in targets, 35 times in rows.  A window beyond them is a
 * mistyped one far more often than a wanted one, and it is refused on the host before anything is allocated.  Limits: one window per call; a bp radius only, no cM; scores for the study's SNPs
 * that the panel has; no stratified scores from files (gauss_window_desc.lds_annot through a job). */
#define GAUSS_HOST_LDSCORE_MAX_TARGETS 8192
#define GAUSS_HOST_LDSCORE_MAX_ROWS 131072
int gauss_host_dist_ldscore(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                            const char* study_pop, const char* input_file, const char* reference_index_file,
                            const char* reference_data_file, const char* reference_pop_desc_file,
                            double af1_cutoff, double n, gauss_table** out);
int gauss_host_distmix_ldscore(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                               const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                               const char* input_file, const char* reference_index_file,
                               const char* reference_data_file, const char* reference_pop_desc_file,
                               double af1_cutoff, double n, gauss_table** out);
/* The chi^2 (1 df) threshold of a two-sided p-value: the smallest double chi2 with 2 pnorm(-sqrt(chi2)) < p in the library's own
 * normal tail, found by bisection on the bit pattern -- monotone in p, and exact to the last bit that changes the comparison.
 * p must be positive. */
int gauss_host_slct_chi2(double p, double* out_chi2);

/* Many traits per window from one LD build.  A consortium array or a biobank has tens to hundreds of traits measured at the same
 * SNPs, and a window's LD -- the Gram products, B11's factorisation: nine tenths of a step -- depends on the panel, the weights
 * and the measured SNP set only.  Same arguments, same window, same data layer and the same single job as gauss_host_dist /
 * gauss_host_distmix; the job's window sets n_traits_more / z_more / out_z_more of gauss_window_desc (include/gauss_hip.h).
 *   input_file         trait 1: it defines the window, the measured set, the allele orientation and the AF filter exactly as in
 *                      the plain call, and its table is the plain call's, unchanged
 *   more_input_files   n_more (<= GAUSS_TRAITS_MORE_MAX = 63) further studies in the same format (rsid chr bp a1 a2 z).  Every
 *                      measured SNP of the extended window is looked up in each by (chr, bp, a1, a2): the same allele order gives
 *                      z, the swapped order -z (gauss.cpp:358-370), a key listed twice its later row; rows for SNPs trait 1 does
 *                      not measure are ignored.  A measured SNP that a file lacks (the message names the file, the first missing
 *                      rsid and the number missing), a z that is not finite and n_more > 63 are refused before any GPU work.
 * Two named matrices are added to the table (gauss_table_named): z_traits and pval_traits, [nrow x (1 + n_more)], column 0 the
 * table's own z / pval, column k trait k + 1 -- for a measured SNP its own oriented study z, for an unmeasured one the imputed z;
 * info is the same for every trait. */
int gauss_host_dist_traits(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                           const char* study_pop, const char* input_file, const char* reference_index_file,
                           const char* reference_data_file, const char* reference_pop_desc_file,
                           double af1_cutoff, const char* const* more_input_files, int n_more, gauss_table** out);
int gauss_host_distmix_traits(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                              const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                              const char* input_file, const char* reference_index_file,
                              const char* reference_data_file, const char* reference_pop_desc_file,
                              double af1_cutoff, const char* const* more_input_files, int n_more, gauss_table** out);

/* The same two calls for traits whose files lack some of trait 1's measured SNPs -- per-trait quality control (call rate in the
 * trait's own samples, MAF, HWE) drops a handful of SNPs per window from every file.  Arguments as above.  A measured SNP of the
 * extended window that a further file lacks is no error here: it becomes a bit of miss_more of gauss_window_desc, and the trait is
 * imputed as if it had been run alone on the SNPs it has -- the SNP itself is imputed for that trait like an unmeasured one, and
 * the trait's info at every unmeasured SNP is its own (a rank-|missing| downdate of the window's factorisation, no LD build per
 * trait; include/gauss_hip.h).  A z that is present and not finite is still refused.  Refused before any GPU work, naming the file,
 * the count and the limit: a file that lacks more than GAUSS_TRAITS_MISS_MAX = 32 of the window's measured SNPs, a window in which
 * more than GAUSS_TRAITS_MISS_UNION_MAX = 128 distinct SNPs are missing, and a file left with 10 or fewer of the window's measured
 * SNPs (min_num_measured_snp: the reference would refuse that trait, dist.cpp:145-151).
 * The table is trait 1's plain table, unchanged.  Named matrices [nrow x (1 + n_more)]: z_traits, pval_traits, info_traits,
 * type_traits; column 0 holds the table's own columns, column k trait k + 1.  A SNP that trait k + 1 lacks and that lies in the
 * prediction window shows its imputed z, its info and type 0 there (one in a wing has no row); n_missing [1 + n_more] gives, per
 * trait, how many of the window's measured SNPs its file lacked.
 * Column k is exactly the stand-alone gauss_host_dist / gauss_host_distmix table of file k + 1 (up to the rounding of another,
 * equally valid order of sums) when that file's SNPs in the extended window are a subset of trait 1's measured SNPs: rows for SNPs
 * trait 1 does not measure are ignored, as in the calls above, whereas a stand-alone call would use them. */
int gauss_host_dist_traits_miss(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                                const char* study_pop, const char* input_file, const char* reference_index_file,
                                const char* reference_data_file, const char* reference_pop_desc_file,
                                double af1_cutoff, const char* const* more_input_files, int n_more, gauss_table** out);
int gauss_host_distmix_traits_miss(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                                   const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                                   const char* input_file, const char* reference_index_file,
                                   const char* reference_data_file, const char* reference_pop_desc_file,
                                   double af1_cutoff, const char* const* more_input_files, int n_more, gauss_table** out);

/* QCAT / QCATMIX: same feeder as dist / distmix, the window core is
 * run_qcat (qcat.cpp:134-262) / run_qcatmix (qcatmix.cpp:144-297).  af1_cutoff NaN -> 0.05 for qcat
 * (qcat.cpp:53-57), 0.01 for qcatmix (qcatmix.cpp:61-65).  Output columns: rsid chr bp a1 a2
 * af1ref|af1mix z qcat_m qcat_t qcat_chisq qcat_pval type. */
int gauss_host_qcat(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                    const char* study_pop, const char* input_file, const char* reference_index_file,
                    const char* reference_data_file, const char* reference_pop_desc_file,
                    double af1_cutoff, gauss_table** out);
int gauss_host_qcatmix(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                       const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                       const char* input_file, const char* reference_index_file,
                       const char* reference_data_file, const char* reference_pop_desc_file,
                       double af1_cutoff, gauss_table** out);

/* Raw LD export.  prep_qcat (prep_qcat.cpp:16-205): snplist = every SNP of the
 * extended window after the AF filter (rsid chr bp a1 a2 af1ref z type); z_vec [M]; cor_mat1 [M x M] pooled
 * LD among the measured SNPs, unit diagonal; cor_mat2 [A x M] LD of ALL prediction-window SNPs (measured and
 * unmeasured) against them.  prep_recessive_impute (prep_qcatmix.cpp:36-316): SNPs are first re-oriented to
 * the minor allele (UpdateSnpToMinorAllele, gauss.cpp:1137-1184); snplist = the prediction-window SNPs
 * (rsid chr bp a1 a2 af1mix z type); zvec [M]; cormat [M x M] weighted LD; cormat_add / cormat_dom /
 * cormat_rec [A x M] with the prediction-window SNPs additive / dominant / recessive coded
 * (gauss.cpp:1196-1250, recoded on the device). */
int gauss_host_prep_qcat(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                         const char* study_pop, const char* input_file, const char* reference_index_file,
                         const char* reference_data_file, const char* reference_pop_desc_file,
                         double af1_cutoff, gauss_table** out);
int gauss_host_prep_recessive_impute(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                                     const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                                     const char* input_file, const char* reference_index_file,
                                     const char* reference_data_file, const char* reference_pop_desc_file,
                                     double af1_cutoff, gauss_table** out);

/* prep_zmix5 (zmix.cpp:44-190): every `interval`-th measured SNP, keep those whose
 * across-population allele-frequency variance var(AF)/(mean(1-mean)) exceeds its `percentile` quantile
 * (R stats::quantile type 7, restated), and tabulate for every pair of them z_i*z_j and the Pearson
 * correlation of their genotypes inside each of the panel's populations (on the GPU).  Result: named
 * matrix "data_mat", [n_pairs x (1 + n_pop)] column-major like the reference's NumericMatrix; the table
 * lists the selected SNPs (rsid chr bp a1 a2 z norm_var).  percentile NaN -> 0.99, interval <= 0 -> 1. */
int gauss_host_prep_zmix5(gauss_ctx* ctx, const char* input_file, const char* reference_index_file,
                          const char* reference_data_file, const char* reference_pop_desc_file,
                          double percentile, int interval, gauss_table** out);
/* The other pair selectors of the family (R/RcppExports.R:231-311, zmix.cpp:201-1076); same files, same output layout
 * (named matrix "data_mat": one row per listed SNP pair, z_i * z_j then one correlation column per population), which
 * pairs they list differs:
 *   prep_zmix      every interval-th measured SNP (<= 0: 1), all pairs                       zmix.cpp:940-1076
 *   prep_zmix2     pairs (i, i + offset), i = 0, interval, 2 interval, ... (<= 0: 1000, 3)   zmix.cpp:651-760
 *   prep_zmix3     every interval-th SNP with its next `steps` neighbours (<= 0: 1000, 5)    zmix.cpp:511-650
 *   prep_zmix4     for h = 0 .. interval-1: pairs (i, i + offset), i = h, h + interval, ...; data_mat has a leading
 *                  column h (<= 0: 1000, 3)                                                  zmix.cpp:363-510
 *   prep_zmix5_sup prep_zmix5's SNPs; correlations pooled per super-population, columns in order of first
 *                  appearance in the description file (CalCorSup)                            zmix.cpp:201-361, 1221-1246
 * The table lists the SNPs that occur in some pair (rsid chr bp a1 a2 z [norm_var]); named matrix "pairs" [n_pairs x 2]
 * gives each pair as rows of that table; the table's messages name the correlation columns (populations / groups). */
int gauss_host_prep_zmix(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                         const char* reference_pop_desc_file, int interval, gauss_table** out);
int gauss_host_prep_zmix2(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                          const char* reference_pop_desc_file, int interval, int offset, gauss_table** out);
int gauss_host_prep_zmix3(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                          const char* reference_pop_desc_file, int interval, int steps, gauss_table** out);
int gauss_host_prep_zmix4(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                          const char* reference_pop_desc_file, int interval, int offset, gauss_table** out);
int gauss_host_prep_zmix5_sup(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                              const char* reference_pop_desc_file, double percentile, int interval, gauss_table** out);

/* afmix() / cpw2(): population weights of a mixed-ancestry study from allele frequencies (afmix.cpp:30-215, cpw2.cpp:31-211).
 * input_file: header, then "rsid chr bp a1 a2 af1" per line (ReadInputAf, gauss.cpp:211-262; a key listed twice keeps its last
 * row).  The study is merged with the panel index like ReadReferenceIndexAll (gauss.cpp:431-518: a SNP whose alleles the panel
 * lists the other way round takes the panel's order and af1 -> 1 - af1; both orders in the study is "ERROR: input file contains
 * duplicates").  The S measured SNPs, in map order, are dealt round-robin to `interval` intervals (<= 0: 1000, R's NULL); each
 * interval's rows [af1, AF of every panel population] (cpw2: asin(sqrt(.)) of each) give W_i = MakePosDef(Cxx)^-1 Cxy on the GPU
 * (gauss_pop_weights); W = sum_i W_i / interval, negative -> 0, else rounded to 3 decimals.  S < interval is an error naming
 * both.  Result: the populations with wgt > 0 in panel order, columns sup.pop pop wgt (afmix) or pop wgt (cpw2); named matrices
 * "w_raw" [P x 1] (W of every population before the clamp and rounding, NaN kept), "w_interval" [interval x P] and "status"
 * [interval x 1] (GAUSS_ST_* bits); a message when weights are NaN -- an interval with one SNP (interval <= S < 2 interval)
 * has covariance 0/0 and the reference returns no population. */
int gauss_host_afmix(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                     const char* reference_pop_desc_file, int interval, gauss_table** out);
int gauss_host_cpw2(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                    const char* reference_pop_desc_file, int interval, gauss_table** out);
/* The host data layer of afmix / cpw2 alone (no GPU; kind = GAUSS_KIND_AFMIX or GAUSS_KIND_CPW2): the measured SNPs in the
 * reference's order (rsid chr bp a1 a2 af1study, af1study after the allele flip, untransformed), named matrices "x" [S x (P + 1)],
 * the interval-major matrix exactly as gauss_pop_weights receives it, and "interval_off" [(interval + 1) x 1]. */
int gauss_host_popwgt_inputs(int kind, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                             const char* reference_pop_desc_file, int interval, gauss_table** out);

/* zmix(): ancestry proportions of a study from its Z-scores (zmix.R).  level: GAUSS_ZMIX_POPULATION or
 * GAUSS_ZMIX_SUPERPOPULATION.  percentile NaN -> 0.9, interval <= 0 -> 10 (zmix.R's defaults, not prep_zmix5's 0.99 / 1).  The SNPs
 * are prep_zmix5's (every interval-th measured SNP whose norm_var is above the percentile); over every pair i < j of them the row
 * [z_i z_j, r_1 .. r_G] (r_g per population, or per super-population pooled as prep_zmix5_sup) is kept iff finite, and only
 * D = X^T X and d = X^T y are formed, on the GPU (gauss_zmix_normal_eq).  Then solve.QP's problem min 1/2 w^T D w - d^T w,
 * sum w = 1, w >= 0, -w >= -1 (gauss_host_zmix_qp), w / sum w, rounded to 5 decimals, / sum again.  Result: columns
 * Population SuperPopulation Weight (every population, description order) or SuperPopulation Weight (super-populations in order of
 * first appearance); named matrices "dmat" [G x G], "dvec" [G x 1], "w_unrounded" [G x 1] (w / sum w before the rounding),
 * "yty", "n_snp", "n_pairs", "n_rows" [1 x 1].  Errors with zmix.R's / solve.QP's messages: "zmix: no valid rows after
 * filtering." (fewer than two SNPs, or no finite row), a description file without Population_Abbreviation / Super_Population,
 * "matrix D in quadratic function is not positive definite!"; more than 64 groups is refused. */
/* simulateLD(): the LD of a simulated cohort with the ancestry mix pop_names / pop_wgts (simulateLD.cpp:34-252).  The SNPs are
 * computeLD's (same arguments, same selection, same snplist, same "Not enough number of SNPs loaded - computeLD not performed"
 * error).  Every population of the weight map (names upper-cased; unknown names ignored, weight 0 included) gets
 * (int)(w * sim_size) draws in PANEL order, each uniform_int_distribution<>(0, n_k - 1) -- written out as libstdc++ >= 11 draws it,
 * Lemire's method on a 64-bit product -- from ONE std::mt19937(seed).  seed = -1 draws the seed from std::random_device (the
 * reference's behaviour); 0 <= seed < 2^32 replays.  cormat is CalCor with n = sim_size over the drawn columns and
 * sim_size - n_drawn zero columns (simulateLD.cpp:161-199, util.cpp:49-70), 1.0 on the diagonal, NaN where a row is constant.
 * Refused where the reference is undefined: sim_size < 1, a negative or non-finite weight, sum of counts > sim_size.  Result:
 * computeLD's table and matrix, named members "counts" [P x 1] (flagged populations, panel order), "draws" [n_drawn x 2]
 * (flagged population index, sample) and "seed" [1 x 1], the seed used. */
int gauss_host_simulateLD(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, const char* const* pop_names,
                          const double* pop_wgts, int n_pop_wgt, int64_t sim_size, const char* input_file,
                          const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                          double af1_cutoff, int64_t seed, gauss_table** out);
/* The draws of gauss_host_simulateLD alone (no GPU, no panel: the description file gives the population sizes).  Result: columns
 * pop n count (the flagged populations, panel order) and the named members "counts", "draws", "seed" above. */
int gauss_host_simulate_draws(const char* reference_pop_desc_file, const char* const* pop_names, const double* pop_wgts,
                              int n_pop_wgt, int64_t sim_size, int64_t seed, gauss_table** out);

/* clump(): LD clumping (PLINK's --clump) of a region of a mixed-ancestry study on the ancestry-weighted LD of computeLD, which never
 * leaves the GPU (gauss_ld_clump_rows, include/gauss_hip.h: the rule).  The arguments are gauss_host_computeLD's plus four thresholds;
 * the SNPs are exactly computeLD's selection for the same arguments (same snplist, same "Not enough number of SNPs loaded" error).
 * key = z^2; a SNP is an index iff its two-sided p-value is below p1 and a member iff it is below p2: key_index =
 * gauss_host_slct_chi2(p1), key_member = gauss_host_slct_chi2(p2); r2: the smallest squared LD to the index; radius = kb * 1000 bp.
 * A NaN threshold (not given) takes PLINK's default: 1e-4, 1e-2, 0.5, 250.  Refused: p1 or p2 outside (0, 1], p2 < p1, r2 outside
 * [0, 1], kb < 0, a region of
 * more than GAUSS_CLUMP_MAX_M (8 192) SNPs.  Result: one row per SNP, columns rsid chr bp a1 a2 af1mix z pval clump index_rsid r2
 * (clump: the rank of the SNP's clump, 1 = the most significant index, 0 = in no clump; index_rsid "." and r2 NaN for none), and the
 * named matrix "clumps" [n_clumps x 4], one row per clump in rank order: the index SNP's table row (from 0), the clump's size, the bp
 * of its first and of its last member.  One region per call; clumps are cut at the region's edges (ask for kb more on each side); a bp
 * radius only; the study file decides which SNPs exist -- to clump imputed SNPs write the imputed table out as the study file; pval
 * is the file's z taken at face value (an imputed z has variance `info`). */
int gauss_host_clump(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, const char* const* pop_names, const double* pop_wgts,
                     int n_pop_wgt, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                     const char* reference_pop_desc_file, double af1_cutoff, double p1, double p2, double r2, double kb, gauss_table** out);

/* sumchi2() / sumchi2mix(): the gene-based sum-of-chi2 test (fastBAT, VEGAS, MAGMA's SNP-wise mean model) on the pooled /
 * ancestry-weighted LD, which never leaves the GPU (gauss_gene_sumchi2, include/gauss_hip.h: the pruning and the eigenvalues).  The
 * arguments are gauss_host_jepeg's / gauss_host_jepegmix's plus prune_r2 (NaN, not given: 0.9, fastBAT's default; outside (0, 1]:
 * refused).  The genes and their SNPs are exactly jepeg's for the same files (the annotation's categ and wgt columns are not used).
 * Inside a gene the SNPs are taken in position order (the order of the SNP list), whatever order jepeg's sort by gene id left them in.
 * Q = sum z^2 over the gene's SNPs that survive the pruning in position order; under the null Q ~ sum lambda_i chi2_1 with lambda the
 * eigenvalues of the kept SNPs' LD; pval = gauss_host_sumchi2_pval(lambda, Q).  Result: one row per gene, columns geneid num_snp
 * num_kept chisq pval lam_max n_pos status top_snp top_snp_pval message (top_snp: the SNP with the largest z^2 among all the gene's
 * SNPs, top_snp_pval = 2 pnorm(-|z|) of it; status: GAUSS_ST_* bits of gauss_gene_sumchi2; message: why pval is NaN, else empty),
 * and the named matrix "lam" [n_gene x 128]: each gene's eigenvalues, descending, NaN beyond num_kept.  A gene of more than
 * GAUSS_SUMCHI2_MAX_N (1 024) SNPs is refused; one whose pruned set exceeds GAUSS_SUMCHI2_MAX_KEPT (128), or whose solve did not
 * converge, gets pval NaN and a message.  z is taken at face value (an imputed z has variance `info`, not 1).  One rank only. */
int gauss_host_sumchi2(gauss_ctx* ctx, const char* study_pop, const char* input_file, const char* annotation_file,
                       const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                       double af1_cutoff, double prune_r2, gauss_table** out);
int gauss_host_sumchi2mix(gauss_ctx* ctx, const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                          const char* input_file, const char* annotation_file, const char* reference_index_file,
                          const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff,
                          double prune_r2, gauss_table** out);
/* P(sum_i lam_i chi2_1 > q), a pure function (no GPU).  lam [n]; lam_i <= 0 or NaN are left out (the weighted LD estimator is not
 * exactly positive semidefinite) and *n_pos (may be NULL) reports how many stay.  None left, or q NaN: NaN.  q <= 0: 1.  One left: the
 * exact tail 2 pnorm(-sqrt(q / lam)).  Else Kuonen's saddlepoint approximation (Biometrika 86, 1999): K(zeta) = -1/2 sum log1p(-2 zeta
 * lam_i); K'(zeta) = q solved on zeta < 1 / (2 lam_max) by 100 halvings of the bracket [0, 1 / (2 lam_max)] (q above the mean sum lam)
 * or [-n_pos / (2 q), 0] (below it); w = sign(zeta) sqrt(2 (zeta q - K)), v = zeta sqrt(K''), p = pnorm_upper(w + log(v / w) / w) in the
 * library's own normal tail (1e-300 is reachable).  Where x = (q - sum lam) / sqrt(2 sum lam^2) has |x| < 1e-3 that formula is 0 / 0:
 * there the one-term Edgeworth tail pnorm_upper(x) + dnorm(x) (kappa3 / 6) (x^2 - 1), kappa3 = 8 sum lam^3 / (2 sum lam^2)^1.5.  An
 * approximation: DESIGN.md states its measured accuracy against numerical inversion. */
int gauss_host_sumchi2_pval(const double* lam, int n, double q, double* p, int* n_pos);

/* ldsplit(): approximately independent LD blocks of a region of a mixed-ancestry study -- the splits of the region's SNPs into
 * K = 1 .. max_K contiguous blocks of min_size .. max_size SNPs that minimise the sum of r^2 between blocks -- on the ancestry-weighted
 * LD of computeLD, which never leaves the GPU (gauss_ld_split_rows, include/gauss_hip.h: the rule).  The arguments are
 * gauss_host_computeLD's plus the split's; the SNPs are exactly computeLD's selection for the same arguments (same snplist, same "Not
 * enough number of SNPs loaded" error).  thr_r2: a pair with r^2 below it costs nothing; max_r2: no pair with r^2 above it may end in
 * two blocks (1: off); kb: pairs further apart cost nothing.  NaN / 0 (not given) takes the default: thr_r2 0.02, min_size 50,
 * max_size 1000, max_K GAUSS_LDSPLIT_MAX_K, max_r2 0.3, kb none.  Refused: thr_r2 or max_r2 outside [0, 1], max_size outside
 * 1 .. GAUSS_LDSPLIT_MAX_SIZE (4 096), min_size outside 1 .. max_size, max_K outside 1 .. GAUSS_LDSPLIT_MAX_K (128), kb < 0, a region
 * of more than GAUSS_LDSPLIT_MAX_M (8 192) SNPs.  Result: computeLD's snplist (one row per SNP: rsid chr bp a1 a2 af1mix) and four
 * named matrices: "splits" [n x 5], one row per K that has a split, ascending: n_block, cost, perc_kept (sum of size^2 / M^2), cost2
 * (sum of size^2), max_size_used; "last" [n x the largest such K]: the snplist row (from 0) of every block's last SNP, -1 beyond the
 * row's K; "max_r2_at" [M + 1 x 1]: the largest r^2 that boundary b cuts; "n_nonfinite" [1 x 1]: band entries of the LD that are not
 * finite (a monomorphic SNP) and count as 0.  Which K to use is the caller's choice.  One region per call; sizes in SNPs, not in bp
 * or cM; the study file decides which SNPs exist. */
int gauss_host_ldsplit(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, const char* const* pop_names, const double* pop_wgts,
                       int n_pop_wgt, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                       const char* reference_pop_desc_file, double af1_cutoff, double thr_r2, int min_size, int max_size, int max_K,
                       double max_r2, double kb, gauss_table** out);

/* hess(): the eigenvalues of the ancestry-weighted LD of a block and the projections of one or more traits on its leading
 * eigenvectors -- what local heritability (HESS), local genetic covariance (rho-HESS) and LAVA's local correlation are computed
 * from -- on the LD of computeLD, which never leaves the GPU (gauss_ld_hess_rows, include/gauss_hip.h: the rule, the repair of
 * non-finite entries, n_pos and the projections).  The arguments are gauss_host_computeLD's with n_files study files in place of one:
 * the SNPs are exactly computeLD's selection for the first file and the same arguments (same snplist, same "Not enough number of
 * SNPs loaded" error); every further file is read as dist_traits reads its further files -- it must hold every selected SNP (refused
 * with a message naming the file and the first SNP it lacks), swapped alleles flip the sign of z.  k_max: projections per trait (0:
 * 256); eig_min: NaN takes 1e-6.  Refused: n_files outside 1 .. GAUSS_HESS_MAX_TRAITS (64), k_max outside 1 .. GAUSS_HESS_MAX_K
 * (1 024), eig_min outside [0, 1), a block of more than GAUSS_HESS_MAX_M (4 096) SNPs.  Result: computeLD's snplist (one row per SNP:
 * rsid chr bp a1 a2 af1mix) and four named matrices: "z" [M x n_files]; "lam" [M x 1], descending; "proj" [n_files x k_max], NaN
 * beyond min(k_max, n_pos); "solve" [1 x 4]: n_pos, sweeps, n_nonfinite, status (GAUSS_ST_HESS_NOCONV / GAUSS_ST_NONFINITE).  The
 * estimators -- h2, its standard error, covariance and correlation at the caller's k -- are a few sums over proj: api.hess_estimates
 * states them; they are not computed here.  One block per call; cut a region with gauss_host_ldsplit first. */
int gauss_host_hess(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, const char* const* pop_names, const double* pop_wgts,
                    int n_pop_wgt, const char* const* input_files, int n_files, const char* reference_index_file,
                    const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff, int k_max, double eig_min,
                    gauss_table** out);

#define GAUSS_ZMIX_POPULATION      0
#define GAUSS_ZMIX_SUPERPOPULATION 1
int gauss_host_zmix(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                    const char* reference_pop_desc_file, double percentile, int interval, int level, gauss_table** out);
/* zmix's quadratic program alone (no context, no GPU): D [P x P] row-major symmetric, d [P]; the Goldfarb-Idnani dual active-set
 * method of quadprog::solve.QP.  w_unrounded (may be NULL): the solution / its sum; w_final (may be NULL): that rounded to 5
 * decimals and normalised again.  Returns 0, or -1 with gauss_host_last_error() set (D not positive definite). */
int gauss_host_zmix_qp(const double* D, const double* d, int P, double* w_unrounded, double* w_final);

/* ---- packed panel -------------------------------------------------
 * Converts the reference's BGZF text panel (index + data + population description) into one mmap-able
 * file: SNP table, per-population allele frequencies and allele counts, and 2-bit genotype rows
 * (gauss_amd/csrc/host/packed_panel.h).  Passing that file as reference_data_file to any entry point
 * above selects the packed feeder (reference_index_file is then ignored): no inflate, no text parsing,
 * windows entered by binary search, each SNP row read once -- results are identical to the text path.
 * Returns the number of SNPs packed or -1. */
int64_t gauss_host_pack_panel(const char* reference_index_file, const char* reference_data_file,
                              const char* reference_pop_desc_file, const char* out_file);
/* The packed-panel cache ("auto-pack on first use").  The packed form of a text panel lives in a cache directory
 * ($GAUSS_PANEL_CACHE, else ".gauss_panel_cache" beside the data file, else /tmp/gauss_panel_cache_<uid>) under a name that
 * carries path, size and mtime of all three panel files.  Returns 0 and the packed panel's path in out_path (the data file
 * itself when it is packed already; *snps_packed_now > 0 when this call made it), 1 when there is no cached panel and
 * create == 0, -1 on error.  Concurrent callers (one rank per GPU) are serialised by a lock file; the panel appears by
 * rename.  Policy of the entry points, env GAUSS_AUTO_PACK: 0 = never use the cache; 1 = pack on first use everywhere;
 * unset = the one-window entry points use a cached panel when one exists, gauss_host_impute_chromosome makes it. */
int gauss_host_panel_cache(const char* reference_index_file, const char* reference_data_file,
                           const char* reference_pop_desc_file, int create, char* out_path, int out_len,
                           int64_t* snps_packed_now);
/* For a prepared window that reads a packed panel: the panel's genotype section (host pointer into the
 * mmap), its size and row stride, so a harness can upload it once with gauss_store_upload and run its
 * windows with on_device = 1.  base = NULL for byte-matrix windows. */
int gauss_prepared_packed_store(const gauss_prepared* p, const uint8_t** base, int64_t* bytes, int64_t* row_bytes);

/* ---- resident panels and whole-chromosome runs (the farm's native side) --------------------------------
 * gauss_host_panel_resident uploads the genotype section of a packed panel to the context's GPU once (pinned
 * double-buffered hipMemcpyAsync; later calls for the same file and context are no-ops) -- 288 GB of HBM hold
 * the whole 33KG panel.  gauss_host_panel_evict frees it (packed_file NULL: every panel of the context). */
int gauss_host_panel_resident(gauss_ctx* ctx, const char* packed_file, int64_t* bytes_uploaded);
int gauss_host_panel_evict(gauss_ctx* ctx, const char* packed_file);
/* Device pointer of row 0 of a resident panel (error if it is not resident on this context), and, for a prepared
 * object that reads a packed panel, the panel rows of its measured / unmeasured SNPs and the byte offset of each
 * selected population block inside a row: what gauss_ld_rows / gauss_gene_ld_batch_rows / a window descriptor take. */
int gauss_host_panel_device_rows(gauss_ctx* ctx, const char* packed_file, const void** out_device_ptr);
int gauss_prepared_store_rows(const gauss_prepared* p, const int32_t** rows_m, const int32_t** rows_u,
                              const int32_t** pop_src_off, int* n_pop_selected);

typedef struct gauss_chrom_stats {
    int32_t n_windows, n_windows_mine, n_skipped, n_failed, n_batches;
    int32_t n_merged_giveups;      /* batches whose merged Gram launch gave up waiting and were run again in the two-launch form
                                      inside their fetch (gauss_hip_counters; 0 in a healthy run)                              */
    int64_t imputed;               /* unmeasured SNPs imputed by this rank                                  */
    int64_t panel_bytes_uploaded;  /* 0 when the panel was already resident                                 */
    double t_total, t_plan, t_panel_upload;
    double t_feeder_wait;          /* main thread waiting for the data layer of the next batch              */
    double t_job_create;           /* planning + queuing the batches (the GPU keeps running meanwhile)      */
    double t_gpu_wait;             /* main thread waiting for a batch's results                             */
    double t_tables;               /* building and concatenating the result tables                          */
    double gpu_span_ms;            /* device time from the first batch's start to the last batch's results  */
    double t_tables_tail;          /* the part of t_tables behind the LAST batch's results (nothing overlaps it) */
} gauss_chrom_stats;

/* dist / distmix / qcat / qcatmix over every window [start_bp + k*window_size, ...] of [start_bp, end_bp] -- the
 * caller-level loop the reference leaves to the R user (one R call = one window, dist.cpp:30-126) -- as one native
 * call per rank.  Windows are sharded over `world` ranks by LPT on their LD flops (the same plan on every rank,
 * no communication); this rank's windows run as a pipeline of n_batches jobs (<= 0: chosen here): host threads
 * prepare batch b+1 and build the tables of batch b-1 while the GPU works on batch b.  reference_data_file is a packed
 * panel (reference_index_file may then be NULL) or the reference's BGZF text panel (gauss.cpp:293-399, 720-785), whose
 * packed form is made on first use and kept in the panel cache (gauss_host_panel_cache); it is made resident on first use.  The result holds the reference's output table of every
 * window of this rank in window order, an extra int column "window", a named matrix "windows"
 * [n_windows x 6: start_bp end_bp owner status measured unmeasured; status 0 done, 1 skipped by the ">10" guards
 * (dist.cpp:145-151), 2 failed, -1 another rank's] and one message per failed window (gauss_table_message):
 * a window that fails never takes the others with it. */
/* The planner's cost of a window with n_measured / n_unmeasured SNPs, per sample: the fp32 matrix flops the Gram kernel issues
 * for it (128-row tiles, 32 / 16 granular edges, B11's tile triangle) plus 8 % on B21's share for the per-entry tails.  What
 * gauss_host_impute_chromosome balances the ranks on; gauss_amd/farm.py:piece_cost is its Python twin. */
double gauss_host_plan_cost(int n_measured, int n_unmeasured);
int gauss_host_impute_chromosome(gauss_ctx* ctx, int kind, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                                 int64_t window_size, const char* study_pop, const char* const* pop_names,
                                 const double* pop_wgts, int n_pop_wgt, const char* input_file, const char* reference_index_file,
                                 const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff,
                                 int rank, int world, int n_batches, gauss_table** out, gauss_chrom_stats* stats);
/* The loop over chromosomes above that loop over windows: gauss_host_impute_chromosome for chromosome chr[c] over
 * [start_bp[c], end_bp[c]], c = 0 .. n_chrom-1, the same study / panel files and arguments for all of them (the reference's user
 * passes the same files and another `chr` per call, dist.cpp:30-60), with `depth` calls in flight on the context at any time
 * (<= 0: 2; host threads of the library): while one call's host part runs -- plan, data layer, job tables, result tables: ~2.5 ms
 * that nothing overlaps when a rank's share of a chromosome is a few windows -- the other call's batches keep the GPU busy.
 * out[c] / stats[c] (stats may be NULL) receive chromosome c's table and statistics exactly as gauss_host_impute_chromosome
 * returns them (same bits); a chromosome that fails leaves out[c] = NULL, the others still complete, and the call returns -1
 * with the first failure's message.  The caller frees every table. */
int gauss_host_impute_genome(gauss_ctx* ctx, int kind, int n_chrom, const int32_t* chr, const int64_t* start_bp, const int64_t* end_bp,
                             int64_t wing_size, int64_t window_size, const char* study_pop, const char* const* pop_names,
                             const double* pop_wgts, int n_pop_wgt, const char* input_file, const char* reference_index_file,
                             const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff,
                             int rank, int world, int depth, gauss_table** out, gauss_chrom_stats* stats);
/* A test / debugging view (no GPU): ONE window as gauss_host_impute_chromosome builds it on a sorted packed panel -- by a merge of
 * the study's rows and the panel's SNP table, both ordered by position, instead of the reference's per-SNP objects in a std::map
 * (gauss.cpp:121-190, 293-399, 543-693: what gauss_host_prepare restates).  Columns as gauss_prepared_snps (fpos = panel row; a
 * wing's unmeasured SNPs, which nothing reads, are not listed), named matrices "rows_m", "rows_u", "z1" and "counts" =
 * [measured, unmeasured, n_head, n_predm]; the ">10" guard's text, if the window trips it, is message 0. */
int gauss_host_chrom_window_view(int kind, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                                 const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                                 const char* packed_file, const char* reference_pop_desc_file, double af1_cutoff, gauss_table** out);
/* The host part of jepeg()/jepegmix() for ONE gene, given the CorG block the GPU produced (diagonal 1 + lambda):
 * Gene::RunJepeg bookkeeping + CalJepegPval from W on (gene.cpp:88-185, 317-550).  corg [n x n], has / wgt [n x 6]
 * row-major (category present, category weight).  top_categ / top_snp are indices (-1 when df = 0).  No GPU needed. */
int gauss_host_jepeg_gene_tail(int n, const double* corg, const double* z, const double* info, const int32_t* has,
                               const double* wgt, double* chisq, int32_t* df, double* jepeg_pval, int32_t* top_categ,
                               double* top_categ_pval, int32_t* top_snp, double* top_snp_pval);
int gauss_table_n_messages(const gauss_table* t);
const char* gauss_table_message(const gauss_table* t, int k);
/* A whole string column as one fixed-width, NUL-padded byte matrix [nrow x *width]. */
const char* gauss_table_strcol_fixed(const gauss_table* t, int c, int* width);

/* Re-block a BGZF text file line by line (reader + writer round trip); returns lines copied or -1. */
int64_t gauss_host_bgzf_copy(const char* in_path, const char* out_path);

/* Host threads used to inflate and split panel lines inside one prepare call (default 4). */
void gauss_host_set_threads(int n);

/* ---- host data layer only (no GPU) ----------------------------------------------------------- */
/* Runs everything up to and including ReadGenotype + the measured/unmeasured partition.
 * kind = GAUSS_KIND_*; arguments that a kind does not take are ignored (pass 0/NULL). */
int gauss_host_prepare(int kind, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                       const char* study_pop, const char* const* pop_names, const double* pop_wgts,
                       int n_pop_wgt, const char* input_file, const char* annotation_file,
                       const char* reference_index_file, const char* reference_data_file,
                       const char* reference_pop_desc_file, double af1_cutoff,
                       gauss_prepared** out);
/* SNP list after the AF filter (snp_vec of the reference), columns:
 * rsid chr bp a1 a2 af1 z info type fpos geneid
 * dist / distmix on a PACKED panel: wing SNPs of the panel that no study SNP shares a position with are not listed
 * (the reference enters them as type 0, filters them, and then neither imputes nor prints them: dist.cpp:91-93,132-140;
 * the text feeder lists them).  The window's result table is the same either way. */
const gauss_table* gauss_prepared_snps(const gauss_prepared* p);
int gauss_prepared_counts(const gauss_prepared* p, int* n_measured, int* n_unmeasured,
                          int* n_samples, int* n_pop, int* n_gene);
/* row indices (into the SNP list) of the measured / unmeasured SNPs, in matrix row order */
const int32_t* gauss_prepared_measured_rows(const gauss_prepared* p);
const int32_t* gauss_prepared_unmeasured_rows(const gauss_prepared* p);
/* genotype matrices exactly as they go to gauss_impute_window / gauss_ld (ASCII digits) */
const uint8_t* gauss_prepared_geno_m(const gauss_prepared* p, int64_t* ld);
const uint8_t* gauss_prepared_geno_u(const gauss_prepared* p, int64_t* ld);
const int32_t* gauss_prepared_pop_off(const gauss_prepared* p);
const double* gauss_prepared_pop_wgt(const gauss_prepared* p);
const double* gauss_prepared_z1(const gauss_prepared* p);
const int32_t* gauss_prepared_gene_off(const gauss_prepared* p);
/* QCAT windows: number of measured SNPs left of the prediction window and inside it (qcat.cpp:147-150) */
int gauss_prepared_qcat_counts(const gauss_prepared* p, int* n_head_measured, int* n_pred_measured);
/* Fill a window descriptor for gauss_job_create from a prepared dist/distmix/qcat/qcatmix window; the outputs
 * point into the prepared object and are written back into its SNP list by gauss_prepared_finish. */
int gauss_prepared_window_desc(gauss_prepared* p, gauss_window_desc* out);
/* After the GPU results are in: build the reference's output DataFrame (dist.cpp:91-124). */
int gauss_prepared_finish(gauss_prepared* p, gauss_table** out);
void gauss_prepared_free(gauss_prepared* p);

#ifdef __cplusplus
}
#endif
#endif /* GAUSS_HOST_H */
