/*
 * gauss_hip.h -- C ABI of libgauss_hip.so: the MI355X (gfx950) replacement for the numeric
 * hot path of statsleelab/gauss (LD matrix + DIST/DISTMIX Z-score imputation + JEPEG LD step).
 *
 * Boundary: the Rcpp entry points computeLD()/dist()/distmix()/jepeg()/
 * jepegmix() keep their signatures (R/RcppExports.R:28,57,74,88,102).  Inside the drivers, the
 * code between "genotype strings are in memory" (ReadGenotype, src/gauss.cpp:720-785) and
 * "z / info / cormat doubles" is replaced by one call into this library:
 *
 *   reference code being replaced                          entry point here
 *   -----------------------------------------------------  ---------------------------------
 *   computeLD.cpp:95-116  (CalWgtCov pair loops)           gauss_ld(mode=WEIGHTED, diag=1.0)
 *   dist.cpp:129-227      run_dist                         gauss_impute_window(mode=POOLED)
 *   distmix.cpp:138-253   run_distmix                      gauss_impute_window(mode=WEIGHTED)
 *   qcat.cpp:134-262      run_qcat                         gauss_impute_window(kind=QCAT, POOLED)
 *   qcatmix.cpp:145-286   run_qcatmix                      gauss_impute_window(kind=QCAT, WEIGHTED)
 *   gene.cpp:305-315      CorG via CalCor   (jepeg)        gauss_gene_ld_batch(mode=POOLED)
 *   gene.cpp:571-586      CorG via CalWgtCov (jepegmix)    gauss_gene_ld_batch(mode=WEIGHTED)
 *   util.cpp:49-70,103-124 (sumxy accumulation)            gauss_gram_counts (integer parity)
 *
 * Conventions
 *   - plain C types only; no exceptions cross the boundary.  Every call returns 0 on success
 *     or a negative GAUSS_E_* code; gauss_last_error() gives a thread-local message.  The
 *     Rcpp driver turns non-zero into Rcpp::stop(msg) (reference convention, dist.cpp:150).
 *   - the caller owns every input and output buffer; the library keeps nothing past return
 *     except inside handles it created (contexts, jobs).
 *   - genotype matrices are SNP-major: one SNP = one row of n_samples bytes, row stride `ld`
 *     bytes.  A byte is either the ASCII digit the reference stores ('0','1','2';
 *     Snp::genotype_vec_, src/snp.h:109) or the raw count 0..2; both decode as (byte & 0x0F).
 *     A row is the concatenation, in panel order, of the per-population strings of the
 *     selected populations: population p occupies columns [pop_off[p], pop_off[p+1]).
 *   - host-pointer calls are blocking (R's .Call semantics); the *_dev / job API is
 *     asynchronous on the context's streams and is what the multi-window farm uses.
 */
#ifndef GAUSS_HIP_H
#define GAUSS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAUSS_MODE_POOLED   0  /* CalCor, util.cpp:49-70   (dist, jepeg)                 */
#define GAUSS_MODE_WEIGHTED 1  /* CalWgtCov, util.cpp:103-124 (distmix, computeLD, jepegmix) */

#define GAUSS_OK            0
#define GAUSS_E_INVALID    -1  /* bad argument                                   */
#define GAUSS_E_DEVICE     -2  /* HIP runtime error                              */
#define GAUSS_E_NOMEM      -3  /* host or device allocation failed               */
#define GAUSS_E_RANGE      -4  /* exact-integer Gram range would be exceeded     */

/* per-window status bits returned in out_status */
#define GAUSS_ST_CLAMPED    1  /* MakePosDef rebuilt B11 (some eigenvalue < min_abs_eig, util.cpp:310) */
#define GAUSS_ST_NONFINITE  2  /* B11 not finite / not factorisable: outputs are NaN like the reference's */
#define GAUSS_ST_NOCONV     4  /* gauss_pop_weights: the Jacobi eigen-clamp hit its sweep cap (outputs NaN, NONFINITE set too) */
#define GAUSS_ST_SLCT_SKIPPED 8 /* signal selection: a forced SNP failed the collinearity guard and was left out */
#define GAUSS_ST_SUSIE_NOCONV 16 /* multi-causal fit: susie_max_sweeps sweeps ran without delta < susie_tol (values of the last sweep) */
#define GAUSS_ST_SUSIE_NOFIT  32 /* multi-causal fit: MakePosDef repaired B11 (GAUSS_ST_CLAMPED), the window is not fitted      */
#define GAUSS_ST_PRS_NOCONV  64 /* polygenic score weights: a (s, lam) ran prs_max_sweeps sweeps without delta < prs_tol r_max (last sweep's values) */
#define GAUSS_ST_SUMCHI2_TOOLARGE 128 /* gauss_gene_sumchi2: more than GAUSS_SUMCHI2_MAX_KEPT SNPs of the gene survive the pruning (eigenvalues NaN) */
#define GAUSS_ST_SUMCHI2_EMPTY    256 /* gauss_gene_sumchi2: no SNP of the gene is kept (an empty gene, or every row NaN) */
#define GAUSS_ST_HESS_NOCONV      512 /* gauss_ld_hess_rows: 30 sweeps of the block Jacobi ran and the last still rotated (last sweep's values) */

typedef struct gauss_ctx gauss_ctx;
typedef struct gauss_job gauss_job;

/* One imputation window (one R call of dist()/distmix()).  geno_m/geno_u may be host or
 * device pointers (see gauss_job_create's `on_device`). */
typedef struct gauss_window_desc {
    int mode;                 /* GAUSS_MODE_*                                                      */
    int n_pop;                /* P: selected populations (pooled mode may pass 1)                  */
    const int32_t* pop_off;   /* [P+1] column ranges; pop_off[P] = n_samples                       */
    const double* pop_wgt;    /* [P] weights in the same order (ignored for POOLED; may be NULL)   */
    int n_measured;           /* M: type-1 SNPs of the extended window (dist.cpp:137-138)          */
    int n_unmeasured;         /* U: type-0 SNPs of the prediction window (dist.cpp:135-136); 0 = LD only */
    const uint8_t* geno_m;    /* [M x ld] measured genotypes                                       */
    const uint8_t* geno_u;    /* [U x ld] unmeasured genotypes                                     */
    int64_t ld;               /* row stride in bytes (>= n_samples)                                */
    const double* z1;         /* [M] measured z-scores (host pointer, always)                      */
    double lambda;            /* ridge added to diag(B11): Arguments::lambda = 0.1 (gauss.cpp:20)  */
    double min_abs_eig;       /* MakePosDef floor: 1e-5 (gauss.cpp:21)                             */
    /* ---- polygenic score weights of the window (GAUSS_WIN_IMPUTE windows only) ------------------------------------
     * lassosum's model (Mak et al. 2017): elastic-net-penalised regression on summary statistics, solved by cyclic coordinate
     * descent on the window's own LD, over a grid of shrinkage values s and a path of penalties lam.  lam = 0 is ridge
     * regression (LDpred-inf's estimator).  Notation: B = B11 [M x M] as the job holds it -- lambda on the diagonal, pooled or
     * weighted as `mode` says, MakePosDef's repair included (the matrix the selection runs on); z = z1.
     *   r_j = z_j / sqrt(n - 2 + z_j^2)  (lassosum's p2cor; n = prs_n, the study's sample size);  r_max = max |r_j|
     *   a measured SNP whose z_j is not finite is FROZEN: r_j = 0, beta_j = 0, never updated
     * For s in (0, 1] and lam >= 0 the fit minimises
     *   f(beta) = beta' ((1 - s) B + s I) beta - 2 beta' r + 2 lam |beta|_1
     * One CHAIN per s = prs_s[i_s]: it starts from beta = 0, g = 0 (g stands for B beta) and takes prs_lam[0 .. n_lam) in the
     * caller's order, each from the solution of the one before it (a warm start).  One sweep at (s, lam), for j = 0 .. M - 1 in
     * order, frozen j skipped, den_j = (1 - s) B_jj + s:
     *   u  = r_j - (1 - s) (g_j - B_jj beta_j)
     *   b' = sign(u) (|u| - lam) / den_j  if |u| > lam, else 0
     *   D  = b' - beta_j;  if D != 0:  g_i += D * B_ji for every i (one multiply, one add, not contracted),  beta_j = b'
     * delta = max |D| over the sweep.  The chain leaves this lam when delta < prs_tol * r_max, or after prs_max_sweeps sweeps:
     * then GAUSS_ST_PRS_NOCONV is set and the values are those of the last sweep.  r_max = 0 (every z frozen, or zero): one
     * sweep, beta = 0, no status bit.  The algorithm has no reductions: every g_i is a fixed sequence of scalar updates, the
     * result does not depend on how the i are spread over lanes.
     * Per (s, lam), grid cell c = i_s * n_lam + i_lam:  beta [M];  nnz = #{beta_j != 0};  the sweeps run;  the last delta;
     *   br = beta' r and bg = beta' g, both summed in index order (the caller's in-sample predicted R^2 is br^2 / bg);
     *   kkt = the largest KKT residual of the stored beta, from g: with q_j = r_j - (1 - s) g_j - s beta_j,
     *         |q_j - lam sign(beta_j)| where beta_j != 0, max(0, |q_j| - lam) where it is 0 (frozen j skipped).
     * GAUSS_ST_NONFINITE windows return NaN, nnz 0, sweeps 0.  prs_n_s = 0: off (a zeroed block asks for nothing).
     * GAUSS_E_INVALID: QCAT / LD windows that ask; prs_n_s outside 1 .. GAUSS_PRS_MAX_S; prs_n_lam outside 1 ..
     * GAUSS_PRS_MAX_LAM; an s outside (0, 1]; a lam negative or not finite; prs_n <= 2 or not finite; prs_tol < 0 or not
     * finite; prs_max_sweeps outside 1 .. GAUSS_PRS_MAX_SWEEPS (the cap bounds what one window can keep a workgroup busy for:
     * with the caps every loop of the kernel is bounded); n_measured above GAUSS_PRS_MAX_M (beta, g, r and diag(B) of a chain
     * live in LDS).  The kernel (k_prs.hip) runs at the end of the job's tail, one workgroup per chain; fp64, not contracted,
     * no atomics.  Independent of every other rider.
     * Limits: weights for the measured SNPs of the extended window only (an imputed SNP adds no information to a score);
     * standardised-genotype units; one trait; the tuning value (s, lam) is the caller's choice -- pseudovalidation needs
     * genotypes of the target cohort.  (The block sits between the window's inputs and its outputs: every later field keeps its
     * neighbours.) */
    int      prs_n_s;          /* shrinkage values; 0 = off; at most GAUSS_PRS_MAX_S                           */
    int      prs_n_lam;        /* penalties of the path; 1 .. GAUSS_PRS_MAX_LAM                                */
    const double* prs_s;       /* [prs_n_s] each in (0, 1]                                     host pointer    */
    const double* prs_lam;     /* [prs_n_lam] each finite and >= 0, in the order the chain takes host pointer  */
    double   prs_n;            /* the study's sample size, finite and > 2                                      */
    double   prs_tol;          /* >= 0: a lam is left when delta < prs_tol * r_max                             */
    int      prs_max_sweeps;   /* 1 .. GAUSS_PRS_MAX_SWEEPS                                                    */
    double*  out_prs_beta;     /* [n_s][n_lam][M]                                host pointer / NULL, optional */
    int32_t* out_prs_nnz;      /* [n_s][n_lam]                                                 optional        */
    int32_t* out_prs_sweeps;   /* [n_s][n_lam]                                                 optional        */
    double*  out_prs_delta;    /* [n_s][n_lam]                                                 optional        */
    double*  out_prs_br;       /* [n_s][n_lam]                                                 optional        */
    double*  out_prs_bg;       /* [n_s][n_lam]                                                 optional        */
    double*  out_prs_kkt;      /* [n_s][n_lam]                                                 optional        */
    double* out_z;            /* [U] imputed z / sqrt(info)    (dist.cpp:200)  host pointer        */
    double* out_info;         /* [U] info = |b21 B11^-1 b12|   (dist.cpp:198)  host pointer        */
    int32_t* out_status;      /* [1] GAUSS_ST_* bits                           host pointer        */
    /* ---- LD scores of the window's measured SNPs (GAUSS_WIN_LD windows only) --------------------------------------
     * l_j = sum_k r_jk^2 over the window's SNPs within lds_radius bp of SNP j: the input of LD-score regression, reduced on the
     * device from the B11 / B21 the LD step leaves in HBM -- one number per SNP comes back, not the matrix (an asking window may
     * pass out_b11 = out_b21 = NULL: then nothing of the matrices is exported).  The SNP being scored is a TARGET: the M measured
     * rows are the targets, the U geno_u rows are the other reference SNPs.  Rows k = 0 .. M - 1 of the concatenated row space
     * are the measured rows (r_kj from B11), rows M .. M + U - 1 the geno_u rows (from B21); bp(k) = lds_bp_m[k] or
     * lds_bp_u[k - M].  Row k CONTRIBUTES to target j iff |bp(k) - lds_bp_m[j]| <= lds_radius.  With a_0(k) = 1 and a_c(k) =
     * lds_annot[c - 1][k] for the categories c = 1 .. C = lds_n_annot, over the contributing rows:
     *   raw[c][j]  = sum_k a_c(k) r_kj^2         mass[c][j] = sum_k a_c(k)         (mass[0][j]: the number of contributing rows)
     *   l2[c][j]   = raw (1 + 1 / (n - 2)) - mass / (n - 2),  n = lds_n: ldsc's r^2 - (1 - r^2) / (n - 2) summed, formed on the
     *                device in fp64 from the two totals in exactly that expression
     * The self term is in (it is 1: lambda must be 0).  A row outside the band is NOT READ into the sum (a select, not a product
     * with 0): a non-finite r outside a target's band does not reach that target.  Inside the band the arithmetic is plain: a NaN
     * r gives NaN, under a zero weight too.  Order of summation (fixed): rows are cut into chunks of
     * GAUSS_LDS_CHUNK, first the measured rows from row 0, then the geno_u rows from row M (a chunk never holds rows of both); a
     * chunk's partial starts at 0 and takes its contributing rows in ascending order, t = r r, then raw += a t, mass += a; the
     * totals start at 0 and take the chunks' partials in ascending order.  Not contracted, no atomics (k_ldscore.hip).
     * An LD window raises no status bit, with or without its scores (out_status is 0): a non-finite r shows as NaN in exactly the
     * targets whose band holds it.  lds_on = 0: off (a zeroed block asks for nothing).  GAUSS_E_INVALID: an asking
     * window that is not GAUSS_WIN_LD; lambda != 0; u_codings other than additive; lds_bp_m NULL, lds_bp_u NULL with U > 0, a
     * decreasing list; lds_n not finite or <= 2; lds_radius < 0; lds_n_annot outside 0 .. GAUSS_LDS_MAX_ANNOT; lds_annot NULL
     * with C > 0; a weight that is not finite; more than 65 535 chunks (4.19 M rows).  Limits: a bp radius only (no cM); the targets are the measured rows.  (The block
     * sits in front of the two matrices it stands in for: every other field keeps its neighbours.) */
    int      lds_on;           /* 0 = off, 1 = on                                                                 */
    int      lds_n_annot;      /* C: annotation categories beside the plain score, 0 .. GAUSS_LDS_MAX_ANNOT       */
    int64_t  lds_radius;       /* >= 0, in bp                                                                     */
    const int32_t* lds_bp_m;   /* [M] positions of the measured rows, non-decreasing             host pointer     */
    const int32_t* lds_bp_u;   /* [U] positions of the geno_u rows, non-decreasing; NULL only when U = 0          */
    double   lds_n;            /* the sample size of the bias adjustment, finite and > 2                          */
    const double* lds_annot;   /* [C][M + U] weights, measured rows first; NULL iff C = 0        host pointer     */
    double*  out_lds_raw;      /* [1 + C][M]                                    host pointer / NULL, optional     */
    double*  out_lds_l2;       /* [1 + C][M]                                                   optional           */
    double*  out_lds_mass;     /* [1 + C][M]                                                   optional           */
    double* out_b11;          /* optional [M x M] B11 incl. lambda (symmetric)  host pointer / NULL */
    double* out_b21;          /* optional [U x M] row-major                     host pointer / NULL */
    /* ---- joint fine-mapping across studies: one fit over 2 .. GAUSS_XS_MAX windows of one job (needs susie_L > 0) ----
     * The windows of a job that carry the same xs_group > 0 form a GROUP: one study each (its own populations or weights, its
     * own measured SNPs and scores), fitted together under the assumption that effect l sits at the SAME SNP in every study,
     * with its own size in each (the cross-population "sum of single effects" model, SuSiEx / MESuSiE).  Studies k = 1 .. K in
     * job order; study 1 is the LEADER.  Study k has the per-window quantities of susie_* unchanged, in its own candidate
     * order (measured first): B_k, C_k, z_k, W_k = B_k^-1 C_k^T, zhat_k, d_k and adm_k.
     * Candidates: the joint candidates are the leader's candidates that are candidates of every study (a SNP may be measured in
     * one study and imputed in another).  xs_from_lead of study k maps leader candidate j to study k's candidate index, -1 for
     * absent; the leader's is NULL; NULL on a peer means the same index and needs equal n_measured and n_unmeasured.  Joint
     * admissible: every map entry >= 0 and adm_k true in every study (each study's own rules: a non-finite z_k makes that
     * study's unmeasured SNPs inadmissible; susie_measured_only applies).
     * Fit (IBSS, Gauss-Seidel over l; every sum in a fixed order: candidates in LEADER order, studies ascending):
     * V_lk = omega, bbar_lk = 0, f_k = 0.  One step (sweep, l):
     *   r_k     = zhat_k - (f_k - R_k bbar_lk)                                    per study, own order
     *   lbf_j   = sum_k ( r_kj^2 V_lk / (1 + V_lk d_kj) - log1p(V_lk d_kj) ) / 2  joint candidates (every V_lk = 0: lbf_j = 0)
     *   alpha_l = softmax over the admissible joint candidates;  lse_l = max + log(sum / n_adm)
     *   mu_lkj  = V_lk / (1 + V_lk d_kj) r_kj;  bbar_lk = alpha_l o mu_lk;  f_k and R_k bbar_lk as in susie_*
     *   susie_estimate_var:  V'_k = sum_j alpha_lj (mu_lkj^2 + s2_kj);  if lse(V'_1 .. V'_K) <= 0 every V_lk = 0 (joint,
     *                        absorbing), else V_lk = V'_k from the next sweep on
     * delta, the stop rule, GAUSS_ST_SUSIE_NOCONV, susie_tol = 0 and susie_max_sweeps are those of susie_*.
     * Sets: membership is that of susie_* on the joint lbf row in leader order.  purity_lk is the deterministic purity of susie_*
     * of the leader's <= 128 top members, evaluated in study k's LD through its map.  A set is kept when V_lk > 0 for some k,
     * max_k purity_lk >= susie_min_abs_corr and no kept earlier set has the same members.  (The maximum is this project's
     * decision: a set is pure if it is tight in at least one ancestry.)  pip, set and set_pip are those of susie_*, from the
     * shared alpha.
     * Outputs: the LEADER's out_susie_* carry the joint pip / set / set_pip / lse / mass / size / kept / alpha / sweeps in leader
     * order; its out_susie_V holds study 1's V, out_susie_purity the maximum, out_susie_mu study 1's mu.  out_xs_* on the leader
     * only.  A peer returns its own z / info (and whatever else it asks for) as it would alone.
     * Limits: the candidates are an intersection; residual variance is 1; the prior over the candidates is uniform; K <=
     * GAUSS_XS_MAX and L <= GAUSS_SUSIE_MAX_L.  A group in which ANY window is repaired by MakePosDef (GAUSS_ST_CLAMPED) or is
     * GAUSS_ST_NONFINITE is not fitted: the leader's sections get NaN / 0 / -1 and every member GAUSS_ST_SUSIE_NOFIT (a
     * NONFINITE member keeps that bit instead); every member's other outputs keep their bits.
     * GAUSS_E_INVALID: a group of one or of more than GAUSS_XS_MAX windows; members that differ in a susie_* argument; a peer
     * with out_susie_* / out_coloc_lbf or out_xs_* pointers; coloc_traits_more > 0 in a group; xs_from_lead with an entry
     * outside -1 .. M + U - 1 or one target named twice; a NULL xs_from_lead on a peer whose n_measured / n_unmeasured differ
     * from the leader's; xs_from_lead on a leader or without xs_group; xs_group < 0 or without susie_L; xs_group in
     * gauss_impute_window (a group needs a job).  Kernels: k_xsusie.hip; a job without a group launches what it launched before.
     * (The block sits in front of the QCAT block.) */
    int xs_group;                  /* 0 = off; equal positive ids in one job form a group, the first window is its leader */
    const int32_t* xs_from_lead;   /* [M_lead + U_lead] leader candidate -> this window's candidate, -1 = absent; NULL = the same index   host pointer */
    double*  out_xs_V;             /* [K][L] every study's V                                  leader, optional */
    double*  out_xs_purity;        /* [K][L] every study's purity                             leader, optional */
    double*  out_xs_mu;            /* [K][L][M_lead + U_lead] every study's mu, leader order  leader, optional */
    int32_t* out_xs_n;             /* [1] joint admissible candidates                         leader, optional */
    /* ---- QCAT / QCATMIX windows (run_qcat qcat.cpp:134-262, run_qcatmix qcatmix.cpp:145-286) ----
     * kind = GAUSS_WIN_QCAT tests, for the n_pred_measured measured SNPs of the prediction window
     * (rows n_head_measured .. of geno_m) and then the U unmeasured ones, the Pearson correlation
     * between L^-1 Z1 and L^-1 b (b = their row of B11 / B21; L = Cholesky factor of B11). */
    int kind;                 /* GAUSS_WIN_IMPUTE (0, default), GAUSS_WIN_QCAT or GAUSS_WIN_LD        */
    int n_head_measured;      /* measured SNPs with bp < start_bp (qcat.cpp:146-147)               */
    int n_pred_measured;      /* measured SNPs inside the prediction window (qcat.cpp:148-149)     */
    double eig_cutoff;        /* CountPC cutoff: Arguments::eig_cutoff = 0.01 (gauss.cpp:22)       */
    double* out_r;            /* [n_pred_measured + U] correlations, measured first   host pointer */
    int32_t* out_num_eig;     /* [1] CountPC(B11, eig_cutoff)                          host pointer */
    /* ---- every trait of the window in one fit, and the colocalisation of their signals (needs susie_L > 0) ---------
     * coloc_traits_more = k fits the first k rows of z_more as well as z1, with the window's susie_* arguments: 1 + k traits, at
     * most 1 + GAUSS_SUSIE_TRAITS_MORE_MAX.  For further trait t (row t - 1 of z_more) the definition above applies word for word
     * with z = z_more[t - 1] and m = out_z_more[t - 1] o sqrt(out_info); a non-finite value in z_more[t - 1] makes that trait's
     * unmeasured SNPs inadmissible.  B, C, W and d are the window's, formed once; each trait keeps its own state and stops at its
     * own sweep; the traits share every launch (the same susie_max_sweeps x L x 2 step launches).  Trait 1's out_susie_* keep the
     * bits of a window without coloc_traits_more, and a further trait's bits depend on its own row of z_more only: not on k, not
     * on the other rows, not on its place among them.  out_coloc_more_* are the further traits' out_susie_* with a leading [k]
     * dimension, every one optional; out_coloc_more_status [k] carries GAUSS_ST_SUSIE_NOCONV (and GAUSS_ST_SUSIE_NOFIT) per
     * trait, the window's own status word keeps meaning trait 1.  out_coloc_lbf / out_coloc_more_lbf: the log Bayes factors of
     * the last sweep's update of every effect, -inf at an inadmissible candidate.
     * Colocalisation (coloc's bf_bf, Wallace 2021, on the fit's per-effect Bayes factors; coloc_p1 = coloc_p2 = coloc_p12 = 0:
     * off): for fitted traits a < b, a kept effect la of a and a kept effect lb of b, with l1 = lbf row la of a, l2 = lbf row lb of
     * b, J = the candidates admissible in both fits, n = |J|:
     *   S1 = sum_J e^l1_j,  S2 = sum_J e^l2_j,  S12 = sum_J e^(l1_j + l2_j)
     *   lH0 = 0,  lH1 = log p1 + log S1,  lH2 = log p2 + log S2,  lH3 = log p1 + log p2 + log max(S1 S2 - S12, 0),
     *   lH4 = log p12 + log S12;   out_coloc_pp = softmax(lH) [5]: no causal SNP, one for a only, one for b only, two different
     *   ones, one shared;   out_coloc_hit = argmax_J (l1_j + l2_j) (ties: the smaller index), a candidate index, measured first --
     *   an imputed SNP can be the shared causal SNP of two traits that neither study measured;  out_coloc_hit_pp = e^(l1_hit +
     *   l2_hit) / S12.  Sums are shifted by their maxima and S1 S2 - S12 is formed in logs: with n = 1 PP.H3 is an exact 0.
     * Pairs are in the order (0, 1), (0, 2), .., (k - 1, k), trait 0 being z1.  A pair of effects that are not both kept gives
     * NaN / -1, and so does every pair when a fit was not made (GAUSS_ST_SUSIE_NOFIT, GAUSS_ST_NONFINITE) or n = 0.
     * GAUSS_E_INVALID: coloc_traits_more < 0, > n_traits_more or > GAUSS_SUSIE_TRAITS_MORE_MAX; coloc_traits_more > 0 with
     * susie_L = 0 or with miss_more (traits that lack measured SNPs are not fitted); a coloc parameter that is not finite, not in
     * (0, 1), or coloc_p12 > min(coloc_p1, coloc_p2); coloc parameters with fewer than two fitted traits; an out_coloc_more_* or
     * out_coloc_* pointer without what it belongs to.  Kernels: k_susie.hip (the trait is a grid dimension), k_coloc.hip (one
     * launch behind the fit).  (The block sits in front of u_codings: every later field keeps its neighbours, and every field of it
     * is named coloc_* / out_coloc_*: the traits are fitted for the sake of their pairs.) */
    int      coloc_traits_more;        /* k: rows of z_more fitted beside z1; 0 = trait 1 alone                             */
    double   coloc_p1;                 /* prior probability that a SNP is causal for the first trait of a pair only          */
    double   coloc_p2;                 /* ... for the second only                                                             */
    double   coloc_p12;                /* ... for both; <= min(coloc_p1, coloc_p2)                                            */
    double*  out_coloc_lbf;            /* [L][M+U] trait 1                                           optional              */
    double*  out_coloc_more_pip;       /* [k][M+U]                                                   optional              */
    int32_t* out_coloc_more_set;       /* [k][M+U]                                                   optional              */
    double*  out_coloc_more_set_pip;   /* [k][M+U]                                                   optional              */
    double*  out_coloc_more_V;         /* [k][L]                                                     optional              */
    double*  out_coloc_more_lse;       /* [k][L]                                                     optional              */
    double*  out_coloc_more_mass;      /* [k][L]                                                     optional              */
    double*  out_coloc_more_purity;    /* [k][L]                                                     optional              */
    int32_t* out_coloc_more_size;      /* [k][L]                                                     optional              */
    int32_t* out_coloc_more_kept;      /* [k][L]                                                     optional              */
    double*  out_coloc_more_alpha;     /* [k][L][M+U]                                                optional              */
    double*  out_coloc_more_mu;        /* [k][L][M+U]                                                optional              */
    double*  out_coloc_more_lbf;       /* [k][L][M+U]                                                optional              */
    double*  out_coloc_more_sweeps;    /* [k][2] sweeps run, the last delta                          optional              */
    int32_t* out_coloc_more_status;    /* [k] GAUSS_ST_SUSIE_NOCONV / GAUSS_ST_SUSIE_NOFIT           optional              */
    double*  out_coloc_pp;             /* [pairs][L][L][5], pairs = (k + 1) k / 2                    optional              */
    int32_t* out_coloc_hit;            /* [pairs][L][L] candidate index, -1: none                    optional              */
    double*  out_coloc_hit_pp;         /* [pairs][L][L]                                              optional              */
    int32_t* out_coloc_n;              /* [pairs] candidates admissible in both fits                 optional              */
    /* ---- raw LD export (prep_qcat prep_qcat.cpp:104-132, prep_recessive_impute prep_qcatmix.cpp:136-221) ----
     * kind = GAUSS_WIN_LD stops after the LD step: out_b11 = B11 (diagonal 1 + lambda; pass lambda = 0 for
     * the reference's 1.0) and out_b21 = the LD of the geno_u rows against the measured rows; no z1 needed.
     * u_codings (any kind, 0 = additive only) makes the device derive several codings of every geno_u row
     * (gauss.cpp:1196-1250): B21 then holds one block of n_unmeasured rows per selected coding, in the
     * order additive, dominant (0/1/2 -> 0/1/1), recessive (0/1/2 -> 0/0/1); out_b21 is
     * [n_codings * U x M].  Codes outside 0..2 are left unchanged, as in the reference. */
    int u_codings;            /* bit mask of GAUSS_CODE_*                                          */
    /* ---- multi-causal fine-mapping of the window (GAUSS_WIN_IMPUTE windows only) ----------------------------------
     * The "sum of single effects" model (SuSiE; on summary statistics SuSiE-RSS, Zou et al. 2022) fitted to the measured z,
     * with the unmeasured SNPs as candidates beside the measured ones, each with the variance an imputed SNP really has.
     * Unlike the credible sets of the stepwise selection (out_cs_*) it does not condition on one SNP per signal: a measured
     * SNP that tags two causal SNPs does not mislead it.  Notation: B = B11 [M x M] (lambda on the diagonal), C = B21 [U x M],
     * z = z1, A = [B | C^T] [M x T], T = M + U; candidates are indexed as in out_cs_*: measured first, then unmeasured.
     *   R = A^T B^-1 A [T x T, rank M];  zhat = A^T B^-1 z = [z ; m], m_u = out_z[u] sqrt(out_info[u]) (the conditional mean);
     *   d_j = R_jj = B_jj (measured), out_info[u] (unmeasured)
     * Model: z ~ N(A sum_l b_l, B), l = 1 .. L = susie_L; b_l has exactly one non-zero entry, at a candidate drawn uniformly from
     * the admissible ones, with value ~ N(0, V_l).  Residual variance 1 (z units), fixed.
     * Admissible: zhat_j finite, d_j finite and > 0; with susie_measured_only no unmeasured SNP; a non-finite value in z1 makes
     * every unmeasured SNP inadmissible.  An inadmissible candidate has alpha = mu = 0 and enters no sum.
     * Fit (IBSS, Gauss-Seidel over l, every sum in a fixed order): bbar_l = 0, V_l = omega = susie_prior_var, f = 0.  One sweep,
     * for l = 1 .. L in order:
     *   r      = zhat - (f - R bbar_l)
     *   lbf_j  = ( r_j^2 V_l / (1 + V_l d_j) - log1p(V_l d_j) ) / 2                    (V_l = 0: lbf_j = 0)
     *   lse_l  = log( (1 / n_adm) sum_j exp(lbf_j) ),   alpha_lj = exp(lbf_j - max) / sum_j exp(lbf_j - max)
     *   s2_j   = V_l / (1 + V_l d_j),   mu_lj = s2_j r_j
     *   bbar_l = alpha_l o mu_l;   f = (f - R bbar_l_old) + R bbar_l_new
     *   susie_estimate_var:  V' = sum_j alpha_lj (mu_lj^2 + s2_j);  V' = 0 if log((1 / n_adm) sum_j exp(lbf_j(V'))) <= 0;
     *                        V_l = V' from the next sweep on (susieR's "EM"); V_l = 0 is absorbing
     * After each sweep delta = max_lj |alpha_lj - alpha_lj(previous sweep)|; the fit stops when delta < susie_tol or after
     * susie_max_sweeps sweeps -- then GAUSS_ST_SUSIE_NOCONV is set and the values are those of the last sweep (susie_tol = 0
     * runs exactly susie_max_sweeps sweeps).  Nothing T x T is formed: with W = B^-1 C^T = X^T (X C^T) (X = L^-1, the rows the
     * solve holds), v = bbar_meas + W bbar_unmeas and R bbar = [B v ; C v]: two dependent matrix-vector products per (sweep, l).
     * Sets and summaries, from the final alpha:
     *   membership of set l: the rule of out_cs_set on alpha_l: alpha_lj > 0 and the mass ranked ahead (larger alpha; ties: the
     *     smaller index) below rho = susie_coverage; rho = 1 takes every alpha_lj > 0
     *   purity_l: the minimum, over the pairs of the min(size, 128) members of largest alpha (ties: the smaller index), of
     *     |R_ij| / sqrt(d_i d_j), R_ij = B_ij, C_ui or c_u . W_v; one member: 1; no member: NaN.  (susieR subsamples at random;
     *     this rule is deterministic on purpose.)
     *   kept_l = V_l > 0 and purity_l >= susie_min_abs_corr and no kept set l' < l has the same members
     *   per SNP: out_susie_pip = 1 - prod_{l: V_l > 0} (1 - alpha_lj);  out_susie_set = the kept l (0-based) of largest alpha_lj
     *     among the kept sets that hold it (ties: the smaller l; -1: none);  out_susie_set_pip = that alpha_lj (0: none)
     *   per effect: V_l (after the last sweep's update), lse_l, size, mass (of the members), purity, kept
     *   per window: out_susie_sweeps = sweeps run, the last delta
     * Not fitted: GAUSS_ST_NONFINITE windows return NaN, size 0, kept 0, set -1.  A window that MakePosDef repairs
     * (GAUSS_ST_CLAMPED) is NOT fitted either -- the same NaN / 0 / -1 and GAUSS_ST_SUSIE_NOFIT; its other outputs keep their
     * bits: the repaired path forms no rows of the inverse, and eigenvalues at 1e-5 are no ground for some hundred dependent
     * products.  susie_L = 0: off (a zeroed block asks for nothing).  GAUSS_E_INVALID: QCAT / LD windows that ask; susie_L
     * outside 1 .. GAUSS_SUSIE_MAX_L; susie_coverage outside (0, 1]; susie_prior_var <= 0; susie_tol < 0; susie_max_sweeps outside
     * 1 .. GAUSS_SUSIE_MAX_SWEEPS (every run queues susie_max_sweeps x L x 2 launches up front: the cap bounds what one window puts
     * on the queue); susie_min_abs_corr outside [0, 1]; any of them non-finite.  (A window without unmeasured SNPs is refused
     * as it is without the fit, with susie_measured_only too.)  No admissible candidate at all (every z1
     * non-finite): alpha = mu = 0, pip 0, lse NaN, sizes 0, purity NaN, nothing kept; no status bit.  Independent of the selection and of every other rider.  The
     * kernels (k_susie.hip) are queued behind the credible sets: susie_max_sweeps x L x 2 launches up front, a converged window
     * leaves its launches at once; fp64, no atomics.  (The block sits in front of the packed-rows block: every later field
     * keeps its neighbours.) */
    int      susie_L;             /* effects; 0 = off; at most GAUSS_SUSIE_MAX_L                              */
    double   susie_coverage;      /* rho in (0, 1]                                                           */
    double   susie_prior_var;     /* omega > 0: prior variance of an effect, in z units                      */
    double   susie_tol;           /* >= 0: the fit stops when no alpha moved by this much in a sweep          */
    double   susie_min_abs_corr;  /* in [0, 1]: purity a kept set needs                                       */
    double*  out_susie_pip;       /* [M+U] measured first                          host pointer / NULL       */
    int32_t* out_susie_set;       /* [M+U]                                                     optional      */
    double*  out_susie_set_pip;   /* [M+U]                                                     optional      */
    double*  out_susie_V;         /* [L]                                                       optional      */
    double*  out_susie_lse;       /* [L]                                                       optional      */
    double*  out_susie_mass;      /* [L]                                                       optional      */
    double*  out_susie_purity;    /* [L]                                                       optional      */
    int32_t* out_susie_size;      /* [L]                                                       optional      */
    int32_t* out_susie_kept;      /* [L]                                                       optional      */
    double*  out_susie_alpha;     /* [L][M+U]                                                  optional      */
    double*  out_susie_mu;        /* [L][M+U]                                                  optional      */
    double*  out_susie_sweeps;    /* [2] sweeps run, the last delta                            optional      */
    int      susie_max_sweeps;    /* 1 .. GAUSS_SUSIE_MAX_SWEEPS                                             */
    int      susie_estimate_var;  /* non-zero: V_l is re-estimated every sweep                               */
    int      susie_measured_only; /* non-zero: only the measured SNPs are candidates                         */
    /* ---- packed panel rows -------------------------------------------------
     * geno_format = GAUSS_GENO_2BIT: a genotype row is a 2-bit stream (sample s of a population block at bits
     * 2*(s%4) of byte s/4, codes 0..2), each selected population's block starting on a 16-byte boundary and
     * zero padded to a multiple of 64 samples.  pop_src_off[q] is the byte offset of selected population q
     * inside a row (NULL: the blocks follow each other in pop_off order); ld is the row stride in bytes.
     * rows_m / rows_u (either format): when non-NULL, geno_m / geno_u point at a row store (e.g. a whole
     * chromosome resident in HBM, see gauss_store_upload) and matrix row r is store row rows_x[r]. */
    int geno_format;          /* GAUSS_GENO_U8 (0, default) or GAUSS_GENO_2BIT                      */
    const int32_t* rows_m;    /* [M] store row of each measured SNP, or NULL          host pointer */
    const int32_t* rows_u;    /* [U] store row of each geno_u SNP, or NULL            host pointer */
    const int32_t* pop_src_off; /* [P] 2-bit format: byte offset of each population block, or NULL */
    /* ---- credible sets of the selected signals (needs slct_max > 0; the notation is that of the two blocks below) --
     * For each selected signal, which SNPs could be the causal one?  The candidates are the M measured SNPs (candidate index
     * 0 .. M-1) and the U unmeasured ones (M .. M+U-1), the latter with the variance an imputed SNP really has.  With B, z, S,
     * L, y, w_u, m_u, info_u of the selection's and the conditional block, w_i = L^-1 B_Si for a measured SNP, P = B_SS^-1,
     * beta = P z_S and g = L^-T w:
     *   given all of S:     measured i:   r_i = z_i - w_i . y,  v_i = B_ii - w_i . w_i
     *                       unmeasured u: r_u = m_u - w_u . y,  v_u = info_u - w_u . w_u
     *   signal a left out:  r' = r + g_a beta_a / P_aa,  v' = v + g_a^2 / P_aa,  zc = r' / sqrt(v')
     *                       (a rank-one update: nothing is factorised per signal)
     *   share of variance:  s = v' / B_ii (measured),  s = v' (unmeasured: the info scale already)
     * SNP sel[a] in its own set has zc = out_slct_joint[a] (the same bits) and v' = 1 / P_aa and is always a candidate;
     * sel[b], b != a, is no candidate of set a.  Any other measured SNP is a candidate of set a while
     * v' > slct_min_var_frac * B_ii and its z is finite, an unmeasured one while v' > cond_min_var_frac * info_u, info_u > 0 and its z is finite:
     * the two existing guards, applied to the leave-one-out variance (cond_min_var_frac is read whether or not out_cond_* ask).
     * With the causal SNP's non-centrality ~ N(0, cs_prior_var = omega), zc ~ N(0, 1 + omega s) under "this SNP is the
     * causal one of signal a", so
     *   lbf_ia = ( zc^2 omega s / (1 + omega s) - log1p(omega s) ) / 2         -inf for a non-candidate
     *   lse_a  = log sum_i exp(lbf_ia),   pip_ia = exp(lbf_ia - lse_a)         uniform prior over the candidates
     * Candidate i is in credible set a iff pip_ia > 0 and the mass ranked ahead of it (larger pip_ia; ties: the smaller
     * candidate index) is below cs_coverage = rho: the shortest prefix whose mass reaches rho (rho = 1: every candidate
     * with pip_ia > 0).  Per candidate:
     *   out_cs_pip = 1 - prod_a (1 - pip_ia);  out_cs_set = the 0-based signal a of largest pip_ia among the sets that hold
     *   it (ties: the smaller a), -1 for none;  out_cs_set_pip = that pip_ia, 0 for none.
     * Per signal: out_cs_size = members, out_cs_mass = the sum of their pip_ia (>= rho), out_cs_lse = lse_a; slots a >= n hold
     * size 0 and NaN.  Nothing selected (n = 0): pip 0, set -1, set_pip 0.  GAUSS_ST_NONFINITE windows return NaN, size 0
     * and set -1.  Any out_cs_* being non-NULL switches the computation on; with slct_max = 0, on QCAT and LD windows,
     * with cs_coverage outside (0, 1] or not finite, and with cs_prior_var <= 0 or not finite, that is GAUSS_E_INVALID.
     * One causal SNP per signal, z units.  Three kernels behind the conditional step (k_cs.hip), fp64, sums in a fixed
     * order.  (The block sits in front of the selection's: every later field keeps its neighbours, the leave-one-out arrays stay last.) */
    double   cs_coverage;      /* rho in (0, 1]                                                             */
    double   cs_prior_var;     /* omega > 0: prior variance of the causal SNP's non-centrality, in z units  */
    double*  out_cs_pip;       /* [M+U] measured first   host pointer / NULL; any out_cs_* non-NULL switches it on */
    int32_t* out_cs_set;       /* [M+U]                                                          optional   */
    double*  out_cs_set_pip;   /* [M+U]                                                          optional   */
    int32_t* out_cs_size;      /* [slct_max]                                                     optional   */
    double*  out_cs_mass;      /* [slct_max]                                                     optional   */
    double*  out_cs_lse;       /* [slct_max]                                                     optional   */
    /* ---- stepwise conditional signal selection among the measured SNPs (GAUSS_WIN_IMPUTE windows only) -----------
     * How many independent signals the window holds: condition on the top SNPs and look at what is left.  With B = B11
     * (lambda on the diagonal, after MakePosDef if it acted), z = z1 and S the ordered set of selected SNPs, the statistic
     * of SNP i given S is
     *   zc_i = (z_i - B_iS B_SS^-1 z_S) / sqrt(B_ii - B_iS B_SS^-1 B_Si).
     * Selection is greedy: at every step the admissible SNP with the largest zc_i^2 enters (ties: the smallest index; a
     * NaN never wins), until the largest falls below slct_chi2_stop or slct_max SNPs are in -- a partial Cholesky
     * factorisation of B whose pivot is the largest conditional chi^2, all in fp64 (k_slct.hip).
     * The collinearity guard: SNP i is admissible while it is not selected and its variance left,
     * v_i = B_ii - B_iS B_SS^-1 B_Si, exceeds slct_min_var_frac * B_ii.  The ridge caps what a duplicate SNP can explain:
     * for two identical rows B_ij = 1 and B_ii = 1 + lambda, so the explained share 1 - v_i / B_ii is 1 / (1 + lambda)^2
     * (0.826 at lambda = 0.1) and a plain "r^2 >= 0.9" test on it would never fire.  A caller that means "un-ridged
     * r^2 >= collin" passes slct_min_var_frac = 1 - collin / (1 + lambda)^2 (gauss_host_dist_slct does, collin = 0.9):
     * for one selected SNP that is exactly the pair's un-ridged r^2 >= collin, for several the same rule applied to the
     * explained share.
     * Forced SNPs (slct_forced, window-relative measured indices, distinct) enter first, in the caller's order, whatever
     * their chi^2; one that fails the guard is left out and sets GAUSS_ST_SLCT_SKIPPED, and it still uses up one of the
     * slct_max steps.  slct_max == n_slct_forced is a pure conditional analysis on a given list.
     * slct_max = 0: off.  Every output is optional.  GAUSS_ST_NONFINITE windows return n = 0, indices -1 and NaN;
     * M = 1 is computed normally (it enters iff z^2 / (1 + lambda) >= slct_chi2_stop).  QCAT and LD windows that set
     * slct_max, slct_max > GAUSS_SLCT_MAX, a bad forced index and n_measured > 32768 are GAUSS_E_INVALID.
     * (The block sits in front of the leave-one-out arrays, which stay the descriptor's last three fields.) */
    int slct_max;             /* K: most SNPs to select; 0 = off; at most GAUSS_SLCT_MAX                            */
    double slct_chi2_stop;    /* selection stops when the best conditional chi^2 is below this                      */
    double slct_min_var_frac; /* the collinearity guard (above)                                                     */
    const int32_t* slct_forced; /* [n_slct_forced] SNPs that enter first, in [0, M), distinct   host pointer / NULL */
    int n_slct_forced;        /* <= slct_max                                                                        */
    int32_t* out_slct_n;      /* [1] number of SNPs selected                           host pointer / NULL          */
    int32_t* out_slct_idx;    /* [slct_max] selected indices in order of entry, -1 beyond n            optional     */
    double* out_slct_zin;     /* [slct_max] conditional z at entry, NaN beyond n                       optional     */
    double* out_slct_joint;   /* [slct_max] joint z: (B_SS^-1 z_S)_a / sqrt((B_SS^-1)_aa), NaN beyond n  optional   */
    double* out_slct_zc;      /* [M] final conditional z, NaN where the SNP is not admissible          optional     */
    double* out_slct_var;     /* [M] variance left v_i / B_ii, every SNP                               optional     */
    /* ---- the imputed SNPs conditioned on the selected signals (needs slct_max > 0) --------------------------------
     * Whether an imputed hit is a signal of its own or the shadow of a selected SNP.  With B, z, S as above, L the Cholesky
     * factor of B_SS, y = L^-1 z_S (out_slct_zin), b_u row u of B21, m_u = b_u B^-1 z the unnormalised mean and
     * info_u = |b_u B^-1 b_u^T| (out_info):
     *   w_u = L^-1 b_u[S]^T      (forward substitution, sums in ascending order)
     *   out_cond_z[u]   = (m_u - w_u . y) / sqrt(info_u - w_u . w_u)
     *   out_cond_var[u] = (info_u - w_u . w_u) / info_u           the share of the imputed SNP's variance the signals leave
     * Under z ~ N(0, B), cov(m_u, z_S) = b_u[S], so m_u - b_u[S] B_SS^-1 z_S has variance info_u - b_u[S] B_SS^-1 b_u[S]^T:
     * out_cond_z is N(0, 1) where S explains everything -- conditioning an imputed z like a measured one (variance 1 in
     * place of info_u) is not.  m_u is taken as out_z[u] sqrt(out_info[u]).
     * The guard: u is admissible while info_u - w_u . w_u > cond_min_var_frac * info_u, else out_cond_z[u] is NaN;
     * out_cond_var is always written.  The ridge does NOT cap what the signals explain of an imputed SNP (an unmeasured
     * duplicate of an isolated selected SNP has info = 1 / (1 + lambda) and nothing left), so a caller that means
     * "r^2 >= collin" passes cond_min_var_frac = 1 - collin, without slct_min_var_frac's (1 + lambda)^2.
     * Nothing selected (n = 0): out_cond_z has the bits of out_z and out_cond_var is 1.  info_u = 0 or a non-finite z: NaN.
     * GAUSS_ST_NONFINITE windows return NaN.  Either output being non-NULL switches the computation on; with slct_max = 0,
     * and on QCAT and LD windows, that is GAUSS_E_INVALID. */
    double cond_min_var_frac; /* the guard of the imputed SNPs (above)                                                      */
    double* out_cond_z;       /* [U] conditional z of the unmeasured SNPs, NaN where not admissible  host pointer / NULL    */
    double* out_cond_var;     /* [U] share of variance left                                          host pointer / NULL    */
    /* ---- further traits on the same window (GAUSS_WIN_IMPUTE windows only) ---------------------------------------
     * A study rarely has one trait: the LD of a window depends on the panel, the weights and the measured SNP set only, so
     * n_traits_more further Z-score vectors measured at the SAME SNPs are imputed from the same B11 / B21 and the same
     * factorisation.  out_z_more[t][u] is what out_z[u] would be were the window run with z1 = z_more[t]: with B = B11
     * (lambda on the diagonal, after MakePosDef if it acted), g_t = B^-1 z_t, mean_ut = b21_u . g_t,
     *   out_z_more[t][u] = mean_ut / sqrt(out_info[u])                                              (dist.cpp:194-202);
     * out_info is the same for every trait.  Two kernels (k_traits.hip) form G = X^T (X Z) from the rows of X = L^-1 the
     * solve holds anyway and B21 G on the fp64 matrix cores.  out_z, out_info and the status are untouched, z1 keeps its own
     * path bit for bit; the further traits take another, equally valid order of fp64 sums.  A trait's values depend on its
     * own row of z_more only: not on n_traits_more, not on the other rows (a non-finite z_more[t] makes row t of the output
     * non-finite and moves no bit of another row).  Leave-one-out values and the signal selection stay statistics of z1.
     * n_traits_more = 0: off.  GAUSS_ST_NONFINITE windows return NaN for every trait.  QCAT and LD windows that ask,
     * n_traits_more < 0 or > GAUSS_TRAITS_MORE_MAX, and n_traits_more > 0 with z_more or out_z_more NULL are
     * GAUSS_E_INVALID.  (The block sits in front of the leave-one-out arrays, which stay the descriptor's last three fields.) */
    /* ---- further traits that lack some of the window's measured SNPs (needs n_traits_more > 0) -------------------
     * Per-trait quality control drops a handful of SNPs from every trait's file.  miss_more[t][m] != 0 says that further trait t
     * has no score at measured SNP m; z_more[t][m] is then not read as a value (anything, a NaN included, gives the bits 0.0
     * gives).  With D the set of SNPs trait t lacks (|D| = k), A = B^-1 = X^T X (X = L^-1), z0 = z_more[t] with zeros on D,
     * g0 = A z0, b_u row u of B21, y_u = A b_u^T and L_D L_D^T = A_DD (a principal block of a positive definite matrix):
     *   c      = -A_DD^-1 g0_D                    the conditional mean of the missing SNPs themselves
     *   mean_u = b_u . g0 + sum_{d in D} y_u[d] c_d
     *   out_info_more[t][u] = | out_info[u] - || L_D^-1 y_u[D] ||^2 |,   out_z_more[t][u] = mean_u / sqrt(out_info_more[t][u])
     *   for d in D: out_info_miss = | B_dd - (A_DD^-1)_dd |,   out_z_miss = c_d / sqrt(out_info_miss)
     * which is what run_dist / run_distmix return for trait t alone when the window is run with the measured SNPs outside D as
     * its measured set and the SNPs of D as further unmeasured SNPs -- a rank-k downdate of what the job holds, no
     * factorisation per trait; out_loo_* is the case k = 1.
     * Where MakePosDef does not act on B it does not act on a principal submatrix either (interlacing), so the identity with a
     * stand-alone run is exact; where it acted the values are defined on the repaired B, like every other rider's.
     * out_z_miss / out_info_miss hold one entry per set mask bit, in mask order (t ascending, then m ascending).  A trait with
     * an empty mask row gets its out_z_more bits of a call without a mask and the bits of out_info in out_info_more.
     * A trait's values depend on its own scores and its own mask row only: not on n_traits_more, not on the other traits'
     * scores or masks, not on how many distinct SNPs are missing in the window.  z1, out_z, out_info, the status, the
     * leave-one-out values and the selection stay statistics of trait 1 on all M SNPs, bit for bit.
     * miss_more = NULL: nobody lacks anything; the three outputs are not written.  More than GAUSS_TRAITS_MISS_MAX missing
     * SNPs in one trait, more than GAUSS_TRAITS_MISS_UNION_MAX distinct missing SNPs in the window, a trait left without a
     * measured SNP, miss_more without n_traits_more, miss_more with one of the three outputs NULL, and QCAT / LD windows that
     * pass it are GAUSS_E_INVALID.  (The block sits in front of the traits block.) */
    const uint8_t* miss_more; /* [T x M] row-major: non-zero = further trait t has no score at measured SNP m   host pointer / NULL */
    double* out_info_more;    /* [T x U] row-major: info per further trait                                      host pointer */
    double* out_z_miss;       /* [n_miss] imputed Z-scores of the SNPs a trait lacks, in mask order             host pointer */
    double* out_info_miss;    /* [n_miss] their info                                                            host pointer */
    int n_traits_more;        /* T: further traits; 0 = none; at most GAUSS_TRAITS_MORE_MAX                          */
    const double* z_more;     /* [T x M] row-major: Z-scores of the further traits at the measured SNPs  host pointer */
    double* out_z_more;       /* [T x U] row-major: their imputed Z-scores at the unmeasured SNPs        host pointer */
    /* ---- leave-one-out re-imputation of the measured SNPs (GAUSS_WIN_IMPUTE windows only) ------------------------
     * The input check of summary-statistics imputation: measured SNP i re-imputed from the other M - 1 measured SNPs of
     * the window, i.e. what run_dist / run_distmix return for SNP i when it is presented as the only unmeasured SNP.  With
     * B = B11 (lambda on the diagonal, after MakePosDef if it acted), d = diag(B^-1), g = B^-1 z1:
     *   mean_i = z1_i - g_i / d_i;  out_loo_info[i] = |B_ii - 1 / d_i| (dist.cpp:198);  out_loo_z[i] = mean_i / sqrt(info_i)
     *   (dist.cpp:200);  out_loo_t[i] = (z1_i - mean_i) sqrt(d_i) = g_i / sqrt(d_i), the standardised residual -- N(0, 1) under
     *   z1 ~ N(0, B): a flipped allele or a misplaced SNP shows as a large |t|.
     * Any of the three being non-NULL switches the computation on for that window (one pass over L^-1, which the solve
     * holds anyway); NULL = not wanted.  GAUSS_ST_NONFINITE windows return NaN; M = 1 returns info 0, z NaN,
     * t = z1 / sqrt(1 + lambda).  QCAT and LD windows that set one of them are GAUSS_E_INVALID. */
    double* out_loo_z;        /* [M] optional                                          host pointer */
    double* out_loo_info;     /* [M] optional                                          host pointer */
    double* out_loo_t;        /* [M] optional                                          host pointer */
} gauss_window_desc;

#define GAUSS_SLCT_MAX 32
#define GAUSS_PRS_MAX_S 8
#define GAUSS_PRS_MAX_LAM 32
#define GAUSS_PRS_MAX_SWEEPS 1000
#define GAUSS_PRS_MAX_M 4096
#define GAUSS_LDS_MAX_ANNOT 32          /* annotation categories of a window's LD scores */
#define GAUSS_LDS_CHUNK 64              /* rows of a chunk of the LD scores' summation order */
#define GAUSS_SUSIE_MAX_L 32
#define GAUSS_XS_MAX 4
#define GAUSS_SUSIE_MAX_SWEEPS 1000
#define GAUSS_SUSIE_TRAITS_MORE_MAX 7   /* further traits in one fit: eight traits, 28 pairs at the most */
#define GAUSS_TRAITS_MORE_MAX 63
#define GAUSS_TRAITS_MISS_MAX 32        /* missing SNPs per further trait and window */
#define GAUSS_TRAITS_MISS_UNION_MAX 128 /* distinct missing SNPs per window          */

#define GAUSS_GENO_U8   0
#define GAUSS_GENO_2BIT 1

#define GAUSS_WIN_IMPUTE 0
#define GAUSS_WIN_QCAT   1
#define GAUSS_WIN_LD     2

#define GAUSS_CODE_ADDITIVE  1
#define GAUSS_CODE_DOMINANT  2
#define GAUSS_CODE_RECESSIVE 4

/* ---- pinned host buffers ---------------------------------------------------------------------
 * Page-locked host memory for the genotype matrices a driver marshals (pack_genotypes): the
 * upload of a window is then one DMA at PCIe speed instead of a staged copy of pageable memory (a full-size
 * window is 101 MB of genotype bytes).  Plain pointers; any host pointer remains valid input. */
int gauss_pinned_alloc(gauss_ctx* ctx, int64_t bytes, void** out_host_ptr);
int gauss_pinned_free(gauss_ctx* ctx, void* host_ptr);

/* ---- resident row store ---------------------------------------------------------------------
 * Copies `bytes` of genotype rows to the context's GPU and returns the device pointer to use as
 * geno_m / geno_u (with gauss_job_create's on_device = 1 and rows_m / rows_u).  288 GB of HBM hold a
 * whole 2-bit panel (33 k samples x 10 M SNPs = 82 GB), so a panel is uploaded once, not per window. */
int gauss_store_upload(gauss_ctx* ctx, const void* host_rows, int64_t bytes, void** out_device_ptr);
/* The rows are `bytes` bytes of an open file from file_offset on (a packed panel's genotype section): read with pread
 * straight into the pinned staging buffers -- no page of a mapping of the file is touched (a memcpy out of a fresh mapping
 * costs a page fault per 4 KB).  Blocking, like gauss_store_upload. */
int gauss_store_upload_fd(gauss_ctx* ctx, int fd, int64_t file_offset, int64_t bytes, void** out_device_ptr);
int gauss_store_free(gauss_ctx* ctx, void* device_ptr);
/* The same store filled piece by piece: gauss_store_alloc reserves `bytes` on the GPU (contents undefined until filled) and
 * gauss_store_fill copies host_rows[offset .. offset + len) to the same offsets of the store, returning when they have landed.
 * The copy travels through the pinned double buffers on a queue of its own, so whatever the context's other queues are
 * computing keeps running: a driver that walks a chromosome fills the rows of batch k + 1 while batch k computes
 * (gauss_host_impute_chromosome on a panel that is not resident yet).  A job may only name rows that have been filled. */
int gauss_store_alloc(gauss_ctx* ctx, int64_t bytes, void** out_device_ptr);
int gauss_store_fill(gauss_ctx* ctx, void* device_ptr, const void* host_rows, int64_t offset, int64_t len);
/* gauss_store_fill from a file: store bytes [offset, offset + len) come from file bytes [file_offset + offset, ...). */
int gauss_store_fill_fd(gauss_ctx* ctx, void* device_ptr, int fd, int64_t file_offset, int64_t offset, int64_t len);
/* The same upload without waiting for it: returns at once with the device pointer; a library thread streams the rows
 * IN ORDER (pinned double buffers, a stream of its own).  host_rows must stay valid until the upload is complete.
 * gauss_store_wait(ctx, ptr, n) makes the context's main stream wait until the first n bytes have landed -- a job queued
 * afterwards that reads rows below that mark starts while the rest of the panel is still crossing PCIe -- and blocks the
 * host only until those bytes have been queued; n <= 0: the whole store, and the host waits for completion.  Stores
 * made by gauss_store_upload need no wait (it is a no-op on them); a pointer that is not (or no longer) a row store of this
 * context is an error (a store freed by another call is not waited for, nor read). */
int gauss_store_upload_async(gauss_ctx* ctx, const void* host_rows, int64_t bytes, void** out_device_ptr);
/* The rows are `bytes` bytes of an open file starting at file_offset (a packed panel's genotype section): read with
 * pread straight into the pinned staging buffers -- no page of the caller's address space is touched, so the upload
 * does not contend with the threads that parse the study beside it.  fd must stay open until the upload is complete. */
int gauss_store_upload_fd_async(gauss_ctx* ctx, int fd, int64_t file_offset, int64_t bytes, void** out_device_ptr);
int gauss_store_wait(gauss_ctx* ctx, const void* device_ptr, int64_t bytes_needed);

/* ---- context ------------------------------------------------------------------------------- */
int gauss_hip_init(int device, gauss_ctx** out_ctx);
/* Number of HIP devices visible to the process (no context is created; a farm rank picks
 * LOCAL_RANK modulo this), and the device index a context was created on. */
int gauss_hip_device_count(int* out_n);
int gauss_hip_device_of(const gauss_ctx* ctx);
/* Lifetime rule.  A context may be destroyed while jobs (gauss_job_create) and row stores (gauss_store_upload) made on
 * it are still alive: gauss_hip_destroy waits for their queued work, frees every device / pinned block they hold and
 * leaves the job handles behind as empty shells.  After that
 *   - gauss_job_destroy(job) is still required (it frees the shell) and is safe in any order with the context;
 *   - every other call on such a job returns GAUSS_E_INVALID ("the job's context has been destroyed");
 *   - device pointers returned by gauss_store_upload are dead; gauss_store_free on them must not be called.
 * So the destructors of an Rcpp driver's RAII wrappers may run in whatever order an Rcpp::stop unwinds them
 * (RcppExports.cpp:66,81: exceptions leave the driver through the generated try / catch).  Destroying a context
 * must not race with calls that use it from other threads.  (Round 2 had no such rule: a job destroyed after its
 * context wrote into the freed context -- the heap corruption behind the one process abort of that round.) */
void gauss_hip_destroy(gauss_ctx* ctx);
/* A number that identifies the context for the life of the process and is never reused (a pointer may be: a new
 * context can land at a freed context's address).  Caches keyed per context key on this. */
uint64_t gauss_hip_context_id(const gauss_ctx* ctx);
/* fn(ctx, id, user) is called at the start of every gauss_hip_destroy, while the context is still whole: whoever
 * caches device memory per context (libgauss_host's resident panels) releases it there.  Process-wide, idempotent. */
int gauss_hip_add_destroy_hook(void (*fn)(gauss_ctx* ctx, uint64_t id, void* user), void* user);
/* Freed job workspaces are kept per context for reuse (hipFree would stall a pipeline that retires job k while job
 * k + 1 runs), up to a third of the device's memory.  Every allocation of the library flushes this cache and retries
 * before it reports GAUSS_E_NOMEM; gauss_hip_trim_cache gives the memory back at once (it waits for the context's
 * streams first), e.g. before another context or another library needs the device. */
int gauss_hip_trim_cache(gauss_ctx* ctx, int64_t* out_bytes_freed);
/* How the runs of this context's jobs were queued, since the context was made:
 *   out4[0] runs queued in the merged form (ONE Gram launch whose B11 items count themselves off for a waiting kernel at the
 *           head of the chain queue);
 *   out4[1] runs of jobs built for that form that were queued as two launches joined by an event instead, because the
 *           context could not be sure of a hardware queue per stream (the runtime shares queues once a priority class holds
 *           more streams than GPU_MAX_HW_QUEUES -- a second context on the device is enough);
 *   out4[2] merged runs whose waiting kernel gave up at its bound; gauss_job_fetch ran each of them again in the
 *           two-launch form inside the same call;
 *   out4[3] of those, the ones whose second form failed too (gauss_job_fetch returned GAUSS_E_DEVICE).
 * One call of the reference is one window or an error (dist.cpp:30-126): a give-up is never handed to the caller as results. */
int gauss_hip_counters(gauss_ctx* ctx, int64_t* out4);
/* The same four counts for ONE job (its own runs only): what a caller with several jobs -- or several calls -- in flight on a
 * context sums over ITS jobs (the context's counters are shared by everything that runs on it). */
int gauss_job_counters(gauss_job* job, int64_t* out4);
/* What the merged form's condition rests on, for diagnostics: out4[0] / out4[1] the library's live high- / low-priority streams on
 * the context's device (all contexts of the process), out4[2] the hardware queues the runtime makes per priority class
 * (GPU_MAX_HW_QUEUES, default 4; 0: unknown), out4[3] = 1 if gauss_hip_init SAW the context's chain and low-priority queues run a
 * kernel beside a later kernel of its main queue (a probe of a few microseconds: three different hardware queues), else 0.  A run
 * is queued merged only while out4[3] = 1 and both stream counts are within out4[2]. */
int gauss_hip_queues(gauss_ctx* ctx, int32_t* out4);
const char* gauss_last_error(void);
const char* gauss_hip_version(void);
/* Hash of the sources this library was built from (gauss_amd/build.py:source_hash): profiles/<tag>_provenance.json record it,
 * and bench.py only quotes a profile-derived figure (roofline.traffic) when it matches. */
const char* gauss_hip_source_hash(void);

/* Arithmetic of the LD Gram kernel for jobs created afterwards on this context.
 *   GAUSS_GRAM_F32 (default): v_mfma_f32_32x32x2_f32 on e4m3-coded operands, exact f32 integer sums.
 *   GAUSS_GRAM_I8           : v_mfma_i32_32x32x32_i8 on the raw codes, exact int32 sums.
 * Both produce bit-identical LD, z and info (the partial sums are the same integers). */
#define GAUSS_GRAM_F32 0
#define GAUSS_GRAM_I8  1
int gauss_hip_set_gram_dtype(gauss_ctx* ctx, int dtype);

/* ---- blocking host-pointer calls (what the Rcpp drivers bind) ------------------------------ */

/* LD matrix among S SNPs.  mode WEIGHTED + diag 1.0 = computeLD.cpp:95-116;
 * mode POOLED + diag 1+lambda = CorG of gene.cpp:305-315.  out_cor: S x S doubles (symmetric,
 * so column-major == row-major; fits an Rcpp::NumericMatrix directly). */
int gauss_ld(gauss_ctx* ctx, int mode, const uint8_t* geno, int n_snp, int64_t ld,
             const int32_t* pop_off, const double* pop_wgt, int n_pop, double diag,
             double* out_cor);

/* One window: run_dist (POOLED) / run_distmix (WEIGHTED).  Blocking. */
int gauss_impute_window(gauss_ctx* ctx, const gauss_window_desc* win);

/* LD blocks of many genes in one launch: gene g owns SNP rows [gene_off[g], gene_off[g+1]).
 * out_blocks receives the n_g x n_g blocks back to back (block g at sum_{h<g} n_h^2), each
 * with `diag` on its diagonal. */
int gauss_gene_ld_batch(gauss_ctx* ctx, int mode, const uint8_t* geno, int n_snp, int64_t ld,
                        const int32_t* pop_off, const double* pop_wgt, int n_pop,
                        const int32_t* gene_off, int n_gene, double diag, double* out_blocks);

/* gauss_ld / gauss_gene_ld_batch over rows of a row store instead of a contiguous byte matrix: `store` holds rows of
 * `ld` bytes in geno_format (GAUSS_GENO_U8 or GAUSS_GENO_2BIT, with pop_src_off as in gauss_window_desc), SNP s is store
 * row rows[s] (rows NULL: row s).  on_device != 0: `store` is a device pointer, e.g. a packed panel made resident
 * with gauss_store_upload -- nothing but the row indices travels to the GPU and only the LD blocks come back. */
int gauss_ld_rows(gauss_ctx* ctx, int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows, int n_snp,
                  const int32_t* pop_off, const int32_t* pop_src_off, const double* pop_wgt, int n_pop, double diag,
                  int on_device, double* out_cor);
int gauss_gene_ld_batch_rows(gauss_ctx* ctx, int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows,
                             int n_snp, const int32_t* pop_off, const int32_t* pop_src_off, const double* pop_wgt, int n_pop,
                             const int32_t* gene_off, int n_gene, double diag, int on_device, double* out_blocks);

/* Resampled pooled LD (simulateLD(), simulateLD.cpp:134-199): the correlation matrix of n_snp rows over n_cols samples, of
 * which sample k < n_drawn is sample draw_sample[k] of selected population draw_pop[k] (0 <= draw_pop[k] < n_pop, 0 <=
 * draw_sample[k] < pop_off[q + 1] - pop_off[q]; repeats allowed) and the other n_cols - n_drawn are zeros -- CalCor with
 * n = n_cols (util.cpp:49-70 operation order), `diag` on the diagonal, 0/0 = NaN where a row is constant.  Rows as in
 * gauss_ld_rows (U8 or 2-bit with pop_src_off, host or resident store).  Only the drawn columns are packed and multiplied; the
 * order of the draws changes no bit.  n_drawn = 0: NaN off the diagonal, no GPU work.  Sample counts whose exact integer sums
 * would leave int range (n_drawn >= 9.5 M, n_cols > INT32_MAX) are GAUSS_E_RANGE.  Blocking. */
int gauss_ld_resampled_rows(gauss_ctx* ctx, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows, int n_snp,
                            const int32_t* pop_off, const int32_t* pop_src_off, int n_pop,
                            const int32_t* draw_pop, const int32_t* draw_sample, int64_t n_drawn, int64_t n_cols,
                            double diag, int on_device, double* out_cor);

/* LD clumping (PLINK's --clump rule) of the n_snp rows of a region on their LD, which is formed as gauss_ld_rows forms it (same rows,
 * same bits) and never leaves the device: only owner, rank, r2 and n_clumps come back.  Rows as in gauss_ld_rows (U8 or 2-bit with
 * pop_src_off, host or resident store, rows NULL: row s).  bp [n_snp]: positions, never decreasing.  key [n_key][n_snp]: one row per
 * trait, the traits share the LD; a larger key is more significant; a row whose key is NaN is neither an index nor a member.
 * For each trait t on its own, with R the LD matrix:
 *     owner[i] = -1, rank[i] = 0, r2[i] = NaN for every i;  n = 0
 *     order = rows with key_i >= key_index, by (key descending, row ascending)
 *     for i in order:
 *         if owner[i] != -1: continue                        (a SNP already clumped never leads)
 *         n += 1;  owner[i] = i;  rank[i] = n;  r2[i] = 1.0
 *         for j != i with |bp_j - bp_i| <= radius, owner[j] == -1, key_j >= key_member:
 *             t2 = R_ij * R_ij                               (one rounded fp64 product of the LD entry as the LD step left it)
 *             if t2 >= r2_min: owner[j] = i;  r2[j] = t2     (a NaN compares false)
 *     n_clumps = n
 * A SNP goes to the FIRST (most significant) index that claims it, not to the one it correlates with most: PLINK's rule.  The key is
 * the caller's: with key = z^2 this is clumping; with key = minor-allele frequency, key_index = key_member = 0 it is LD pruning
 * (the commoner SNP of a correlated pair stays).  No floating-point sum is formed anywhere: the outputs do not depend on the thread
 * mapping, on the source format of the rows or on the run.  A monomorphic row (NaN LD) is never a member; where it leads, it leads
 * alone.  out_owner, out_rank [n_key][n_snp] int32, out_r2 [n_key][n_snp], out_n_clumps [n_key]; all but out_owner may be NULL.
 * Refused (GAUSS_E_INVALID, before anything is allocated): NULL bp / key / out_owner; n_key outside 1 .. GAUSS_CLUMP_MAX_KEYS; n_snp
 * outside 1 .. GAUSS_CLUMP_MAX_M; a bp that decreases; radius < 0; r2_min outside [0, 1] or NaN; a threshold that is not finite;
 * key_member > key_index; and whatever gauss_ld_rows refuses.  One region per call; clumps are cut at the region's edges (ask for
 * `radius` more on each side); a radius above 2^32 is taken as 2^32 (positions are 32-bit: every band is the whole region already,
 * so INT64_MAX may stand for "no limit"); the LD matrix takes 8 n_snp^2 bytes of device memory (0.5 GiB at the limit).  Blocking. */
#define GAUSS_CLUMP_MAX_M    8192
#define GAUSS_CLUMP_MAX_KEYS 64
int gauss_ld_clump_rows(gauss_ctx* ctx, int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows,
                        int n_snp, const int32_t* pop_off, const int32_t* pop_src_off, const double* pop_wgt, int n_pop,
                        int on_device, const int32_t* bp, const double* key, int n_key, int64_t radius, double r2_min,
                        double key_index, double key_member,
                        int32_t* out_owner, int32_t* out_rank, double* out_r2, int32_t* out_n_clumps);

/* Optimal LD-block boundaries of the n_snp rows of a region on their LD, which is formed as gauss_ld_rows forms it (same rows, same
 * bits, diag 1) and never leaves the device: the split of rows 0 .. M - 1 (M = n_snp, in position order) into K contiguous blocks of
 * min_size .. max_size rows that minimises the sum of r^2 over the pairs that land in different blocks, for every K = 1 .. max_K at
 * once.  Rows as in gauss_ld_rows.  bp [n_snp]: positions, never decreasing.  With R the LD matrix and W = max_size:
 *     pair value, i < j:  the pair is in the band iff j - i < W and bp_j - bp_i <= radius; a pair outside the band is never read
 *                         (further apart than max_size it is cut by every split: a constant).  e_ij = R_ij * R_ij, one rounded fp64
 *                         product; where R_ij is not finite the pair counts 0 everywhere and 1 in n_nonfinite
 *     row suffix sums:    hi_i = one past row i's last band column;  S[i][hi_i] = 0;  S[i][b] = S[i][b + 1] + (e_ib < thr_r2 ? 0 : e_ib)
 *                         for b = hi_i - 1 down to i + 1, in that order;  SM[i][b] = max(SM[i][b + 1], e_ib) likewise (no threshold)
 *     block cost:         T[b][0] = 0;  T[b][k] = T[b][k - 1] + S[b - k][b], k = 1 .. min(W, b), in that order: the pairs between
 *                         block [b - k, b) and everything to its right
 *     boundaries:         Mx[b] = max over k of SM[b - k][b];  0 < b < M is admissible iff Mx[b] <= max_r2 (max_r2 = 1: all are)
 *     the programme:      C[0][0] = 0, C[0][b] = +inf;  C[k][b] = min over a in [b - max_size, b - min_size], a >= 0, of
 *                         C[k - 1][a] + T[b][b - a], ties to the smaller a, the minimiser in P[k][b];  C[k][b] = +inf, P[k][b] = -1
 *                         where no candidate is finite or b < M is not admissible
 * Every step is in a fixed order or does not depend on one: the outputs do not depend on the thread mapping, on the source format of
 * the rows or on the run.  out_cost [max_K]: C[K][M], +inf where no split into K blocks exists (K min_size > M, K max_size < M, or
 * max_r2 closes too many boundaries).  out_prev [max_K][n_snp + 1] int32: P[K][b]; the best K-block split is read backwards from
 * b = M: b <- P[k][b] for k = K .. 1.  out_max_r2 [n_snp + 1]: Mx (0 at b = 0 and b = M).  out_n_nonfinite [1]: non-finite band
 * entries.  All but out_cost may be NULL.
 * Refused (GAUSS_E_INVALID, before anything is allocated or launched): NULL bp / out_cost; n_snp outside 1 .. GAUSS_LDSPLIT_MAX_M;
 * max_size outside 1 .. GAUSS_LDSPLIT_MAX_SIZE; min_size < 1 or > max_size; max_K outside 1 .. GAUSS_LDSPLIT_MAX_K; a bp that
 * decreases; radius < 0; thr_r2 or max_r2 outside [0, 1] or NaN; and whatever gauss_ld_rows refuses.  One region per call; a radius
 * above 2^32 is taken as 2^32; beside the matrix (8 n_snp^2 bytes) the call takes 24 min(max_size, n_snp) n_snp bytes of device
 * memory (0.8 GiB at the limits).  Blocking. */
#define GAUSS_LDSPLIT_MAX_M    8192
#define GAUSS_LDSPLIT_MAX_SIZE 4096
#define GAUSS_LDSPLIT_MAX_K    128
int gauss_ld_split_rows(gauss_ctx* ctx, int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows,
                        int n_snp, const int32_t* pop_off, const int32_t* pop_src_off, const double* pop_wgt, int n_pop,
                        int on_device, const int32_t* bp, int64_t radius, double thr_r2, int min_size, int max_size, int max_K,
                        double max_r2, double* out_cost, int32_t* out_prev, double* out_max_r2, int64_t* out_n_nonfinite);

/* Local heritability and genetic covariance of an LD block (the statistic of HESS, rho-HESS and LAVA): every eigenvalue of the
 * block's LD and the traits' projections on its leading eigenvectors.  The LD matrix R (M = n_snp) is formed as gauss_ld_rows forms
 * it (same rows, same bits, diag 1) and never leaves the device.  Rows as in gauss_ld_rows.  z [n_trait][n_snp]: one row per trait.
 *     repair:      a SNP whose every off-diagonal entry of R is NaN (M > 1) is monomorphic: its row, its column AND its diagonal
 *                  are set to 0 and its z is ignored (taken as 0).  Any other non-finite entry counts as 0 and, once per pair
 *                  i <= j, in n_nonfinite.  A non-finite z value is taken as 0 for that trait.  R' is the repaired matrix.
 *     eigenpairs:  R' = sum_i lam_i v_i v_i^T by block one-sided Jacobi (k_hess.hip), at most 30 sweeps; a sweep that rotates nothing
 *                  ends the solve.  A column of R' V whose norm is at or below M 2^-52 (the largest eigenvalue is at most M) is
 *                  numerically null and is not rotated: in a rank-deficient block (more SNPs than samples) the eigenvalues of the
 *                  null space come back within M 2^-52 of 0, with orthonormal vectors.
 *                  out_lam [n_snp]: all M eigenvalues, descending; a tie goes to the smaller column of the solver.
 *     n_pos:       the number of i with lam_i > eig_min * lam_0 and lam_i > 0 (a prefix of the sorted order); 0 <= eig_min < 1.
 *     projections: out_proj [n_trait][k_max]: proj[t][i] = (v_i^T z_t) / sqrt(lam_i) for i < min(k_max, n_pos), NaN beyond.  The
 *                  sign of v_i is arbitrary; every quantity built from proj downstream (H_t(k) = sum_{i<k} proj[t][i]^2, C_ab(k) =
 *                  sum_{i<k} proj[a][i] proj[b][i]) is a product of two projections on the same i and so does not depend on it.
 *                  A trait's projections depend on its own z only.
 * out_n_pos, out_sweeps (the last, rotation-free sweep counts), out_n_nonfinite, out_status [1] each: status = 0, or
 * GAUSS_ST_HESS_NOCONV (30 sweeps ran and the last still rotated: the values are those of the last sweep), GAUSS_ST_NONFINITE
 * (n_nonfinite > 0, or an eigenvalue is not finite: then n_pos = 0).  out_vectors [n_snp][n_snp] (row i = v_i) and out_order
 * [n_snp] (the solver's column of lam_i) are for the tests.  Every output but out_lam and out_proj may be NULL.
 * No floating-point atomics and every sum in a fixed order: the outputs do not depend on the source format of the rows, on a host
 * or device store, on the launch form of the LD build or on the run.
 * Refused (GAUSS_E_INVALID, before anything is allocated or launched): NULL z / out_lam / out_proj; n_snp outside 1 ..
 * GAUSS_HESS_MAX_M; n_trait outside 1 .. GAUSS_HESS_MAX_TRAITS; k_max outside 1 .. GAUSS_HESS_MAX_K; eig_min outside [0, 1) or NaN;
 * and whatever gauss_ld_rows refuses.  One block per call; beside the matrix (8 n_snp^2 bytes) the call takes 16 n_snp^2 bytes of
 * device memory for G = R' V and V, n_snp rounded up to 64: 24 n_snp^2 in all, 0.4 GB at the limit.  Blocking. */
#define GAUSS_HESS_MAX_M      4096
#define GAUSS_HESS_MAX_TRAITS 64
#define GAUSS_HESS_MAX_K      1024
int gauss_ld_hess_rows(gauss_ctx* ctx, int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows,
                       int n_snp, const int32_t* pop_off, const int32_t* pop_src_off, const double* pop_wgt, int n_pop,
                       int on_device, const double* z, int n_trait, int k_max, double eig_min, double* out_lam, double* out_proj,
                       int32_t* out_n_pos, int32_t* out_sweeps, int64_t* out_n_nonfinite, int32_t* out_status,
                       double* out_vectors, int32_t* out_order);

/* Gene-based sum-of-chi2 test (the statistic of fastBAT, VEGAS and MAGMA's SNP-wise mean model) of n_gene genes on their LD
 * blocks, which are formed as gauss_gene_ld_batch[_rows] forms them with diag = 1 (same rows, same bits) and never leave the
 * device.  Gene g owns rows [gene_off[g], gene_off[g+1]), n of them, with block R.  z [n_trait][n_snp]: one row per trait, the
 * traits share the LD, the pruning and the eigenvalues.  Per gene:
 *     nanrow[i] = n > 1 and R_ij is NaN for every j != i        (a monomorphic SNP; in a gene of one SNP the row is kept)
 *     for i = 0 .. n-1 in row order (never by z: pruning by significance would bias the test):
 *         nanrow[i] or dropped[i]: continue
 *         i is kept;  every j > i with R_ij * R_ij > prune_r2 is dropped    (one rounded fp64 product, strict; a NaN compares false)
 *     k = kept rows;  out_kept[row] = 1 for a kept row, else 0;  out_n_kept[g] = k
 *     lambda = eigenvalues of R[kept][kept], descending: out_lam[g][0 .. k), NaN beyond k
 *     per trait t:  out_q[t][g] = sum of z_ti^2 over the kept rows, added in ascending row order (a NaN z of a kept row makes that
 *                   trait's Q NaN);  out_top[t][g] = the row, counted inside the gene, with the largest z^2 among ALL n rows whose z is
 *                   finite, kept or not (ties: the smaller row; none: -1)
 * prune_r2 = 1 prunes nothing (r^2 > 1 never holds); fastBAT's default is 0.9.  Under the null Q ~ sum lambda_i chi2_1:
 * gauss_host_sumchi2_pval (include/gauss_host.h) turns lambda and Q into a p-value.  The eigenvalues come from a cyclic two-sided
 * Jacobi solve in LDS (k_sumchi2.hip states the rotation order, the skip rule |a_pq| <= 4 * 2^-52 ||A||_F and the summation order of
 * the norm): every sum has a fixed order, so the outputs do not depend on the source format of the rows, on the other genes of the
 * call or on the run.  The weighted LD estimator is not exactly positive semidefinite: a lambda may be slightly negative.
 * out_status[g]: 0, or GAUSS_ST_SUMCHI2_EMPTY (k = 0: an empty gene, or every row NaN; Q = 0), GAUSS_ST_SUMCHI2_TOOLARGE (k >
 * GAUSS_SUMCHI2_MAX_KEPT: every lambda NaN, out_n_kept = k, Q and top still written), GAUSS_ST_NOCONV (30 sweeps without
 * convergence: every lambda NaN).  out_sweeps[g]: Jacobi sweeps made, the last, rotation-free one included (0 where nothing was
 * solved).  out_kept [n_snp] int32, out_n_kept [n_gene], out_lam [n_gene][GAUSS_SUMCHI2_MAX_KEPT], out_q [n_trait][n_gene] are
 * required; out_top [n_trait][n_gene], out_status [n_gene], out_sweeps [n_gene] may be NULL.
 * Refused (GAUSS_E_INVALID, before anything is allocated): a NULL required pointer; n_trait outside 1 .. GAUSS_SUMCHI2_MAX_TRAITS;
 * prune_r2 outside (0, 1] or NaN; a gene of more than GAUSS_SUMCHI2_MAX_N SNPs; and whatever gauss_gene_ld_batch[_rows] refuses.
 * A row outside every gene gets out_kept 0.  Blocking. */
#define GAUSS_SUMCHI2_MAX_N      1024   /* SNPs of one gene before pruning */
#define GAUSS_SUMCHI2_MAX_KEPT    128
#define GAUSS_SUMCHI2_MAX_TRAITS   64
int gauss_gene_sumchi2(gauss_ctx* ctx, int mode, const uint8_t* geno, int n_snp, int64_t ld,
                       const int32_t* pop_off, const double* pop_wgt, int n_pop,
                       const int32_t* gene_off, int n_gene, const double* z, int n_trait, double prune_r2,
                       int32_t* out_kept, int32_t* out_n_kept, double* out_lam, double* out_q,
                       int32_t* out_top, int32_t* out_status, int32_t* out_sweeps);
/* ... over rows of a row store: store / ld / geno_format / rows / pop_src_off / on_device as gauss_gene_ld_batch_rows */
int gauss_gene_sumchi2_rows(gauss_ctx* ctx, int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows,
                            int n_snp, const int32_t* pop_off, const int32_t* pop_src_off, const double* pop_wgt, int n_pop,
                            const int32_t* gene_off, int n_gene, int on_device, const double* z, int n_trait, double prune_r2,
                            int32_t* out_kept, int32_t* out_n_kept, double* out_lam, double* out_q,
                            int32_t* out_top, int32_t* out_status, int32_t* out_sweeps);

/* Per-population Pearson correlations of every SNP pair (prep_zmix5, zmix.cpp:158-176: CalCor on each
 * population's genotype strings, util.cpp:153-169).  out is [n_pop][n_snp*(n_snp-1)/2], population-major,
 * pairs in the reference's row order (i ascending, then j > i): column k+1 of the reference's column-major
 * NumericMatrix data_mat is out + k * npairs.  A population in which a SNP is monomorphic gives NaN there,
 * as in the reference. */
int gauss_ld_per_pop(gauss_ctx* ctx, const uint8_t* geno, int n_snp, int64_t ld,
                     const int32_t* pop_off, int n_pop, double* out);

/* The same correlations for LISTED pairs only, per population or per GROUP of populations pooled: what the other
 * prep_zmix selectors need (zmix.cpp:201-1076 -- prep_zmix, prep_zmix2, prep_zmix3, prep_zmix4 list pairs by interval /
 * offset / steps; prep_zmix5_sup pools the populations of a super-population, CalCorSup zmix.cpp:1221-1246).  pair k is
 * (pair_i[k], pair_j[k]) with 0 <= i < j < n_snp; pop_group[p] in 0..n_group-1 names the group of population p (NULL:
 * every population its own group, n_group ignored).  Only the tile pairs the listed pairs touch are multiplied.
 * out is [n_group][n_pairs]. */
int gauss_ld_per_pop_pairs(gauss_ctx* ctx, const uint8_t* geno, int n_snp, int64_t ld, const int32_t* pop_off, int n_pop,
                           const int32_t* pop_group, int n_group, const int32_t* pair_i, const int32_t* pair_j, int64_t n_pairs,
                           double* out);

/* Population weights from allele frequencies: the numeric core of afmix() / cpw2() (afmix.cpp:114-215, cpw2.cpp:110-211).
 * x is an interval-major matrix of n_pop + 1 columns, row-major: rows [interval_off[i], interval_off[i+1]) belong to interval i
 * and hold [af1study, AF_pop0 .. AF_pop(n_pop-1)] (cpw2: already asin(sqrt(.))-transformed by the caller).  For every interval:
 * the two-pass sample covariance C of the columns (CalCovMat, util.cpp:205-213, 243-253), Cxy = C[1:, 0], Cxx = C[1:, 1:];
 * MakePosDef(Cxx, min_abs_eig) (util.cpp:302-318: rebuilt as V max(Lambda, min_abs_eig) V^T only if an eigenvalue is below
 * min_abs_eig); W_i = Cxx^-1 Cxy.  out_w_interval is [n_interval x n_pop] row-major; out_status (may be NULL) gets per interval
 * GAUSS_ST_CLAMPED when Cxx was rebuilt, GAUSS_ST_NONFINITE when W_i is NaN (non-finite input, an interval of fewer than two
 * rows), GAUSS_ST_NOCONV with it if the eigen-solve did not converge.  1 <= n_pop <= 64.  Blocking; the bits do not depend on
 * the run.  The caller accumulates W = sum_i W_i / n_interval in interval order (afmix.cpp:192-195). */
int gauss_pop_weights(gauss_ctx* ctx, const double* x, const int64_t* interval_off, int n_interval, int n_pop,
                      double min_abs_eig, double* out_w_interval, int32_t* out_status);

/* Normal equations of the zmix regression (zmix(), zmix.R): over every pair i < j of the n_snp genotype rows, the row
 * [y, x_1 .. x_G] = [z[i] * z[j], r_1(i, j) .. r_G(i, j)], r_g the Pearson correlation of the pair inside group g.  pop_group NULL:
 * one group per population (G = n_pop, the columns of prep_zmix5 and the bits of gauss_ld_per_pop); else population p belongs to
 * group pop_group[p] in 0 .. n_group - 1 and a group's populations are pooled (G = n_group, prep_zmix5_sup's columns, CalCorSup
 * zmix.cpp:1221-1246, the bits of gauss_ld_per_pop_pairs).  A row is kept iff all its 1 + G entries are finite
 * (is.finite(rowSums(mat))).  Out: X^T X [G x G] row-major, X^T y [G], y^T y and the number of kept rows, over the kept rows.
 * The per-pair rows are never stored: only pack + Gram run, then a fixed-order reduction (no atomics: the bits do not depend on
 * the run).  1 <= G <= 64; n_snp >= 2.  Blocking. */
int gauss_zmix_normal_eq(gauss_ctx* ctx, const uint8_t* geno, int n_snp, int64_t ld, const int32_t* pop_off, int n_pop,
                         const int32_t* pop_group, int n_group, const double* z, double* out_xtx, double* out_xty, double* out_yty,
                         int64_t* out_n_rows);

/* Exact co-occurrence counts sum_n x_i[n] x_j[n] over all columns -- the integer the reference
 * accumulates as `sumxy` (util.cpp:62,114).  out: S x S int64, row-major.  Integer parity hook. */
int gauss_gram_counts(gauss_ctx* ctx, const uint8_t* geno, int n_snp, int n_samples, int64_t ld,
                      int64_t* out_counts);

/* ---- asynchronous multi-window jobs (farm harness, bench) ----------------------------------- */

/* Build a job of n_win windows.  If on_device != 0, geno_m/geno_u are device pointers that stay
 * resident for the life of the job; otherwise they are host pointers and are uploaded once here.
 * All windows of a job run through the same batched launches. */
int gauss_job_create(gauss_ctx* ctx, const gauss_window_desc* wins, int n_win, int on_device,
                     gauss_job** out_job);
/* Enqueue one full pass (pack -> Gram -> LD epilogue -> factorisation + inverse factor -> closing product) on the
 * context's streams; returns at once.  Up to TWO runs of a job may be in flight: a second gauss_job_run before the first
 * has been fetched is allowed (the job keeps two result mirrors), a third is refused (GAUSS_E_INVALID). */
int gauss_job_run(gauss_job* job);
/* Wait for the OLDEST run that has not been fetched and copy its z / info / status (and optional b11/b21) to the host
 * pointers of each window descriptor.  run, fetch, run, fetch ... behaves as before; run, run, fetch, run, fetch ...
 * keeps the GPU busy while the host handles the previous run's results. */
int gauss_job_fetch(gauss_job* job);
void gauss_job_destroy(gauss_job* job);
/* Device time from the moment `first` started to run until `last` had delivered its results (HIP events on the
 * context's stream; both jobs must have run, on the same context).  With a pipeline of jobs this is the span the
 * GPU was busy with them, whatever the host did meanwhile. */
int gauss_job_span_ms(gauss_job* first, gauss_job* last, double* out_ms);

/* Profiling hooks for bench.py: HIP events are recorded around every launch of the Gram kernel
 * on the job's own stream while enabled. */
int gauss_job_profile(gauss_job* job, int enable);
/* kernel 0 = gram (LD GEMM), 1 = pack/stats, 2 = LD epilogue, 3 = factor, 4 = solve.
 * Returns accumulated milliseconds and launch count since profiling was enabled. */
int gauss_job_profile_get(gauss_job* job, int kernel, double* out_ms, int64_t* out_launches);
/* Algorithmic work of one run of the job (SURVEY.md section 8d definitions). */
int gauss_job_work(gauss_job* job, double* out_ld_flops, double* out_solve_flops,
                   double* out_bytes, int64_t* out_imputed_snps);

/* Launch geometry of the job: out[0] = Gram work items, out[1] = MFMA flops actually issued per run
 * (padding included, skipped padding halves excluded), out[2] = bytes of partial-Gram slabs,
 * out[3] = device workspace bytes.  Diagnostic only. */
int gauss_job_stats(gauss_job* job, double* out4);

/* Device-side conversion of one-byte genotype rows [n_snp x ld_in] into GAUSS_GENO_2BIT rows [n_snp x ld_out]
 * (population blocks consecutive, 16-byte aligned, zero padded to 64 samples; ld_out >= their total and a
 * multiple of 16).  Both pointers are device pointers.  Used to build a resident row store from rows that are
 * already in HBM (bench plumbing; a packed panel file is uploaded as it is).  The packer keeps the low two bits
 * of every byte, so the codes must be 0..3 or the ASCII digits '0'..'3'.  pop_off starts at 0 or above and never
 * decreases, and ld_in >= pop_off[n_pop]: anything else is GAUSS_E_INVALID, and d_out is left as it was. */
int gauss_pack2bit_device(gauss_ctx* ctx, const uint8_t* d_in, int64_t ld_in, uint8_t* d_out, int64_t ld_out,
                          int n_snp, const int32_t* pop_off, int n_pop);

/* Synthetic genotype generator on the device (bench plumbing; mirrors gauss_amd/synth.py's
 * model with a counter-based RNG).  Writes n_snp rows of n_samples bytes {0,1,2} at d_out with
 * row stride ld.  thr is a host array [n_snp x n_pop] of per-population latent thresholds,
 * rho a host array [n_snp] of AR(1) coefficients (rho[0] is not used).  n_samples = pop_off[n_pop];
 * pop_off starts at 0 or above and never decreases, and ld >= pop_off[n_pop]: anything else is
 * GAUSS_E_INVALID, and d_out is left as it was.  Bytes n_samples .. ld of a row are not written. */
int gauss_synth_device(gauss_ctx* ctx, uint8_t* d_out, int n_snp, int64_t ld,
                       const int32_t* pop_off, int n_pop, const float* thr, const float* rho,
                       uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* GAUSS_HIP_H */
