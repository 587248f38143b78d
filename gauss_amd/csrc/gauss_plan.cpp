// libgauss_hip.so -- the planner: one window -> Plan (segments, tile pairs, tables), a batch of windows -> a job.
//
// A job is a batch of independent windows that share every launch: one pack, one Gram, one
// epilogue, nblk factor steps and one solve launch serve all windows of the job, so the chip is
// filled by work items of many windows at once (the per-window matrices are too small to fill
// 256 CUs on their own) and the latency-bound factor steps are amortised over the batch.
#include "gauss_job.h"
#include "k_gram_common.h"

// K segment length: short segments give a single window enough work items to fill 256 CUs;
// a batch of windows has plenty of items already, and longer segments mean fewer partial slabs
// for the epilogue to read back.  Either way a partial sum stays an exact f32 integer
// (15 * 15 * 8192 < 2^24).
static int seg_max_for(const std::vector<WinSpec>& specs)
{
    // 4096 for batched jobs (8192 until the chain moved beside the Gram kernel: with B11's and B21's items in launches of their
    // own the shorter items balance each launch's last round better -- 5 / 9 / 18 / 36 windows: step 4.86 -> 4.75, 8.97 -> 8.93,
    // 19.47 -> 19.29, 41.00 -> 40.96 ms -- for 19 % more work items)
    if (specs.size() >= 4) return 4096;
    // One to three windows: a work item per (tile pair, segment), so the segment length decides how many workgroups the launch
    // has.  A window with few tile pairs -- computeLD()'s one 3 Mb window: 529 SNPs, 15 pairs -- left three quarters of the chip's
    // 1 024 workgroup slots empty at 2 048 samples a segment; segments are cut so that the job has ~1 300 items, down to 384 samples
    // (below that the epilogue's reads of the partial slabs cost what the Gram launch gains).  Measured on that window, Gram
    // launch / LD epilogue in us: 2048: 196 / 59 (46 TFLOP/s); 1024: 154 / 67; 768: 140 / 69; 512: 127 / 74; 384: 120 / 81
    // (75 TFLOP/s); 256: 116 / 92.  Any cut is exact (integer partial sums); listed-pair and gene jobs keep 2 048.
    // (tests/percor_ref.py restates this rule and plan_problem's cut -- 1 300, 384, 2 048, the chunk arithmetic -- to place its
    // population tables on the cuts: change them together, or its multi-segment cases quietly become single-segment ones.)
    double pairs = 0, kp = 0;
    for (const WinSpec& w : specs) {
        if (w.gene_off || w.pair_i || w.M < 1 || w.n_pop < 1 || w.n_pop > 64 || !w.pop_off) return SEG_MAX;      // (plan_problem reports what is wrong)
        int nc = 0;
        for (int c = 0; c < 3; c++) nc += (w.u_codings >> c) & 1;
        const double mt = (w.M + TILE - 1) / TILE, ut = ((double)w.U * std::max(nc, 1) + TILE - 1) / TILE;
        pairs += mt * (mt + 1) / 2 + ut * mt;
        kp = std::max(kp, w.draw_pop ? (double)w.n_drawn + 32.0 : (double)w.pop_off[w.n_pop] + 32.0 * w.n_pop);
    }
    const double want = pairs * kp / 1300.0;
    return (int)std::min<double>(SEG_MAX, std::max<double>(384.0, std::floor(want / KC) * KC));
}
// Consecutive segments are chained into one work item until the run reaches this many samples
// (a fresh item costs a pipeline fill: descriptor, first operand tiles, barrier).  0 = no chaining.
static int group_target_for(size_t n_windows)
{
    // 2048 rather than 4096: same kernel time on the bench workload, 13 % less fabric read traffic (the tiles
    // co-resident items share stay in the XCD's L2 more often; tools/group_pmc.sh)
    return n_windows >= 4 ? 2048 : 0;
}
int plan_problem(const WinSpec& w, Plan& pl, int seg_max, int group_target)
{
    if (w.mode != GAUSS_MODE_POOLED && w.mode != GAUSS_MODE_WEIGHTED) return fail(GAUSS_E_INVALID, "bad mode %d", w.mode);
    if (w.n_pop < 1 || w.n_pop > 64) return fail(GAUSS_E_INVALID, "n_pop must be in 1..64 (got %d)", w.n_pop);
    if (!w.pop_off) return fail(GAUSS_E_INVALID, "pop_off is NULL");
    if (w.M < 1) return fail(GAUSS_E_INVALID, "need at least one measured SNP row (got %d)", w.M);
    if (w.U < 0) return fail(GAUSS_E_INVALID, "negative n_unmeasured");
    if (w.mode == GAUSS_MODE_WEIGHTED && !w.pop_wgt) return fail(GAUSS_E_INVALID, "pop_wgt is NULL in weighted mode");
    if (!w.geno_m || (w.U > 0 && !w.geno_u)) return fail(GAUSS_E_INVALID, "genotype pointer is NULL");
    for (int p = 0; p < w.n_pop; p++)
        if (w.pop_off[p + 1] < w.pop_off[p]) return fail(GAUSS_E_INVALID, "pop_off must be non-decreasing");
    if (w.pop_off[0] != 0) return fail(GAUSS_E_INVALID, "pop_off[0] must be 0");
    const int N = w.pop_off[w.n_pop];
    if (N < 1) return fail(GAUSS_E_INVALID, "no samples");
    // sums of code products are kept as exact integers: 15 * 15 * n must stay below 2^31
    if ((long long)N * 225 >= (1LL << 31)) return fail(GAUSS_E_RANGE, "%d samples exceed the exact-integer range (9.5 M)", N);
    if (w.geno_fmt != GAUSS_GENO_U8 && w.geno_fmt != GAUSS_GENO_2BIT) return fail(GAUSS_E_INVALID, "bad geno_format %d", w.geno_fmt);
    if (w.geno_fmt == GAUSS_GENO_U8 && w.ld < N) return fail(GAUSS_E_INVALID, "ld (%lld) < n_samples (%d)", w.ld, N);
    if (w.geno_fmt == GAUSS_GENO_2BIT) {
        if (w.ld % 16) return fail(GAUSS_E_INVALID, "2-bit rows need a stride that is a multiple of 16 bytes (got %lld)", w.ld);
        long long end = 0;
        for (int q = 0; q < w.n_pop; q++) {
            const long long blk = (long long)rup((size_t)(w.pop_off[q + 1] - w.pop_off[q]), 64) / 4;
            const long long off = w.pop_src_off ? w.pop_src_off[q] : end;
            if (off < 0 || off % 16) return fail(GAUSS_E_INVALID, "pop_src_off[%d] = %lld is not a multiple of 16", q, off);
            if (off + blk > w.ld) return fail(GAUSS_E_INVALID, "population block %d ends past the row stride", q);
            if (!w.pop_src_off) end = off + blk;
        }
    }
    if (w.kind != GAUSS_WIN_IMPUTE && w.kind != GAUSS_WIN_QCAT && w.kind != GAUSS_WIN_LD)
        return fail(GAUSS_E_INVALID, "bad window kind %d", w.kind);
    if (!w.ld_only && w.kind != GAUSS_WIN_LD && (w.U > 0 || w.kind == GAUSS_WIN_QCAT) && !w.z1) return fail(GAUSS_E_INVALID, "z1 is NULL");
    if (w.u_codings & ~(GAUSS_CODE_ADDITIVE | GAUSS_CODE_DOMINANT | GAUSS_CODE_RECESSIVE))
        return fail(GAUSS_E_INVALID, "bad u_codings mask %d", w.u_codings);
    if (w.kind == GAUSS_WIN_QCAT && (w.n_head < 0 || w.n_predm < 0 || w.n_head + w.n_predm > w.M))
        return fail(GAUSS_E_INVALID, "QCAT: n_head_measured + n_pred_measured exceeds n_measured");
    // the riders work on B11, z1 and the rows of L^-1 that an imputation window's solve leaves behind: QCAT and LD windows are refused
    const bool imputes = !w.ld_only && w.kind == GAUSS_WIN_IMPUTE;
    const char* const not_imputing = w.kind == GAUSS_WIN_QCAT ? "QCAT" : "LD";
    // leave-one-out values (k_loo.hip)
    const bool loo = w.out.loo_z || w.out.loo_info || w.out.loo_t;
    if (loo && !imputes)
        return fail(GAUSS_E_INVALID, "leave-one-out values (out_loo_z / out_loo_info / out_loo_t) are for imputation windows only (%s window)", not_imputing);
    // signal selection (k_slct.hip)
    if (w.slct_max < 0 || w.slct_max > SLCT_K)
        return fail(GAUSS_E_INVALID, "slct_max = %d: signal selection takes 0 .. %d SNPs", w.slct_max, SLCT_K);
    if (w.slct_max > 0) {
        if (!imputes) return fail(GAUSS_E_INVALID, "signal selection (slct_max) is for imputation windows only (%s window)", not_imputing);
        if (w.M > SLCT_M_MAX)
            return fail(GAUSS_E_INVALID, "signal selection takes windows of at most %d measured SNPs (n_measured = %d)", SLCT_M_MAX, w.M);
        if (w.n_slct_forced < 0 || w.n_slct_forced > w.slct_max || (w.n_slct_forced > 0 && !w.slct_forced))
            return fail(GAUSS_E_INVALID, "n_slct_forced = %d: 0 .. slct_max (%d) forced SNPs, with their list", w.n_slct_forced, w.slct_max);
        for (int a = 0; a < w.n_slct_forced; a++) {
            if (w.slct_forced[a] < 0 || w.slct_forced[a] >= w.M)
                return fail(GAUSS_E_INVALID, "slct_forced[%d] = %d is not a measured SNP of the window (n_measured = %d)", a, (int)w.slct_forced[a], w.M);
            for (int b = 0; b < a; b++)
                if (w.slct_forced[b] == w.slct_forced[a])
                    return fail(GAUSS_E_INVALID, "slct_forced[%d] = slct_forced[%d] = %d: forced SNPs must be distinct", b, a, (int)w.slct_forced[a]);
        }
    }
    // the imputed SNPs conditioned on the selection (k_cond.hip)
    const bool cond = w.out.cond_z || w.out.cond_var;
    if (cond && !imputes)
        return fail(GAUSS_E_INVALID, "conditional statistics of the imputed SNPs (out_cond_z / out_cond_var) are for imputation windows only (%s window)", not_imputing);
    if (cond && w.slct_max <= 0)
        return fail(GAUSS_E_INVALID, "conditional statistics of the imputed SNPs (out_cond_z / out_cond_var) condition on the signal selection: they need slct_max > 0");
    // credible sets of the selected signals (k_cs.hip)
    const bool cs = w.out.cs_pip || w.out.cs_set || w.out.cs_set_pip || w.out.cs_size || w.out.cs_mass || w.out.cs_lse;
    if (cs && !imputes)
        return fail(GAUSS_E_INVALID, "credible sets (out_cs_*) are for imputation windows only (%s window)", not_imputing);
    if (cs && w.slct_max <= 0)
        return fail(GAUSS_E_INVALID, "credible sets (out_cs_*) are those of the selected signals: they need slct_max > 0");
    if (cs && !(w.cs_coverage > 0.0 && w.cs_coverage <= 1.0))
        return fail(GAUSS_E_INVALID, "cs_coverage = %g: the coverage of a credible set lies in (0, 1]", w.cs_coverage);
    if (cs && !(w.cs_prior_var > 0.0 && std::isfinite(w.cs_prior_var)))
        return fail(GAUSS_E_INVALID, "cs_prior_var = %g: the prior variance of the causal SNP's non-centrality is positive and finite", w.cs_prior_var);
    // polygenic score weights (k_prs.hip)
    const bool prs = w.prs_n_s != 0;
    if (prs && !imputes)
        return fail(GAUSS_E_INVALID, "polygenic score weights (prs_n_s) are for imputation windows only (%s window)", not_imputing);
    if (prs && (w.prs_n_s < 1 || w.prs_n_s > PRS_S || !w.prs_s))
        return fail(GAUSS_E_INVALID, "prs_n_s = %d: the score takes 1 .. %d shrinkage values, with their list (prs_s)", w.prs_n_s, PRS_S);
    if (prs && (w.prs_n_lam < 1 || w.prs_n_lam > PRS_LAM || !w.prs_lam))
        return fail(GAUSS_E_INVALID, "prs_n_lam = %d: the score takes 1 .. %d penalties, with their list (prs_lam)", w.prs_n_lam, PRS_LAM);
    for (int a = 0; prs && a < w.prs_n_s; a++)
        if (!(w.prs_s[a] > 0.0 && w.prs_s[a] <= 1.0))
            return fail(GAUSS_E_INVALID, "prs_s[%d] = %g: a shrinkage value lies in (0, 1]", a, w.prs_s[a]);
    for (int a = 0; prs && a < w.prs_n_lam; a++)
        if (!(w.prs_lam[a] >= 0.0 && std::isfinite(w.prs_lam[a])))
            return fail(GAUSS_E_INVALID, "prs_lam[%d] = %g: a penalty is finite and not negative", a, w.prs_lam[a]);
    if (prs && !(w.prs_n > 2.0 && std::isfinite(w.prs_n)))
        return fail(GAUSS_E_INVALID, "prs_n = %g: the study's sample size is finite and above 2", w.prs_n);
    if (prs && !(w.prs_tol >= 0.0 && std::isfinite(w.prs_tol)))
        return fail(GAUSS_E_INVALID, "prs_tol = %g: the stopping tolerance is finite and not negative", w.prs_tol);
    // (the cap bounds what one window can keep a workgroup busy for: n_lam x max_sweeps sweeps per chain at the most)
    if (prs && (w.prs_max_sweeps < 1 || w.prs_max_sweeps > PRS_MAX_SWEEPS))
        return fail(GAUSS_E_INVALID, "prs_max_sweeps = %d: a penalty takes 1 .. %d sweeps", w.prs_max_sweeps, PRS_MAX_SWEEPS);
    if (prs && w.M > PRS_M_MAX)
        return fail(GAUSS_E_INVALID, "n_measured = %d: the score (prs_n_s) takes windows of at most %d measured SNPs", w.M, PRS_M_MAX);
    // LD scores of the measured SNPs (k_ldscore.hip): the one rider of an LD window
    const bool lds = w.lds_on != 0;
    if (lds && (w.ld_only || w.kind != GAUSS_WIN_LD))
        return fail(GAUSS_E_INVALID, "LD scores (lds_on) are for LD windows only (%s window)", w.kind == GAUSS_WIN_QCAT ? "QCAT" : "imputation");
    if (lds && w.lambda != 0.0)
        return fail(GAUSS_E_INVALID, "lambda = %g: LD scores (lds_on) take correlations, a window with lambda = 0", w.lambda);
    if (lds && (w.u_codings & ~GAUSS_CODE_ADDITIVE))
        return fail(GAUSS_E_INVALID, "u_codings = %d: LD scores (lds_on) take the additive coding only", w.u_codings);
    if (lds && (!w.lds_bp_m || (w.U > 0 && !w.lds_bp_u)))
        return fail(GAUSS_E_INVALID, "LD scores (lds_on) need the positions of the window's rows: %s is NULL", !w.lds_bp_m ? "lds_bp_m" : "lds_bp_u");
    for (int a = 1; lds && a < w.M; a++)
        if (w.lds_bp_m[a] < w.lds_bp_m[a - 1])
            return fail(GAUSS_E_INVALID, "lds_bp_m[%d] = %d < lds_bp_m[%d] = %d: the positions do not decrease", a, (int)w.lds_bp_m[a], a - 1, (int)w.lds_bp_m[a - 1]);
    for (int a = 1; lds && a < w.U; a++)
        if (w.lds_bp_u[a] < w.lds_bp_u[a - 1])
            return fail(GAUSS_E_INVALID, "lds_bp_u[%d] = %d < lds_bp_u[%d] = %d: the positions do not decrease", a, (int)w.lds_bp_u[a], a - 1, (int)w.lds_bp_u[a - 1]);
    if (lds && !(w.lds_n > 2.0 && std::isfinite(w.lds_n)))
        return fail(GAUSS_E_INVALID, "lds_n = %g: the sample size of the bias adjustment is finite and above 2", w.lds_n);
    if (lds && w.lds_radius < 0)
        return fail(GAUSS_E_INVALID, "lds_radius = %lld: the radius of an LD score is not negative", w.lds_radius);
    if (lds && (w.lds_n_annot < 0 || w.lds_n_annot > LDS_C))
        return fail(GAUSS_E_INVALID, "lds_n_annot = %d: LD scores take 0 .. %d annotation categories", w.lds_n_annot, LDS_C);
    if (lds && lds_chunks(w.M, w.U) > LDS_MAX_CHUNKS)
        return fail(GAUSS_E_INVALID, "LD scores (lds_on): %d + %d rows make %d chunks of %d; a window takes at most %d (shorten it)", w.M, w.U,
                    lds_chunks(w.M, w.U), LDS_CHUNK, LDS_MAX_CHUNKS);
    if (lds && w.lds_n_annot > 0 && !w.lds_annot)
        return fail(GAUSS_E_INVALID, "lds_n_annot = %d: the categories' weights (lds_annot) are NULL", w.lds_n_annot);
    for (size_t a = 0; lds && a < (size_t)w.lds_n_annot * (size_t)(w.M + w.U); a++)
        if (!std::isfinite(w.lds_annot[a]))
            return fail(GAUSS_E_INVALID, "lds_annot[%d][%d] = %g: an annotation weight is finite", (int)(a / (size_t)(w.M + w.U)), (int)(a % (size_t)(w.M + w.U)), w.lds_annot[a]);
    // multi-causal fine-mapping (k_susie.hip)
    const bool susie = w.susie_L != 0;
    if (susie && !imputes)
        return fail(GAUSS_E_INVALID, "multi-causal fine-mapping (susie_L) is for imputation windows only (%s window)", not_imputing);
    if (susie && (w.susie_L < 1 || w.susie_L > SUSIE_L))
        return fail(GAUSS_E_INVALID, "susie_L = %d: multi-causal fine-mapping takes 1 .. %d effects", w.susie_L, SUSIE_L);
    if (susie && !(w.susie_coverage > 0.0 && w.susie_coverage <= 1.0))
        return fail(GAUSS_E_INVALID, "susie_coverage = %g: the coverage of a credible set lies in (0, 1]", w.susie_coverage);
    if (susie && !(w.susie_prior_var > 0.0 && std::isfinite(w.susie_prior_var)))
        return fail(GAUSS_E_INVALID, "susie_prior_var = %g: the prior variance of an effect is positive and finite", w.susie_prior_var);
    if (susie && !(w.susie_tol >= 0.0 && std::isfinite(w.susie_tol)))
        return fail(GAUSS_E_INVALID, "susie_tol = %g: the stopping tolerance is finite and not negative", w.susie_tol);
    // (every run queues max_sweeps x L x 2 launches up front: the cap bounds what one window can put on the queue)
    if (susie && (w.susie_max_sweeps < 1 || w.susie_max_sweeps > SUSIE_MAX_SWEEPS))
        return fail(GAUSS_E_INVALID, "susie_max_sweeps = %d: the fit takes 1 .. %d sweeps", w.susie_max_sweeps, SUSIE_MAX_SWEEPS);
    if (susie && !(w.susie_min_abs_corr >= 0.0 && w.susie_min_abs_corr <= 1.0))
        return fail(GAUSS_E_INVALID, "susie_min_abs_corr = %g: the purity threshold lies in [0, 1]", w.susie_min_abs_corr);
    // (an imputation window without unmeasured SNPs never gets here: gauss_job_create refuses it)
    // further traits (k_traits.hip)
    if (w.n_traits_more < 0 || w.n_traits_more > TRAITS_MAX)
        return fail(GAUSS_E_INVALID, "n_traits_more = %d: a window takes 0 .. %d further traits", w.n_traits_more, TRAITS_MAX);
    if (w.n_traits_more > 0) {
        if (!imputes) return fail(GAUSS_E_INVALID, "further traits (n_traits_more) are for imputation windows only (%s window)", not_imputing);
        if (!w.z_more || !w.out.z_more)
            return fail(GAUSS_E_INVALID, "n_traits_more = %d needs z_more and out_z_more (%s is NULL)", w.n_traits_more, !w.z_more ? "z_more" : "out_z_more");
    }
    // every trait of the window in one fit, and the colocalisation of their signals (k_susie.hip, k_coloc.hip)
    if (w.susie_traits_more < 0 || w.susie_traits_more > w.n_traits_more || w.susie_traits_more > SUSIE_K)
        return fail(GAUSS_E_INVALID, "coloc_traits_more = %d: the fit takes 0 .. min(n_traits_more = %d, %d) further traits", w.susie_traits_more,
                    w.n_traits_more, SUSIE_K);
    if (w.susie_traits_more > 0 && !susie)
        return fail(GAUSS_E_INVALID, "coloc_traits_more = %d fits further traits beside z1: it needs susie_L > 0", w.susie_traits_more);
    if (w.susie_traits_more > 0 && w.miss_more)
        return fail(GAUSS_E_INVALID, "coloc_traits_more = %d with miss_more: traits that lack measured SNPs are not fitted", w.susie_traits_more);
    const bool more_out = w.out.more_pip || w.out.more_set || w.out.more_set_pip || w.out.more_V || w.out.more_lse || w.out.more_mass ||
                          w.out.more_purity || w.out.more_size || w.out.more_kept || w.out.more_alpha || w.out.more_mu || w.out.more_lbf ||
                          w.out.more_sweeps || w.out.more_status;
    if (more_out && w.susie_traits_more <= 0)
        return fail(GAUSS_E_INVALID, "out_coloc_more_* are the further traits' fits: they need coloc_traits_more > 0");
    if (w.out.susie_lbf && !susie) return fail(GAUSS_E_INVALID, "out_coloc_lbf belongs to the multi-causal fit: it needs susie_L > 0");
    const bool coloc = w.coloc_p1 != 0.0 || w.coloc_p2 != 0.0 || w.coloc_p12 != 0.0;
    if (coloc) {
        if (!(w.coloc_p1 > 0.0 && w.coloc_p1 < 1.0)) return fail(GAUSS_E_INVALID, "coloc_p1 = %g: a prior probability lies in (0, 1)", w.coloc_p1);
        if (!(w.coloc_p2 > 0.0 && w.coloc_p2 < 1.0)) return fail(GAUSS_E_INVALID, "coloc_p2 = %g: a prior probability lies in (0, 1)", w.coloc_p2);
        if (!(w.coloc_p12 > 0.0 && w.coloc_p12 < 1.0)) return fail(GAUSS_E_INVALID, "coloc_p12 = %g: a prior probability lies in (0, 1)", w.coloc_p12);
        if (w.coloc_p12 > std::min(w.coloc_p1, w.coloc_p2))
            return fail(GAUSS_E_INVALID, "coloc_p12 = %g exceeds min(coloc_p1, coloc_p2) = %g", w.coloc_p12, std::min(w.coloc_p1, w.coloc_p2));
        if (!susie || w.susie_traits_more < 1)
            return fail(GAUSS_E_INVALID, "coloc_p1 / coloc_p2 / coloc_p12 colocalise pairs of fitted traits: they need susie_L > 0 and coloc_traits_more >= 1");
    }
    if ((w.out.coloc_pp || w.out.coloc_hit || w.out.coloc_hit_pp || w.out.coloc_n) && !coloc)
        return fail(GAUSS_E_INVALID, "out_coloc_* need coloc_p1, coloc_p2 and coloc_p12");
    // joint fine-mapping across studies (k_xsusie.hip): what one window can be asked alone; the group itself is job_build's
    if (w.xs_group < 0) return fail(GAUSS_E_INVALID, "xs_group = %d: a group id is positive (0: off)", w.xs_group);
    if (w.xs_group > 0 && !susie) return fail(GAUSS_E_INVALID, "xs_group = %d joins the window's multi-causal fit to a group: it needs susie_L > 0", w.xs_group);
    if (w.xs_group > 0 && w.susie_traits_more > 0)
        return fail(GAUSS_E_INVALID, "coloc_traits_more = %d in a group (xs_group = %d): a group fits one trait per study", w.susie_traits_more, w.xs_group);
    if (w.xs_from_lead && w.xs_group <= 0) return fail(GAUSS_E_INVALID, "xs_from_lead maps a group leader's candidates: it needs xs_group > 0");
    if ((w.out.xs_V || w.out.xs_purity || w.out.xs_mu || w.out.xs_n) && w.xs_group <= 0)
        return fail(GAUSS_E_INVALID, "out_xs_* are a group leader's outputs: they need xs_group > 0");
    // further traits that lack some measured SNPs (k_traits_miss.hip): the mask as index lists (MissTab)
    std::vector<int> miss_tab;
    int miss_n = 0, miss_nm = 0, miss_ne = 0;
    if (w.miss_more) {
        if (w.n_traits_more <= 0)
            return fail(GAUSS_E_INVALID, "miss_more says which SNPs the further traits lack: it needs n_traits_more > 0 (n_traits_more = %d)", w.n_traits_more);
        if (!w.out.info_more || !w.out.z_miss || !w.out.info_miss)
            return fail(GAUSS_E_INVALID, "miss_more needs out_info_more, out_z_miss and out_info_miss (%s is NULL)",
                        !w.out.info_more ? "out_info_more" : !w.out.z_miss ? "out_z_miss" : "out_info_miss");
        miss_tab.assign(MissTab::count, 0);
        std::vector<int> pos_of((size_t)w.M, -1);
        for (int t = 0; t < w.n_traits_more; t++)
            for (int m = 0; m < w.M; m++)
                if (w.miss_more[(size_t)t * w.M + m]) pos_of[(size_t)m] = 0;
        for (int e = 0; e < MISS_E; e++) miss_tab[MissTab::e + e] = -1;
        for (int m = 0; m < w.M; m++)
            if (pos_of[(size_t)m] == 0) {
                if (miss_ne < MISS_E) miss_tab[MissTab::e + miss_ne] = m;
                pos_of[(size_t)m] = miss_ne++;
            }
        if (miss_ne > MISS_E)
            return fail(GAUSS_E_INVALID, "miss_more: %d distinct measured SNPs are missing in some trait; a window takes at most %d", miss_ne, MISS_E);
        for (int t = 0; t < w.n_traits_more; t++) {
            int k = 0;
            for (int m = 0; m < w.M; m++) k += w.miss_more[(size_t)t * w.M + m] ? 1 : 0;
            if (k > MISS_K)
                return fail(GAUSS_E_INVALID, "miss_more: further trait %d lacks %d of the window's measured SNPs; a trait may lack at most %d", t, k, MISS_K);
            if (k >= w.M)
                return fail(GAUSS_E_INVALID, "miss_more: further trait %d lacks all %d measured SNPs of the window; every trait keeps at least one", t, w.M);
            miss_tab[MissTab::k + t] = k;
            miss_tab[MissTab::off + t] = miss_n;
            if (k) miss_tab[MissTab::masked + miss_nm++] = t;
            for (int m = 0, j = 0; m < w.M; m++)
                if (w.miss_more[(size_t)t * w.M + m]) {
                    miss_tab[MissTab::idx + t * MISS_K + j] = m;
                    miss_tab[MissTab::pos + t * MISS_K + j++] = pos_of[(size_t)m];
                }
            miss_n += k;
        }
    }

    Prob& p = pl.p;
    memset(&p, 0, sizeof(p));
    p.mode = w.mode;
    p.M = w.M; p.N = N;
    {
        int nc = 0;
        for (int c = 0; c < 3; c++) if (w.u_codings & (1 << c)) p.code_blk[nc++] = c;
        if (nc == 0) { p.code_blk[0] = 0; nc = 1; }
        p.U_raw = std::max(w.U, 1);
        p.U = w.U * nc;                          // one block of U rows per coding
    }
    p.lambda = w.lambda; p.diag = w.diag;
    p.ld_only = w.ld_only;
    p.kind = w.kind; p.n_head = w.n_head; p.n_predm = w.n_predm;
    // the shifted factorisation tests lambda_min against MakePosDef's floor (imputation, util.cpp:310)
    // or against CountPC's cutoff (QCAT, util.cpp:379)
    p.eps = (w.kind == GAUSS_WIN_QCAT) ? w.eig_cutoff : w.eps;
    p.n_rhs = (w.kind == GAUSS_WIN_QCAT) ? w.n_predm + p.U : p.U;
    if (w.mode == GAUSS_MODE_POOLED) {
        // CalCor pools every selected population (util.cpp:53-64): one pseudo-population
        p.P = 1;
        pl.pop_raw_off = {0, N};
        pl.pop_w = {1.0};
    } else {
        p.P = w.n_pop;
        pl.pop_raw_off.assign(w.pop_off, w.pop_off + w.n_pop + 1);
        pl.pop_w.assign(w.pop_wgt, w.pop_wgt + w.n_pop);
    }
    const int P = p.P;
    for (int q = 0; q < P; q++) {
        const int m = pl.pop_raw_off[q + 1] - pl.pop_raw_off[q];
        const double factor = ((double)m) / (m - 1);           // util.cpp:117 (inf for m == 1, like the reference)
        pl.pop_wf.push_back(pl.pop_w[q] * factor);             // util.cpp:118: wgt_val*factor*(...) groups left to right
        pl.pop_md.push_back((double)m);
    }
    pl.pop_pk_off.assign(P + 1, 0);
    for (int q = 0; q < P; q++) {
        const int m = pl.pop_raw_off[q + 1] - pl.pop_raw_off[q];
        pl.pop_pk_off[q + 1] = pl.pop_pk_off[q] + (int)rup((size_t)m, KC);
    }
    p.geno_fmt = w.geno_fmt;
    pl.row_bytes = (size_t)N;
    if (w.geno_fmt == GAUSS_GENO_2BIT) {
        // every selected population is one source block ("run") padded to 64 samples, in the source row and in
        // the packed operand row alike; pooled statistics still see one pseudo-population spanning all runs
        pl.run_pk_off.assign(w.n_pop + 1, 0);
        long long end = 0;
        pl.row_bytes = 0;
        for (int q = 0; q < w.n_pop; q++) {
            const int blk = (int)rup((size_t)(w.pop_off[q + 1] - w.pop_off[q]), 64);
            pl.run_pk_off[q + 1] = pl.run_pk_off[q] + blk;
            const long long off = w.pop_src_off ? w.pop_src_off[q] : end;
            pl.run_src.push_back((int)off);
            pl.run_len.push_back(w.pop_off[q + 1] - w.pop_off[q]);
            if (!w.pop_src_off) end = off + blk / 4;
            pl.row_bytes = std::max(pl.row_bytes, (size_t)(off + blk / 4));
        }
        if (P == 1) pl.pop_pk_off[1] = pl.run_pk_off[w.n_pop];
        p.n_run = w.n_pop;
        pl.word_run.assign(pl.run_pk_off[w.n_pop] / 16, 0);
        for (int q = 0; q < w.n_pop; q++)
            for (int b = pl.run_pk_off[q] / 16; b < pl.run_pk_off[q + 1] / 16; b++) pl.word_run[b] = (uint8_t)q;
    }
    if (w.draw_pop) {
        // Resampled window (simulateLD.cpp:161-199): the operand row holds the n_drawn drawn samples in ascending source order
        // (the sums are exact integers: no order changes a bit), the statistics see one pseudo-population of n_cols samples
        // whose other n_cols - n_drawn are the reference's zero columns.  Only the drawn columns are packed and multiplied.
        if (w.mode != GAUSS_MODE_POOLED || !w.ld_only || w.U > 0 || w.gene_off || w.pair_i || w.gram_only)
            return fail(GAUSS_E_INVALID, "a resampled window is a pooled LD-only window of measured rows");
        if (w.n_drawn < 1 || !w.draw_sample) return fail(GAUSS_E_INVALID, "a resampled window needs at least one draw");
        if (w.n_cols < w.n_drawn) return fail(GAUSS_E_INVALID, "n_cols (%lld) < n_drawn (%lld)", (long long)w.n_cols, (long long)w.n_drawn);
        // Prob::N and Kp are ints, and the row sums (15 * 15 per drawn column at most) are int32 on the device
        if (w.n_cols > INT32_MAX) return fail(GAUSS_E_RANGE, "n_cols = %lld exceeds the int range of a window's sample count", (long long)w.n_cols);
        if (w.n_drawn * 225 >= (1LL << 31))
            return fail(GAUSS_E_RANGE, "%lld drawn samples exceed the exact-integer range (9.5 M)", (long long)w.n_drawn);
        const int nd = (int)w.n_drawn;
        std::vector<int32_t> col((size_t)nd);
        for (int k = 0; k < nd; k++) {
            const int q = w.draw_pop[k], s = w.draw_sample[k];
            if (q < 0 || q >= w.n_pop) return fail(GAUSS_E_INVALID, "draw %d: population %d is outside 0..%d", k, q, w.n_pop - 1);
            const int m = w.pop_off[q + 1] - w.pop_off[q];
            if (s < 0 || s >= m) return fail(GAUSS_E_INVALID, "draw %d: sample %d is outside population %d's 0..%d", k, s, q, m - 1);
            // a byte index into a one-byte row, a 2-bit sample index into a packed row (run_src: byte offset of the block)
            const long long c = w.geno_fmt == GAUSS_GENO_2BIT ? 4LL * pl.run_src[(size_t)q] + s : (long long)w.pop_off[q] + s;
            if (c > INT32_MAX) return fail(GAUSS_E_RANGE, "draw %d: source column %lld exceeds the int range", k, c);
            col[(size_t)k] = (int32_t)c;
        }
        std::sort(col.begin(), col.end());
        const int Kp = (int)rup((size_t)nd, KC);
        col.resize((size_t)Kp, -1);
        pl.draw_col.swap(col);
        p.N = (int)w.n_cols;
        pl.pop_raw_off = {0, (int)w.n_cols};
        pl.pop_w = {1.0};
        pl.pop_wf = {((double)w.n_cols) / (w.n_cols - 1)};
        pl.pop_md = {(double)w.n_cols};
        pl.pop_pk_off = {0, Kp};
        p.row_src_bytes = (int)std::min<size_t>(pl.row_bytes, INT32_MAX);
    }
    if (w.rows_m) pl.rows_m.assign(w.rows_m, w.rows_m + w.M);
    if (w.rows_u && w.U > 0) pl.rows_u.assign(w.rows_u, w.rows_u + w.U);
    p.Kp = pl.pop_pk_off[P];
    // the Gram kernel addresses a lane's place inside an operand tile (TILE rows) with a 32-bit offset (k_gram.hip: run_item)
    if ((long long)TILE * p.Kp > INT32_MAX) return fail(GAUSS_E_RANGE, "%d packed samples per row: a tile of %d rows exceeds 2^31 bytes", p.Kp, TILE);
    // 16-bit partial slabs: 2-bit sources carry codes 0..3 (recoding only lowers them), so a segment of at most 7168
    // samples sums to <= 9 * 7168 < 2^16; the fast epilogue reads them (windows with LDS-resident population tables);
    // LD-only calls and gene batches keep f32 / int32 slabs
    p.slab16 = (w.geno_fmt == GAUSS_GENO_2BIT && !w.ld_only && !w.gene_off && P <= 32) ? 1 : 0;
    if (p.slab16) seg_max = std::min(seg_max, 7168);
    pl.word_pop.assign(p.Kp / 16, 0);
    // K chunks that end a zero-padded block (a population, or a 2-bit source block) with fewer than 64 live samples: how many
    // units of 8 samples are live (Item::chunk_live; 0 = the whole chunk)
    pl.chunk_live.assign((p.Kp / KC + 7) / 8 + 1, 0u);
    auto set_live = [&](int chunk, int samples) {
        const int units = (samples + 7) / 8;
        if (units >= 1 && units < 8) pl.chunk_live[chunk >> 3] |= (uint32_t)units << (4 * (chunk & 7));
    };
    if (!pl.draw_col.empty()) {
        if (w.n_drawn % KC) set_live(p.Kp / KC - 1, (int)(w.n_drawn % KC));      // the draws end in zero padding
    } else if (w.geno_fmt == GAUSS_GENO_2BIT) {
        for (int q = 0; q < w.n_pop; q++) {
            const int m = w.pop_off[q + 1] - w.pop_off[q], rem = m % KC;
            if (m > 0 && rem) set_live(pl.run_pk_off[q + 1] / KC - 1, rem);
        }
    } else {
        for (int q = 0; q < P; q++) {
            const int m = pl.pop_raw_off[q + 1] - pl.pop_raw_off[q], rem = m % KC;
            if (m > 0 && rem) set_live(pl.pop_pk_off[q + 1] / KC - 1, rem);
        }
    }
    pl.pop_seg0.assign(P + 1, 0);
    for (int q = 0; q < P; q++) {
        for (int b = pl.pop_pk_off[q] / 16; b < pl.pop_pk_off[q + 1] / 16; b++) pl.word_pop[b] = (uint8_t)q;
        const int chunks = (pl.pop_pk_off[q + 1] - pl.pop_pk_off[q]) / KC;
        pl.pop_seg0[q] = (int)pl.seg_pop.size();
        if (chunks > 0) {
            const int max_chunks = seg_max / KC;
            const int ns = (chunks + max_chunks - 1) / max_chunks;
            const int per = (chunks + ns - 1) / ns;
            for (int c = 0; c < chunks; c += per) {
                const int c1 = std::min(chunks, c + per);
                pl.seg_pop.push_back(q);
                pl.seg_k0.push_back(pl.pop_pk_off[q] + c * KC);
                pl.seg_k1.push_back(pl.pop_pk_off[q] + c1 * KC);
            }
        }
    }
    pl.pop_seg0[P] = (int)pl.seg_pop.size();
    p.nseg = (int)pl.seg_pop.size();
    for (int s0 = 0; s0 < p.nseg;) {
        int s1 = s0 + 1;
        int len = pl.seg_k1[s0] - pl.seg_k0[s0];
        while (s1 < p.nseg && len < group_target) { len += pl.seg_k1[s1] - pl.seg_k0[s1]; s1++; }
        pl.groups.push_back(std::make_pair(s0, s1));
        s0 = s1;
    }
    for (int s0 = 0; s0 < p.nseg; s0++) pl.fine.push_back(std::make_pair(s0, s0 + 1));

    p.Mp = (int)rup((size_t)w.M, TILE);
    p.Up = (int)rup((size_t)p.U, TILE);
    p.Sp = p.Mp + p.Up;
    p.nT = p.Sp / TILE;
    const int mt = p.Mp / TILE;
    pl.pair_lut.assign((size_t)p.nT * p.nT, -1);
    auto add_pair = [&](int ti, int tj) {
        if (pl.pair_lut[(size_t)ti * p.nT + tj] >= 0) return;
        const int id = (int)pl.pair_ti.size();
        pl.pair_ti.push_back(ti); pl.pair_tj.push_back(tj);
        pl.pair_lut[(size_t)ti * p.nT + tj] = id;
        pl.pair_lut[(size_t)tj * p.nT + ti] = id;
    };
    if (w.gene_off) {
        // LD is only needed inside genes (gene.cpp:305-315): tile pairs touched by some gene
        pl.gene_off.assign(w.gene_off, w.gene_off + w.n_gene + 1);
        long long off = 0;
        for (int g = 0; g < w.n_gene; g++) {
            const int r0 = pl.gene_off[g], r1 = pl.gene_off[g + 1];
            if (r0 < 0 || r1 < r0 || r1 > w.M) return fail(GAUSS_E_INVALID, "gene_off out of range at gene %d", g);
            pl.gene_out_off.push_back(off);
            off += (long long)(r1 - r0) * (r1 - r0);
            if (r1 > r0)
                for (int ti = r0 / TILE; ti <= (r1 - 1) / TILE; ti++)
                    for (int tj = ti; tj <= (r1 - 1) / TILE; tj++) add_pair(ti, tj);
        }
        pl.out_ld_count = (size_t)off;
        p.n_gene = w.n_gene;
    } else if (w.pair_i) {
        // listed pairs (prep_zmix selectors): the tile pairs they touch
        for (int64_t k = 0; k < w.n_pairs; k++) {
            const int i = w.pair_i[k], j = w.pair_j[k];
            if (i < 0 || j <= i || j >= w.M) return fail(GAUSS_E_INVALID, "pair %lld = (%d, %d) is not i < j < n_snp", (long long)k, i, j);
            add_pair(i / TILE, j / TILE);
        }
        pl.out_ld_count = 0;
    } else {
        for (int ti = 0; ti < mt; ti++)
            for (int tj = ti; tj < mt; tj++) add_pair(ti, tj);          // B11 (upper tiles)
        for (int tu = mt; tu < p.nT; tu++)
            for (int tj = 0; tj < mt; tj++) add_pair(tu, tj);           // B21
        if (w.ld_only && !w.gram_only) pl.out_ld_count = (size_t)w.M * w.M;
    }
    p.npair = (int)pl.pair_ti.size();
    p.Mld = (int)rup((size_t)w.M, NB);
    p.nblk = p.Mld / NB;
    p.npanel = (w.ld_only || w.kind == GAUSS_WIN_LD) ? 0 : (p.n_rhs + NRU - 1) / NRU;
    p.npi = p.npanel > 0 ? (w.M + 1 + NR - 1) / NR : 0;
    p.Up128 = (int)rup((size_t)std::max(p.n_rhs, 1), 128);
    pl.U_user = w.U;
    if (w.z1) pl.z1.assign(w.z1, w.z1 + w.M);
    pl.h_geno_m = w.geno_m; pl.h_geno_u = w.geno_u; pl.user_ld = w.ld;
    pl.out_b11 = w.out_b11; pl.out_b21 = w.out_b21;
    Riders& rd = pl.rd;
    rd = Riders();
    rd.out = w.out;
    rd.loo = loo;
    rd.slct_K = w.slct_max;
    if (w.slct_max > 0) {
        rd.slct_forced.assign(w.slct_forced, w.slct_forced + w.n_slct_forced);
        p.slct_max = w.slct_max; p.n_slct_forced = w.n_slct_forced;
        p.slct_chi2_stop = w.slct_chi2_stop; p.slct_min_var_frac = w.slct_min_var_frac;
    }
    rd.cond = cond;
    p.cond_min_var_frac = cond || cs ? w.cond_min_var_frac : 0.0;
    rd.cs = cs;
    if (prs) {
        rd.prs_n_s = w.prs_n_s; rd.prs_n_lam = w.prs_n_lam;
        p.prs_n_s = w.prs_n_s; p.prs_n_lam = w.prs_n_lam; p.prs_max_sweeps = w.prs_max_sweeps; p.prs_n = w.prs_n; p.prs_tol = w.prs_tol;
        for (int a = 0; a < PRS_S; a++) p.prs_s[a] = a < w.prs_n_s ? w.prs_s[a] : 0.0;
        for (int a = 0; a < PRS_LAM; a++) p.prs_lam[a] = a < w.prs_n_lam ? w.prs_lam[a] : 0.0;
    }
    if (lds) {
        // positions and weights in the concatenated row space, the measured rows first; any radius from 2^32 on holds every 32-bit position
        rd.lds = true; rd.lds_C = w.lds_n_annot;
        rd.lds_bp.assign(w.lds_bp_m, w.lds_bp_m + w.M);
        if (w.U > 0) rd.lds_bp.insert(rd.lds_bp.end(), w.lds_bp_u, w.lds_bp_u + w.U);
        if (w.lds_n_annot > 0) rd.lds_annot.assign(w.lds_annot, w.lds_annot + (size_t)w.lds_n_annot * (size_t)(w.M + w.U));
        p.lds_on = 1; p.lds_C = w.lds_n_annot; p.lds_n = w.lds_n;
        p.lds_radius = std::min<long long>(w.lds_radius, 1LL << 32);
    }
    p.cs_coverage = cs ? w.cs_coverage : 0.0;
    p.cs_prior_var = cs ? w.cs_prior_var : 0.0;
    if (susie) {
        rd.susie_L = w.susie_L;
        rd.susie_am = w.out.susie_alpha || w.out.susie_mu;
        p.susie_L = w.susie_L; p.susie_max_sweeps = w.susie_max_sweeps; p.susie_am = rd.susie_am ? 1 : 0;
        p.susie_estimate_var = w.susie_estimate_var ? 1 : 0; p.susie_measured_only = w.susie_measured_only ? 1 : 0;
        p.susie_coverage = w.susie_coverage; p.susie_prior_var = w.susie_prior_var; p.susie_tol = w.susie_tol;
        p.susie_min_abs_corr = w.susie_min_abs_corr;
    }
    rd.traits_T = w.n_traits_more;
    if (w.n_traits_more > 0) {
        // SNP-major and padded to the kernels' tiles: row g = the T traits' Z-scores at measured SNP g
        const int T16 = traits_t16(w.n_traits_more);
        rd.traits_z.assign((size_t)p.Mld * T16, 0.0);
        for (int t = 0; t < w.n_traits_more; t++)
            for (int g = 0; g < w.M; g++)      // (a score the trait lacks is not read: an exact zero takes its place)
                rd.traits_z[(size_t)g * T16 + t] = (w.miss_more && w.miss_more[(size_t)t * w.M + g]) ? 0.0 : w.z_more[(size_t)t * w.M + g];
        p.traits_T = w.n_traits_more;
    }
    if (susie) {
        rd.susie_k = w.susie_traits_more;
        rd.susie_lbf = w.out.susie_lbf || w.out.more_lbf;
        rd.coloc = coloc;
        p.susie_k = rd.susie_k; p.susie_lbf = rd.susie_lbf ? 1 : 0; p.coloc = coloc ? 1 : 0;
        p.coloc_p1 = w.coloc_p1; p.coloc_p2 = w.coloc_p2; p.coloc_p12 = w.coloc_p12;
    }
    rd.xs_group = w.xs_group;
    rd.miss = !miss_tab.empty();
    rd.miss_n = miss_n;
    rd.miss_tab.swap(miss_tab);
    p.miss_E = miss_ne; p.miss_nm = miss_nm; p.miss_n = miss_n;
    return GAUSS_OK;
}

// Arena layout helper
struct Arena {
    size_t off = 0;
    size_t take(size_t bytes) { size_t o = off; off = rup(off + bytes, 256); return o; }
};

template <typename T>
static size_t put(std::vector<char>& blob, Arena& a, const std::vector<T>& v)
{
    const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 1);
    const size_t o = a.take(bytes);
    if (blob.size() < a.off) blob.resize(a.off);
    if (!v.empty()) memcpy(blob.data() + o, v.data(), v.size() * sizeof(T));
    return o;
}
// The groups of the joint fit across studies (gauss_window_desc.xs_group; k_xsusie.hip): the windows of equal id in job order, the
// first its leader.  Checks what only the group can be asked (its size, equal susie_* arguments, who may carry outputs, the maps)
// and leaves every member's place, peers and validated maps in its plan.  No kernel checks a map again.
static int plan_xs_groups(const std::vector<WinSpec>& specs, std::vector<Plan>& plans)
{
    std::map<int, std::vector<int>> groups;
    for (size_t i = 0; i < specs.size(); i++)
        if (specs[i].xs_group > 0) groups[specs[i].xs_group].push_back((int)i);
    for (const auto& kv : groups) {
        const std::vector<int>& mem = kv.second;
        const int id = kv.first, K = (int)mem.size(), lead = mem[0];
        if (K < 2 || K > XS_MAX)
            return fail(GAUSS_E_INVALID, "xs_group = %d has %d window%s: a group is 2 .. %d windows of one job", id, K, K == 1 ? "" : "s", XS_MAX);
        const WinSpec& a = specs[(size_t)lead];
        const int TL = a.M + a.U;
        if (a.xs_from_lead) return fail(GAUSS_E_INVALID, "window %d: xs_from_lead on the leader of xs_group = %d (the first window of a group has no map)", lead, id);
        for (int k = 0; k < K; k++) {
            const int i = mem[(size_t)k];
            const WinSpec& w = specs[(size_t)i];
            Riders& rd = plans[(size_t)i].rd;
            Prob& p = plans[(size_t)i].p;
            const char* differs = w.susie_L != a.susie_L ? "susie_L" : w.susie_coverage != a.susie_coverage ? "susie_coverage" :
                w.susie_prior_var != a.susie_prior_var ? "susie_prior_var" : w.susie_tol != a.susie_tol ? "susie_tol" :
                w.susie_min_abs_corr != a.susie_min_abs_corr ? "susie_min_abs_corr" : w.susie_max_sweeps != a.susie_max_sweeps ? "susie_max_sweeps" :
                (w.susie_estimate_var != 0) != (a.susie_estimate_var != 0) ? "susie_estimate_var" :
                (w.susie_measured_only != 0) != (a.susie_measured_only != 0) ? "susie_measured_only" : nullptr;
            if (differs) return fail(GAUSS_E_INVALID, "window %d: %s differs from the leader's (window %d): the windows of xs_group = %d share their susie_* arguments", i, differs, lead, id);
            const RiderOuts& o = w.out;
            if (k > 0 && (o.susie_pip || o.susie_set || o.susie_set_pip || o.susie_V || o.susie_lse || o.susie_mass || o.susie_purity || o.susie_size ||
                          o.susie_kept || o.susie_alpha || o.susie_mu || o.susie_sweeps || o.susie_lbf))
                return fail(GAUSS_E_INVALID, "window %d: out_susie_* on a peer of xs_group = %d: the joint fit is returned on the leader (window %d)", i, id, lead);
            if (k > 0 && (o.xs_V || o.xs_purity || o.xs_mu || o.xs_n))
                return fail(GAUSS_E_INVALID, "window %d: out_xs_* on a peer of xs_group = %d: they are the leader's (window %d)", i, id, lead);
            const int T = w.M + w.U;
            if (k > 0 && !w.xs_from_lead && (w.M != a.M || w.U != a.U))
                return fail(GAUSS_E_INVALID, "window %d: xs_from_lead is NULL (the same index) but n_measured / n_unmeasured = %d / %d differ from the leader's %d / %d",
                            i, w.M, w.U, a.M, a.U);
            if (w.xs_from_lead) {
                rd.xs_from_lead.assign(w.xs_from_lead, w.xs_from_lead + TL);
                rd.xs_to_lead.assign((size_t)T, -1);
                for (int j = 0; j < TL; j++) {
                    const int c = rd.xs_from_lead[(size_t)j];
                    if (c < -1 || c >= T)
                        return fail(GAUSS_E_INVALID, "window %d: xs_from_lead[%d] = %d is neither -1 nor a candidate of the window (0 .. %d)", i, j, c, T - 1);
                    if (c >= 0 && rd.xs_to_lead[(size_t)c] >= 0)
                        return fail(GAUSS_E_INVALID, "window %d: xs_from_lead[%d] = xs_from_lead[%d] = %d: two leader candidates cannot be one SNP", i,
                                    rd.xs_to_lead[(size_t)c], j, c);
                    if (c >= 0) rd.xs_to_lead[(size_t)c] = j;
                }
            }
            rd.xs_K = K; rd.xs_pos = k; rd.xs_lead = lead; rd.xs_mu = k == 0 && o.xs_mu != nullptr;
            p.xs_n = K; p.xs_pos = k; p.xs_mu = rd.xs_mu ? 1 : 0;
            for (int s = 0; s < XS_MAX; s++) p.xs_peer[s] = mem[(size_t)std::min(s, K - 1)];
        }
    }
    return GAUSS_OK;
}

// ---- job_build: the planned windows of a batch -> tables, work lists, workspace and device descriptors ----

// live rows of row tile t of a plan (the job-wide rows keep a table: their clusters end in padding rows)
static inline int live_rows(const Plan& pl, int t)
{
    const Prob& p = pl.p;
    const int mt = p.Mp / TILE;
    if (!pl.tile_live.empty()) return pl.tile_live[(size_t)t];
    const int left = (t < mt) ? p.M - t * TILE : p.U - (t - mt) * TILE;
    return left > TILE ? TILE : left;
}
// f(ti, tj) for every job-wide tile pair ti <= tj that `rows` measured rows from job-wide row `row0` on lie in
template <typename F>
static void for_tile_pairs(size_t row0, size_t rows, F f)
{
    const int lo = (int)(row0 / TILE), hi = (int)((row0 + rows - 1) / TILE);
    for (int ti = lo; ti <= hi; ti++)
        for (int tj = ti; tj <= hi; tj++) f(ti, tj);
}
struct ItemH { int prob, pair, group, len, b11, ord = 0; };     // b11: an item of B11 (job-wide pairs, or a window's own measured x measured pairs); ord: launch-order key (item_keys)

// What job_build's steps share.  Name once, bind later: the device bases are known only after the allocations, so a table,
// a map or a workspace block is named ONCE, where it is placed -- tab() copies a host vector into the table image, ws() and
// slab() take a block of the zeroed workspace or of the slab arena -- and each call records (the pointer field, the offset,
// the base); relocate() writes base + offset into every recorded field.  The fields live in job->plans (sized before the first
// call), in *job->gplan and in the job itself: none of them moves while the job is built.
struct JobBuild {
    gauss_ctx* ctx;
    const std::vector<WinSpec>& specs;
    int on_device;
    const StreamSetup* stream;
    gauss_job* job;
    bool streamed() const { return stream != nullptr; }
    bool shm() const { return job->gplan != nullptr; }
    int n_prob() const { return job->n + (shm() ? 1 : 0); }      // descriptors on the device: the windows, then the job-wide rows
    Plan& plan_of(int i) const { return i < job->n ? job->plans[i] : *job->gplan; }
    size_t exp_doubles = 0;                                // doubles of the pinned export mirror
    std::vector<ItemH> items;
    std::vector<uint8_t> item_class;                       // launch class of items[n]: 0 B11 (or everything), 1 early B21, 2 late B21
    std::vector<char> late_window;                         // early epilogue: windows whose B21 items end the merged launch
    std::vector<int2> rowmap, tilemap, tilemap_b21, panelmap, dpanelmap, gemmmap, finmap, loomap;
    std::vector<int> slctmap, condmap, csmap, susiemap, xsmap, xsleadmap, prsmap, ldsmap;
    std::vector<int2> traitsmap, traitsumap, missmap, misstmap, missumap;
    std::vector<const uint32_t*> chunk_live;               // per descriptor: its Plan::chunk_live on the device (Item::chunk_live)
    Arena ta;         // table image (job->h_tab)
    Arena wa;         // zeroed once per job: operand padding, B21 padding and the solve matrices rely on it
    Arena wslab;      // partial slabs: every entry a reader keeps is written by the Gram kernel first, so no zeroing
    size_t o_items = 0, o_probs = 0, o_exports = 0, slab_base = 0, res = 0;
    size_t pin_tab = 0, pin_res = 0, pin_st = 0;
    std::deque<std::vector<uint8_t>> stage;                // host gather buffers, alive until the copies have drained

    enum Base { TAB, WS, SLAB };
    struct Reloc { void* field; size_t off; Base base; };
    std::vector<Reloc> rel;
    template <typename P> size_t at(P*& field, size_t off, Base base, bool bound = true)
    { field = nullptr; if (bound) rel.push_back(Reloc{(void*)&field, off, base}); return off; }
    // a host vector in the table image (an empty one still takes its 256 bytes); !bound: placed all the same, the field stays null
    template <typename P, typename V> void tab(P*& field, const std::vector<V>& v, bool bound = true)
    {
        static_assert(sizeof(P) == sizeof(V), "the field points to the vector's elements");
        at(field, put(job->h_tab, ta, v), TAB, bound);
    }
    // a work list and its count (a list that nobody asked for takes nothing and points to the image's start)
    template <typename P, typename V> void tab(P*& field, int& count, const std::vector<V>& v, bool if_any = false)
    { count = (int)v.size(); if (if_any && v.empty()) at(field, 0, TAB); else tab(field, v); }
    template <typename P> size_t tab_block(P*& field, size_t bytes) { return at(field, ta.take(bytes), TAB); }      // written later, at the offset returned
    template <typename P> void ws(P*& field, size_t bytes, bool bound = true) { at(field, wa.take(bytes), WS, bound); }
    template <typename P> void slab(P*& field, size_t bytes) { at(field, wslab.take(bytes), SLAB); }
    void relocate()
    {
        char* const base[3] = {job->d_tab, job->d_ws, job->d_ws + slab_base};
        for (const Reloc& r : rel) { char* const addr = base[r.base] + r.off; memcpy(r.field, &addr, sizeof(addr)); }
    }
    // the steps, in job_build's order; each returns a status
    int plan_windows(), plan_exports(), share_measured(), check_row_lists(), place_all_tables(), work_lists(), order_items(), place_lists();
    int layout_workspace(), allocate(), events_and_zeroing(), bind(), upload_host_rows(), write_items(), fill_report(), export_descriptors();
    int upload_tables();
    // ... and their parts
    void place_tables(Plan& pl, const uint32_t*& d_chunk_live, bool window), layout_window(Plan& pl);
    void item_keys(), sort_items(), launch_classes(), stream_groups(), xcd_interleave();
    int upload_rows(const Plan& pl, const uint8_t* dst_rows, const uint8_t* src, const std::vector<int32_t>& rows, int nrows);
};
int JobBuild::plan_windows()
{
    job->ctx = ctx;
    job->n = (int)specs.size();
    job->on_device = on_device;
    job->gram_i8 = ctx->gram_i8;
    job->gram_packed = (ctx->gram_packed && !ctx->gram_i8) ? 1 : 0;
    // Narrow layouts for the f32 kernel's half-empty tiles (k_gram_common.h: tile_layout); the int8 kernel keeps the quadrants (it is
    // bound by operand delivery, not by a wave's MFMA issue).  GAUSS_GRAM_ROTATE=0 restores the quadrant roles for every item (the
    // switch was named for a rotation of the roles, which the placement probe ruled out: tools/wave_simd_probe.py);
    // GAUSS_GRAM_NARROW=0 does the same.  Read per job: the tests build both forms in one process.
    job->gram_narrow = (!ctx->gram_i8 && env_int("GAUSS_GRAM_ROTATE", 1) != 0 && env_int("GAUSS_GRAM_NARROW", 1) != 0) ? 1 : 0;
    job->plans.resize(job->n);
    for (const WinSpec& w : specs)
        if (w.draw_pop && (specs.size() != 1 || streamed())) return fail(GAUSS_E_INVALID, "a resampled window is a job of its own");
    const int seg_max = seg_max_for(specs);
    for (int i = 0; i < job->n; i++) {
        int rc = plan_problem(specs[i], job->plans[i], seg_max, group_target_for(specs.size()));
        if (rc) return rc;
        job->plans[i].p.gram_i8 = job->gram_i8;
        if (!job->plans[i].draw_col.empty()) job->resample_lds = resample_pack_lds_bytes(job->plans[i].p.row_src_bytes);
    }
    return plan_xs_groups(specs, job->plans);
}
// Matrix exports (gauss_job.h): which matrices the caller wants back, and where each lands in the pinned mirror
int JobBuild::plan_exports()
{
    if (streamed()) return GAUSS_OK;
    for (int i = 0; i < job->n; i++) {
        const Plan& pl = job->plans[i];
        const Prob& p = pl.p;
        const bool has = p.kind == GAUSS_WIN_LD || p.npanel > 0;          // (the windows gauss_job_fetch exports matrices for)
        if (!has) continue;
        if (pl.out_b11) { job->exports.push_back(gauss_job::Export{i, 0, exp_doubles, p.M, p.M, p.Mld, pl.out_b11}); exp_doubles += (size_t)p.M * p.M; }
        if (pl.out_b21 && p.U > 0) { job->exports.push_back(gauss_job::Export{i, 1, exp_doubles, p.U, p.M, p.Mld, pl.out_b21}); exp_doubles += (size_t)p.U * p.M; }
        exp_doubles = rup(exp_doubles, 32);                                // every window's block starts on a 256-byte boundary
    }
    if (exp_doubles * sizeof(double) > ((size_t)256 << 20)) { job->exports.clear(); exp_doubles = 0; }      // pinned budget: per matrix instead
    return GAUSS_OK;
}
// Shared measured rows: every window reads its measured SNPs from the same resident store under the same populations.
// The job keeps ONE list of measured rows, made of CLUSTERS: a window whose rows continue a run of the current cluster
// (the next window of a chromosome: half its measured SNPs are the previous window's) joins it at that offset -- when
// that costs no more B11 tile pairs than tiles of its own would -- and every other window starts a new cluster on a
// tile boundary (padding rows in between: never packed, all zero), where it costs exactly what its own tiles would.
// So sharing can only save work: the scattered windows of a multi-GPU share keep their own tiles, two neighbours that
// landed on the same rank share theirs (round 3 had one all-or-nothing list whose tiles started where the LIST started:
// a share's scattered windows paid an extra row tile each and sharing was switched off for them).
int JobBuild::share_measured()
{
    if (!(on_device && !streamed() && job->n >= 2 && env_int("GAUSS_SHARE_MEASURED", 1) != 0)) return GAUSS_OK;
    const Plan& a = job->plans[0];
    bool ok = true;
    std::vector<int32_t> gl;
    std::vector<int> g0((size_t)job->n, 0);
    std::set<std::pair<int, int>> have;                     // job-wide B11 tile pairs so far
    size_t cl0 = 0, own_pairs = 0;                          // start of the current cluster in gl
    for (int i = 0; i < job->n && ok; i++) {
        const Plan& b = job->plans[i];
        ok = !b.rows_m.empty() && !b.p.ld_only && !b.p.n_gene && b.p.P <= 32 && b.h_geno_m == a.h_geno_m && b.user_ld == a.user_ld &&
             b.p.mode == a.p.mode && b.p.P == a.p.P && b.p.geno_fmt == a.p.geno_fmt && b.p.slab16 == a.p.slab16 && b.p.Kp == a.p.Kp &&
             b.pop_raw_off == a.pop_raw_off && b.pop_pk_off == a.pop_pk_off && b.pop_w == a.pop_w && b.seg_k0 == a.seg_k0 &&
             b.seg_k1 == a.seg_k1 && b.seg_pop == a.seg_pop && b.run_src == a.run_src && b.run_pk_off == a.run_pk_off &&
             b.groups == a.groups;
        if (!ok) break;
        const size_t M = b.rows_m.size(), mt = (M + TILE - 1) / TILE;
        own_pairs += mt * (mt + 1) / 2;
        // does the window continue a run of the current cluster?  (the cluster is ascending where that matters: a window
        // only joins through a binary search for its first row and an element-wise comparison of the overlap)
        size_t pos = gl.size();
        bool join = false;
        if (gl.size() > cl0 && std::is_sorted(gl.begin() + (ptrdiff_t)cl0, gl.end())) {
            const int32_t first = b.rows_m[0];
            const size_t p0 = (size_t)(std::lower_bound(gl.begin() + (ptrdiff_t)cl0, gl.end(), first) - gl.begin());
            if (p0 < gl.size() && gl[p0] == first) {
                join = true;
                for (size_t k = 0; k < M && join; k++) {
                    if (k > 0 && b.rows_m[k] <= b.rows_m[k - 1]) join = false;
                    else if (p0 + k < gl.size() && gl[p0 + k] != b.rows_m[k]) join = false;
                }
                if (join) {
                    // tile pairs the window would ADD as part of the cluster, against tiles of its own
                    size_t add = 0;
                    for_tile_pairs(p0, M, [&](int ti, int tj) { add += have.count(std::make_pair(ti, tj)) ? 0 : 1; });
                    join = add <= mt * (mt + 1) / 2;
                    pos = p0;
                }
            }
        }
        if (!join) {
            gl.resize(rup(gl.size(), TILE), -1);               // a new cluster on a tile boundary (padding rows: never packed)
            cl0 = pos = gl.size();
        }
        g0[(size_t)i] = (int)pos;
        for (size_t k = 0; k < M; k++)
            if (pos + k >= gl.size()) gl.push_back(b.rows_m[k]);
        for_tile_pairs(pos, M, [&](int ti, int tj) { have.insert(std::make_pair(ti, tj)); });
    }
    // worth the extra descriptor only if something IS shared (GAUSS_SHARE_MEASURED=2: always, for the tests)
    if (!(ok && (long long)gl.size() < (1 << 24) && (have.size() < own_pairs || env_int("GAUSS_SHARE_MEASURED", 1) == 2))) return GAUSS_OK;
    job->gplan.reset(new Plan(a));
    job->g0 = g0;
    Plan& g = *job->gplan;
    g.rows_m = gl;
    g.rows_u.clear(); g.z1.clear(); g.gene_off.clear(); g.gene_out_off.clear();
    Prob& q = g.p;
    q.M = (int)gl.size(); q.U = 0; q.U_raw = 1; q.n_rhs = 0;
    q.Mp = (int)rup((size_t)q.M, TILE); q.Up = 0; q.Sp = q.Mp; q.nT = q.Mp / TILE;
    q.Mld = 0; q.nblk = 0; q.npanel = 0; q.npi = 0; q.kind = 0; q.ld_only = 0; q.n_head = q.n_predm = 0;
    g.U_user = 0; g.h_geno_u = nullptr; g.rd = Riders(); clear_riders(q);
    // job-wide B11 pairs: the tile pairs some window lies in
    g.pair_ti.clear(); g.pair_tj.clear(); g.pair_lut.assign((size_t)q.nT * q.nT, -1);
    for (int i = 0; i < job->n; i++)
        for_tile_pairs((size_t)g0[(size_t)i], (size_t)job->plans[i].p.M, [&](int ti, int tj) {
            if (g.pair_lut[(size_t)ti * q.nT + tj] < 0) {
                g.pair_lut[(size_t)ti * q.nT + tj] = g.pair_lut[(size_t)tj * q.nT + ti] = (int)g.pair_ti.size();
                g.pair_ti.push_back(ti); g.pair_tj.push_back(tj);
            }
        });
    q.npair = (int)g.pair_ti.size();
    // live rows per job-wide row tile: up to the last real row in it (a cluster's last tile ends in padding rows, whose
    // dead 32-row halves the Gram kernel skips exactly as it does in a window's own last tile)
    g.tile_live.assign((size_t)q.nT, 0);
    for (size_t r = 0; r < gl.size(); r++)
        if (gl[r] >= 0) g.tile_live[r / TILE] = (int)(r % TILE) + 1;
    return GAUSS_OK;
}
// Row lists are resolved by the pack kernel: an index beyond the store would be an out-of-bounds read on the
// GPU.  Host stores cannot be checked (only a pointer is known), stores made by gauss_store_upload can.
int JobBuild::check_row_lists()
{
    std::map<const void*, size_t> stores;
    { std::lock_guard<std::mutex> lock(ctx->mu); stores = ctx->stores; }
    for (int i = 0; i < job->n; i++) {
        const Plan& pl = job->plans[i];
        for (int side = 0; side < 2; side++) {
            const std::vector<int32_t>& rows = side ? pl.rows_u : pl.rows_m;
            const uint8_t* base = side ? pl.h_geno_u : pl.h_geno_m;
            if (rows.empty()) continue;
            long long mx = -1;
            for (int32_t r : rows) {
                if (r < 0) { return fail(GAUSS_E_INVALID, "window %d: negative row index %d", i, (int)r); }
                mx = std::max<long long>(mx, r);
            }
            if (!on_device) continue;
            // the store that contains `base` (a window may point into the middle of an uploaded store)
            auto it = stores.upper_bound(base);
            if (it == stores.begin()) continue;                      // not one of ours: caller's responsibility
            --it;
            const uint8_t* s0 = (const uint8_t*)it->first;
            if (base >= s0 + it->second) continue;
            const size_t need = (size_t)(base - s0) + (size_t)mx * (size_t)pl.user_ld + pl.row_bytes;
            if (need > it->second) {
                return fail(GAUSS_E_INVALID, "window %d: row index %lld reaches past the end of the row store (%zu bytes)", i, mx, it->second);
            }
        }
    }
    return GAUSS_OK;
}
// The tables of one descriptor -- a window's, or the job-wide measured rows' -- in the order of the image.  Every list of the
// plan is placed, asked or not (the image does not depend on who reads it); the riders' lists only where they exist.
void JobBuild::place_tables(Plan& pl, const uint32_t*& d_chunk_live, bool window)
{
    Prob& p = pl.p;
    tab(p.pop_raw_off, pl.pop_raw_off); tab(p.pop_pk_off, pl.pop_pk_off);
    tab(p.pop_w, pl.pop_w); tab(p.pop_wf, pl.pop_wf); tab(p.pop_md, pl.pop_md);
    tab(p.seg_pop, pl.seg_pop); tab(p.seg_k0, pl.seg_k0); tab(p.seg_k1, pl.seg_k1); tab(p.pop_seg0, pl.pop_seg0);
    tab(p.pair_ti, pl.pair_ti); tab(p.pair_tj, pl.pair_tj); tab(p.pair_lut, pl.pair_lut);
    tab(p.word_pop, pl.word_pop);
    tab(p.z1, pl.z1, window);      // (the job-wide rows have no Z-scores)
    tab(p.gene_off, pl.gene_off, p.n_gene != 0); tab(p.gene_out_off, pl.gene_out_off, p.n_gene != 0);
    tab(p.word_run, pl.word_run); tab(p.run_pk_off, pl.run_pk_off); tab(p.run_src, pl.run_src);
    // row lists are resolved on the device only for a resident store; host rows are gathered while staging
    tab(p.rows_m, pl.rows_m, on_device && !pl.rows_m.empty()); tab(p.rows_u, pl.rows_u, on_device && !pl.rows_u.empty());
    tab(d_chunk_live, pl.chunk_live);
    tab(p.draw_col, pl.draw_col, !pl.draw_col.empty());
    if (!pl.rd.slct_forced.empty()) tab(p.slct_forced, pl.rd.slct_forced);
    if (!pl.rd.traits_z.empty()) tab(p.traits_Z, pl.rd.traits_z, pl.rd.traits_T != 0);
    if (!pl.rd.miss_tab.empty()) tab(p.miss_tab, pl.rd.miss_tab, pl.rd.miss);
    if (!pl.rd.xs_from_lead.empty()) tab(p.xs_from_lead, pl.rd.xs_from_lead);
    if (!pl.rd.xs_to_lead.empty()) tab(p.xs_to_lead, pl.rd.xs_to_lead);
    if (pl.rd.lds) tab(p.lds_bp, pl.rd.lds_bp);
    if (!pl.rd.lds_annot.empty()) tab(p.lds_annot, pl.rd.lds_annot);
}
// ---- table arena (host mirrored) ----
int JobBuild::place_all_tables()
{
    rel.reserve((size_t)n_prob() * 64 + 64);
    chunk_live.assign((size_t)n_prob(), nullptr);
    for (int i = 0; i < n_prob(); i++) place_tables(plan_of(i), chunk_live[(size_t)i], i < job->n);
    return GAUSS_OK;
}
// The work items of the Gram launch and the work lists of every other launch, in window order; the riders' largest dimensions
int JobBuild::work_lists()
{
    job->max_nblk = 0;
    {
        // tiles of the closing product at 128 right-hand sides each: a small job (an 8-rank share: ~570) cannot fill the
        // chip's 512 workgroup slots with them and is bound by the tiles' K loops, so it takes 64 (k_solve.hip)
        size_t t128 = 0;
        for (int i = 0; i < job->n; i++) {
            const Prob& p = job->plans[i].p;
            if (p.npanel > 0) t128 += (size_t)(p.Up128 / 128) * ((p.Mld + 127) / 128);
        }
        job->tail.gemm_ut = t128 < (size_t)GEMM_SMALL_TILES ? 64 : 128;
    }
    job->win_tiles.assign((size_t)job->n, std::vector<int2>());
    if (shm()) {
        // the job-wide measured rows are packed once, and B11's job-wide tile pairs multiplied once
        const Plan& g = *job->gplan;
        for (int pr = 0; pr < g.p.npair; pr++)
            for (size_t k = 0; k < g.groups.size(); k++)
                items.push_back(ItemH{job->n, pr, (int)k, g.seg_k1[g.groups[k].second - 1] - g.seg_k0[g.groups[k].first], 1});
        for (int r = 0; r < g.p.M; r++)
            if (g.rows_m[(size_t)r] >= 0) rowmap.push_back(make_int2(job->n, r));      // (padding rows between clusters stay zero)
    }
    // Every `fine_every`-th tile pair is cut into one work item per K segment (a population: 64 ... 3 600 samples)
    // instead of runs of >= 2048 samples: sorted by length they end up last and fill the launch's final round, in which
    // the 1 024 workgroup slots otherwise finish up to one 0.75 ms item apart.  Same segments, same slabs: same bits.
    // Measured on the bench job (Gram kernel): none 37.43 ms; every 16th / 8th / 4th / 2nd pair 37.11 / 37.15 / 37.11 /
    // 37.10; every pair 37.08 ms with twice the work items.
    const int fine_every = job->n >= 4 ? 16 : 0;
    int pair_no = 0;
    for (int i = 0; i < job->n; i++) {
        const Prob& p = job->plans[i].p;
        const int mt_i = p.Mp / TILE;
        for (int pr = 0; pr < p.npair; pr++) {
            const int b11 = job->plans[i].pair_ti[pr] < mt_i ? 1 : 0;
            if (shm() && b11) continue;                                    // a B11 pair: done on the job-wide tiles
            if (fine_every > 0 && ++pair_no % fine_every == 0 && job->plans[i].groups.size() < job->plans[i].fine.size()) {
                for (size_t g = 0; g < job->plans[i].fine.size(); g++) {
                    const std::pair<int, int>& gr = job->plans[i].fine[g];
                    items.push_back(ItemH{i, pr, -1 - (int)g, job->plans[i].seg_k1[gr.second - 1] - job->plans[i].seg_k0[gr.first], b11});
                }
                continue;
            }
            for (size_t g = 0; g < job->plans[i].groups.size(); g++) {
                const std::pair<int, int>& gr = job->plans[i].groups[g];
                items.push_back(ItemH{i, pr, (int)g, job->plans[i].seg_k1[gr.second - 1] - job->plans[i].seg_k0[gr.first], b11});
            }
        }
        for (int r = shm() ? p.M : 0; r < p.M + p.U; r++) rowmap.push_back(make_int2(i, r));
        if (shm()) {
            // this window's view of the job-wide B11 pairs it lies in
            const Plan& g = *job->gplan;
            for_tile_pairs((size_t)job->g0[(size_t)i], (size_t)p.M, [&](int ti, int tj) {
                const int2 e = make_int2(i, g.pair_lut[(size_t)ti * g.p.nT + tj] | TILE_GB11);
                tilemap.push_back(e); job->win_tiles[(size_t)i].push_back(e);
            });
        }
        if (!p.n_gene)
            for (int pr = 0; pr < p.npair; pr++) {
                const bool b21 = !p.ld_only && job->plans[i].pair_ti[pr] >= p.Mp / TILE;      // a tile of U rows x M columns
                if (shm() && !b21) continue;
                (b21 ? tilemap_b21 : tilemap).push_back(make_int2(i, pr));
                job->win_tiles[(size_t)i].push_back(make_int2(i, pr));
            }
        for (int pn = 0; pn < p.npi; pn++) panelmap.push_back(make_int2(i, pn));
        for (int pn = 0; pn < p.npanel; pn++) dpanelmap.push_back(make_int2(i, pn));
        const Riders& rd = job->plans[i].rd;
        if (rd.loo)
            for (int pn = 0; pn < (p.M + NR - 1) / NR; pn++) loomap.push_back(make_int2(i, pn));      // the panels that hold columns of X
        if (rd.slct_K) slctmap.push_back(i);
        if (rd.cond) { condmap.push_back(i); job->tail.cond_max_U = std::max(job->tail.cond_max_U, p.U); }
        if (rd.cs) { csmap.push_back(i); job->tail.cs_max_T = std::max(job->tail.cs_max_T, p.M + p.U); }
        if (rd.prs_n_s) { prsmap.push_back(i); job->tail.prs_max_s = std::max(job->tail.prs_max_s, rd.prs_n_s); job->tail.prs_max_M = std::max(job->tail.prs_max_M, p.M); }
        if (rd.lds) {
            ldsmap.push_back(i);
            job->tail.lds_max_M = std::max(job->tail.lds_max_M, p.M); job->tail.lds_max_C = std::max(job->tail.lds_max_C, rd.lds_C);
            job->tail.lds_max_chunks = std::max(job->tail.lds_max_chunks, lds_chunks(p.M, p.U));
        }
        if (rd.susie_L && rd.xs_group) {       // a member of a group of the joint fit across studies: launches and map of its own
            xsmap.push_back(i);
            if (rd.xs_pos == 0) xsleadmap.push_back(i);
            job->tail.xs_dims.grow(p, rd);
        } else if (rd.susie_L) {
            susiemap.push_back(i);
            job->tail.susie_dims.grow(p, rd);
            job->tail.susie_max_k = std::max(job->tail.susie_max_k, rd.susie_k); job->tail.susie_coloc = job->tail.susie_coloc || rd.coloc;
        }
        if (rd.traits_T) {
            for (int b = 0; b < p.nblk; b++) traitsmap.push_back(make_int2(i, b));
            for (int us = 0; us < (p.U + NB - 1) / NB; us++) traitsumap.push_back(make_int2(i, us));
        }
        if (rd.miss) {
            if (p.miss_nm) for (int b = 0; b < p.nblk; b++) missmap.push_back(make_int2(i, b));
            for (int k = 0; k < p.miss_nm; k++) misstmap.push_back(make_int2(i, k));
            for (int us = 0; us < (p.U + NB - 1) / NB; us++) missumap.push_back(make_int2(i, us));
        }
        if (p.npanel > 0) {
            job->max_nblk = std::max(job->max_nblk, p.nblk); job->max_npanel = std::max(job->max_npanel, p.npi);
            for (int up = 0; up < p.Up128 / job->tail.gemm_ut; up++)
                for (int kb = 0; kb < (p.Mld + 127) / 128; kb++) gemmmap.push_back(make_int2(i, (up << 8) | kb));
            for (int c = 0; c < (p.n_rhs + 255) / 256; c++) finmap.push_back(make_int2(i, c));
        }
        if (p.mode != 0) job->max_pop = std::max(job->max_pop, p.P);
    }
    return GAUSS_OK;
}
// The order key: the item's K length scaled by how much of the tile its slowest wave multiplies (a wave issues na x nb 32 x 32
// blocks per K step, 4 at most; the waves of a workgroup meet at a barrier every chunk, so the fullest wave sets the item's
// pace): full tiles start first, edge tiles (a window's last 17 rows are a quarter of a tile's work) end the launch.  Measured:
// one 529-SNP window (1.3 rounds of the chip's workgroup slots) Gram 115 -> 109 us; the 36-window job 36.62 -> 36.52 ms; an
// 8-rank share unchanged.  The order changes no bit (items are independent).
void JobBuild::item_keys()
{
    gauss_job* const job = this->job;
    std::vector<ItemH> items(std::move(this->items));      // (the steps of order_items work on locals, as the loops did inside one function: through `this` every store reloads them)
    for (ItemH& h : items) {
        h.ord = h.len;
        if (job->gram_i8) continue;          // (the int8 kernel is bound by operand delivery: it keeps items of one K range together -- 5.40 against 5.53 ms)
        const Plan& pl = plan_of(h.prob);
        const int ti = pl.pair_ti[h.pair], tj = pl.pair_tj[h.pair];
        const int ra = live_rows(pl, ti), rb = live_rows(pl, tj);
        // (packed items, k_gram.hip: a wave with any live A half issues one MFMA per live B half -- 2 at most, half a full unpacked wave)
        const bool packed = job->gram_packed && pl.p.slab16;
        // the waves' blocks by the item's layout (k_gram_common.h): a narrow layout halves the fullest wave's blocks, and the key follows
        const int layout = job->gram_narrow ? tile_layout(ra, rb, packed) : LAYOUT_QUAD;
        int mx = 0;
        for (int w = 0; w < 4; w++) {
            const WaveWork ww = wave_work(ra, rb, ti == tj, packed, false, w, layout);
            mx = std::max(mx, (packed ? std::min(ww.na, 1) : ww.na) * ww.nb);
        }
        h.ord = std::max(KC, (h.len * std::max(mx, 1) / 4 + KC - 1) / KC * KC);
    }
    items.swap(this->items);
}
// The launch order: longest segments first (the tail of the launch is then made of short items), inside up to three classes --
// B11's items, the early windows' B21 items, the late windows' (launch_classes).  One stable counting pass over (class, length): lengths
// are whole K chunks and a job has a handful of distinct ones (three stable sorts through the plans' tables were 0.3 ms of the
// 0.53 ms a three-window job took to plan; a rank of eight waits for exactly that before its GPU starts).
void JobBuild::sort_items()
{
    std::vector<ItemH> items(std::move(this->items));
    std::vector<uint8_t> item_class(std::move(this->item_class));
    int L = 0;
    bool whole = true;
    for (const ItemH& h : items) { L = std::max(L, h.ord / KC); whole = whole && h.ord % KC == 0 && h.ord >= 0; }
    if (!whole || (size_t)L > 4 * items.size() + 1024) {            // (never on a plan of this file: lengths are multiples of KC)
        std::vector<size_t> idx(items.size());
        for (size_t n = 0; n < idx.size(); n++) idx[n] = n;
        std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {
            return item_class[a] != item_class[b] ? item_class[a] < item_class[b] : items[a].ord > items[b].ord; });
        std::vector<ItemH> out(items.size());
        for (size_t n = 0; n < idx.size(); n++) out[n] = items[idx[n]];
        this->items.swap(out); this->item_class.swap(item_class);
        return;
    }
    const size_t nb = (size_t)3 * (size_t)(L + 1);
    std::vector<uint32_t> start(nb + 1, 0u);
    auto bucket = [&](size_t n) { return (size_t)item_class[n] * (size_t)(L + 1) + (size_t)(L - items[n].ord / KC); };
    for (size_t n = 0; n < items.size(); n++) start[bucket(n) + 1]++;
    for (size_t b = 0; b < nb; b++) start[b + 1] += start[b];
    std::vector<ItemH> out(items.size());
    for (size_t n = 0; n < items.size(); n++) out[start[bucket(n)]++] = items[n];
    this->items.swap(out); this->item_class.swap(item_class);
}
// Which launches the job's Gram items make, and the class of every item in them
void JobBuild::launch_classes()
{
    gauss_job* const job = this->job;
    std::vector<ItemH> items(std::move(this->items));
    auto is_b11 = [&](const ItemH& h) { return h.b11 != 0; };
    std::vector<uint8_t> item_class(items.size(), 0);
    std::vector<char> late_window;
    // Chain beside the Gram kernel (k_solve_lite.hip): B11's items become a launch of their own, B11's epilogue tiles and
    // the factorisation chain follow it on the chain queue, and the chain's latency hides under the Gram launch of
    // B21's items.  Worth it when that launch is long enough to cover B11's small-footprint epilogue tiles (~0.5 ms) and
    // the chain, which runs ~3 x slower beside the Gram kernel than alone (~100 us per block step: two launches);
    // GAUSS_CHAIN_ASIDE = 0 never, 2 always (tests), 1 (default) by this estimate.
    const int mode = env_int("GAUSS_CHAIN_ASIDE", 1);
    bool genes = false;
    double b21_len = 0.0;
    // an item's K length in the time units of the unpacked f32 kernel (the 120e12 below): a packed item (k_gram.hip) issues half
    // the MFMAs and pays the A-side combine and the sub-flushes on top -- GRAM_PACKED_COST of the unpacked time per sample
    auto cost_len = [&](const ItemH& h) { return (double)h.len * ((job->gram_packed && plan_of(h.prob).p.slab16) ? GRAM_PACKED_COST : 1.0); };
    for (const ItemH& h : items) if (!is_b11(h)) b21_len += cost_len(h);
    for (int i = 0; i < job->n; i++) genes = genes || job->plans[i].p.n_gene > 0;
    // (the int8 Gram kernel is ~8 x faster: an 8-rank share's B21 launch, 0.5 ms, no longer covers its chain)
    const double t_b21 = b21_len * 2.0 * TILE * TILE / (job->gram_i8 ? 960e12 : 120e12), t_chain = 0.5e-3 + 100e-6 * job->max_nblk;
    {
        double all_len = 0.0;
        for (const ItemH& h : items) all_len += cost_len(h);
        job->wait_bound_us = 50.0 * 1e6 * all_len * 2.0 * TILE * TILE / (job->gram_i8 ? 960e12 : 120e12);      // a whole-genome job must not trip a fixed bound
    }
    job->chain_aside = !streamed() && mode != 0 && !panelmap.empty() && !tilemap_b21.empty() && !genes && job->ctx->chain &&
                       job->ctx->side && (mode == 2 || t_b21 >= 1.2 * t_chain);
    if (job->chain_aside)
        for (size_t n = 0; n < items.size(); n++) {
            item_class[n] = is_b11(items[n]) ? 0 : 1;
            job->n_items_b11 += is_b11(items[n]) ? 1 : 0;
        }
    // Merged launch (round 4): B11's items and B21's items are ONE launch, B11's first; they count themselves off and the
    // chain queue starts when the count is complete (k_gram.hip: wait_count_kernel) -- the chip is never drained between
    // the two halves (two launches: 37.1 ms, one: 36.6 on the 36-window job).  GAUSS_CHAIN_MERGED=0: two launches + event.
    // (f32 only: the int8 Gram kernel is operand-delivery bound and the chain's memory traffic beside ALL of it costs more than
    // the second launch's start-up -- measured 8.70 ms per step merged against 8.35 ms as two launches; =2 forces it for both)
    {
        const int mm = env_int("GAUSS_CHAIN_MERGED", 1);
        job->merged = job->chain_aside && mm != 0 && (!job->gram_i8 || mm == 2);
        // =2 (tests): merged whatever the queue registry says -- job_queue_run otherwise takes the two-launch form for a run
        // whose context cannot be sure of a hardware queue per stream (gauss_ctx.cpp)
        job->force_merged = job->merged && mm == 2;
    }
    // Early epilogue: the smallest windows of the job that together hold about a third of B21's Gram work are "late" -- their
    // items end the launch -- and every other window is "early" (GAUSS_EPI_EARLY=0: off.  Measured by the late share,
    // 36-window step / slowest 8-rank share: off 40.04 / 5.45 ms; 6 % 39.89 / 5.51; 12 % 39.76 / 5.51; 25 % 39.75 / 5.45; 35 %
    // 39.67 / 5.40; 50 % 39.64 / 5.47 -- a late part that is too small opens the gate only when the launch is all but over and
    // the two epilogue launches cost their event hops).  One window: nothing to split.
    late_window.assign((size_t)job->n + 1, 0);
    if (job->merged && job->n >= 2 && job->ctx->side && env_int("GAUSS_EPI_EARLY", 1) != 0) {
        std::vector<double> w21((size_t)job->n, 0.0);
        double tot = 0;
        for (const ItemH& h : items) if (!is_b11(h)) { w21[(size_t)h.prob] += h.len; tot += h.len; }
        const double want = tot * 0.35;
        double acc = 0;
        int n_late = 0;
        // (the windows with the least B21 work: a share of four windows gives up its smallest one, not whichever comes last)
        std::vector<int> by_work((size_t)job->n);
        for (int i = 0; i < job->n; i++) by_work[(size_t)i] = i;
        std::stable_sort(by_work.begin(), by_work.end(), [&](int a, int b) { return w21[(size_t)a] < w21[(size_t)b]; });
        for (int k = 0; k + 1 < job->n && acc < want; k++) { late_window[(size_t)by_work[(size_t)k]] = 1; acc += w21[(size_t)by_work[(size_t)k]]; n_late++; }
        if (n_late > 0 && acc < tot) {
            for (size_t n = 0; n < items.size(); n++) {
                if (is_b11(items[n])) continue;
                if (late_window[(size_t)items[n].prob]) item_class[n] = 2;
                else job->n_items_b21_early++;
            }
        } else late_window.assign((size_t)job->n + 1, 0);
    }
    items.swap(this->items); item_class.swap(this->item_class); late_window.swap(this->late_window);
}
// streamed window: B11's items (measured rows only) first, then B21's items by chunk of `ct` unmeasured row
// tiles; each group is one Gram launch that starts as soon as its rows have landed
void JobBuild::stream_groups()
{
    const Plan& pl0 = job->plans[0];
    const int mt = pl0.p.Mp / TILE;
    const std::vector<int>& tile_group = stream->tile_group;
    const std::vector<int>& first_tile = stream->first_tile;
    const int ngrp = (int)first_tile.size() - 1;
    auto grp = [&](const ItemH& h) { const int ti = pl0.pair_ti[h.pair]; return ti < mt ? 0 : tile_group[(size_t)(ti - mt)]; };
    std::stable_sort(items.begin(), items.end(), [&](const ItemH& a, const ItemH& b) { return grp(a) < grp(b); });
    job->sgroups.assign((size_t)ngrp, gauss_job::StreamGroup{0, 0, 0, 0, 0, 0});
    for (size_t n = 0; n < items.size(); n++) {
        gauss_job::StreamGroup& g = job->sgroups[(size_t)grp(items[n])];
        if (g.n_items == 0) g.item0 = (int)n;
        g.n_items++;
    }
    job->sgroups[0].row0 = 0; job->sgroups[0].n_rows = pl0.p.M;
    for (int g = 1; g < ngrp; g++) {
        const int u0 = first_tile[(size_t)g] * TILE, u1 = std::min(pl0.p.U, first_tile[(size_t)g + 1] * TILE);
        job->sgroups[g].row0 = pl0.p.M + u0; job->sgroups[g].n_rows = std::max(0, u1 - u0);
        // B21's epilogue tiles are listed in pair order (row tile, then column tile): a chunk's tiles are contiguous
        job->sgroups[g].tile0 = first_tile[(size_t)g] * mt;
        job->sgroups[g].n_tiles = (first_tile[(size_t)g + 1] - first_tile[(size_t)g]) * mt;
    }
}
// XCD-aware launch order.  Workgroup b runs on XCD b % 8 (each XCD has its own 4 MiB L2).  Neighbours in
// the sorted list share operand tiles (same window, same K range, adjacent tile pairs), so the list is
// cut into super-blocks of xcd_block items and super-block j is queued on XCD j % 8: the items that are
// resident together on one XCD then read the same tiles at about the same K position.  Measured on the
// bench workload (rocprofv3 FETCH_SIZE): 22.0 GB -> 16.0 GB per launch at 36, same kernel time; larger
// blocks start to cost time (load balance).
void JobBuild::xcd_interleave()
{
    gauss_job* const job = this->job;
    std::vector<ItemH> items(std::move(this->items));
    // Small jobs (the 4-5 windows an 8-rank run leaves per GPU, ~7 000 items) take blocks of 8: a block of 36 is
    // 4 % of an XCD's share there, and the XCD that gets one more than the others finishes last (Gram kernel of
    // the 8-rank shares 5.10 -> 5.03 ms; 36 windows: 38.5 ms either way, but 36 reads 27 % less from the fabric).
    const int xcd_block = items.size() >= 20000 ? 36 : 8;
    // (a job whose B11 items are a launch of their own interleaves each launch's list by itself)
    auto interleave = [&](size_t i0, size_t i1) {
        if (xcd_block <= 0 || i1 - i0 <= (size_t)8 * xcd_block) return;
        std::vector<std::vector<ItemH>> q(8);
        for (size_t i = i0; i < i1; i++) q[((i - i0) / xcd_block) % 8].push_back(items[i]);
        size_t pos[8] = {0, 0, 0, 0, 0, 0, 0, 0}, n = i0;
        while (n < i1)
            for (int x = 0; x < 8; x++)
                if (pos[x] < q[x].size()) items[n++] = q[x][pos[x]++];
    };
    interleave(0, (size_t)job->n_items_b11);
    if (job->n_items_b21_early > 0) {
        interleave((size_t)job->n_items_b11, (size_t)(job->n_items_b11 + job->n_items_b21_early));
        interleave((size_t)(job->n_items_b11 + job->n_items_b21_early), items.size());
    } else interleave((size_t)job->n_items_b11, items.size());
    items.swap(this->items);
}
int JobBuild::order_items()
{
    item_keys();
    launch_classes();
    sort_items();
    if (streamed()) stream_groups();
    else xcd_interleave();
    return GAUSS_OK;
}
// The work items' block and every work list in the table image, behind the descriptors' tables
int JobBuild::place_lists()
{
    o_items = tab_block(job->d_items, sizeof(Item) * std::max<size_t>(items.size(), 1));
    job->n_items = (int)items.size();
    tab(job->d_rowmap, job->n_rows, rowmap);
    job->n_tiles_b11 = (int)tilemap.size();
    if (job->n_items_b21_early > 0) {
        std::stable_partition(tilemap_b21.begin(), tilemap_b21.end(), [&](const int2& a) { return !late_window[(size_t)a.x]; });
        for (const int2& t : tilemap_b21) job->n_tiles_b21_early += late_window[(size_t)t.x] ? 0 : 1;
    }
    tilemap.insert(tilemap.end(), tilemap_b21.begin(), tilemap_b21.end());
    tab(job->d_tilemap, job->n_tiles, tilemap);
    // the product's tiles with the longest K loop (highest k block) first
    std::stable_sort(gemmmap.begin(), gemmmap.end(), [](const int2& x, const int2& y) { return (x.y & 255) > (y.y & 255); });
    tab(job->d_panelmap, job->n_panels, panelmap); tab(job->d_dpanelmap, job->n_dpanels, dpanelmap);
    tab(job->tail.d_gemmmap, job->tail.n_gemm, gemmmap); tab(job->tail.d_finmap, job->tail.n_fin, finmap);
    tab(job->tail.d_loomap, job->tail.n_loo, loomap);
    const bool if_any = true;                              // (a job in which nobody asks takes nothing)
    tab(job->tail.d_slctmap, job->tail.n_slct, slctmap, if_any); tab(job->tail.d_condmap, job->tail.n_cond, condmap, if_any);
    tab(job->tail.d_csmap, job->tail.n_cs, csmap, if_any); tab(job->tail.d_prsmap, job->tail.n_prs, prsmap, if_any);
    tab(job->tail.d_susiemap, job->tail.n_susie, susiemap, if_any);
    tab(job->tail.d_xsmap, job->tail.n_xs, xsmap, if_any); tab(job->tail.d_xsleadmap, job->tail.n_xs_lead, xsleadmap, if_any);
    tab(job->tail.d_traitsmap, job->tail.n_traits, traitsmap, if_any); tab(job->tail.d_traitsumap, job->tail.n_traits_u, traitsumap, if_any);
    tab(job->tail.d_missmap, job->tail.n_miss_blk, missmap, if_any); tab(job->tail.d_misstmap, job->tail.n_miss_t, misstmap, if_any);
    tab(job->tail.d_missumap, job->tail.n_miss_u, missumap, if_any);
    tab(job->tail.d_ldsmap, job->tail.n_lds, ldsmap, if_any);
    o_probs = tab_block(job->d_probs, sizeof(Prob) * (size_t)n_prob());
    o_exports = tab_block(job->d_exports, sizeof(ExportD) * std::max<size_t>(job->exports.size(), 1));
    job->h_tab.resize(ta.off);
    return GAUSS_OK;
}
// ---- workspace arena ----
// One window's blocks.  A rider registers its blocks here, under the `if` that says it was asked: a field that is not
// registered stays null.
void JobBuild::layout_window(Plan& pl)
{
    Prob& p = pl.p;
    const Riders& rd = pl.rd;
    if (streamed()) {
        p.ld_raw = stream->ldraw; p.raw_m = stream->d_m; p.raw_u = stream->d_u;      // the rows land in the context's landing buffer
    } else if (!on_device) {
        // contiguous host matrices whose stride is close to the row length keep their stride on the device:
        // the upload is then ONE linear copy (a pitched copy of 3 000 rows runs at a fraction of that rate)
        const bool linear = pl.rows_m.empty() && pl.rows_u.empty() && (size_t)pl.user_ld <= pl.row_bytes + pl.row_bytes / 8 + 64;
        p.ld_raw = linear ? pl.user_ld : (long long)rup(pl.row_bytes, 16);
        ws(p.raw_m, (size_t)p.M * p.ld_raw + 64);
        ws(p.raw_u, (size_t)std::max(pl.U_user, 1) * p.ld_raw + 64);
    } else {
        p.ld_raw = pl.user_ld; p.raw_m = pl.h_geno_m; p.raw_u = pl.h_geno_u;
    }
    ws(p.packed, (size_t)p.Sp * p.Kp);
    ws(p.sx, (size_t)p.Sp * p.P * sizeof(int)); ws(p.sxx, (size_t)p.Sp * p.P * sizeof(int));
    slab(p.slab, (size_t)p.npair * p.nseg * TILE * TILE * (p.slab16 ? sizeof(uint16_t) : sizeof(float)));
    ws(p.rt_sd, (size_t)p.Sp * sizeof(double)); ws(p.rt_wm, (size_t)p.Sp * sizeof(double));
    ws(p.rt_mu, (size_t)p.Sp * p.P * sizeof(double)); ws(p.rt_wmu, (size_t)p.Sp * p.P * sizeof(double));
    if (!p.ld_only) {
        // the LD epilogue writes B11 (and its shifted twin) and B21 for every window that is not a plain
        // gauss_ld / gene batch; the factor and solve scratch only exists when there is something to solve
        ws(p.A, (size_t)(p.npanel > 0 ? 5 : 2) * p.Mld * p.Mld * sizeof(double));   // A0 A1 [L0 L1 W0]
        ws(p.B21, (size_t)std::max(p.U, 1) * p.Mld * sizeof(double));
    }
    if (p.npanel > 0) {
        ws(p.Linv, (size_t)2 * p.nblk * NB * NB * sizeof(double));
        ws(p.V, (size_t)std::max(p.npanel, p.npi) * p.Mld * NR * sizeof(double));
        ws(p.Gsum, (size_t)((p.Mld + 127) / 128) * p.Up128 * 3 * sizeof(double));
        ws(p.Part, (size_t)2 * p.npi * 4 * NB * NR * sizeof(double));      // double buffered by row parity
        ws(pl.d_b11_copy, (size_t)p.Mld * p.Mld * sizeof(double));
    }
    if (rd.slct_K) ws(p.slct_W, (size_t)SLCT_K * p.Mld * sizeof(double));      // the selected columns of the partial factor
    if (rd.cs) {                        // the candidates' log Bayes factors / pips per signal, and their membership bytes
        ws(p.cs_lbf, (size_t)rd.slct_K * cs_tld(p.M + p.U) * sizeof(double));
        ws(p.cs_mem, (size_t)rd.slct_K * cs_tld(p.M + p.U));
    }
    if (rd.susie_L) {                   // W, the fit's state and the sets' membership bytes
        ws(p.susie_ws, susie_ws(p.M, p.U, p.Mld, rd.susie_L, !p.susie_measured_only).total(rd.susie_k) * sizeof(double));
        ws(p.susie_mem, (size_t)(1 + rd.susie_k) * rd.susie_L * cs_tld(p.M + p.U));
    }
    if (rd.traits_T) {                  // Y = X Z and G = X^T Y of the further traits
        ws(p.traits_Y, (size_t)p.Mld * traits_t16(rd.traits_T) * sizeof(double));
        ws(p.traits_G, (size_t)p.Mld * traits_t16(rd.traits_T) * sizeof(double));
    }
    if (rd.miss && p.miss_nm) {         // the columns of X and of B11^-1 of the missing SNPs, B21 times them, every trait's L_D and c
        const size_t E16 = (size_t)traits_t16(p.miss_E);
        ws(p.miss_YE, (size_t)p.Mld * E16 * sizeof(double));
        ws(p.miss_AE, (size_t)p.Mld * E16 * sizeof(double));
        ws(p.miss_YU, E16 * (size_t)p.U * sizeof(double));
        ws(p.miss_LD, (size_t)p.miss_nm * MISS_LD * sizeof(double));
    }
    if (rd.lds)                         // every chunk's partial raw and mass, per category and target
        ws(p.lds_part, (size_t)(1 + rd.lds_C) * lds_chunks(p.M, p.U) * 2 * p.Mld * sizeof(double));
    ws(p.out_ld, std::max<size_t>(pl.out_ld_count, 1) * sizeof(double));
    pl.res_off = res;
    res += pl.res_count();
}
int JobBuild::layout_workspace()
{
    {
        // The early products of a row of the inverse (k_solve.hip, ride_pre) are a chain of dependent tile products:
        // rows with at least `solve_split` of them give one workgroup to each of their SOLVE_SPLIT classes, shorter rows
        // run the classes in one workgroup; 0 = never cut.  Either form sums in the same order.  Cutting from two
        // products on is what keeps every riding workgroup shorter than the diagonal tile's (36 windows, factorisation
        // with riding rows: never 1.72 ms, >= 8 1.70, >= 4 1.49, >= 2 1.46 before the pre / fin form, 1.31 with it; factorisation alone 1.10).
        // few windows: every launch of the factorisation is a latency-bound link of a chain -- drop the panel launches
        // (k_solve.hip, factor_update_kernel own_panel); same bits either way.  Factorisation + riding rows, with /
        // without panel launches: 5 windows 0.65 / 0.58 ms, 9 windows 0.82 / 0.78, 18 windows 0.87 / 0.84, 36 windows
        // 1.31 / 1.42 (the repeated panel products start to cost workgroup slots)
        int n_solve = 0;
        for (int i = 0; i < job->n; i++) n_solve += job->plans[i].p.npanel > 0 ? 1 : 0;
        job->own_panel = (n_solve > 0 && n_solve <= OWN_PANEL_MAX_WINDOWS) ? 1 : 0;
        job->solve_split = job->n_panels > 0 ? SOLVE_SPLIT_MIN : 0;
    }
    for (int i = 0; i < job->n; i++) layout_window(job->plans[i]);
    // job-wide measured rows (shared measured rows): one more tile of rows than Mp, because a window's last row tile
    // starts wherever the window starts and may reach past the chromosome's last measured SNP (zero rows there)
    if (shm()) {
        Prob& q = job->gplan->p;
        const size_t rows = (size_t)q.Mp + TILE;
        ws(q.packed, rows * q.Kp);
        ws(q.sx, rows * q.P * sizeof(int)); ws(q.sxx, rows * q.P * sizeof(int));
        ws(q.rt_sd, rows * sizeof(double)); ws(q.rt_wm, rows * sizeof(double));
        ws(q.rt_mu, rows * q.P * sizeof(double)); ws(q.rt_wmu, rows * q.P * sizeof(double));
        slab(q.slab, (size_t)q.npair * q.nseg * TILE * TILE * (q.slab16 ? sizeof(uint16_t) : sizeof(float)));
    }
    ws(job->d_status, sizeof(int) * (4 * job->n + 4));     // [n][4], then 4 job-wide ints ([4 n]: the chain queue timed out)
    ws(job->d_b11_done, 128);                                // counters of the merged Gram launch, a cache line each: [0] B11's items, [8] the early windows' B21 items (zeroed once; they only grow)
    ws(job->d_code3, 64, ctx->gram_pkf_geno != 0);         // stamp of the latest pack launch that met a code 3 (gauss_job::d_code3; zeroed once, only grows)
    ws(job->d_results, sizeof(double) * std::max<size_t>(res, 1));
    job->n_results = res;
    slab_base = rup(wa.off, 4096);
    job->ws_bytes = slab_base + wslab.off;
    job->tab_bytes = rup(job->h_tab.size(), 16);                               // (copied in 16-byte words: upload_tables)
    return GAUSS_OK;
}
// The three allocations, the result mirrors and the export chunks
int JobBuild::allocate()
{
    hipError_t e = ctx_dev_alloc(ctx, job->ws_bytes, (void**)&job->d_ws);
    if (e != hipSuccess) { job->d_ws = nullptr; return fail(GAUSS_E_NOMEM, "hipMalloc(%zu bytes workspace) failed: %s", wa.off, hipGetErrorString(e)); }
    e = ctx_dev_alloc(ctx, job->tab_bytes, (void**)&job->d_tab);
    if (e != hipSuccess) { job->d_tab = nullptr; return fail(GAUSS_E_NOMEM, "hipMalloc(%zu bytes tables) failed", job->h_tab.size()); }
    // one pinned block for the table image and the result mirrors: the table upload is then a true asynchronous
    // DMA and a job over resident rows is created without waiting for the stream (another job may be running on it)
    pin_tab = rup(job->tab_bytes, 256); pin_res = rup(sizeof(double) * std::max<size_t>(res, 1), 256);
    pin_st = rup(sizeof(int) * (4 * job->n + 4), 256);
    const size_t pin_exp = rup(sizeof(double) * exp_doubles, 256);
    e = ctx_pin_alloc(ctx, pin_tab + 2 * (pin_res + pin_st) + pin_exp, (void**)&job->h_pin);
    if (e != hipSuccess) { job->h_pin = nullptr; return fail(GAUSS_E_NOMEM, "hipHostMalloc(%zu bytes) failed", pin_tab + 2 * pin_res); }
    for (int k = 0; k < 2; k++) {
        job->h_res2[k] = (double*)(job->h_pin + pin_tab + k * (pin_res + pin_st));
        job->h_st2[k] = (int*)(job->h_pin + pin_tab + k * (pin_res + pin_st) + pin_res);
        HIPCHK(hipEventCreate(&job->done2[k]));
    }
    job->h_results = job->h_res2[0];
    job->h_status = job->h_st2[0];
    job->done = job->done2[0];
    if (!job->exports.empty()) {
        job->h_export = (double*)(job->h_pin + pin_tab + 2 * (pin_res + pin_st));
        // chunks of whole exports, >= 2 MB each (at most ~32): one kernel launch and one event per chunk
        const size_t per = std::max<size_t>((size_t)1 << 18, (exp_doubles + 31) / 32);       // doubles
        size_t acc = 0;
        int first = 0;
        const int nx = (int)job->exports.size();
        for (int x = 0; x < nx; x++) {
            acc += (size_t)job->exports[(size_t)x].rows * job->exports[(size_t)x].width;
            if (acc >= per || x + 1 == nx) { job->exp_chunks.push_back(std::make_pair(first, x + 1)); first = x + 1; acc = 0; }
        }
        job->exp_ev.assign(job->exp_chunks.size(), nullptr);
        for (hipEvent_t& ev : job->exp_ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    return GAUSS_OK;
}
int JobBuild::events_and_zeroing()
{
    HIPCHK(hipEventCreate(&job->begin));
    for (int k = 0; k < 2; k++)
        for (hipEvent_t* e : {&job->rev[k].gram, &job->rev[k].side, &job->rev[k].pack, &job->rev[k].rows, &job->rev[k].epi})
            HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));

    hipStream_t st = ctx->stream;
    // zero once: operand padding, B21 padding and the solve matrices rely on it.  On the (otherwise idle) upload queue, not on the
    // main queue: a pipeline creates the job of batch b + 1 while batch b computes, and 1-2 GB of zeroes at the head of the next
    // batch were a 0.3-0.4 ms gap between the batches of a chromosome (gauss_host_impute_chromosome: 36.4 ms of GPU span for
    // 35.0 ms of batches); beside the previous batch's Gram launch they cost nothing.  The main queue waits for the event IN ORDER,
    // i.e. behind whatever it is computing now.  While a background upload is using that queue the zeroes stay where they were.
    hipStream_t zs = st;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (ctx->upload && ctx->uploads.empty()) zs = ctx->upload;
    }
    job->queue_touched = true;                 // from here on job_release must let the queues drain before the blocks go back
    job->zero_queue = zs;
    HIPCHK(hipMemsetAsync(job->d_ws, 0, slab_base, zs));
    if (zs != st) {
        HIPCHK(hipEventCreateWithFlags(&job->zeroed, hipEventDisableTiming));
        HIPCHK(hipEventRecord(job->zeroed, zs));
        HIPCHK(hipStreamWaitEvent(st, job->zeroed, 0));
    }
    if (streamed()) {
        job->sevp.resize(job->sgroups.size(), nullptr);
        for (hipEvent_t& e : job->sevp) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    return GAUSS_OK;
}
// Every recorded pointer, then what is derived from them, then the descriptors into the table image
int JobBuild::bind()
{
    relocate();
    std::vector<char>& blob = job->h_tab;
    if (shm()) {
        // descriptor n: the job-wide measured rows (pack_stats / row_stats work on it; nothing else is launched for it)
        Plan& g = *job->gplan;
        Prob& q = g.p;
        q.ld_raw = g.user_ld;
        q.raw_m = g.h_geno_m; q.raw_u = nullptr;
        q.packed_u = q.packed; q.sx_u = q.sx; q.sxx_u = q.sxx;
        q.rt_sd_u = q.rt_sd; q.rt_wm_u = q.rt_wm; q.rt_mu_u = q.rt_mu; q.rt_wmu_u = q.rt_wmu;
        q.slab_g = q.slab; q.gpair_ti = q.pair_ti; q.gpair_tj = q.pair_tj; q.g0 = 0; q.n_gpair = q.npair;
        q.status = job->d_status;      // never written for this descriptor
        memcpy(blob.data() + o_probs + sizeof(Prob) * (size_t)job->n, &q, sizeof(Prob));
    }
    for (int i = 0; i < job->n; i++) {
        Plan& pl = job->plans[i];
        Prob& p = pl.p;
        const ResLayout lay = pl.layout();
        double* const out = job->d_results + pl.res_off;
        p.out_z = out + lay.z; p.out_info = out + lay.info;
        p.out_loo = pl.rd.loo ? out + lay.loo : nullptr;
        p.out_slct = pl.rd.slct_K ? out + lay.slct : nullptr;
        p.out_cond = pl.rd.cond ? out + lay.cond : nullptr;
        p.out_cs = pl.rd.cs ? out + lay.cs : nullptr;
        p.out_susie = pl.rd.susie_L && !pl.rd.xs_peer() ? out + lay.susie : nullptr;
        p.out_susie_more = pl.rd.susie_L && lay.xs > lay.susie_more ? out + lay.susie_more : nullptr;
        p.out_xs = lay.prs > lay.xs ? out + lay.xs : nullptr;
        p.out_prs = pl.rd.prs_n_s ? out + lay.prs : nullptr;
        p.out_lds = pl.rd.lds ? out + lay.lds : nullptr;
        p.out_traits = pl.rd.traits_T ? out + lay.traits : nullptr;
        p.out_traits_info = pl.rd.miss ? out + lay.traits_info : nullptr; p.out_traits_miss = pl.rd.miss ? out + lay.traits_miss : nullptr;
        p.status = job->d_status + 4 * i;
        // the unmeasured part of every row array follows the measured part ...
        p.packed_u = p.packed + (size_t)p.Mp * p.Kp;
        p.sx_u = p.sx + (size_t)p.Mp * p.P; p.sxx_u = p.sxx + (size_t)p.Mp * p.P;
        p.rt_sd_u = p.rt_sd + p.Mp; p.rt_wm_u = p.rt_wm + p.Mp;
        p.rt_mu_u = p.rt_mu + (size_t)p.Mp * p.P; p.rt_wmu_u = p.rt_wmu + (size_t)p.Mp * p.P;
        p.g0 = 0; p.n_gpair = 0; p.gpair_ti = p.pair_ti; p.gpair_tj = p.pair_tj; p.slab_g = p.slab;
        if (shm()) {
            // ... unless the measured rows are the job-wide ones: this window's run starts at g0
            const Prob& q = job->gplan->p;
            const size_t g0 = (size_t)job->g0[(size_t)i];
            p.g0 = (int)g0; p.n_gpair = q.npair;
            p.packed = q.packed + g0 * q.Kp;
            p.sx = q.sx + g0 * q.P; p.sxx = q.sxx + g0 * q.P;
            p.rt_sd = q.rt_sd + g0; p.rt_wm = q.rt_wm + g0;
            p.rt_mu = q.rt_mu + g0 * q.P; p.rt_wmu = q.rt_wmu + g0 * q.P;
            p.gpair_ti = q.pair_ti; p.gpair_tj = q.pair_tj;
            p.slab_g = q.slab;
        }
        memcpy(blob.data() + o_probs + sizeof(Prob) * i, &p, sizeof(Prob));
    }
    return GAUSS_OK;
}
// Rows of a host matrix into a window's raw block: one copy, or the listed store rows gathered first
int JobBuild::upload_rows(const Plan& pl, const uint8_t* dst_rows, const uint8_t* src, const std::vector<int32_t>& rows, int nrows)
{
    void* const dst = (void*)dst_rows;
    const long long ldraw = pl.p.ld_raw;
    hipStream_t st = ctx->stream;
    if (nrows <= 0) return GAUSS_OK;
    if (rows.empty()) {
        if (ldraw == pl.user_ld)      // same stride: one linear copy (the last row stops at its data)
            HIPCHK(hipMemcpyAsync(dst, src, (size_t)(nrows - 1) * pl.user_ld + pl.row_bytes,
                                  hipMemcpyHostToDevice, st));
        else
            HIPCHK(hipMemcpy2DAsync(dst, (size_t)ldraw, src, (size_t)pl.user_ld, pl.row_bytes,
                                    (size_t)nrows, hipMemcpyHostToDevice, st));
        return GAUSS_OK;
    }
    stage.emplace_back((size_t)nrows * ldraw);               // gather the listed store rows
    std::vector<uint8_t>& buf = stage.back();
    for (int r = 0; r < nrows; r++)
        memcpy(buf.data() + (size_t)r * ldraw, src + (size_t)rows[r] * pl.user_ld, pl.row_bytes);
    HIPCHK(hipMemcpyAsync(dst, buf.data(), buf.size(), hipMemcpyHostToDevice, st));
    return GAUSS_OK;
}
int JobBuild::upload_host_rows()
{
    if (on_device || streamed()) return GAUSS_OK;
    for (const Plan& pl : job->plans) {
        int rc = upload_rows(pl, pl.p.raw_m, pl.h_geno_m, pl.rows_m, pl.p.M);
        if (!rc) rc = upload_rows(pl, pl.p.raw_u, pl.h_geno_u, pl.rows_u, pl.U_user);
        if (rc) return rc;
    }
    return GAUSS_OK;
}
// device work items: every pointer is resolved here so the kernel starts loading operands at once
int JobBuild::write_items()
{
    for (size_t n = 0; n < items.size(); n++) {
        const ItemH& h = items[n];
        const Plan& pl = plan_of(h.prob);
        const Prob& p = pl.p;
        const std::pair<int, int>& gr = h.group >= 0 ? pl.groups[h.group] : pl.fine[(size_t)(-1 - h.group)];
        const int ti = pl.pair_ti[h.pair], tj = pl.pair_tj[h.pair];
        const int mt = p.Mp / TILE;
        // a row tile of the measured part (for a window that shares its measured rows: inside the job-wide array, from
        // wherever the window starts) or of the unmeasured part
        auto tile_rows = [&](int t) { return t < mt ? p.packed + (size_t)t * TILE * p.Kp : p.packed_u + (size_t)(t - mt) * TILE * p.Kp; };
        Item it;
        it.a = tile_rows(ti);
        it.b = tile_rows(tj);
        it.slab = p.slab + ((size_t)h.pair * p.nseg + gr.first) * (p.slab16 ? TILE * TILE / 2 : TILE * TILE);
        it.seg_k1 = p.seg_k1 + gr.first;
        it.chunk_live = chunk_live[(size_t)h.prob];
        it.Kp = p.Kp; it.k0 = pl.seg_k0[gr.first]; it.nseg = gr.second - gr.first;
        it.rows_a = live_rows(pl, ti); it.rows_b = live_rows(pl, tj); it.flags = (ti == tj ? 1 : 0) | (p.slab16 ? 2 : 0) | (p.slab16 && job->gram_packed ? 4 : 0);
        if (job->gram_narrow) it.flags |= tile_layout(it.rows_a, it.rows_b, (it.flags & 4) != 0) << LAYOUT_SHIFT;
        if (job->merged && (int)n < job->n_items_b11) it.flags |= 16;         // counts itself off in b11_done[0]
        else if (job->merged && (int)n < job->n_items_b11 + job->n_items_b21_early) it.flags |= 32;      // ... in b11_done[8] (the early windows' B21 items)
        memcpy(job->h_tab.data() + o_items + sizeof(Item) * n, &it, sizeof(Item));
    }
    return GAUSS_OK;
}
// GAUSS_PLAN_FILL=1: how unequal the four waves of the job's items are.  Per item, the waves' MFMA issue per K step as shares of
// a full wave's (k_gram_common.h: wave_load); the waves meet at a barrier every chunk, so an item runs at the pace of its
// fullest wave.  Printed per class (B11's items, B21's), in K samples x full waves: the issue of the fullest wave (`max`: the
// item's time while its fullest wave has its SIMD's matrix pipe to itself), the mean of the four (`mean`: its time if every
// SIMD of the CU saw an equal share), for the quadrant roles and for the layouts this job's items carry.
int JobBuild::fill_report()
{
    if (!(env_int("GAUSS_PLAN_FILL", 0) != 0 && !job->gram_i8)) return GAUSS_OK;
    double mx[2][2] = {{0, 0}, {0, 0}}, mean[2][2] = {{0, 0}, {0, 0}}, full[2] = {0, 0};
    long n_narrow[2] = {0, 0}, n_uneven[2] = {0, 0}, n_cls[2] = {0, 0};
    for (const ItemH& h : items) {
        const Plan& pl = plan_of(h.prob);
        const int ti = pl.pair_ti[h.pair], tj = pl.pair_tj[h.pair];
        const int ra = live_rows(pl, ti), rb = live_rows(pl, tj), c = h.b11 ? 0 : 1;
        const bool packed = job->gram_packed && pl.p.slab16;
        n_cls[c]++;
        full[c] += h.len;
        for (int f = 0; f < 2; f++) {
            const int layout = (f && job->gram_narrow) ? tile_layout(ra, rb, packed) : LAYOUT_QUAD;
            double m = 0, s = 0;
            for (int w = 0; w < 4; w++) {
                const double l = wave_load(wave_work(ra, rb, ti == tj, packed, true, w, layout), packed);
                m = std::max(m, l); s += l;
            }
            mx[f][c] += h.len * m; mean[f][c] += h.len * s / 4;
            if (f && layout != LAYOUT_QUAD) n_narrow[c]++;
            if (!f && m * 4 > s + 1e-9) n_uneven[c]++;
        }
    }
    for (int c = 0; c < 2; c++) {
        if (!n_cls[c]) continue;
        fprintf(stderr, "[fill] %s: %ld items (%ld with unequal waves, %ld narrow), K x tiles %.4e; quadrant roles: max %.4e mean %.4e mean/max %.4f; "
                        "this job's layouts: max %.4e mean %.4e mean/max %.4f\n", c ? "B21" : "B11", n_cls[c], n_uneven[c], n_narrow[c], full[c],
                mx[0][c], mean[0][c], mean[0][c] / mx[0][c], mx[1][c], mean[1][c], mean[1][c] / mx[1][c]);
    }
    return GAUSS_OK;
}
int JobBuild::export_descriptors()
{
    for (size_t x = 0; x < job->exports.size(); x++) {
        const gauss_job::Export& ex = job->exports[x];
        const Plan& pl = job->plans[(size_t)ex.plan];
        ExportD d;
        d.src = ex.which ? pl.p.B21 : (pl.p.kind == GAUSS_WIN_LD ? pl.p.A : pl.d_b11_copy);
        d.dst = job->h_export + ex.off;
        d.rows = ex.rows; d.width = ex.width; d.pitch = ex.pitch; d.pad_ = 0;
        memcpy(job->h_tab.data() + o_exports + sizeof(ExportD) * x, &d, sizeof(ExportD));
    }
    return GAUSS_OK;
}
int JobBuild::upload_tables()
{
    memcpy(job->h_pin, job->h_tab.data(), job->h_tab.size());
    // The table image crosses PCIe by kernel, not by hipMemcpyAsync: while a background upload keeps the DMA engines busy
    // (gauss_store_upload_async: a chromosome's first call) the runtime made the CALLER wait for an engine -- one job creation in
    // five stalled for 11-16 ms on these few MB (GAUSS_JOB_TRACE=1, round 4), the GPU idle meanwhile.
    launch_h2d_copy(job->d_tab, job->h_pin, job->tab_bytes, ctx->stream);
    HIPCHK(hipGetLastError());
    return GAUSS_OK;
}
// streamed: one window on contiguous host matrices whose upload is left to job_run_streamed (chunk by chunk on the
// copy stream, overlapped with the pack / Gram launches of the rows that have landed)
int job_build(gauss_ctx* ctx, const std::vector<WinSpec>& specs, int on_device, gauss_job** out, const StreamSetup* stream)
{
    typedef std::chrono::steady_clock clk;
    const auto tb0 = clk::now();
    gauss_job* job = new gauss_job();
    // every early return below (bad arguments, a failed HIP call) releases the job and what it owns
    std::unique_ptr<gauss_job, void (*)(gauss_job*)> guard(job, job_free);
    JobBuild b{ctx, specs, on_device, stream, job};
    int rc;
    if ((rc = b.plan_windows()) || (rc = b.plan_exports())) return rc;
    const auto tb1 = clk::now();
    if ((rc = b.share_measured()) || (rc = b.check_row_lists())) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    job->h_tab.reserve((size_t)b.n_prob() * ((size_t)320 << 10) + ((size_t)64 << 10));      // (~0.3 MB a window: grown in place, not copied over and over)
    const auto tb2 = clk::now();
    if ((rc = b.place_all_tables()) || (rc = b.work_lists()) || (rc = b.order_items()) || (rc = b.place_lists()) || (rc = b.layout_workspace())) return rc;
    const bool job_trace = trace_on("job");
    const auto tj0 = clk::now();
    if ((rc = b.allocate())) return rc;
    const auto tj1 = clk::now();
    if ((rc = b.events_and_zeroing()) || (rc = b.bind()) || (rc = b.upload_host_rows()) || (rc = b.write_items()) || (rc = b.fill_report()) ||
        (rc = b.export_descriptors())) return rc;
    const auto tj2 = clk::now();
    if ((rc = b.upload_tables())) return rc;
    if (job_trace) {
        auto ms = [](clk::time_point t0, clk::time_point t1) { return std::chrono::duration<double, std::milli>(t1 - t0).count(); };
        fprintf(stderr, "[job] %d windows: plan %.2f ms (the windows' plans %.2f, shared rows + row checks %.2f, tables + work items %.2f), allocations %.2f ms (workspace %.1f MB, tables %.2f MB, pinned %.2f MB), events + zeroing + tables %.2f ms, table copy queued in %.2f ms\n",
                job->n, ms(tb0, tj0), ms(tb0, tb1), ms(tb1, tb2), ms(tb2, tj0), ms(tj0, tj1), job->ws_bytes / 1e6, job->tab_bytes / 1e6, (b.pin_tab + 2 * (b.pin_res + b.pin_st)) / 1e6, ms(tj1, tj2),
                ms(tj2, clk::now()));
    }
    if (!on_device && !stream) HIPCHK(hipStreamSynchronize(ctx->stream));   // uploads from pageable user memory are complete
    std::vector<char>().swap(job->h_tab);
    { std::lock_guard<std::mutex> lock(ctx->mu); ctx->jobs.insert(job); }
    *out = guard.release();
    return GAUSS_OK;
}
