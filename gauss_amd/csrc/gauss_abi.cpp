// libgauss_hip.so -- the C ABI of include/gauss_hip.h: jobs, the blocking window call, the LD entry points.
#include "gauss_job.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

// the kernels' constants that include/gauss_hip.h states to the caller (gauss_internal.h does not see that header)
static_assert(gauss::HESS_M_MAX == GAUSS_HESS_MAX_M && gauss::HESS_TRAITS_MAX == GAUSS_HESS_MAX_TRAITS && gauss::HESS_K_MAX == GAUSS_HESS_MAX_K,
              "hess: gauss_internal.h and include/gauss_hip.h disagree");
static_assert(gauss::LDSPLIT_M_MAX == GAUSS_LDSPLIT_MAX_M && gauss::LDSPLIT_SIZE_MAX == GAUSS_LDSPLIT_MAX_SIZE && gauss::LDSPLIT_K_MAX == GAUSS_LDSPLIT_MAX_K,
              "LD splitting: gauss_internal.h and include/gauss_hip.h disagree");
static_assert(gauss::CLUMP_M_MAX == GAUSS_CLUMP_MAX_M && gauss::CLUMP_KEYS_MAX == GAUSS_CLUMP_MAX_KEYS, "clumping: gauss_internal.h and include/gauss_hip.h disagree");
static_assert(gauss::SC2_N_MAX == GAUSS_SUMCHI2_MAX_N && gauss::SC2_K_MAX == GAUSS_SUMCHI2_MAX_KEPT && gauss::SC2_TRAITS_MAX == GAUSS_SUMCHI2_MAX_TRAITS,
              "sum of chi2: gauss_internal.h and include/gauss_hip.h disagree");
static_assert(gauss::LDS_C == GAUSS_LDS_MAX_ANNOT && gauss::LDS_CHUNK == GAUSS_LDS_CHUNK, "LD scores: gauss_internal.h and include/gauss_hip.h disagree");

// entry points that need the job's context
#define JOB_ALIVE(job)                                                                                          \
    do {                                                                                                        \
        if (!(job)) return fail(GAUSS_E_INVALID, "job is NULL");                                                \
        if (!(job)->ctx) return fail(GAUSS_E_INVALID, "the job's context has been destroyed (gauss_hip_destroy)"); \
    } while (0)

static WinSpec spec_from_desc(const gauss_window_desc& d)
{
    WinSpec w;
    w.mode = d.mode; w.n_pop = d.n_pop; w.pop_off = d.pop_off; w.pop_wgt = d.pop_wgt;
    w.M = d.n_measured; w.U = d.n_unmeasured; w.geno_m = d.geno_m; w.geno_u = d.geno_u; w.ld = d.ld;
    w.z1 = d.z1; w.lambda = d.lambda; w.eps = d.min_abs_eig; w.diag = 1.0; w.ld_only = 0;
    w.gene_off = nullptr; w.n_gene = 0;
    w.kind = d.kind; w.n_head = d.n_head_measured; w.n_predm = d.n_pred_measured; w.eig_cutoff = d.eig_cutoff;
    w.u_codings = d.u_codings;
    w.geno_fmt = d.geno_format; w.rows_m = d.rows_m; w.rows_u = d.rows_u; w.pop_src_off = d.pop_src_off;
    w.out_b11 = d.out_b11; w.out_b21 = d.out_b21;
    w.out.loo_z = d.out_loo_z; w.out.loo_info = d.out_loo_info; w.out.loo_t = d.out_loo_t;
    w.n_traits_more = d.n_traits_more; w.z_more = d.z_more; w.out.z_more = d.out_z_more;
    w.miss_more = d.miss_more; w.out.info_more = d.out_info_more; w.out.z_miss = d.out_z_miss; w.out.info_miss = d.out_info_miss;
    w.slct_max = d.slct_max; w.slct_chi2_stop = d.slct_chi2_stop; w.slct_min_var_frac = d.slct_min_var_frac;
    w.slct_forced = d.slct_forced; w.n_slct_forced = d.n_slct_forced;
    w.out.slct_n = d.out_slct_n; w.out.slct_idx = d.out_slct_idx; w.out.slct_zin = d.out_slct_zin;
    w.out.slct_joint = d.out_slct_joint; w.out.slct_zc = d.out_slct_zc; w.out.slct_var = d.out_slct_var;
    w.cond_min_var_frac = d.cond_min_var_frac; w.out.cond_z = d.out_cond_z; w.out.cond_var = d.out_cond_var;
    w.cs_coverage = d.cs_coverage; w.cs_prior_var = d.cs_prior_var;
    w.out.cs_pip = d.out_cs_pip; w.out.cs_set = d.out_cs_set; w.out.cs_set_pip = d.out_cs_set_pip;
    w.out.cs_size = d.out_cs_size; w.out.cs_mass = d.out_cs_mass; w.out.cs_lse = d.out_cs_lse;
    w.susie_L = d.susie_L; w.susie_coverage = d.susie_coverage; w.susie_prior_var = d.susie_prior_var; w.susie_tol = d.susie_tol;
    w.susie_max_sweeps = d.susie_max_sweeps; w.susie_min_abs_corr = d.susie_min_abs_corr;
    w.susie_estimate_var = d.susie_estimate_var; w.susie_measured_only = d.susie_measured_only;
    w.out.susie_pip = d.out_susie_pip; w.out.susie_set = d.out_susie_set; w.out.susie_set_pip = d.out_susie_set_pip;
    w.out.susie_V = d.out_susie_V; w.out.susie_lse = d.out_susie_lse; w.out.susie_mass = d.out_susie_mass; w.out.susie_purity = d.out_susie_purity;
    w.out.susie_size = d.out_susie_size; w.out.susie_kept = d.out_susie_kept;
    w.out.susie_alpha = d.out_susie_alpha; w.out.susie_mu = d.out_susie_mu; w.out.susie_sweeps = d.out_susie_sweeps;
    w.susie_traits_more = d.coloc_traits_more; w.coloc_p1 = d.coloc_p1; w.coloc_p2 = d.coloc_p2; w.coloc_p12 = d.coloc_p12;
    w.out.susie_lbf = d.out_coloc_lbf;
    w.out.more_pip = d.out_coloc_more_pip; w.out.more_set = d.out_coloc_more_set; w.out.more_set_pip = d.out_coloc_more_set_pip;
    w.out.more_V = d.out_coloc_more_V; w.out.more_lse = d.out_coloc_more_lse; w.out.more_mass = d.out_coloc_more_mass;
    w.out.more_purity = d.out_coloc_more_purity; w.out.more_size = d.out_coloc_more_size; w.out.more_kept = d.out_coloc_more_kept;
    w.out.more_alpha = d.out_coloc_more_alpha; w.out.more_mu = d.out_coloc_more_mu; w.out.more_lbf = d.out_coloc_more_lbf;
    w.out.more_sweeps = d.out_coloc_more_sweeps; w.out.more_status = d.out_coloc_more_status;
    w.out.coloc_pp = d.out_coloc_pp; w.out.coloc_hit = d.out_coloc_hit; w.out.coloc_hit_pp = d.out_coloc_hit_pp; w.out.coloc_n = d.out_coloc_n;
    w.xs_group = d.xs_group; w.xs_from_lead = d.xs_from_lead;
    w.prs_n_s = d.prs_n_s; w.prs_n_lam = d.prs_n_lam; w.prs_s = d.prs_s; w.prs_lam = d.prs_lam; w.prs_n = d.prs_n; w.prs_tol = d.prs_tol;
    w.prs_max_sweeps = d.prs_max_sweeps;
    w.out.prs_beta = d.out_prs_beta; w.out.prs_nnz = d.out_prs_nnz; w.out.prs_sweeps = d.out_prs_sweeps; w.out.prs_delta = d.out_prs_delta;
    w.out.prs_br = d.out_prs_br; w.out.prs_bg = d.out_prs_bg; w.out.prs_kkt = d.out_prs_kkt;
    w.lds_on = d.lds_on; w.lds_n_annot = d.lds_n_annot; w.lds_radius = d.lds_radius; w.lds_bp_m = d.lds_bp_m; w.lds_bp_u = d.lds_bp_u;
    w.lds_n = d.lds_n; w.lds_annot = d.lds_annot;
    w.out.lds_raw = d.out_lds_raw; w.out.lds_l2 = d.out_lds_l2; w.out.lds_mass = d.out_lds_mass;
    w.out.xs_V = d.out_xs_V; w.out.xs_purity = d.out_xs_purity; w.out.xs_mu = d.out_xs_mu; w.out.xs_n = d.out_xs_n;
    return w;
}
extern "C" {

int gauss_job_create(gauss_ctx* ctx, const gauss_window_desc* wins, int n_win, int on_device, gauss_job** out_job)
{
    if (!ctx || !wins || n_win < 1 || !out_job) return fail(GAUSS_E_INVALID, "bad arguments to gauss_job_create");
    std::vector<WinSpec> specs;
    for (int i = 0; i < n_win; i++) {
        if (wins[i].n_unmeasured < 1 && wins[i].kind != GAUSS_WIN_LD &&
            !(wins[i].kind == GAUSS_WIN_QCAT && wins[i].n_pred_measured > 0))
            return fail(GAUSS_E_INVALID, "window %d has no unmeasured SNPs", i);
        specs.push_back(spec_from_desc(wins[i]));
    }
    gauss_job* job = nullptr;
    int rc = job_build(ctx, specs, on_device, &job);
    if (rc) return rc;
    for (int i = 0; i < n_win; i++) {
        Plan& pl = job->plans[i];
        pl.out_z = wins[i].out_z; pl.out_info = wins[i].out_info; pl.out_status = wins[i].out_status;
        pl.out_b11 = wins[i].out_b11; pl.out_b21 = wins[i].out_b21;
        pl.out_r = wins[i].out_r; pl.out_num_eig = wins[i].out_num_eig;
    }
    *out_job = job;
    return GAUSS_OK;
}

int gauss_job_run(gauss_job* job) { JOB_ALIVE(job); return job_run(job, true); }
int gauss_job_fetch(gauss_job* job) { JOB_ALIVE(job); return job_fetch(job); }
void gauss_job_destroy(gauss_job* job) { job_free(job); }

int gauss_job_span_ms(gauss_job* first, gauss_job* last, double* out_ms)
{
    JOB_ALIVE(first); JOB_ALIVE(last);
    if (!out_ms || !first->ran || !last->ran) return fail(GAUSS_E_INVALID, "gauss_job_span_ms: both jobs must have run");
    HIPCHK(hipEventSynchronize(last->done));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, first->begin, last->done));
    *out_ms = (double)ms;
    return GAUSS_OK;
}

int gauss_job_profile(gauss_job* job, int enable)
{
    JOB_ALIVE(job);
    if (job->prof && !enable) prof_collect(job);
    job->prof = enable != 0;
    if (enable) { for (int k = 0; k < 5; k++) { job->prof_ms[k] = 0; job->prof_n[k] = 0; } }
    return GAUSS_OK;
}

int gauss_job_profile_get(gauss_job* job, int kernel, double* out_ms, int64_t* out_launches)
{
    JOB_ALIVE(job);
    if (kernel < 0 || kernel > 4) return fail(GAUSS_E_INVALID, "bad arguments");
    hipStreamSynchronize(job->ctx->stream);
    prof_collect(job);
    if (out_ms) *out_ms = job->prof_ms[kernel];
    if (out_launches) *out_launches = job->prof_n[kernel];
    return GAUSS_OK;
}

int gauss_job_work(gauss_job* job, double* out_ld_flops, double* out_solve_flops, double* out_bytes, int64_t* out_imputed)
{
    if (!job) return fail(GAUSS_E_INVALID, "job is NULL");
    double ldf = 0, sf = 0, by = 0;
    int64_t imp = 0;
    for (const Plan& pl : job->plans) {
        const double M = pl.p.M, U = pl.p.U, N = pl.p.N;
        ldf += N * M * (M + 1) + 2.0 * N * U * M;            // symmetric half of B11 + B21
        sf += M * M * M / 3.0 + 2.0 * U * M * M + 4.0 * U * M;
        by += (M + U) * N + (M * M + U * M) * 8.0;
        imp += pl.p.U;
    }
    if (out_ld_flops) *out_ld_flops = ldf;
    if (out_solve_flops) *out_solve_flops = sf;
    if (out_bytes) *out_bytes = by;
    if (out_imputed) *out_imputed = imp;
    return GAUSS_OK;
}

int gauss_job_counters(gauss_job* job, int64_t* out4)
{
    if (!job || !out4) return fail(GAUSS_E_INVALID, "bad arguments to gauss_job_counters");
    out4[0] = job->n_merged; out4[1] = job->n_demoted; out4[2] = job->n_giveups; out4[3] = job->n_rerun_failed;
    return GAUSS_OK;
}

int gauss_job_stats(gauss_job* job, double* out4)
{
    if (!job || !out4) return fail(GAUSS_E_INVALID, "bad arguments");
    double flops = 0, slab = 0;
    const bool shm = job->gplan != nullptr;
    const bool edge16 = true;                  // (k_gram.hip: the 16-column edge routine is compiled in)
    auto add = [&](const Plan& pl, bool skip_b11) {
        const Prob& p = pl.p;
        const int mt = p.Mp / TILE;
        auto rows = [&](int t) {
            if (!pl.tile_live.empty()) return pl.tile_live[(size_t)t];
            int left = (t < mt) ? p.M - t * TILE : p.U - (t - mt) * TILE; return left > TILE ? TILE : left;
        };
        auto halves = [](int r, int w) { int n = (r - w * 64 + 31) / 32; return n < 0 ? 0 : (n > 2 ? 2 : n); };
        // samples per row the kernel multiplies: every zero-padded block (population, or 2-bit source block) rounded up to
        // the units the K loop can skip -- 8 samples on the f32 path (Item::chunk_live), 32 on the int8 path (whole groups);
        // the 16-column edge routine takes every chunk whole
        double k_main = 0;
        {
            const int gran = job->gram_i8 ? 32 : 8;
            const std::vector<int>& blk = (p.geno_fmt == GAUSS_GENO_2BIT && !pl.run_pk_off.empty()) ? pl.run_pk_off : pl.pop_pk_off;
            const bool runs = &blk == &pl.run_pk_off;
            for (size_t q = 0; q + 1 < blk.size(); q++) {
                // live samples of the block: its real size where known (populations), else its padded size
                int live = blk[q + 1] - blk[q];
                if (!runs && q + 1 < pl.pop_raw_off.size()) live = pl.pop_raw_off[q + 1] - pl.pop_raw_off[q];
                else if (runs && pl.run_len_known(q)) live = pl.run_len[q];
                k_main += (double)((live + gran - 1) / gran * gran);
            }
        }
        // packed items (k_gram.hip: two A rows per lane): a wave with any live A half issues one MFMA per live B half (or B group of 16)
        const bool packed = job->gram_packed && p.slab16;
        int pairs = 0;
        for (int pr = 0; pr < p.npair; pr++) {
            const int ti = pl.pair_ti[pr], tj = pl.pair_tj[pr];
            if (skip_b11 && ti < mt) continue;               // multiplied once, on the job-wide tiles
            pairs++;
            double tiles32 = 0, tiles_edge = 0;
            for (int wr = 0; wr < 2; wr++)
                for (int wc = 0; wc < 2; wc++) {
                    if (ti == tj && wr == 1 && wc == 0) continue;
                    int na = halves(rows(ti), wr);
                    if (packed && na > 1) na = 1;
                    // f32 path: a wave whose last live 32-column half holds at most 16 live columns multiplies 16-column groups
                    // (k_gram.hip, chunk_mfma_edge): 1 or 3 of them
                    int nb16 = (rows(tj) - wc * 64 + 15) / 16;
                    nb16 = nb16 < 0 ? 0 : (nb16 > 4 ? 4 : nb16);
                    if (edge16 && !job->gram_i8 && na > 0 && (nb16 & 1)) { tiles_edge += na * nb16 * 0.5; continue; }
                    double t32 = na * halves(rows(tj), wc);
                    if (ti == tj && wr == wc && t32 == 4) t32 = 3;      // mirrored 32 x 32 sub-block of a diagonal quadrant (not skipped when packed: t32 = 2)
                    tiles32 += t32;
                }
            flops += 32.0 * 32.0 * 2.0 * (tiles32 * k_main + tiles_edge * p.Kp);
        }
        slab += (double)pairs * p.nseg * TILE * TILE * (p.slab16 ? sizeof(uint16_t) : sizeof(float));
    };
    for (const Plan& pl : job->plans) add(pl, shm);
    if (shm) add(*job->gplan, false);
    out4[0] = job->n_items; out4[1] = flops; out4[2] = slab; out4[3] = (double)job->ws_bytes;
    return GAUSS_OK;
}

int gauss_impute_window(gauss_ctx* ctx, const gauss_window_desc* win)
{
    if (!ctx || !win) return fail(GAUSS_E_INVALID, "bad arguments to gauss_impute_window");
    if (win->xs_group != 0)
        return fail(GAUSS_E_INVALID, "xs_group = %d: a group of the joint fit across studies is two or more windows of one job (gauss_job_create)", win->xs_group);
    // Streamed form (default): upload and compute overlap (job_run_streamed).  It covers the windows the drivers make --
    // contiguous host matrices, additive coding, something to solve; the clamp path re-reads the job's buffers and works
    // on either form.  GAUSS_STREAM_WINDOW=0 (or GAUSS_FUSED_SOLVE=0): upload everything, then run.
    const bool fused = env_int("GAUSS_FUSED_SOLVE", 1) != 0;           // read per run: the tests drive both forms
    bool streamed = env_int("GAUSS_STREAM_WINDOW", 1) != 0 && fused && !win->rows_m && !win->rows_u && win->n_unmeasured >= 1 &&
                    win->n_measured >= 1 && win->kind != GAUSS_WIN_LD && (win->u_codings & ~GAUSS_CODE_ADDITIVE) == 0 &&
                    win->geno_m && win->geno_u && win->pop_off && win->n_pop >= 1 && win->n_pop <= 64;
    // bytes of a source row (what plan_problem will find; anything odd is left to the unstreamed path and its messages)
    size_t row_bytes = 0;
    if (streamed) {
        const int N = win->pop_off[win->n_pop];
        if (win->geno_format == GAUSS_GENO_U8) {
            streamed = N >= 1 && win->ld >= N;
            row_bytes = (size_t)std::max(N, 0);
        } else if (win->geno_format == GAUSS_GENO_2BIT && win->ld % 16 == 0) {
            long long end = 0;
            for (int q = 0; q < win->n_pop && streamed; q++) {
                const long long blk = (long long)rup((size_t)std::max(win->pop_off[q + 1] - win->pop_off[q], 0), 64) / 4;
                const long long off = win->pop_src_off ? win->pop_src_off[q] : end;
                if (off < 0 || off % 16 || off + blk > win->ld) streamed = false;
                if (!win->pop_src_off) end = off + blk;
                row_bytes = std::max(row_bytes, (size_t)(off + blk));
            }
        } else streamed = false;
    }
    gauss_job* job = nullptr;
    int rc;
    const bool trace = trace_on("stream");
    const auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (trace) fprintf(stderr, "[stream] %s at %.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    };
    if (streamed) {
        std::lock_guard<std::mutex> one(ctx->stream_mu);
        HIPCHK(hipSetDevice(ctx->device));
        StreamSetup su;
        rc = stream_start_copies(ctx, *win, row_bytes, su);
        if (rc) return rc;
        // On every path out of here the worker has finished its task (`su` lives on this stack) AND the copies it queued
        // have left the caller's matrices: from pinned memory they are true asynchronous DMAs, and the caller may free
        // the matrices the moment this call returns.  A successful fetch has waited for them already (`landed`).
        struct Waiter {
            gauss_ctx* c; bool landed = false;
            ~Waiter() { c->worker->wait(); if (!landed) (void)hipStreamSynchronize(c->copy); }
        } waiter{ctx};
        lap("copies started");
        std::vector<WinSpec> specs{spec_from_desc(*win)};
        rc = job_build(ctx, specs, 0, &job, &su);
        lap("job built");
        if (rc) return rc;
        Plan& pl = job->plans[0];
        pl.out_z = win->out_z; pl.out_info = win->out_info; pl.out_status = win->out_status;
        pl.out_b11 = win->out_b11; pl.out_b21 = win->out_b21; pl.out_r = win->out_r; pl.out_num_eig = win->out_num_eig;
        rc = job_run_streamed(job, su);
        lap("run queued");
        if (!rc) rc = job_fetch(job);
        lap("fetched");
        if (!rc) waiter.landed = true;             // the results were computed from every chunk: all copies are complete
        else {
            // nothing may still be writing into the landing buffer or reading it when the next call reuses it
            ctx->worker->wait();
            for (hipStream_t q : {ctx->copy, ctx->aux, ctx->chain, ctx->stream}) (void)hipStreamSynchronize(q);
        }
        job_free(job);
        lap("freed");
        return rc;
    }
    rc = gauss_job_create(ctx, win, 1, 0, &job);
    if (rc) return rc;
    rc = job_run(job, true);
    if (!rc) rc = job_fetch(job);
    job_free(job);
    return rc;
}

// The window of an LD-only call: M rows of one matrix or store, no unmeasured SNPs, no z.  Whatever else a call sets (row lists, gene
// blocks, a pair list, draws) it sets on the WinSpec it gets back; job_build copies what it keeps.
static WinSpec ld_spec(int mode, const uint8_t* geno, int n_snp, int64_t ld, const int32_t* pop_off, const double* pop_wgt, int n_pop, double diag)
{
    WinSpec w;
    w.mode = mode; w.n_pop = n_pop; w.pop_off = pop_off; w.pop_wgt = pop_wgt;
    w.M = n_snp; w.U = 0; w.geno_m = geno; w.geno_u = nullptr; w.ld = ld; w.z1 = nullptr;
    w.lambda = 0; w.eps = 0; w.diag = diag; w.ld_only = 1; w.gene_off = nullptr; w.n_gene = 0;
    return w;
}
// ... whose rows are named by index in a row store (host or device memory), 2-bit or bytes
static WinSpec ld_spec_rows(int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows, int n_snp, const int32_t* pop_off,
                            const int32_t* pop_src_off, const double* pop_wgt, int n_pop, double diag)
{
    WinSpec w = ld_spec(mode, store, n_snp, ld, pop_off, pop_wgt, n_pop, diag);
    w.geno_fmt = geno_format; w.rows_m = rows; w.pop_src_off = pop_src_off;
    return w;
}

typedef std::unique_ptr<gauss_job, void (*)(gauss_job*)> JobGuard;
static int ld_job(gauss_ctx* ctx, const WinSpec& w, int on_device, JobGuard& guard)
{
    gauss_job* job = nullptr;
    std::vector<WinSpec> specs{w};
    const int rc = job_build(ctx, specs, on_device, &job);
    if (rc == 0) guard.reset(job);
    return rc;
}

// the LD matrix (or the gene blocks) of w into `out`; out_counts (gauss_gram_counts): the Gram as exact integer counts instead
static int ld_common(gauss_ctx* ctx, const WinSpec& w, int on_device, double* out, int64_t* out_counts = nullptr)
{
    if (!ctx || !w.geno_m || (!out && !out_counts)) return fail(GAUSS_E_INVALID, "bad arguments");
    JobGuard job(nullptr, job_free);
    int rc = ld_job(ctx, w, on_device, job);
    if (rc) return rc;
    if (!out_counts) job->plans[0].out_ld_user = out;
    rc = job_run(job.get(), false);
    if (rc) return rc;
    if (out_counts) {
        DevBuf d_cnt;
        const size_t bytes = sizeof(long long) * (size_t)w.M * w.M;
        if (d_cnt.alloc(ctx, bytes) != hipSuccess) return fail(GAUSS_E_NOMEM, "hipMalloc(%zu bytes of counts) failed", bytes);
        launch_counts(job->d_probs, 0, job->plans[0].p.npair, d_cnt.as<long long>(), ctx->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipMemcpy(out_counts, d_cnt.p, bytes, hipMemcpyDeviceToHost));
    }
    return job_fetch(job.get());
}

int gauss_gram_counts(gauss_ctx* ctx, const uint8_t* geno, int n_snp, int n_samples, int64_t ld, int64_t* out_counts)
{
    if (!out_counts) return fail(GAUSS_E_INVALID, "out_counts is NULL");
    const int32_t off1[2] = {0, n_samples};                 // pooled over one population of n_samples
    return ld_common(ctx, ld_spec(GAUSS_MODE_POOLED, geno, n_snp, ld, off1, nullptr, 1, 1.0), 0, nullptr, out_counts);
}

int gauss_ld(gauss_ctx* ctx, int mode, const uint8_t* geno, int n_snp, int64_t ld, const int32_t* pop_off,
             const double* pop_wgt, int n_pop, double diag, double* out_cor)
{
    return ld_common(ctx, ld_spec(mode, geno, n_snp, ld, pop_off, pop_wgt, n_pop, diag), 0, out_cor);
}

int gauss_gene_ld_batch(gauss_ctx* ctx, int mode, const uint8_t* geno, int n_snp, int64_t ld,
                        const int32_t* pop_off, const double* pop_wgt, int n_pop,
                        const int32_t* gene_off, int n_gene, double diag, double* out_blocks)
{
    if (!gene_off || n_gene < 1) return fail(GAUSS_E_INVALID, "gene_off is NULL or n_gene < 1");
    WinSpec w = ld_spec(mode, geno, n_snp, ld, pop_off, pop_wgt, n_pop, diag);
    w.gene_off = gene_off; w.n_gene = n_gene;
    return ld_common(ctx, w, 0, out_blocks);
}

int gauss_ld_rows(gauss_ctx* ctx, int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows, int n_snp,
                  const int32_t* pop_off, const int32_t* pop_src_off, const double* pop_wgt, int n_pop, double diag,
                  int on_device, double* out_cor)
{
    return ld_common(ctx, ld_spec_rows(mode, store, ld, geno_format, rows, n_snp, pop_off, pop_src_off, pop_wgt, n_pop, diag), on_device, out_cor);
}

int gauss_ld_clump_rows(gauss_ctx* ctx, int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows, int n_snp,
                        const int32_t* pop_off, const int32_t* pop_src_off, const double* pop_wgt, int n_pop, int on_device,
                        const int32_t* bp, const double* key, int n_key, int64_t radius, double r2_min, double key_index, double key_member,
                        int32_t* out_owner, int32_t* out_rank, double* out_r2, int32_t* out_n_clumps)
{
    if (!ctx || !store) return fail(GAUSS_E_INVALID, "bad arguments to gauss_ld_clump_rows");
    if (!bp) return fail(GAUSS_E_INVALID, "gauss_ld_clump_rows: bp is NULL");
    if (!key) return fail(GAUSS_E_INVALID, "gauss_ld_clump_rows: key is NULL");
    if (!out_owner) return fail(GAUSS_E_INVALID, "gauss_ld_clump_rows: out_owner is NULL");
    if (n_key < 1 || n_key > CLUMP_KEYS_MAX)
        return fail(GAUSS_E_INVALID, "gauss_ld_clump_rows: n_key = %d; a call clumps 1 .. %d traits", n_key, CLUMP_KEYS_MAX);
    if (n_snp < 1 || n_snp > CLUMP_M_MAX)
        return fail(GAUSS_E_INVALID, "gauss_ld_clump_rows: n_snp = %d; a region holds 1 .. %d SNPs", n_snp, CLUMP_M_MAX);
    for (int i = 1; i < n_snp; i++)
        if (bp[i] < bp[i - 1]) return fail(GAUSS_E_INVALID, "gauss_ld_clump_rows: bp decreases at row %d (%d after %d)", i, bp[i], bp[i - 1]);
    if (radius < 0) return fail(GAUSS_E_INVALID, "gauss_ld_clump_rows: radius = %lld is negative", (long long)radius);
    if (!(r2_min >= 0.0 && r2_min <= 1.0)) return fail(GAUSS_E_INVALID, "gauss_ld_clump_rows: r2_min = %g is outside [0, 1]", r2_min);
    if (!std::isfinite(key_index) || !std::isfinite(key_member))
        return fail(GAUSS_E_INVALID, "gauss_ld_clump_rows: key_index = %g, key_member = %g; both thresholds must be finite", key_index, key_member);
    if (key_member > key_index)
        return fail(GAUSS_E_INVALID, "gauss_ld_clump_rows: key_member = %g is above key_index = %g", key_member, key_index);
    JobGuard job(nullptr, job_free);
    int rc = ld_job(ctx, ld_spec_rows(mode, store, ld, geno_format, rows, n_snp, pop_off, pop_src_off, pop_wgt, n_pop, 1.0), on_device, job);
    if (rc) return rc;
    rc = job_run(job.get(), false);
    if (rc) return rc;
    // the matrix stays where the epilogue wrote it (out_ld, both triangles); the kernel runs behind the job on the same stream
    hipStream_t st = ctx->stream;
    const size_t M = (size_t)n_snp, TM = (size_t)n_key * M;
    DevBuf d_bp, d_key, d_owner, d_rank, d_r2, d_n;
    if (d_bp.alloc(ctx, sizeof(int) * M) != hipSuccess || d_key.alloc(ctx, sizeof(double) * TM) != hipSuccess ||
        d_owner.alloc(ctx, sizeof(int) * TM) != hipSuccess || d_rank.alloc(ctx, sizeof(int) * TM) != hipSuccess ||
        d_r2.alloc(ctx, sizeof(double) * TM) != hipSuccess || d_n.alloc(ctx, sizeof(int) * (size_t)n_key) != hipSuccess)
        return fail(GAUSS_E_NOMEM, "hipMalloc(%zu bytes of keys and clumps) failed", (sizeof(double) * 2 + sizeof(int) * 2) * TM);
    HIPCHK(hipMemcpyAsync(d_bp.p, bp, sizeof(int) * M, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_key.p, key, sizeof(double) * TM, hipMemcpyHostToDevice, st));
    ClumpArgs a;
    a.R = job->plans[0].p.out_ld; a.bp = d_bp.as<int>(); a.key = d_key.as<double>();
    a.owner = d_owner.as<int>(); a.rank = d_rank.as<int>(); a.r2 = d_r2.as<double>(); a.n_clumps = d_n.as<int>();
    a.radius = (long long)std::min<int64_t>(radius, (int64_t)1 << 32);      // positions are 32-bit: 2^32 is every band already, and bp +- radius stays in range
    a.r2_min = r2_min; a.key_index = key_index; a.key_member = key_member; a.M = n_snp;
    launch_clump(a, n_key, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_owner, d_owner.p, sizeof(int) * TM, hipMemcpyDeviceToHost, st));
    if (out_rank) HIPCHK(hipMemcpyAsync(out_rank, d_rank.p, sizeof(int) * TM, hipMemcpyDeviceToHost, st));
    if (out_r2) HIPCHK(hipMemcpyAsync(out_r2, d_r2.p, sizeof(double) * TM, hipMemcpyDeviceToHost, st));
    if (out_n_clumps) HIPCHK(hipMemcpyAsync(out_n_clumps, d_n.p, sizeof(int) * (size_t)n_key, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return job_fetch(job.get());
}

int gauss_ld_split_rows(gauss_ctx* ctx, int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows, int n_snp,
                        const int32_t* pop_off, const int32_t* pop_src_off, const double* pop_wgt, int n_pop, int on_device,
                        const int32_t* bp, int64_t radius, double thr_r2, int min_size, int max_size, int max_K, double max_r2,
                        double* out_cost, int32_t* out_prev, double* out_max_r2, int64_t* out_n_nonfinite)
{
    if (!ctx || !store) return fail(GAUSS_E_INVALID, "bad arguments to gauss_ld_split_rows");
    if (!bp) return fail(GAUSS_E_INVALID, "gauss_ld_split_rows: bp is NULL");
    if (!out_cost) return fail(GAUSS_E_INVALID, "gauss_ld_split_rows: out_cost is NULL");
    if (n_snp < 1 || n_snp > LDSPLIT_M_MAX)
        return fail(GAUSS_E_INVALID, "gauss_ld_split_rows: n_snp = %d; a region holds 1 .. %d SNPs", n_snp, LDSPLIT_M_MAX);
    if (max_size < 1 || max_size > LDSPLIT_SIZE_MAX)
        return fail(GAUSS_E_INVALID, "gauss_ld_split_rows: max_size = %d; a block holds 1 .. %d SNPs", max_size, LDSPLIT_SIZE_MAX);
    if (min_size < 1 || min_size > max_size)
        return fail(GAUSS_E_INVALID, "gauss_ld_split_rows: min_size = %d is outside 1 .. max_size = %d", min_size, max_size);
    if (max_K < 1 || max_K > LDSPLIT_K_MAX)
        return fail(GAUSS_E_INVALID, "gauss_ld_split_rows: max_K = %d; a call splits into 1 .. %d blocks", max_K, LDSPLIT_K_MAX);
    for (int i = 1; i < n_snp; i++)
        if (bp[i] < bp[i - 1]) return fail(GAUSS_E_INVALID, "gauss_ld_split_rows: bp decreases at row %d (%d after %d)", i, bp[i], bp[i - 1]);
    if (radius < 0) return fail(GAUSS_E_INVALID, "gauss_ld_split_rows: radius = %lld is negative", (long long)radius);
    if (!(thr_r2 >= 0.0 && thr_r2 <= 1.0)) return fail(GAUSS_E_INVALID, "gauss_ld_split_rows: thr_r2 = %g is outside [0, 1]", thr_r2);
    if (!(max_r2 >= 0.0 && max_r2 <= 1.0)) return fail(GAUSS_E_INVALID, "gauss_ld_split_rows: max_r2 = %g is outside [0, 1]", max_r2);
    JobGuard job(nullptr, job_free);
    int rc = ld_job(ctx, ld_spec_rows(mode, store, ld, geno_format, rows, n_snp, pop_off, pop_src_off, pop_wgt, n_pop, 1.0), on_device, job);
    if (rc) return rc;
    rc = job_run(job.get(), false);
    if (rc) return rc;
    // the matrix stays where the epilogue wrote it (out_ld, both triangles); the kernels run behind the job on the same stream
    hipStream_t st = ctx->stream;
    const size_t M = (size_t)n_snp, Mp = M + 1, W = std::min((size_t)max_size, M), K = (size_t)max_K;
    DevBuf d_bp, d_sd, d_smd, d_tk, d_c, d_cfin, d_mx, d_prev, d_n;
    if (d_bp.alloc(ctx, sizeof(int) * M) != hipSuccess || d_sd.alloc(ctx, sizeof(double) * W * M) != hipSuccess ||
        d_smd.alloc(ctx, sizeof(double) * W * M) != hipSuccess || d_tk.alloc(ctx, sizeof(double) * W * Mp) != hipSuccess ||
        d_c.alloc(ctx, sizeof(double) * 2 * Mp) != hipSuccess || d_cfin.alloc(ctx, sizeof(double) * K) != hipSuccess ||
        d_mx.alloc(ctx, sizeof(double) * Mp) != hipSuccess || d_prev.alloc(ctx, sizeof(int) * K * Mp) != hipSuccess ||
        d_n.alloc(ctx, sizeof(unsigned long long)) != hipSuccess)
        return fail(GAUSS_E_NOMEM, "hipMalloc(%zu bytes of suffix sums, block costs and boundaries) failed",
                    sizeof(double) * (2 * W * M + W * Mp + 3 * Mp + K) + sizeof(int) * (K * Mp + M));
    HIPCHK(hipMemcpyAsync(d_bp.p, bp, sizeof(int) * M, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_n.p, 0, sizeof(unsigned long long), st));
    LdSplitArgs a;
    a.R = job->plans[0].p.out_ld; a.bp = d_bp.as<int>();
    a.Sd = d_sd.as<double>(); a.SMd = d_smd.as<double>(); a.Tk = d_tk.as<double>();
    a.C0 = d_c.as<double>(); a.C1 = d_c.as<double>() + Mp; a.cfin = d_cfin.as<double>(); a.mx = d_mx.as<double>();
    a.prev = d_prev.as<int>(); a.n_nonfinite = d_n.as<unsigned long long>();
    a.radius = (long long)std::min<int64_t>(radius, (int64_t)1 << 32);      // positions are 32-bit: 2^32 is every band already
    a.thr_r2 = thr_r2; a.max_r2 = max_r2;
    a.M = n_snp; a.W = (int)W; a.min_size = min_size; a.max_size = max_size; a.max_K = max_K;
    launch_ldsplit(a, st);
    HIPCHK(hipGetLastError());
    unsigned long long n_bad = 0;
    HIPCHK(hipMemcpyAsync(out_cost, d_cfin.p, sizeof(double) * K, hipMemcpyDeviceToHost, st));
    if (out_prev) HIPCHK(hipMemcpyAsync(out_prev, d_prev.p, sizeof(int) * K * Mp, hipMemcpyDeviceToHost, st));
    if (out_max_r2) HIPCHK(hipMemcpyAsync(out_max_r2, d_mx.p, sizeof(double) * Mp, hipMemcpyDeviceToHost, st));
    if (out_n_nonfinite) HIPCHK(hipMemcpyAsync(&n_bad, d_n.p, sizeof(n_bad), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out_n_nonfinite) *out_n_nonfinite = (int64_t)n_bad;
    return job_fetch(job.get());
}

int gauss_ld_hess_rows(gauss_ctx* ctx, int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows, int n_snp,
                       const int32_t* pop_off, const int32_t* pop_src_off, const double* pop_wgt, int n_pop, int on_device,
                       const double* z, int n_trait, int k_max, double eig_min, double* out_lam, double* out_proj,
                       int32_t* out_n_pos, int32_t* out_sweeps, int64_t* out_n_nonfinite, int32_t* out_status,
                       double* out_vectors, int32_t* out_order)
{
    if (!ctx || !store) return fail(GAUSS_E_INVALID, "bad arguments to gauss_ld_hess_rows");
    if (!z) return fail(GAUSS_E_INVALID, "gauss_ld_hess_rows: z is NULL");
    if (!out_lam) return fail(GAUSS_E_INVALID, "gauss_ld_hess_rows: out_lam is NULL");
    if (!out_proj) return fail(GAUSS_E_INVALID, "gauss_ld_hess_rows: out_proj is NULL");
    if (n_snp < 1 || n_snp > HESS_M_MAX)
        return fail(GAUSS_E_INVALID, "gauss_ld_hess_rows: n_snp = %d; a block holds 1 .. %d SNPs", n_snp, HESS_M_MAX);
    if (n_trait < 1 || n_trait > HESS_TRAITS_MAX)
        return fail(GAUSS_E_INVALID, "gauss_ld_hess_rows: n_trait = %d; a call takes 1 .. %d traits", n_trait, HESS_TRAITS_MAX);
    if (k_max < 1 || k_max > HESS_K_MAX)
        return fail(GAUSS_E_INVALID, "gauss_ld_hess_rows: k_max = %d; a call projects on 1 .. %d eigenvectors", k_max, HESS_K_MAX);
    if (!(eig_min >= 0.0 && eig_min < 1.0)) return fail(GAUSS_E_INVALID, "gauss_ld_hess_rows: eig_min = %g is outside [0, 1)", eig_min);
    JobGuard job(nullptr, job_free);
    int rc = ld_job(ctx, ld_spec_rows(mode, store, ld, geno_format, rows, n_snp, pop_off, pop_src_off, pop_wgt, n_pop, 1.0), on_device, job);
    if (rc) return rc;
    rc = job_run(job.get(), false);
    if (rc) return rc;
    // the matrix stays where the epilogue wrote it (out_ld, both triangles); the kernels run behind the job on the same stream
    hipStream_t st = ctx->stream;
    const size_t M = (size_t)n_snp, T = (size_t)n_trait, K = (size_t)k_max;
    const size_t np = (M + HESS_PW - 1) / HESS_PW * HESS_PW, ldn = (M + HESS_RC - 1) / HESS_RC * HESS_RC;
    DevBuf d_g, d_v, d_z, d_zr, d_mono, d_lam, d_ord, d_ls, d_proj, d_cnt;
    if (d_g.alloc(ctx, sizeof(double) * np * ldn) != hipSuccess || d_v.alloc(ctx, sizeof(double) * np * ldn) != hipSuccess ||
        d_z.alloc(ctx, sizeof(double) * T * M) != hipSuccess || d_zr.alloc(ctx, sizeof(double) * T * ldn) != hipSuccess ||
        d_mono.alloc(ctx, sizeof(int) * M) != hipSuccess || d_lam.alloc(ctx, sizeof(double) * M) != hipSuccess ||
        d_ord.alloc(ctx, sizeof(int) * K) != hipSuccess || d_ls.alloc(ctx, sizeof(double) * K) != hipSuccess ||
        d_proj.alloc(ctx, sizeof(double) * T * K) != hipSuccess || d_cnt.alloc(ctx, 2 * sizeof(unsigned long long)) != hipSuccess)
        return fail(GAUSS_E_NOMEM, "hipMalloc(%zu bytes of G, V, z and projections) failed",
                    sizeof(double) * (2 * np * ldn + T * (M + ldn + K) + M + K) + sizeof(int) * (M + K));
    HIPCHK(hipMemcpyAsync(d_z.p, z, sizeof(double) * T * M, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_cnt.p, 0, 2 * sizeof(unsigned long long), st));
    HessArgs a;
    a.R = job->plans[0].p.out_ld; a.z = d_z.as<double>();
    a.Gm = d_g.as<double>(); a.V = d_v.as<double>(); a.zr = d_zr.as<double>(); a.mono = d_mono.as<int>();
    a.lam = d_lam.as<double>(); a.order = d_ord.as<int>(); a.lam_sorted = d_ls.as<double>(); a.proj = d_proj.as<double>();
    a.n_nonfinite = d_cnt.as<unsigned long long>(); a.n_rot = reinterpret_cast<unsigned int*>(d_cnt.as<unsigned long long>() + 1);
    a.M = n_snp; a.np = (int)np; a.ldn = (int)ldn; a.T = n_trait; a.kk = 0; a.k_max = k_max;
    a.null2 = ((double)n_snp * 0x1p-52) * ((double)n_snp * 0x1p-52);
    launch_hess_prep(a, st);
    HIPCHK(hipGetLastError());
    int sweeps = 0;
    bool converged = false;
    HIPCHK(hess_solve(a, st, &sweeps, &converged));
    launch_hess_lambda(a, st);
    HIPCHK(hipGetLastError());
    // the M eigenvalues back (a few KB), sorted here: descending, a tie to the smaller solver column
    std::vector<double> lam(M);
    unsigned long long n_bad = 0;
    HIPCHK(hipMemcpyAsync(lam.data(), d_lam.p, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&n_bad, d_cnt.p, sizeof(n_bad), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int> order(M);
    for (size_t i = 0; i < M; i++) order[i] = (int)i;
    bool finite = true;
    for (size_t i = 0; i < M; i++) finite = finite && std::isfinite(lam[i]);
    if (finite)       // (with a NaN among them the comparison is no ordering: the eigenvalues stay in solver order, n_pos = 0)
        std::sort(order.begin(), order.end(), [&](int x, int y) { return lam[x] > lam[y] || (lam[x] == lam[y] && x < y); });
    for (size_t i = 0; i < M; i++) out_lam[i] = lam[order[i]];
    int n_pos = 0;
    const double floor = eig_min * out_lam[0];
    for (size_t i = 0; i < M; i++) n_pos += (finite && out_lam[i] > 0.0 && out_lam[i] > floor) ? 1 : 0;      // (sorted: a prefix)
    const int kk = std::min(n_pos, k_max);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t e = 0; e < T * K; e++) out_proj[e] = nan;
    if (kk > 0) {
        a.kk = kk;
        HIPCHK(hipMemcpyAsync(d_ord.p, order.data(), sizeof(int) * kk, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_ls.p, out_lam, sizeof(double) * kk, hipMemcpyHostToDevice, st));
        launch_hess_proj(a, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy2DAsync(out_proj, sizeof(double) * K, d_proj.p, sizeof(double) * K, sizeof(double) * kk, T, hipMemcpyDeviceToHost, st));
    }
    if (out_vectors) {      // the tests' export: row i = the eigenvector of out_lam[i]
        std::vector<double> v(np * ldn);
        HIPCHK(hipMemcpyAsync(v.data(), d_v.p, sizeof(double) * np * ldn, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t i = 0; i < M; i++) std::memcpy(out_vectors + i * M, v.data() + (size_t)order[i] * ldn, sizeof(double) * M);
    }
    HIPCHK(hipStreamSynchronize(st));
    if (out_order) for (size_t i = 0; i < M; i++) out_order[i] = order[i];
    if (out_n_pos) *out_n_pos = n_pos;
    if (out_sweeps) *out_sweeps = sweeps;
    if (out_n_nonfinite) *out_n_nonfinite = (int64_t)n_bad;
    if (out_status) *out_status = (converged ? 0 : GAUSS_ST_HESS_NOCONV) | ((n_bad || !finite) ? GAUSS_ST_NONFINITE : 0);
    return job_fetch(job.get());
}

int gauss_ld_resampled_rows(gauss_ctx* ctx, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows, int n_snp,
                            const int32_t* pop_off, const int32_t* pop_src_off, int n_pop,
                            const int32_t* draw_pop, const int32_t* draw_sample, int64_t n_drawn, int64_t n_cols,
                            double diag, int on_device, double* out_cor)
{
    if (!ctx || !store || !pop_off || !out_cor) return fail(GAUSS_E_INVALID, "bad arguments to gauss_ld_resampled_rows");
    if (n_snp < 1) return fail(GAUSS_E_INVALID, "need at least one SNP row (got %d)", n_snp);
    if (n_cols < 1) return fail(GAUSS_E_INVALID, "n_cols must be >= 1 (got %lld)", (long long)n_cols);
    if (n_drawn < 0 || n_drawn > n_cols)
        return fail(GAUSS_E_INVALID, "n_drawn = %lld is outside 0..n_cols (%lld)", (long long)n_drawn, (long long)n_cols);
    if (n_drawn > 0 && (!draw_pop || !draw_sample)) return fail(GAUSS_E_INVALID, "draw_pop / draw_sample is NULL");
    if (n_drawn == 0) {
        // every column is a zero column: CalCor is 0/0 off the diagonal (no Gram work to launch)
        const size_t S = (size_t)n_snp;
        for (size_t i = 0; i < S; i++)
            for (size_t j = 0; j < S; j++) out_cor[i * S + j] = i == j ? diag : NAN;
        return GAUSS_OK;
    }
    WinSpec w = ld_spec_rows(GAUSS_MODE_POOLED, store, ld, geno_format, rows, n_snp, pop_off, pop_src_off, nullptr, n_pop, diag);
    w.draw_pop = draw_pop; w.draw_sample = draw_sample; w.n_drawn = n_drawn; w.n_cols = n_cols;
    return ld_common(ctx, w, on_device, out_cor);
}

int gauss_gene_ld_batch_rows(gauss_ctx* ctx, int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows,
                             int n_snp, const int32_t* pop_off, const int32_t* pop_src_off, const double* pop_wgt, int n_pop,
                             const int32_t* gene_off, int n_gene, double diag, int on_device, double* out_blocks)
{
    if (!gene_off || n_gene < 1) return fail(GAUSS_E_INVALID, "gene_off is NULL or n_gene < 1");
    WinSpec w = ld_spec_rows(mode, store, ld, geno_format, rows, n_snp, pop_off, pop_src_off, pop_wgt, n_pop, diag);
    w.gene_off = gene_off; w.n_gene = n_gene;
    return ld_common(ctx, w, on_device, out_blocks);
}

// gauss_gene_sumchi2[_rows]: the gene job of `w` (diag 1, gene blocks set by the caller), then sumchi2_kernel on its blocks
static int sumchi2_common(gauss_ctx* ctx, const char* who, WinSpec w, int on_device, const double* z, int n_trait, double prune_r2,
                          int32_t* out_kept, int32_t* out_n_kept, double* out_lam, double* out_q, int32_t* out_top,
                          int32_t* out_status, int32_t* out_sweeps)
{
    if (!ctx || !w.geno_m) return fail(GAUSS_E_INVALID, "bad arguments to %s", who);
    if (!w.gene_off || w.n_gene < 1) return fail(GAUSS_E_INVALID, "%s: gene_off is NULL or n_gene < 1", who);
    if (!z) return fail(GAUSS_E_INVALID, "%s: z is NULL", who);
    if (!out_kept) return fail(GAUSS_E_INVALID, "%s: out_kept is NULL", who);
    if (!out_n_kept) return fail(GAUSS_E_INVALID, "%s: out_n_kept is NULL", who);
    if (!out_lam) return fail(GAUSS_E_INVALID, "%s: out_lam is NULL", who);
    if (!out_q) return fail(GAUSS_E_INVALID, "%s: out_q is NULL", who);
    if (n_trait < 1 || n_trait > SC2_TRAITS_MAX)
        return fail(GAUSS_E_INVALID, "%s: n_trait = %d; a call tests 1 .. %d traits", who, n_trait, SC2_TRAITS_MAX);
    if (!(prune_r2 > 0.0 && prune_r2 <= 1.0)) return fail(GAUSS_E_INVALID, "%s: prune_r2 = %g is outside (0, 1]", who, prune_r2);
    int max_n = 0;
    for (int g = 0; g < w.n_gene; g++) {
        const long long n = (long long)w.gene_off[g + 1] - w.gene_off[g];
        if (n > SC2_N_MAX)
            return fail(GAUSS_E_INVALID, "%s: gene %d holds %lld SNPs; a gene holds at most %d before pruning", who, g, n, SC2_N_MAX);
        max_n = std::max(max_n, (int)std::max(n, 0ll));
    }
    JobGuard job(nullptr, job_free);
    int rc = ld_job(ctx, w, on_device, job);
    if (rc) return rc;
    rc = job_run(job.get(), false);
    if (rc) return rc;
    // the blocks stay where the gene epilogue wrote them (out_ld, both triangles); the kernel runs behind the job on the same stream
    hipStream_t st = ctx->stream;
    const size_t S = (size_t)w.M, NG = (size_t)w.n_gene, T = (size_t)n_trait;
    DevBuf d_z, d_kept, d_nk, d_lam, d_q, d_top, d_st, d_sw;
    if (d_z.alloc(ctx, sizeof(double) * T * S) != hipSuccess || d_kept.alloc(ctx, sizeof(int) * S) != hipSuccess ||
        d_nk.alloc(ctx, sizeof(int) * NG) != hipSuccess || d_lam.alloc(ctx, sizeof(double) * NG * SC2_K_MAX) != hipSuccess ||
        d_q.alloc(ctx, sizeof(double) * T * NG) != hipSuccess || d_top.alloc(ctx, sizeof(int) * T * NG) != hipSuccess ||
        d_st.alloc(ctx, sizeof(int) * NG) != hipSuccess || d_sw.alloc(ctx, sizeof(int) * NG) != hipSuccess)
        return fail(GAUSS_E_NOMEM, "hipMalloc(%zu bytes of Z-scores and eigenvalues) failed", sizeof(double) * (T * S + NG * SC2_K_MAX));
    HIPCHK(hipMemcpyAsync(d_z.p, z, sizeof(double) * T * S, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_kept.p, 0, sizeof(int) * S, st));           // a row outside every gene is not kept
    const Prob& p = job->plans[0].p;
    Sumchi2Args a;
    a.R = p.out_ld; a.gene_off = p.gene_off; a.gene_out_off = p.gene_out_off; a.z = d_z.as<double>();
    a.kept = d_kept.as<int>(); a.n_kept = d_nk.as<int>(); a.lam = d_lam.as<double>(); a.q = d_q.as<double>();
    a.top = d_top.as<int>(); a.status = d_st.as<int>(); a.sweeps = d_sw.as<int>();
    a.prune_r2 = prune_r2; a.n_snp = w.M; a.n_gene = w.n_gene; a.n_trait = n_trait; a.m_lds = 0;
    launch_sumchi2(a, max_n, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_kept, d_kept.p, sizeof(int) * S, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_n_kept, d_nk.p, sizeof(int) * NG, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_lam, d_lam.p, sizeof(double) * NG * SC2_K_MAX, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_q, d_q.p, sizeof(double) * T * NG, hipMemcpyDeviceToHost, st));
    if (out_top) HIPCHK(hipMemcpyAsync(out_top, d_top.p, sizeof(int) * T * NG, hipMemcpyDeviceToHost, st));
    if (out_status) HIPCHK(hipMemcpyAsync(out_status, d_st.p, sizeof(int) * NG, hipMemcpyDeviceToHost, st));
    if (out_sweeps) HIPCHK(hipMemcpyAsync(out_sweeps, d_sw.p, sizeof(int) * NG, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return job_fetch(job.get());
}

int gauss_gene_sumchi2(gauss_ctx* ctx, int mode, const uint8_t* geno, int n_snp, int64_t ld,
                       const int32_t* pop_off, const double* pop_wgt, int n_pop,
                       const int32_t* gene_off, int n_gene, const double* z, int n_trait, double prune_r2,
                       int32_t* out_kept, int32_t* out_n_kept, double* out_lam, double* out_q,
                       int32_t* out_top, int32_t* out_status, int32_t* out_sweeps)
{
    WinSpec w = ld_spec(mode, geno, n_snp, ld, pop_off, pop_wgt, n_pop, 1.0);
    w.gene_off = gene_off; w.n_gene = n_gene;
    return sumchi2_common(ctx, "gauss_gene_sumchi2", w, 0, z, n_trait, prune_r2, out_kept, out_n_kept, out_lam, out_q, out_top,
                          out_status, out_sweeps);
}

int gauss_gene_sumchi2_rows(gauss_ctx* ctx, int mode, const uint8_t* store, int64_t ld, int geno_format, const int32_t* rows,
                            int n_snp, const int32_t* pop_off, const int32_t* pop_src_off, const double* pop_wgt, int n_pop,
                            const int32_t* gene_off, int n_gene, int on_device, const double* z, int n_trait, double prune_r2,
                            int32_t* out_kept, int32_t* out_n_kept, double* out_lam, double* out_q,
                            int32_t* out_top, int32_t* out_status, int32_t* out_sweeps)
{
    WinSpec w = ld_spec_rows(mode, store, ld, geno_format, rows, n_snp, pop_off, pop_src_off, pop_wgt, n_pop, 1.0);
    w.gene_off = gene_off; w.n_gene = n_gene;
    return sumchi2_common(ctx, "gauss_gene_sumchi2_rows", w, on_device, z, n_trait, prune_r2, out_kept, out_n_kept, out_lam, out_q,
                          out_top, out_status, out_sweeps);
}

// The per-population calls (gauss_ld_per_pop, _pairs, gauss_zmix_normal_eq) run the WEIGHTED layout with every weight 1: it keeps
// one exact Gram partial per population, which is all they read.  `w` points into `ones`.
struct UnitWeightSpec {
    std::vector<double> ones;
    WinSpec w;
    UnitWeightSpec(const uint8_t* geno, int n_snp, int64_t ld, const int32_t* pop_off, int n_pop)
        : ones((size_t)std::max(n_pop, 1), 1.0), w(ld_spec(GAUSS_MODE_WEIGHTED, geno, n_snp, ld, pop_off, ones.data(), n_pop, 1.0)) {}
};

// pack + Gram only, for the jobs whose Gram partials another kernel reads: the LD epilogue has nothing to write for them
static int pack_and_gram(gauss_job* job, hipStream_t st)
{
    launch_pack_stats(job->d_probs, job->d_rowmap, job->n_rows, st);
    launch_gram(job->d_items, job->n_items, job->gram_i8, st);
    HIPCHK(hipGetLastError());
    return GAUSS_OK;
}

static int check_pop_group(const int32_t* pop_group, int n_pop, int n_group)
{
    if (pop_group)
        for (int p = 0; p < n_pop; p++)
            if (pop_group[p] < 0 || pop_group[p] >= n_group) return fail(GAUSS_E_INVALID, "pop_group[%d] = %d is outside 0..%d", p, pop_group[p], n_group - 1);
    return GAUSS_OK;
}

int gauss_ld_per_pop(gauss_ctx* ctx, const uint8_t* geno, int n_snp, int64_t ld, const int32_t* pop_off, int n_pop,
                     double* out)
{
    if (!ctx || !geno || !pop_off || !out) return fail(GAUSS_E_INVALID, "bad arguments to gauss_ld_per_pop");
    if (n_snp < 2) return fail(GAUSS_E_INVALID, "need at least two SNPs");
    const UnitWeightSpec u(geno, n_snp, ld, pop_off, n_pop);
    JobGuard job(nullptr, job_free);
    int rc = ld_job(ctx, u.w, 0, job);
    if (rc) return rc;
    rc = job_run(job.get(), false);
    if (rc) return rc;
    const size_t npairs = (size_t)n_snp * (n_snp - 1) / 2;
    const size_t bytes = sizeof(double) * npairs * (size_t)n_pop;
    DevBuf d_out;
    if (d_out.alloc(ctx, bytes) != hipSuccess) return fail(GAUSS_E_NOMEM, "hipMalloc(%zu bytes per-population LD) failed", bytes);
    launch_pop_cor(job->d_probs, 0, job->plans[0].p.npair, d_out.as<double>(), ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(out, d_out.p, bytes, hipMemcpyDeviceToHost));
    return GAUSS_OK;
}

int gauss_ld_per_pop_pairs(gauss_ctx* ctx, const uint8_t* geno, int n_snp, int64_t ld, const int32_t* pop_off, int n_pop,
                           const int32_t* pop_group, int n_group, const int32_t* pair_i, const int32_t* pair_j, int64_t n_pairs,
                           double* out)
{
    if (!ctx || !geno || !pop_off || !out || !pair_i || !pair_j) return fail(GAUSS_E_INVALID, "bad arguments to gauss_ld_per_pop_pairs");
    if (n_snp < 2 || n_pairs < 1) return fail(GAUSS_E_INVALID, "need at least two SNPs and one pair");
    if (!pop_group) n_group = n_pop;
    if (n_group < 1) return fail(GAUSS_E_INVALID, "n_group < 1");
    int rc = check_pop_group(pop_group, n_pop, n_group);
    if (rc) return rc;
    UnitWeightSpec u(geno, n_snp, ld, pop_off, n_pop);
    u.w.pair_i = pair_i; u.w.pair_j = pair_j; u.w.n_pairs = n_pairs;
    JobGuard job(nullptr, job_free);
    if ((rc = ld_job(ctx, u.w, 0, job)) != 0) return rc;
    hipStream_t st = ctx->stream;
    if ((rc = pack_and_gram(job.get(), st)) != 0) return rc;
    std::vector<int2> pairs((size_t)n_pairs);
    for (int64_t k = 0; k < n_pairs; k++) pairs[(size_t)k] = make_int2(pair_i[k], pair_j[k]);
    DevBuf d_pairs, d_grp, d_out;
    const size_t out_bytes = sizeof(double) * (size_t)n_pairs * (size_t)n_group;
    if (d_pairs.alloc(ctx, sizeof(int2) * pairs.size()) != hipSuccess || d_grp.alloc(ctx, sizeof(int) * (size_t)std::max(n_pop, 1)) != hipSuccess ||
        d_out.alloc(ctx, out_bytes) != hipSuccess)
        return fail(GAUSS_E_NOMEM, "hipMalloc(%zu bytes of pair correlations) failed", out_bytes);
    HIPCHK(hipMemcpyAsync(d_pairs.p, pairs.data(), sizeof(int2) * pairs.size(), hipMemcpyHostToDevice, st));
    if (pop_group) HIPCHK(hipMemcpyAsync(d_grp.p, pop_group, sizeof(int) * (size_t)n_pop, hipMemcpyHostToDevice, st));
    launch_pair_cor(job->d_probs, 0, d_pairs.as<int2>(), n_pairs, pop_group ? d_grp.as<int>() : nullptr, n_group, d_out.as<double>(), st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost));
    return GAUSS_OK;
}

int gauss_zmix_normal_eq(gauss_ctx* ctx, const uint8_t* geno, int n_snp, int64_t ld, const int32_t* pop_off, int n_pop,
                         const int32_t* pop_group, int n_group, const double* z, double* out_xtx, double* out_xty, double* out_yty,
                         int64_t* out_n_rows)
{
    if (!ctx || !geno || !pop_off || !z || !out_xtx || !out_xty || !out_yty || !out_n_rows)
        return fail(GAUSS_E_INVALID, "bad arguments to gauss_zmix_normal_eq");
    if (n_snp < 2) return fail(GAUSS_E_INVALID, "need at least two SNPs");
    if (n_pop < 1) return fail(GAUSS_E_INVALID, "n_pop < 1");
    if (!pop_group) n_group = n_pop;
    if (n_group < 1 || n_group > 64)
        return fail(GAUSS_E_INVALID, "gauss_zmix_normal_eq: %d groups; the normal equations hold 1 .. 64", n_group);
    int rc = check_pop_group(pop_group, n_pop, n_group);
    if (rc) return rc;
    UnitWeightSpec u(geno, n_snp, ld, pop_off, n_pop);
    u.w.gram_only = 1;                  // the correlations are formed and reduced in k_zmix.hip, never stored
    JobGuard job(nullptr, job_free);
    if ((rc = ld_job(ctx, u.w, 0, job)) != 0) return rc;
    hipStream_t st = ctx->stream;
    if ((rc = pack_and_gram(job.get(), st)) != 0) return rc;
    const int npair = job->plans[0].p.npair;
    const int ne = (n_group + 1) * (n_group + 2) / 2;
    DevBuf d_z, d_grp, d_part, d_part_n, d_out, d_out_n;
    const size_t part_bytes = sizeof(double) * (size_t)std::max(npair, 1) * ne;
    if (d_z.alloc(ctx, sizeof(double) * (size_t)n_snp) != hipSuccess || d_grp.alloc(ctx, sizeof(int) * (size_t)n_pop) != hipSuccess ||
        d_part.alloc(ctx, part_bytes) != hipSuccess || d_part_n.alloc(ctx, sizeof(long long) * (size_t)std::max(npair, 1)) != hipSuccess ||
        d_out.alloc(ctx, sizeof(double) * (size_t)ne) != hipSuccess || d_out_n.alloc(ctx, sizeof(long long)) != hipSuccess)
        return fail(GAUSS_E_NOMEM, "hipMalloc(%zu bytes of normal-equation partials) failed", part_bytes);
    HIPCHK(hipMemcpyAsync(d_z.p, z, sizeof(double) * (size_t)n_snp, hipMemcpyHostToDevice, st));
    if (pop_group) HIPCHK(hipMemcpyAsync(d_grp.p, pop_group, sizeof(int) * (size_t)n_pop, hipMemcpyHostToDevice, st));
    launch_zmix_normal_eq(job->d_probs, 0, npair, pop_group ? d_grp.as<int>() : nullptr, n_group, d_z.as<double>(), d_part.as<double>(),
                          d_part_n.as<long long>(), d_out.as<double>(), d_out_n.as<long long>(), st);
    HIPCHK(hipGetLastError());
    std::vector<double> tri((size_t)ne);
    long long nrows = 0;
    HIPCHK(hipMemcpyAsync(tri.data(), d_out.p, sizeof(double) * (size_t)ne, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&nrows, d_out_n.p, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // upper triangle of [y | X]^T [y | X] in row order: (0, 0) = y^T y, (0, b) = (X^T y)[b - 1], (a, b) = (X^T X)[a - 1][b - 1]
    const int nc = n_group + 1;
    size_t k = 0;
    for (int a = 0; a < nc; a++)
        for (int b = a; b < nc; b++, k++) {
            const double v = tri[k];
            if (a == 0) { if (b == 0) *out_yty = v; else out_xty[b - 1] = v; }
            else { out_xtx[(size_t)(a - 1) * n_group + (b - 1)] = v; out_xtx[(size_t)(b - 1) * n_group + (a - 1)] = v; }
        }
    *out_n_rows = (int64_t)nrows;
    return GAUSS_OK;
}

int gauss_pop_weights(gauss_ctx* ctx, const double* x, const int64_t* interval_off, int n_interval, int n_pop, double min_abs_eig,
                      double* out_w_interval, int32_t* out_status)
{
    if (!ctx || !interval_off || !out_w_interval || n_interval < 1) return fail(GAUSS_E_INVALID, "bad arguments to gauss_pop_weights");
    if (n_pop < 1 || n_pop > 64)
        return fail(GAUSS_E_INVALID, "gauss_pop_weights: n_pop = %d populations; the device eigen-solve holds 1 .. 64", n_pop);
    if (interval_off[0] != 0) return fail(GAUSS_E_INVALID, "gauss_pop_weights: interval_off[0] must be 0");
    for (int i = 0; i < n_interval; i++)
        if (interval_off[i + 1] < interval_off[i]) return fail(GAUSS_E_INVALID, "gauss_pop_weights: interval_off is not ascending at %d", i);
    const int64_t S = interval_off[n_interval];
    if (S > 0 && !x) return fail(GAUSS_E_INVALID, "gauss_pop_weights: x is NULL");
    const int nc = n_pop + 1, npair = nc * (nc + 1) / 2;
    // chunks of at most PW_CHUNK rows, each inside one interval: the split depends on the interval sizes alone
    constexpr int64_t PW_CHUNK = 512;
    std::vector<PwChunk> chunks;
    std::vector<int> chunk_off((size_t)n_interval + 1, 0);
    for (int i = 0; i < n_interval; i++) {
        for (int64_t r = interval_off[i]; r < interval_off[i + 1]; r += PW_CHUNK)
            chunks.push_back(PwChunk{(long long)r, (long long)std::min(r + PW_CHUNK, interval_off[i + 1]), i, 0});
        if (chunks.size() > (size_t)INT32_MAX / 4) return fail(GAUSS_E_INVALID, "gauss_pop_weights: too many rows");
        chunk_off[(size_t)i + 1] = (int)chunks.size();
    }
    const int n_chunk = (int)chunks.size();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf d_x, d_chunks, d_coff, d_off, d_part1, d_mean, d_part2, d_w, d_status;
    const size_t x_bytes = sizeof(double) * (size_t)S * nc;
    if (d_x.alloc(ctx, x_bytes) != hipSuccess || d_chunks.alloc(ctx, sizeof(PwChunk) * chunks.size()) != hipSuccess ||
        d_coff.alloc(ctx, sizeof(int) * chunk_off.size()) != hipSuccess || d_off.alloc(ctx, sizeof(int64_t) * ((size_t)n_interval + 1)) != hipSuccess ||
        d_part1.alloc(ctx, sizeof(double) * (size_t)n_chunk * nc) != hipSuccess || d_mean.alloc(ctx, sizeof(double) * (size_t)n_interval * nc) != hipSuccess ||
        d_part2.alloc(ctx, sizeof(double) * (size_t)n_chunk * npair) != hipSuccess ||
        d_w.alloc(ctx, sizeof(double) * (size_t)n_interval * n_pop) != hipSuccess || d_status.alloc(ctx, sizeof(int) * (size_t)n_interval) != hipSuccess)
        return fail(GAUSS_E_NOMEM, "hipMalloc(%zu bytes of allele frequencies and workspace) failed", x_bytes);
    if (x_bytes) HIPCHK(hipMemcpyAsync(d_x.p, x, x_bytes, hipMemcpyHostToDevice, st));
    if (n_chunk) HIPCHK(hipMemcpyAsync(d_chunks.p, chunks.data(), sizeof(PwChunk) * chunks.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_coff.p, chunk_off.data(), sizeof(int) * chunk_off.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_off.p, interval_off, sizeof(int64_t) * ((size_t)n_interval + 1), hipMemcpyHostToDevice, st));
    launch_pop_weights(d_x.as<double>(), n_pop, d_chunks.as<PwChunk>(), n_chunk, d_coff.as<int>(), d_off.as<long long>(), n_interval,
                       min_abs_eig, d_part1.as<double>(), d_mean.as<double>(), d_part2.as<double>(), d_w.as<double>(), d_status.as<int>(), st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_w_interval, d_w.p, sizeof(double) * (size_t)n_interval * n_pop, hipMemcpyDeviceToHost, st));
    std::vector<int> stat((size_t)n_interval);
    HIPCHK(hipMemcpyAsync(stat.data(), d_status.p, sizeof(int) * stat.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out_status) for (int i = 0; i < n_interval; i++) out_status[i] = stat[(size_t)i];
    return GAUSS_OK;
}

// The bench plumbing's kernels index a caller's device buffer by pop_off and a row stride: offsets that start below 0 or
// decrease, or a stride shorter than a row of pop_off[n_pop] samples, would put them outside it.
static int check_pop_off(const char* who, const int32_t* pop_off, int n_pop, const char* ld_name, int64_t ld)
{
    if (pop_off[0] < 0) return fail(GAUSS_E_INVALID, "%s: pop_off[0] = %d is negative", who, pop_off[0]);
    for (int q = 0; q < n_pop; q++)
        if (pop_off[q + 1] < pop_off[q])
            return fail(GAUSS_E_INVALID, "%s: pop_off is not ascending at %d (%d after %d)", who, q + 1, pop_off[q + 1], pop_off[q]);
    if (ld < pop_off[n_pop])
        return fail(GAUSS_E_INVALID, "%s: %s = %lld is shorter than a row of pop_off[n_pop] = %d samples", who, ld_name, (long long)ld,
                    pop_off[n_pop]);
    return GAUSS_OK;
}

int gauss_pack2bit_device(gauss_ctx* ctx, const uint8_t* d_in, int64_t ld_in, uint8_t* d_out, int64_t ld_out,
                          int n_snp, const int32_t* pop_off, int n_pop)
{
    if (!ctx || !d_in || !d_out || !pop_off || n_snp < 1 || n_pop < 1) return fail(GAUSS_E_INVALID, "bad arguments");
    if (int rc = check_pop_off("gauss_pack2bit_device", pop_off, n_pop, "ld_in", ld_in)) return rc;
    std::vector<int> blk(n_pop + 1, 0);
    for (int q = 0; q < n_pop; q++) blk[q + 1] = blk[q] + (int)rup((size_t)(pop_off[q + 1] - pop_off[q]), 64) / 4;
    if (ld_out % 16 || ld_out < blk[n_pop]) return fail(GAUSS_E_INVALID, "ld_out must be a multiple of 16 and >= %d", blk[n_pop]);
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf tab;
    HIPCHK(tab.alloc(sizeof(int) * 2 * (n_pop + 1)));
    int* d_tab = tab.as<int>();
    HIPCHK(hipMemcpy(d_tab, pop_off, sizeof(int) * (n_pop + 1), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_tab + n_pop + 1, blk.data(), sizeof(int) * (n_pop + 1), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(d_out, 0, (size_t)n_snp * ld_out, ctx->stream));
    launch_pack2bit(d_in, ld_in, d_out, ld_out, n_snp, d_tab, d_tab + n_pop + 1, n_pop, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GAUSS_OK;
}

int gauss_synth_device(gauss_ctx* ctx, uint8_t* d_out, int n_snp, int64_t ld, const int32_t* pop_off, int n_pop,
                       const float* thr, const float* rho, uint64_t seed)
{
    if (!ctx || !d_out || !pop_off || !thr || !rho || n_snp < 1 || n_pop < 1) return fail(GAUSS_E_INVALID, "bad arguments");
    if (int rc = check_pop_off("gauss_synth_device", pop_off, n_pop, "ld", ld)) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const int N = pop_off[n_pop];
    DevBuf b_off, b_thr, b_rho;
    HIPCHK(b_off.alloc(sizeof(int) * (n_pop + 1)));
    HIPCHK(b_thr.alloc(sizeof(float) * (size_t)n_snp * n_pop));
    HIPCHK(b_rho.alloc(sizeof(float) * n_snp));
    HIPCHK(hipMemcpy(b_off.p, pop_off, sizeof(int) * (n_pop + 1), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b_thr.p, thr, sizeof(float) * (size_t)n_snp * n_pop, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b_rho.p, rho, sizeof(float) * n_snp, hipMemcpyHostToDevice));
    launch_synth(d_out, n_snp, ld, b_off.as<int>(), n_pop, N, b_thr.as<float>(), b_rho.as<float>(), seed, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GAUSS_OK;
}

}  // extern "C"
