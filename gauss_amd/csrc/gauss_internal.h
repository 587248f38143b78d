// Internal declarations shared by the HIP translation units of libgauss_hip.so.
#pragma once
#ifndef GAUSS_LAYOUTS_ONLY      // defined: the result block's layouts alone, for a host program without HIP (gauss_deliver.h)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <atomic>
#include <mutex>

namespace gauss {
#ifndef GAUSS_LAYOUTS_ONLY

constexpr int TILE = 128;      // Gram output tile edge per workgroup (4 waves x 64x64)
constexpr int KC = 64;         // packed K chunk in bytes (= samples); pops are padded to it
// chunk_unit_layout: inside every 32-sample group of a packed row the eight dwords (4 samples each) are stored transposed --
// sample dword d = 2 q + h sits at position 4 h + q -- so that the two lane halves of the 32 x 32 x 2 MFMA (half h reads bytes
// 16 h .. 16 h + 15 of the group) meet samples 8 q .. 8 q + 7 of the group in their dword q: a population whose last chunk
// holds r live samples needs only the first ceil(r / 8) dword steps of it (Item::chunk_live).  Sums over k do not depend on
// the order, every row is stored the same way, and nothing but the Gram kernels reads packed rows.
constexpr int SEG_MAX = 2048;  // K segment cap for small jobs (< 4 windows); larger jobs use 4096 (seg_max_for); any cap up to 8192
                               // keeps a partial sum below 2^24 (15 * 15 * 8192), the exactness bound of the f32 accumulators
constexpr int NB = 64;         // fp64 factor / solve block edge
constexpr int NR = 64;         // right-hand sides per solve panel (63 SNPs + the z1 column); the solve kernel is
                               // written for any multiple of 64 -- 128 was measured slower (2.23 vs 1.80 ms: half as
                               // many workgroups, each more than twice as long)
constexpr int NRU = NR - 1;
constexpr int WIN_QCAT = 1;          // gauss_window_desc.kind == GAUSS_WIN_QCAT
constexpr int WIN_LD = 2;            // gauss_window_desc.kind == GAUSS_WIN_LD
constexpr int TILE_GB11 = 1 << 30;   // tilemap.y flag: the entry is a job-wide B11 pair (Prob::gpair_*), seen from this window

// Pointers stored inside a Prob are loaded from memory, so the compiler could not infer their
// address space and would emit flat_* accesses.  Everything a Prob points to is device global
// memory: in the device pass the members are declared address_space(1) (same size and layout).
#if defined(__HIP_DEVICE_COMPILE__)
#define GP(T) T __attribute__((address_space(1)))*
#else
#define GP(T) T*
#endif

// Device-visible description of one window ("problem").  Built on the host by the planner,
// uploaded once per job.  All pointers are device pointers.
struct Prob {
    int mode, P;            // P = populations as seen by the kernels (1 pseudo-pop when pooled)
    int M, U;               // measured / unmeasured SNP rows
    int Mp, Up, Sp;         // row counts padded to TILE; Sp = Mp + Up
    int N;                  // samples (sum of population sizes)
    int Kp;                 // packed row length in bytes (multiple of KC)
    int nseg, npair, nT;    // K segments, tile pairs, row tiles (Sp / TILE)
    int Mld, nblk;          // solve leading dimension (M padded to NB) and block count
    int npanel;             // panels of the stand-alone solve (ceil(n_rhs / NRU)), 0 for LD-only problems
    int npi;                // panels of the fused path's right-hand sides [I | z1]: ceil((M + 1) / NR) (k_solve.hip)
    int Up128;              // n_rhs rounded up to 128: row count of a k block of Gsum
    int ld_only;            // 1: write out_ld (S x S) instead of B11/B21
    int kind;               // 0 imputation (z, info), 1 QCAT (correlation of whitened vectors)
    int n_head, n_predm;    // QCAT: measured rows before / inside the prediction window
    int n_rhs;              // right-hand sides of the solve: U (imputation) or n_predm + U (QCAT)
    int U_raw;              // rows of raw_u; U = U_raw * (number of codings)
    int code_blk[3];        // coding of B21 row block b: 0 additive, 1 dominant, 2 recessive (gauss.cpp:1196-1250)
    int n_run;              // 2-bit sources: number of source blocks (selected populations)
    int geno_fmt;           // 0: one byte per genotype (ASCII digit or small integer); 1: 2-bit packed blocks
    int gram_i8;            // 1: operands are raw codes and slabs hold int32 (i8 MFMA path); 0: e4m3 codes, f32 slabs
    int slab16;             // 1: partial slabs hold exact uint16 sums, two rows per dword (2-bit sources: codes <= 3 and
                            // segments <= 7168 samples keep a partial below 2^16); halves the slab traffic
    double lambda, eps, diag;
    long long ld_raw;
    GP(const uint8_t) raw_m;   // [M x ld_raw]
    GP(const uint8_t) raw_u;   // [U x ld_raw]
    // Row arrays come in two parts: the measured rows [0, Mp) behind `X`, the unmeasured rows [Mp, Sp) behind `X_u`
    // (indexed from 0).  Ordinarily X_u = X + Mp rows of one array.  In a job whose windows share their measured SNPs
    // (gauss_plan.cpp: shared measured rows) X points INTO the job-wide arrays of the chromosome's measured SNPs, at this
    // window's first one (g0): rows the windows have in common are packed once, and the tile pairs of B11 -- formed on
    // job-wide row tiles, `gpair_*` / `slab_g` -- are multiplied once for all the windows they lie in.
    GP(uint8_t) packed;        // [Mp x Kp]
    GP(uint8_t) packed_u;      // [Up x Kp]
    GP(int) sx;                // [.. x P] per-population sum x
    GP(int) sxx;               // [.. x P] per-population sum x^2
    GP(int) sx_u;
    GP(int) sxx_u;
    GP(const int) pop_raw_off; // [P+1]
    GP(const int) pop_pk_off;  // [P+1] packed column offsets (multiples of KC)
    GP(const double) pop_w;    // [P]
    GP(const double) pop_wf;   // [P] wgt_val * ((double)m / (m - 1))   (util.cpp:117-118)
    GP(const double) pop_md;   // [P] (double)m
    GP(const int) seg_pop;     // [nseg]
    GP(const int) seg_k0;      // [nseg] packed byte range
    GP(const int) seg_k1;
    GP(const int) pop_seg0;    // [P+1] segment range per population
    GP(const int) pair_ti;     // [npair]
    GP(const int) pair_tj;
    GP(const int) pair_lut;    // [nT x nT] -> pair index or -1
    GP(const uint8_t) word_pop;// [Kp/16] population of each packed 16-byte word
    GP(const int) rows_m;      // store row of each measured / unmeasured matrix row, or null (contiguous)
    GP(const int) rows_u;
    GP(const uint8_t) word_run;// 2-bit sources: [Kp/16] source block ("run") of each packed word
    GP(const int) run_pk_off;  // [n_run+1] packed column range of each run
    GP(const int) run_src;     // [n_run] byte offset of each run inside a source row
    GP(float) slab;            // [npair*nseg][TILE*TILE] exact integer partial Grams
    GP(double) rt_sd;          // [..] weighted: sqrt(self cov); pooled: sqrt(n*Sxx - Sx^2)
    GP(double) rt_wm;          // [..] weighted: sum_p w_p mu_p ; pooled: Sx (as double)
    GP(double) rt_mu;          // [.. x P] Sx_p / m_p
    GP(double) rt_wmu;         // [.. x P] w_p * mu_p
    GP(double) rt_sd_u;
    GP(double) rt_wm_u;
    GP(double) rt_mu_u;
    GP(double) rt_wmu_u;
    int g0;                    // shared measured rows: job-wide index of this window's first measured SNP (else 0)
    int n_gpair;               // shared measured rows: job-wide B11 tile pairs (0: B11's pairs are pair_ti / pair_tj / slab)
    GP(const int) gpair_ti;    // [n_gpair] job-wide row tiles of the pair (gi <= gj)
    GP(const int) gpair_tj;
    GP(float) slab_g;          // [n_gpair * nseg][TILE*TILE] partial Grams of the job-wide B11 pairs
    GP(const double) z1;       // [M]
    GP(double) A;              // [5][Mld x Mld] row-major: B11, B11 - eps*I, their factors L0, L1, working copy W0 of B11
    GP(double) Linv;           // [2][nblk][NB x NB] inverses of the diagonal Cholesky blocks
    GP(double) B21;            // [Upad x Mld] row-major (Upad = npanel*NRU rounded)
    GP(double) V;              // [max(npanel, npi)][Mld][NR]: fused path: [X | y] = L^-1 [I | z1] by panels of NR columns
    GP(double) Gsum;           // [ceil(Mld / 128)][Up128][3] z / info / v sums of every k block (impute_gemm_kernel)
    GP(double) Part;           // [2][npi][SOLVE_SPLIT][NB x NR] parked sums of a row's early products, by row parity
    GP(double) out_z;          // [U]
    GP(double) out_info;       // [U]
    GP(int) status;            // [4]: [0] fail flag matrix 0, [1] fail flag matrix 1, [2] nonfinite
    GP(double) out_ld;         // [S x S] for ld_only
    GP(const int) gene_off;    // gene batches: [n_gene+1], else null
    int n_gene;
    GP(long long) gene_out_off;// [n_gene] offsets into out_ld
    // resampled windows (simulateLD, k_simld.hip): the packed columns are drawn samples, not the populations' samples
    GP(const int) draw_col;    // [Kp] source column of every packed column, ascending, -1 past the draws; null: not resampled
    int row_src_bytes;         // bytes of a source row the resample kernel reads
    // The riders of an imputation window.  Where each one's section lies in the result block: res_layout / slct_layout below.
    // leave-one-out re-imputation of the measured SNPs (k_loo.hip): [3][M] loo_z, loo_info, loo_t; null: not asked
    GP(double) out_loo;
    // stepwise conditional signal selection (k_slct.hip); slct_max = 0: not asked
    int slct_max, n_slct_forced;           // K <= SLCT_K; forced SNPs that enter first
    double slct_chi2_stop, slct_min_var_frac;
    GP(const int) slct_forced;             // [n_slct_forced]
    GP(double) slct_W;                     // [SLCT_K][Mld] scratch: row s = column sel[s] of the partial Cholesky factor
    GP(double) out_slct;                   // [slct_layout(M, K).count]
    // the imputed SNPs conditioned on the selected signals (k_cond.hip); out_cond = null: not asked (it needs slct_max > 0)
    double cond_min_var_frac;
    GP(double) out_cond;                   // [2][U] cond_z, then cond_var
    // credible sets of the selected signals (k_cs.hip); out_cs = null: not asked (it needs slct_max > 0, and reads cond_min_var_frac)
    double cs_coverage, cs_prior_var;      // rho in (0, 1], omega > 0
    GP(double) cs_lbf;                     // [slct_max][cs_tld(M + U)] scratch: log Bayes factors, then pip, of every candidate per signal
    GP(uint8_t) cs_mem;                    // [slct_max][cs_tld(M + U)] scratch: 1 where the candidate is in the signal's set
    GP(double) out_cs;                     // [cs_layout(M + U, K).count]
    // multi-causal fine-mapping of the window (k_susie.hip); susie_L = 0: not asked
    int susie_L, susie_max_sweeps;         // effects L <= SUSIE_L, sweeps over them at the most
    int susie_estimate_var, susie_measured_only, susie_am;      // flags; am: the result section also holds alpha and mu
    double susie_coverage, susie_prior_var, susie_tol, susie_min_abs_corr;
    GP(double) susie_ws;                   // [susie_ws(M, U, Mld, L, !measured_only).total(susie_k)] scratch: W = B11^-1 B12, the fit's state (SusieWs below)
    GP(uint8_t) susie_mem;                 // [1 + susie_k][L][cs_tld(M + U)] scratch: 1 where the candidate is in the effect's set
    GP(double) out_susie;                  // [susie_layout(M + U, L, am).count]
    // ... of further traits in the same fit, and the colocalisation of every pair of fitted traits (k_coloc.hip); susie_k = 0: trait 1 alone
    int susie_k;                           // the first susie_k rows of traits_Z are fitted beside z1 (<= SUSIE_K); each has a state of its own in susie_ws
    int susie_lbf, coloc;                  // flags; lbf: the section holds the final lbf rows of every fitted trait; coloc: the pairs are asked
    double coloc_p1, coloc_p2, coloc_p12;  // prior probabilities that a SNP is causal for the first trait only, the second only, both
    GP(double) out_susie_more;             // [susie_more_layout(M + U, L, am, lbf, susie_k, coloc).count]
    // joint fine-mapping across the windows of a group, one study each (k_xsusie.hip); xs_n = 0: the window is in no group
    int xs_n, xs_pos;                      // studies K of the group (2 .. XS_MAX) and this window's place among them (0: the leader)
    int xs_peer[4];                        // the group's windows in job order, as indices into the job's descriptors ([0]: the leader)
    int xs_mu;                             // flag, on the leader: the section holds every study's mu
    GP(const int) xs_from_lead;            // [T_lead] leader candidate -> this window's candidate, -1: not one; null: the same index (the leader; a peer of equal M and U)
    GP(const int) xs_to_lead;              // [M + U] this window's candidate -> leader candidate, -1: none; null with xs_from_lead
    GP(double) out_xs;                     // the leader's: [xs_layout(K, L, T_lead, xs_mu).count]
    // polygenic score weights of the window (k_prs.hip); prs_n_s = 0: not asked
    int prs_n_s, prs_n_lam, prs_max_sweeps;      // chains (<= PRS_S), penalties on each chain's path (<= PRS_LAM), sweeps per (s, lam) at the most
    double prs_n, prs_tol;                 // the study's sample size; a lam is left when delta < prs_tol * r_max
    double prs_s[8], prs_lam[32];          // [PRS_S], [PRS_LAM] the grid
    GP(double) out_prs;                    // [prs_layout(M, n_s, n_lam).count]
    // LD scores of the measured SNPs of an LD window (k_ldscore.hip); lds_on = 0: not asked
    int lds_on, lds_C;                     // categories C <= LDS_C beside the plain score
    long long lds_radius;                  // bp, >= 0 (capped at 2^32 by the planner: positions are 32-bit)
    double lds_n;                          // the sample size of the bias adjustment
    GP(const int) lds_bp;                  // [M + U] positions, the measured rows first
    GP(const double) lds_annot;            // [C][M + U] weights; null: C = 0
    GP(double) lds_part;                   // [1 + C][lds_chunks(M, U)][2][Mld] scratch: every chunk's partial raw, then mass, per target
    GP(double) out_lds;                    // [lds_layout(M, C).count]
    // further traits on the same window (k_traits.hip); traits_T = 0: not asked
    int traits_T;                          // T <= TRAITS_MAX further Z-score vectors
    GP(const double) traits_Z;             // [Mld][T16] their Z-scores, SNP-major, zero beyond M and T (T16 = T rounded up to 16)
    GP(double) traits_Y;                   // [Mld][T16] scratch: Y = X Z
    GP(double) traits_G;                   // [Mld][T16] scratch: G = X^T Y = B11^-1 Z
    GP(double) out_traits;                 // [T][U]
    // further traits that lack some measured SNPs (k_traits_miss.hip); miss_tab = null: no mask was passed
    int miss_E, miss_nm, miss_n;           // distinct missing SNPs of the window, traits that lack some, set mask bits
    GP(const int) miss_tab;                // the mask as index lists: MissTab below
    GP(double) miss_YE;                    // [Mld][E16] scratch: X e_d, the columns of X of the missing SNPs (E16 = miss_E rounded up to 16)
    GP(double) miss_AE;                    // [Mld][E16] scratch: A[:, E] = X^T (X e_d), the columns of B11^-1
    GP(double) miss_YU;                    // [E16][U] scratch: (B21 A[:, E])^T, the entries y_u[d]
    GP(double) miss_LD;                    // [miss_nm][MISS_LD] scratch: L_D ([k][MISS_K] row-major lower triangle), then c
    GP(double) out_traits_info;            // [T][U] info per trait
    GP(double) out_traits_miss;            // [2][miss_n] z, then info, of the SNPs the traits lack, in mask order
};
// a descriptor derived from a window's (the job-wide measured rows) carries no rider
inline void clear_riders(Prob& q)
{
    q.out_loo = nullptr;
    q.slct_max = q.n_slct_forced = 0; q.slct_chi2_stop = q.slct_min_var_frac = 0.0;
    q.slct_forced = nullptr; q.slct_W = nullptr; q.out_slct = nullptr;
    q.cond_min_var_frac = 0.0; q.out_cond = nullptr;
    q.cs_coverage = q.cs_prior_var = 0.0; q.cs_lbf = nullptr; q.cs_mem = nullptr; q.out_cs = nullptr;
    q.susie_L = q.susie_max_sweeps = q.susie_estimate_var = q.susie_measured_only = q.susie_am = 0;
    q.susie_coverage = q.susie_prior_var = q.susie_tol = q.susie_min_abs_corr = 0.0;
    q.susie_ws = nullptr; q.susie_mem = nullptr; q.out_susie = nullptr;
    q.susie_k = q.susie_lbf = q.coloc = 0; q.coloc_p1 = q.coloc_p2 = q.coloc_p12 = 0.0; q.out_susie_more = nullptr;
    q.xs_n = q.xs_pos = q.xs_mu = 0; q.xs_peer[0] = q.xs_peer[1] = q.xs_peer[2] = q.xs_peer[3] = 0;
    q.xs_from_lead = q.xs_to_lead = nullptr; q.out_xs = nullptr;
    q.prs_n_s = q.prs_n_lam = q.prs_max_sweeps = 0; q.prs_n = q.prs_tol = 0.0; q.out_prs = nullptr;
    q.lds_on = q.lds_C = 0; q.lds_radius = 0; q.lds_n = 0.0; q.lds_bp = nullptr; q.lds_annot = nullptr; q.lds_part = q.out_lds = nullptr;
    q.traits_T = 0; q.traits_Z = nullptr; q.traits_Y = q.traits_G = q.out_traits = nullptr;
    q.miss_E = q.miss_nm = q.miss_n = 0; q.miss_tab = nullptr;
    q.miss_YE = q.miss_AE = q.miss_YU = q.miss_LD = q.out_traits_info = q.out_traits_miss = nullptr;
}
constexpr int TRAITS_MAX = 63;         // GAUSS_TRAITS_MORE_MAX
constexpr int traits_t16(int T) { return (T + 15) & ~15; }
constexpr int MISS_K = 32;             // GAUSS_TRAITS_MISS_MAX: missing SNPs per trait
constexpr int MISS_E = 128;            // GAUSS_TRAITS_MISS_UNION_MAX: distinct missing SNPs per window
constexpr int MISS_LD = MISS_K * MISS_K + MISS_K;      // doubles of one trait's L_D and c in Prob::miss_LD
// Prob::miss_tab, ints: the window's distinct missing SNPs in ascending order (-1 beyond miss_E); per trait its count of
// missing SNPs, where its entries start in out_traits_miss, their measured indices (ascending) and their places in `e`; the
// traits that lack some, in ascending order
struct MissTab { enum { e = 0, k = e + MISS_E, off = k + 64, idx = off + 64, pos = idx + 64 * MISS_K, masked = pos + 64 * MISS_K, count = masked + 64 }; };
constexpr int SLCT_K = 32;             // GAUSS_SLCT_MAX
constexpr int SLCT_T = 512;            // threads of slct_kernel; a thread keeps the "selected" flags of its SNPs in one 64-bit word
constexpr int SLCT_M_MAX = 64 * SLCT_T;
constexpr int COND_T = 128;            // threads of cond_kernel: one per unmeasured SNP of its block
constexpr int CS_T = 128;              // threads of cs_lbf_kernel and cs_fold_kernel: one per candidate of its block
constexpr int CS_SET_T = 512;          // threads of cs_set_kernel
constexpr int cs_tld(int T) { return (T + 15) & ~15; }      // row pitch of Prob::cs_lbf / cs_mem
constexpr int SUSIE_L = 32;            // GAUSS_SUSIE_MAX_L: cs_set_row's workspace geometry, one row per effect
constexpr int SUSIE_MAX_SWEEPS = 1000; // GAUSS_SUSIE_MAX_SWEEPS: a run queues max_sweeps x L x 2 launches up front
constexpr int SUSIE_T = 256;           // threads of the fit's kernels
constexpr int SUSIE_CH = 1024;         // unmeasured candidates whose mean effects sit in LDS at a time (susie_ser_v_kernel)
constexpr int SUSIE_VR = 8;            // rows of v = b_meas + W b_unmeas a workgroup writes (two a wave)
constexpr int SUSIE_RR = 8;            // rows of R b = [B v ; C v] a workgroup writes (two a wave)
constexpr int SUSIE_P = 128;           // members of a set the purity looks at
constexpr int SUSIE_PG = 32;           // workgroups that share the pairs of one set's purity
constexpr int SUSIE_K = 7;             // GAUSS_SUSIE_TRAITS_MORE_MAX: further traits in one fit; (SUSIE_K + 1) SUSIE_K / 2 = 28 pairs at the most
constexpr int XS_MAX = 4;              // GAUSS_XS_MAX: studies (windows) in one group of the joint fit (k_xsusie.hip)
constexpr int PRS_S = 8;               // GAUSS_PRS_MAX_S: chains of a window (Prob::prs_s)
constexpr int PRS_LAM = 32;            // GAUSS_PRS_MAX_LAM: penalties on a chain's path (Prob::prs_lam)
constexpr int PRS_MAX_SWEEPS = 1000;   // GAUSS_PRS_MAX_SWEEPS: with it every loop of prs_kernel is bounded
constexpr int PRS_M_MAX = 4096;        // GAUSS_PRS_MAX_M: beta, g, r and diag(B) of a chain in LDS: 4 M doubles, 128 KB of gfx950's 160
constexpr int PRS_T = 256;             // threads of prs_kernel: one workgroup per chain
constexpr int LDS_C = 32;              // GAUSS_LDS_MAX_ANNOT: annotation categories of a window's LD scores
constexpr int LDS_CHUNK = 64;          // GAUSS_LDS_CHUNK: rows of a chunk of ldscore_kernel's summation order
constexpr int LDS_COLS = 64;           // targets of a workgroup of ldscore_kernel: one per lane of its wave
constexpr int LDS_MAX_CHUNKS = 65535;  // chunks of a window: they are the y extent of ldscore_kernel's grid (the planner refuses more: 4.19 M rows)
constexpr int CLUMP_T = 512;            // threads of clump_kernel: one workgroup per trait
constexpr int CLUMP_M_MAX = 8192;      // GAUSS_CLUMP_MAX_M: keys, owner and bp of a region in LDS, 16 bytes a SNP (k_clump.hip)
constexpr int CLUMP_KEYS_MAX = 64;     // GAUSS_CLUMP_MAX_KEYS: traits of one call, the x extent of clump_kernel's grid
constexpr int LDSPLIT_M_MAX = 8192;    // GAUSS_LDSPLIT_MAX_M: SNPs of a region that ldsplit_* split (k_ldsplit.hip)
constexpr int LDSPLIT_SIZE_MAX = 4096; // GAUSS_LDSPLIT_MAX_SIZE: SNPs of a block; Sd, SMd and Tk are [min(max_size, M)][M] doubles each
constexpr int LDSPLIT_K_MAX = 128;     // GAUSS_LDSPLIT_MAX_K: blocks of a split = launches of ldsplit_dp_kernel
constexpr int LDSPLIT_ROWS = 64;       // rows of a tile of ldsplit_band_kernel: one per lane of its wave
constexpr int LDSPLIT_OFFS = 64;       // offsets j - i of a tile of ldsplit_band_kernel: the chunk its scan walks out of LDS
constexpr int LDSPLIT_COST_T = 64;     // threads of ldsplit_cost_kernel: one boundary each
constexpr int LDSPLIT_DP_B = 64;       // boundaries of a workgroup of ldsplit_dp_kernel: one per lane
constexpr int LDSPLIT_DP_NW = 16;      // waves of that workgroup: wave w takes every LDSPLIT_DP_NW-th block size from the w-th on
constexpr int HESS_M_MAX = 4096;       // GAUSS_HESS_MAX_M: SNPs of a block; G and V are [M to 32][M to 64] doubles each (k_hess.hip)
constexpr int HESS_TRAITS_MAX = 64;    // GAUSS_HESS_MAX_TRAITS: traits of one call
constexpr int HESS_K_MAX = 1024;       // GAUSS_HESS_MAX_K: projections per trait = workgroups of hess_proj_kernel
constexpr int HESS_B = 16;             // columns of a block of hess_block_round_kernel; a workgroup rotates a pair of blocks
constexpr int HESS_PW = 2 * HESS_B;    // the pair width: the columns are padded to a multiple of it, the order of the Gram matrix S
constexpr int HESS_RC = 64;            // rows of a staged chunk of the pair's columns; the rows are padded to a multiple of it
constexpr int HESS_T = 256;            // threads of every hess_* kernel
constexpr int HESS_INNER_MAX = 1;      // sweeps of the two-sided Jacobi on S per visit (measured: k_hess.hip)
constexpr int HESS_MAX_SWEEPS = 30;    // outer sweeps at the most: GAUSS_ST_HESS_NOCONV
constexpr int SC2_T = 256;             // threads of sumchi2_kernel: one workgroup per gene
constexpr int SC2_N_MAX = 1024;        // GAUSS_SUMCHI2_MAX_N: SNPs of a gene before pruning; flags and the kept list in LDS (k_sumchi2.hip)
constexpr int SC2_K_MAX = 128;         // GAUSS_SUMCHI2_MAX_KEPT: order of the eigenvalue solve; the kept block in LDS, 129 doubles a row
constexpr int SC2_TRAITS_MAX = 64;     // GAUSS_SUMCHI2_MAX_TRAITS: traits of one call, one thread each for Q
constexpr int SC2_MAX_SWEEPS = 30;     // Jacobi sweeps before GAUSS_ST_NOCONV (fp64 Jacobi at order 128 takes 7 .. 9)
constexpr int lds_chunks(int M, int U) { return (M + LDS_CHUNK - 1) / LDS_CHUNK + (U + LDS_CHUNK - 1) / LDS_CHUNK; }      // measured rows' chunks, then the others'
constexpr int susie_uld(int U) { return (U + 63) & ~63; }   // row pitch of W and Y
// Prob::susie_ws in doubles.  Y = X C^T and W = X^T Y = B11^-1 B12 [Mld][uld], the window's; then one block per fitted trait (trait t
// of 0 .. susie_k at t * trait doubles further on): zhat, d, adm [tld] per candidate; alpha, mu, rb (R b_l) and lbf [L][tld]; f [tld];
// v [Mld]; V [2][SUSIE_L] by sweep parity; lse, lse_set, part [SUSIE_L][SUSIE_PG] (partial minima of the purity), top [SUSIE_L][SUSIE_P]
// (candidate indices as ints: half the doubles), ntop [SUSIE_L]; ctl: done, sweeps, last delta, delta by sweep parity [2], the trait's
// scores hold a NaN; keep [L][tld]: the final lbf rows, which susie_set_kernel turns into pips where they stand -- copied there only
// where the lbf output or the colocalisation is asked.  [state, keep) is zeroed by susie_prep_kernel at the start of every run; keep
// itself is not: susie_set_kernel rewrites all of it that anyone reads (l < L, i < T) before the fold and coloc_kernel read it.  (d and its part in adm are the same for every trait: each block has its own
// copy, so that trait 0's offsets are those of a fit of one trait.)
struct SusieWs {
    size_t Y, W, zhat, d, adm, state, alpha, mu, rb, lbf, f, v, V, lse, lse_set, part, top, ntop, ctl, keep, count, trait;
    constexpr size_t total(int k) const { return zhat + (size_t)(1 + k) * trait; }
};
enum { SUSIE_CTL_DONE = 0, SUSIE_CTL_SWEEPS, SUSIE_CTL_LAST, SUSIE_CTL_DELTA, SUSIE_CTL_ZNAN = SUSIE_CTL_DELTA + 2, SUSIE_CTL_N = 8 };
// (w = false: a fit of the measured SNPs alone forms no W)
constexpr SusieWs susie_ws(int M, int U, int Mld, int L, bool w)
{
    const size_t tld = (size_t)cs_tld(M + U), mu = w ? (size_t)Mld * susie_uld(U) : 0, lt = (size_t)L * tld;
    const size_t zhat = 2 * mu, state = zhat + 3 * tld, f = state + 4 * lt, V = f + tld + (size_t)Mld, lse = V + 2 * SUSIE_L;
    const size_t part = lse + 2 * SUSIE_L, top = part + (size_t)SUSIE_L * SUSIE_PG, ntop = top + (size_t)SUSIE_L * SUSIE_P / 2;
    const size_t keep = ntop + SUSIE_L + SUSIE_CTL_N;
    return {0, mu, zhat, zhat + tld, zhat + 2 * tld, state, state, state + lt, state + 2 * lt, state + 3 * lt, f, f + tld, V, lse,
            lse + SUSIE_L, part, top, ntop, ntop + SUSIE_L, keep, keep + lt, keep + lt - zhat};
}

#endif
// ---- the result block ------------------------------------------------------------------------------------------------
// A window's doubles in the job's result block, in this order and nowhere else written down:
//     z[n_rhs], info[n_rhs] [, loo_z[M], loo_info[M], loo_t[M]] [, traits [T][U]] [, traits_info [T][U], traits_miss [2][n_miss]]
//     [, the selection] [, cond_z[U], cond_var[U]] [, cs: size[K], mass[K], lse[K], pip[M+U], set[M+U], set_pip[M+U]]
//     [, susie: susie_layout] [, susie_more: susie_more_layout] [, xs: xs_layout] [, prs: prs_layout] [, lds: lds_layout]
// Offsets in doubles from the window's Plan::res_off; a section nobody asked for takes nothing and its offset is that of the next.
// traits_info and traits_miss exist when the window passed a mask (miss): n_miss = its set bits.  The conditional section
// (cond; k_cond.hip), behind it the credible sets (cs; k_cs.hip), behind them the multi-causal fit (susie; k_susie.hip) and what it holds beyond trait 1's
// values (susie_more; the further traits' fits, the lbf rows, the colocalisation of k_coloc.hip) are the last: every other offset is
// what it is without them.  The leader of a group of the joint fit across studies (xs; k_xsusie.hip) has one more section behind them.
// The polygenic score weights (prs; k_prs.hip) come behind all of them, and behind them the LD scores of an LD window (lds;
// k_ldscore.hip), which has none of the others.
struct ResLayout { size_t z, info, loo, traits, traits_info, traits_miss, slct, cond, cs, susie, susie_more, xs, prs, lds, count; };
// Inside the selection's section, from its start: n, skipped, idx[K], zin[K], joint[K], zc[M], var_left[M] (indices, n and the
// skipped flag travel as exact doubles).  The host and slct_kernel both read it here.
struct SlctLayout { size_t n, skipped, idx, zin, joint, zc, var, count; };
constexpr SlctLayout slct_layout(int M, int K)
{
    return {0, 1, 2, 2 + (size_t)K, 2 + 2 * (size_t)K, 2 + 3 * (size_t)K, 2 + 3 * (size_t)K + (size_t)M, 2 + 3 * (size_t)K + 2 * (size_t)M};
}
// Inside the credible sets' section, from its start: size[K], mass[K], lse[K] per signal, then pip[T], set[T], set_pip[T] per candidate
// (T = M + U, the measured SNPs first; size and set travel as exact doubles).  The host and the cs kernels both read it here.
struct CsLayout { size_t size, mass, lse, pip, set, set_pip, count; };
constexpr CsLayout cs_layout(int T, int K)
{
    return {0, (size_t)K, 2 * (size_t)K, 3 * (size_t)K, 3 * (size_t)K + (size_t)T, 3 * (size_t)K + 2 * (size_t)T, 3 * (size_t)K + 3 * (size_t)T};
}
// Inside the multi-causal fit's section, from its start: V, lse, size, mass, purity, kept [L] per effect, fit [4] = sweeps run, the
// last delta, 1 when the sweeps ran out before delta < tol, unused; pip, set, set_pip [T] per candidate (T = M + U, the measured
// SNPs first); with am, alpha [L][T] and mu [L][T].  Sizes, set, kept and sweeps travel as exact doubles.
struct SusieLayout { size_t V, lse, size, mass, purity, kept, fit, pip, set, set_pip, alpha, mu, count; };
constexpr SusieLayout susie_layout(int T, int L, bool am)
{
    const size_t l = (size_t)L, t = (size_t)T, c = 6 * l + 4;
    return {0, l, 2 * l, 3 * l, 4 * l, 5 * l, 6 * l, c, c + t, c + 2 * t, c + 3 * t, c + 3 * t + (am ? l * t : 0), c + 3 * t + (am ? 2 * l * t : 0)};
}
// Behind the multi-causal fit's section, from its start: with lbf, trait 1's final lbf [L][T]; then one block per further fitted trait
// (k of them, `one` doubles apart): its susie_layout and, with lbf, its lbf [L][T] at `tlbf` inside the block; with coloc, for the
// pairs = (k + 1) k / 2 pairs of fitted traits in the order (0, 1), (0, 2), .., (k - 1, k): pp [pairs][L][L][5], hit [pairs][L][L] (an
// exact double, -1: none), hit_pp [pairs][L][L], n [pairs].  A part nobody asked for takes nothing.
struct SusieMoreLayout { size_t lbf, trait, one, tlbf, pp, hit, hit_pp, n, count; };
constexpr SusieMoreLayout susie_more_layout(int T, int L, bool am, bool lbf, int k, bool coloc)
{
    const size_t lt = lbf ? (size_t)L * T : 0, fit = susie_layout(T, L, am).count, one = fit + lt;
    const size_t pp = lt + (size_t)k * one, ll = (size_t)L * L, np = coloc ? (size_t)(k + 1) * k / 2 : 0;
    return {0, lt, one, fit, pp, pp + 5 * np * ll, pp + 6 * np * ll, pp + 7 * np * ll, pp + 7 * np * ll + np};
}
// The leader's section of the joint fit across the K studies of a group, from its start: V [K][L] and purity [K][L] per study and
// effect, n = the joint admissible candidates (an exact double); with mu, every study's mu [K][L][T] in the leader's candidate order
// (T = the leader's M + U).  The joint pip / set / alpha / lse / sizes are the leader's susie_layout.
struct XsLayout { size_t V, purity, n, mu, count; };
constexpr XsLayout xs_layout(int K, int L, int T, bool mu)
{
    const size_t kl = (size_t)K * L;
    return {0, kl, 2 * kl, 2 * kl + 1, 2 * kl + 1 + (mu ? kl * T : 0)};
}
// Inside the polygenic score's section, from its start: cell [n_s * n_lam][PRS_CELL] = nnz, sweeps, delta, br, bg, kkt, 1 when the
// sweeps ran out, unused, per grid cell c = i_s * n_lam + i_lam; then beta [n_s * n_lam][M].  nnz, sweeps and the flag travel as
// exact doubles.  prs_kernel and the host both read it here.
enum { PRS_NNZ = 0, PRS_SWEEPS, PRS_DELTA, PRS_BR, PRS_BG, PRS_KKT, PRS_NOCONV, PRS_CELL = 8 };
struct PrsLayout { size_t cell, beta, count; };
constexpr PrsLayout prs_layout(int M, int n_s, int n_lam)
{
    const size_t c = (size_t)n_s * n_lam;
    return {0, c * PRS_CELL, c * PRS_CELL + c * (size_t)M};
}
// Inside the LD scores' section, from its start: raw, l2, mass, each [1 + C][M] (category 0 is the plain score).  ldscore_finish_kernel
// and the host both read it here.
struct LdsLayout { size_t raw, l2, mass, count; };
constexpr LdsLayout lds_layout(int M, int C)
{
    const size_t n = (size_t)(1 + C) * M;
    return {0, n, 2 * n, 3 * n};
}
constexpr ResLayout res_layout(int n_rhs, int M, int U, bool loo, int T, int K, bool miss = false, int n_miss = 0, bool cond = false,
                               bool cs = false, int susie_L = 0, bool susie_am = false, bool susie_lbf = false, int susie_k = 0,
                               bool coloc = false, int xs_K = 0, bool xs_mu = false, int prs_n_s = 0, int prs_n_lam = 0, bool lds = false,
                               int lds_C = 0)
{
    const size_t o_loo = 2 * (size_t)n_rhs, o_traits = o_loo + (loo ? 3 * (size_t)M : 0), o_tinfo = o_traits + (size_t)T * U;
    const size_t o_tmiss = o_tinfo + (miss ? (size_t)T * U : 0), o_slct = o_tmiss + (miss ? 2 * (size_t)n_miss : 0);
    const size_t o_cond = o_slct + (K ? slct_layout(M, K).count : 0);
    const size_t o_cs = o_cond + (cond ? 2 * (size_t)U : 0);
    const size_t o_susie = o_cs + (cs ? cs_layout(M + U, K).count : 0);
    const size_t o_more = o_susie + (susie_L ? susie_layout(M + U, susie_L, susie_am).count : 0);
    const size_t o_xs = o_more + (susie_L ? susie_more_layout(M + U, susie_L, susie_am, susie_lbf, susie_k, coloc).count : 0);
    const size_t o_prs = o_xs + (xs_K ? xs_layout(xs_K, susie_L, M + U, xs_mu).count : 0);
    const size_t o_lds = o_prs + (prs_n_s ? prs_layout(M, prs_n_s, prs_n_lam).count : 0);
    return {0, (size_t)n_rhs, o_loo, o_traits, o_tinfo, o_tmiss, o_slct, o_cond, o_cs, o_susie, o_more, o_xs, o_prs, o_lds,
            o_lds + (lds ? lds_layout(M, lds_C).count : 0)};
}

#ifndef GAUSS_LAYOUTS_ONLY
// One unit of Gram work: a 128 x 128 tile pair times a run of consecutive K segments.  The kernel
// streams the whole run without draining its load pipeline and flushes the accumulators into one
// partial slab per segment.  Self-contained (64 bytes, fetched with scalar loads): no pointer
// chasing through the Prob before the first operand load.
struct Item {
    GP(const uint8_t) a;     // packed rows of tile ti (row 0, column 0)
    GP(const uint8_t) b;     // packed rows of tile tj
    GP(float) slab;          // slab of (pair, first segment of the run); later segments follow
    GP(const int) seg_k1;    // end column of each segment of the run
    GP(const uint32_t) chunk_live; // nibble c (word c / 8, bits 4 (c % 8) ..): 0 = all 64 samples of K chunk c are live; n = 1..7:
                             // only the chunk's first n UNITS of 8 samples are (the rest is the zero padding that ends a population
                             // block).  The pack kernel stores every 32-sample group dword-transposed (chunk_unit_layout below), which
                             // puts unit u of a chunk into dword u % 4 of BOTH lane halves of group u / 4 -- the MFMAs of a dead
                             // unit are not issued.  Dwords, read through the scalar cache (uniform_load)
    int Kp;                  // packed row stride
    int k0;                  // first column of the run
    int nseg;                // segments in the run
    int rows_a, rows_b;      // live rows of the two tiles (the rest is zero padding)
    int flags;               // bit 0: ti == tj (diagonal tile); bit 1: slabs are uint16 pairs (Prob::slab16); bit 2 (f32 path, only with bit 1: codes <= 3): the
                             // kernel packs two A rows per lane (k_gram.hip: chunk_mfma_packed); bit 4: a B11 item of a
                             // job built for a merged launch: counts itself off in the launch's `b11_done[0]` when one is passed
                             // (k_gram.hip); bit 5: a B21 item of an "early" window, counted in `b11_done[8]`; bits 6-7: how the four waves share
                             // the tile (k_gram_common.h: LAYOUT_*; 0 = a 64 x 64 quadrant each)
};
static_assert(sizeof(Item) == 64, "work items are fetched as one 64-byte descriptor");

template <typename T> using gptr = T __attribute__((address_space(1)))*;
template <typename T> __device__ __forceinline__ gptr<T> G(T* p) { return (gptr<T>)p; }
template <typename T> __device__ __forceinline__ gptr<T> G(gptr<T> p) { return p; }

// Wave-uniform table reads inside the Gram kernels' K loops (segment ends, half-chunk flags).  The tables are reached
// through pointers that were themselves loaded from memory, so the compiler cannot prove them read-only and emits VECTOR
// loads -- and a vector load's s_waitcnt vmcnt(0) also waits for every LDS-DMA group issued before it, i.e. for the
// operand chunks that were just requested for LATER iterations (round 2's half-chunk flag was a global_load_ubyte in the
// loop: every chunk's MFMAs waited for the next chunk's DMA).  Reading them through the constant address space makes
// them scalar loads (lgkmcnt), which leave the DMA queue alone.
#if defined(__HIPCC__)
template <typename T>
__device__ __forceinline__ T uniform_load(GP(const T) p, int idx)
{
    return ((const T __attribute__((address_space(4)))*)p)[idx];
}
// live units (1..8) of K chunk `chunk` from the nibble table
__device__ __forceinline__ int chunk_live_units(uint32_t word, int chunk)
{
    const int n = (int)((word >> (4 * (chunk & 7))) & 15u);
    return n ? n : 8;
}
#endif

// hipFuncSetAttribute is per device: `set` runs once for every device a launcher is used on (a process may drive
// several GPUs), and a second thread that arrives on the same device meanwhile (another context of bench --streams, a
// farm thread) waits until the attributes are in place instead of launching with the default dynamic-LDS limit.
struct DeviceOnce {
    std::atomic<unsigned long long> done{0};
    std::mutex mu;
    template <typename F> void run(F&& set)
    {
        int d = 0;
        (void)hipGetDevice(&d);
        const unsigned long long bit = 1ull << (d & 63);
        if (done.load(std::memory_order_acquire) & bit) return;
        std::lock_guard<std::mutex> lock(mu);
        if (done.load(std::memory_order_relaxed) & bit) return;
        set();
        done.fetch_or(bit, std::memory_order_release);
    }
};

// ---- launchers (host functions defined in the .hip files) ----
// d_code3 (may be null): a workgroup that meets a code 3 in a row of a 2-bit source raises the word to `pack_stamp` (it only
// grows: the caller numbers its pack launches upwards from 1).  launch_gram compares the word with the stamp of the pack launch
// that wrote ITS operands: below it, no row of this run holds a 3 (k_gram.hip: PK_F_GENO)
void launch_pack_stats(const Prob* d_probs, const int2* d_rowmap, int n_rows, hipStream_t s, unsigned long long* d_code3 = nullptr,
                       unsigned long long pack_stamp = 0);
// resampled windows (k_simld.hip): the pack stage of a job whose window has Prob::draw_col.  lds_bytes: from
// resample_pack_lds_bytes (0: the source row is too long to stage in LDS and is read from global memory)
constexpr int SIMLD_LDS_MAX = 60 << 10;
int resample_pack_lds_bytes(long long row_src_bytes);
void launch_resample_pack(const Prob* d_probs, const int2* d_rowmap, int n_rows, int lds_bytes, hipStream_t s);
// d_b11_done (may be null): items with flag bit 4 count themselves off there when their slabs are out (k_gram.hip)
// d_code3 / pack_stamp: as given to the launch_pack_stats of the same run; null: the packed items split at the interval that any
// 2-bit code admits
void launch_gram(const Item* d_items, int n_items, int dtype_i8, hipStream_t s, unsigned long long* d_b11_done = nullptr,
                 const unsigned long long* d_code3 = nullptr, unsigned long long pack_stamp = 0);
// one wave that returns when *d_count >= target (bounded; on timeout d_status[0 .. n_status) = 1)
// bound_us: give-up bound in microseconds (at least two seconds are always granted)
void launch_wait_count(const unsigned long long* d_count, unsigned long long target, int* d_status, int n_status, hipStream_t s,
                       double bound_us = 0.0);
void launch_wait_count_for(const unsigned long long* d_count, unsigned long long target, int* d_status, hipStream_t s, double bound_us);
void launch_count_up(unsigned long long* d_count, hipStream_t s);
void launch_epilogue(const Prob* d_probs, const int2* d_tilemap, int n_tiles, int max_pop, int dtype_i8, hipStream_t s);
void launch_epilogue_b11_lite(const Prob* d_probs, const int2* d_tilemap, int n_tiles, int dtype_i8, hipStream_t s);
void launch_pop_cor(const Prob* d_probs, int prob, int npair, double* d_out, hipStream_t s);
// zmix normal equations (k_zmix.hip): d_part [npair x ne] and d_part_n [npair] are workspace, ne = (G + 1)(G + 2) / 2;
// d_out [ne] gets the upper triangle of [y | X]^T [y | X] in row order, d_out_n the kept rows
void launch_zmix_normal_eq(const Prob* d_probs, int prob, int npair, const int* d_pop_group, int n_group, const double* d_z,
                           double* d_part, long long* d_part_n, double* d_out, long long* d_out_n, hipStream_t s);
void launch_pair_cor(const Prob* d_probs, int prob, const int2* d_pairs, long long n_pairs, const int* d_pop_group, int n_group,
                     double* d_out, hipStream_t s);
void launch_gene_epilogue(const Prob* d_probs, int prob, int n_gene, hipStream_t s);
void launch_factor_step(const Prob* d_probs, int n_prob, int step, int max_nblk, int max_npanel, int split, int own_panel, hipStream_t s);
// small-footprint twins (k_solve_lite.hip): same bits, built to run beside the Gram kernel
void launch_factor_step_lite(const Prob* d_probs, int n_prob, int step, int max_nblk, int max_npanel, int split, hipStream_t s);
void launch_solve_last_lite(const Prob* d_probs, const int2* d_panelmap, int n_panels, int max_nblk, int split, hipStream_t s);
void launch_shift_cert(const Prob* d_probs, int n_prob, hipStream_t s);
void launch_solve(const Prob* d_probs, const int2* d_panelmap, int n_panels, hipStream_t s);
void launch_impute_gemm(const Prob* d_probs, const int2* d_gmap, int n_tiles, int u_tile, const int2* d_fmap, int n_chunks, hipStream_t s);
void launch_solve_last(const Prob* d_probs, const int2* d_panelmap, int n_panels, int max_nblk, int split, hipStream_t s);
// leave-one-out values of the measured SNPs from [X | y] (k_loo.hip): d_loomap = (window, 64-column panel of X) of the windows that asked
void launch_loo(const Prob* d_probs, const int2* d_loomap, int n_panels, hipStream_t s);
// stepwise conditional signal selection on B11 and z1 (k_slct.hip): one workgroup per asking window; d_slctmap = the windows that asked
// (null: the n windows from d_probs on)
void launch_slct(const Prob* d_probs, const int* d_slctmap, int n, hipStream_t s);
// the imputed SNPs conditioned on the selected signals (k_cond.hip): blocks of COND_T unmeasured SNPs x the asking windows
// (d_condmap; null: the windows d_probs[0 .. n)); max_U = the most unmeasured SNPs one of them has.  It runs behind launch_slct
// and behind the kernel that writes out_z / out_info
void launch_cond(const Prob* d_probs, const int* d_condmap, int n, int max_U, hipStream_t s);
// credible sets of the selected signals (k_cs.hip): three launches over the asking windows (d_csmap; null: the windows
// d_probs[0 .. n)); max_T = the most candidates (M + U) one of them has.  They run behind launch_cond's place: behind launch_slct and
// behind the kernel that writes out_z / out_info
void launch_cs(const Prob* d_probs, const int* d_csmap, int n, int max_T, hipStream_t s);
// polygenic score weights (k_prs.hip) of the asking windows (d_prsmap; null: the windows d_probs[0 .. n)): one workgroup per (chain,
// window), max_s = the most chains, max_M = the most measured SNPs one of them has (the launch's LDS).  B11 in A[0] and z1 are all it
// reads: it needs no fused solve, and runs at the end of the tail, where nothing waits for it
void launch_prs(const Prob* d_probs, const int* d_prsmap, int n, int max_s, int max_M, hipStream_t s);
// LD scores (k_ldscore.hip) of the asking LD windows (d_ldsmap): one wave per (LDS_COLS targets, chunk of LDS_CHUNK rows, category,
// window) parks its partial sums, then a finish launch adds every target's chunks in ascending order and forms l2.  max_M / max_chunks /
// max_C: the largest among the asking windows.  It reads B11 in A[0] and B21 as the LD epilogue left them: queued last, behind the tail
void launch_ldscore(const Prob* d_probs, const int* d_ldsmap, int n, int max_M, int max_chunks, int max_C, hipStream_t s);
// multi-causal fine-mapping (k_susie.hip) of the asking windows (d_susiemap; null: the windows d_probs[0 .. n)).  launch_susie_w:
// W = X^T (X B12) of the windows that fit unmeasured candidates, two launches over (64-row block of X) x (64 unmeasured SNPs); it runs
// where launch_traits_weights runs (B21 is complete there).  launch_susie: the state, then max_sweeps x max_L x 2 dependent launches
// -- a window that has converged, has fewer effects or fewer sweeps leaves at once -- then the sets, their purity and the fold; it runs
// behind launch_cs.  max_M / max_U / max_T / max_L / max_sweeps: the largest among the asking windows
void launch_susie_w(const Prob* d_probs, const int* d_susiemap, int n, int max_nblk, int max_U, hipStream_t s);
// max_k: the most further traits one of them fits -- the trait is a grid dimension of the fit's launches, never a launch of its own;
// coloc: one of them asks for the colocalisation (k_coloc.hip), one launch behind susie_kept_kernel
void launch_susie(const Prob* d_probs, const int* d_susiemap, int n, int max_M, int max_T, int max_L, int max_sweeps, int max_k, bool coloc,
                  hipStream_t s);
void launch_coloc(const Prob* d_probs, const int* d_susiemap, int n, int max_L, int max_k, hipStream_t s);
// single launches of the fit's kernels (k_susie.hip) over the windows of a map, for the joint fit across studies to reuse them as they
// are: the state; R bbar_l and f of one (sweep, l); the sets' membership and their top members; the fold into pip / set / set_pip
void launch_susie_prep(const Prob* d_probs, const int* d_map, int n, hipStream_t s);
void launch_susie_rb(const Prob* d_probs, const int* d_map, int n, int max_T, int sweep, int l, hipStream_t s);
void launch_susie_sets(const Prob* d_probs, const int* d_map, int n, int max_L, hipStream_t s);
void launch_susie_fold(const Prob* d_probs, const int* d_map, int n, int max_T, hipStream_t s);
// joint fine-mapping across the studies of a group (k_xsusie.hip).  d_xsmap: the n windows that are members of a group; d_xsleadmap:
// the n_lead leaders among them.  Queued where launch_susie is (their W by launch_susie_w over d_xsmap where the ungrouped W is
// formed): the members' state, max_sweeps x max_L x 2 step launches (xsusie_ser_v_kernel over the members, susie_rb_kernel over the
// members), then the leaders' sets, every member's purity of the leader's top members, the leaders' kept / outputs and fold.
// max_M / max_T / max_L / max_sweeps: the largest among the members
void launch_xsusie(const Prob* d_probs, const int* d_xsmap, int n, const int* d_xsleadmap, int n_lead, int max_M, int max_T, int max_L,
                   int max_sweeps, hipStream_t s);
// further traits (k_traits.hip).  launch_traits_weights: G = X^T (X Z) of the windows that asked, d_map = (window, 64-row block of X),
// two launches (Y = X Z, then G = X^T Y); it runs where launch_loo runs.  launch_traits_impute: out_traits = B21 G / sqrt(out_info),
// d_umap = (window, strip of 64 unmeasured SNPs); it runs behind the kernel that writes out_info
void launch_traits_weights(const Prob* d_probs, const int2* d_map, int n_blocks, hipStream_t s);
void launch_traits_impute(const Prob* d_probs, const int2* d_umap, int n_strips, hipStream_t s);
// further traits that lack some measured SNPs (k_traits_miss.hip), for the windows that passed a mask.
// launch_traits_miss_solve: the columns A[:, E] of B11^-1 of the window's missing SNPs (d_map = (window, 64-row block of X), two launches:
// the columns of X gathered, then X^T of them), then per (window, trait that lacks some) = d_tmap the Cholesky factor of A_DD, c and the
// section of the missing SNPs; it runs behind launch_traits_weights.  launch_traits_miss_apply: B21 A[:, E], then per
// d_umap = (window, strip of 64 unmeasured SNPs) every trait's downdated mean and info; it runs behind launch_traits_impute.
void launch_traits_miss_solve(const Prob* d_probs, const int2* d_map, int n_blocks, const int2* d_tmap, int n_traits, hipStream_t s);
void launch_traits_miss_apply(const Prob* d_probs, const int2* d_umap, int n_strips, hipStream_t s);
void launch_counts(const Prob* d_probs, int prob, int npair, long long* d_out, hipStream_t s);
// LD clumping (k_clump.hip) on a full M x M LD matrix in device memory (an LD-only job's out_ld): one workgroup per trait.  The
// arguments travel by value; every pointer is a device pointer; rank, r2 and n_clumps may be null
struct ClumpArgs {
    const double* R;        // [M][M], both triangles
    const int* bp;          // [M], never decreasing
    const double* key;      // [n_key][M]
    int* owner;             // [n_key][M]
    int* rank;              // [n_key][M]
    double* r2;             // [n_key][M]
    int* n_clumps;          // [n_key]
    long long radius;
    double r2_min, key_index, key_member;
    int M;
};
void launch_clump(const ClumpArgs& a, int n_key, hipStream_t s);
// Optimal LD-block boundaries (k_ldsplit.hip) on a full M x M LD matrix in device memory (an LD-only job's out_ld).  W = min(max_size,
// M); every pointer is a device pointer.  Sd[d - 1][i] = S[i][i + d], SMd likewise, d = 1 .. W, pitch M; Tk[k - 1][b] = T[b][k],
// k = 1 .. min(W, b), pitch M + 1; C0 / C1 [M + 1] hold C[k - 1] and C[k] in turn; prev [max_K][M + 1]; cfin [max_K]; mx [M + 1]
struct LdSplitArgs {
    const double* R;        // [M][M], both triangles
    const int* bp;          // [M], never decreasing
    double *Sd, *SMd, *Tk;
    double *C0, *C1;
    double* cfin;
    double* mx;
    int* prev;
    unsigned long long* n_nonfinite;      // one counter, zero before the launches
    long long radius;
    double thr_r2, max_r2;
    int M, W, min_size, max_size, max_K;
};
void launch_ldsplit(const LdSplitArgs& a, hipStream_t s);      // band, cost, then max_K launches of the DP, all queued on s
// Eigen-decomposition of a block's LD and the traits' projections on it (k_hess.hip) on a full M x M LD matrix in device memory (an
// LD-only job's out_ld).  np = M rounded up to HESS_PW columns, ldn = M rounded up to HESS_RC rows; Gm and V are column-major
// [np][ldn]; zr [T][ldn] the repaired z; every pointer is a device pointer
struct HessArgs {
    const double* R;        // [M][M], both triangles
    const double* z;        // [T][M] as the caller gave it
    double *Gm, *V, *zr;
    int* mono;              // [M] 1: a monomorphic SNP (every off-diagonal entry NaN)
    double* lam;            // [M] v_j . g_j by solver column
    const int* order;       // [kk] the solver column of the i-th largest eigenvalue
    const double* lam_sorted;      // [kk]
    double* proj;           // [T][k_max]
    unsigned int* n_rot;    // one counter: block pairs rotated since it was last zeroed
    unsigned long long* n_nonfinite;      // one counter, zero before the launches
    double null2;           // (M 2^-52)^2: a column of G with a squared norm at or below it is numerically null, never rotated
    int M, np, ldn, T, kk, k_max;
};
void launch_hess_prep(const HessArgs& a, hipStream_t s);       // mono, Gm = R', V = I, zr
// the block rounds, a sweep at a time until one rotates nothing (the counter is read once per sweep: it waits for s); returns a HIP error
hipError_t hess_solve(const HessArgs& a, hipStream_t s, int* sweeps, bool* converged);
void launch_hess_lambda(const HessArgs& a, hipStream_t s);
void launch_hess_proj(const HessArgs& a, hipStream_t s);
// Gene-based sum-of-chi2 (k_sumchi2.hip) on the blocks a gene job left in out_ld: one workgroup per gene.  The arguments travel by
// value; every pointer is a device pointer and none is null
struct Sumchi2Args {
    const double* R;                // the gene job's out_ld: block g is n_g x n_g, both triangles, at gene_out_off[g]
    const int* gene_off;            // [n_gene + 1] the job's
    const long long* gene_out_off;  // [n_gene] the job's
    const double* z;                // [n_trait][n_snp]
    int* kept;                      // [n_snp] 0 / 1
    int* n_kept;                    // [n_gene]
    double* lam;                    // [n_gene][SC2_K_MAX]
    double* q;                      // [n_trait][n_gene]
    int* top;                       // [n_trait][n_gene]
    int* status;                    // [n_gene]
    int* sweeps;                    // [n_gene]
    double prune_r2;
    int n_snp, n_gene, n_trait;
    int m_lds;                      // order of the kept block the launch's dynamic LDS holds (even, <= SC2_K_MAX)
};
// max_n: the largest gene's SNP count (it sizes the dynamic LDS)
void launch_sumchi2(Sumchi2Args a, int max_n, hipStream_t s);
void launch_pack2bit(const uint8_t* d_in, long long ld_in, uint8_t* d_out, long long ld_out, int n_snp,
                     const int* d_pop_off, const int* d_blk_off, int n_pop, hipStream_t s);
void launch_h2d_copy(void* d_dst, const void* pinned_src, size_t bytes, hipStream_t s);
// Matrix exports (raw LD export / want_mats): `n` device matrices [rows x pitch] are written as compact [rows x width] doubles into the
// job's pinned export mirror by ONE kernel (the stores cross PCIe), instead of a pitched copy per matrix and a compaction on the host.
struct ExportD {
    const double* src;      // device matrix, row pitch `pitch` doubles
    double* dst;            // compact [rows x width] in the pinned mirror (device-visible host memory)
    int rows, width, pitch, pad_;
};
void launch_export_rows(const ExportD* d_exports, int n, long long max_elems, hipStream_t s);
// Population weights (k_popwgt.hip): chunk c is rows [r0, r1) of interval iv of the interval-major matrix
struct PwChunk { long long r0, r1; int iv, pad_; };
void launch_pop_weights(const double* d_x, int n_pop, const PwChunk* d_chunks, int n_chunk, const int* d_chunk_off,
                        const long long* d_off, int n_interval, double eps, double* d_part1, double* d_mean, double* d_part2,
                        double* d_w, int* d_status, hipStream_t s);
void launch_synth(uint8_t* d_out, int n_snp, long long ld, const int* d_pop_off, int n_pop,
                  int n_samples, const float* d_thr, const float* d_rho, uint64_t seed,
                  hipStream_t s);

#endif
}  // namespace gauss
