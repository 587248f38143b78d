// Further traits that lack some of the window's measured SNPs (gauss_window_desc.miss_more): per-trait quality control drops a
// handful of SNPs from every trait's file, and the answer for a trait that lacks the set D (|D| = k <= 32) is a rank-k downdate of
// what the window's job holds -- no factorisation per trait.  With B = B11 (lambda on the diagonal, MakePosDef's repair included),
// A = B^-1 = X^T X (X = L^-1), z0 the trait's Z-scores with zeros on D, g0 = A z0 (column t of traits_G, k_traits.hip), b_u row u
// of B21, y_u = A b_u^T and L_D L_D^T = A_DD:
//     c         = -A_DD^-1 g0_D                                     the conditional mean of the missing SNPs themselves
//     mean_u    = b_u . g0 + sum_{d in D} y_u[d] c_d                 b_u . g0: the raw mean traits_impute_kernel leaves undivided
//     info_ut   = | info_u - || L_D^-1 y_u[D] ||^2 |                 info_u = |b_u . y_u| is the window's own
//     z_ut      = mean_u / sqrt(info_ut)                             dist.cpp:194-202
//     for d in D:  info_dt = | B_dd - (A_DD^-1)_dd |,  z_dt = c_d / sqrt(info_dt)          (k_loo.hip is the case k = 1)
// which is what run_dist / run_distmix return for that trait alone on the measured set without D, the SNPs of D unmeasured.
//
// E = the window's distinct missing SNPs (at most 128, ascending; E16 = |E| rounded up to 16).  Five launches:
//   traits_miss_cols_kernel, pass 0   Y_E = X e_d: column d of X gathered, rows below M (the unit column through the weights' pass 0
//                                     is the same bits: one product by 1.0 and exact zeros)
//   traits_miss_cols_kernel, pass 1   A[:, E] = X^T Y_E, in column groups of 64 through k_traits.hip's X^T Y loop
//   traits_miss_solve_kernel          one wave per (window, trait that lacks some): A_DD gathered into LDS, its Cholesky factor, c, the
//                                     diagonal of A_DD^-1 (column norms of L_D^-1), the section of the missing SNPs; L_D and c stay in
//                                     miss_LD for the apply step
//   -- the closing step and traits_impute_kernel run here --
//   traits_miss_product_kernel        (B21 A[:, E])^T -> miss_YU [E16][U], k_traits.hip's B21 G loop
//   traits_miss_apply_kernel          per strip of 64 unmeasured SNPs, a wave per trait and a lane per SNP: the forward substitution with
//                                     L_D (from LDS; fully unrolled, v[] stays in registers), the sum of squares, the mean, the division;
//                                     then the info rows of the traits that lack nothing (the bits of out_info)
// Every sum runs in ascending order in one thread or one MFMA chain, no atomics: a trait's values depend on its own scores and its own
// mask row only -- not on T, not on the other traits' masks, not on |E| (a column of A[:, E] is a chain of MFMAs whose B operand is that
// column alone; where it lies in the matrix changes an address, not a sum).  Compiled with -ffp-contract=off like the other fp64 tails.
#include "k_traits_common.h"

namespace gauss {

__global__ __launch_bounds__(256) void traits_miss_cols_kernel(const Prob* __restrict__ probs, const int2* __restrict__ map, int pass)
{
    __shared__ __attribute__((aligned(16))) double TA[NB * TLA];
    __shared__ __attribute__((aligned(16))) double TB[TK * TLB];
    const int2 wb = map[blockIdx.x];
    const Prob& pb = probs[wb.x];
    const int blk = wb.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = pb.M, ld = pb.Mld;
    const int E16 = traits_t16(pb.miss_E);
    if (pass == 0) {
        // Y_E[k][e] = X[k][d], d = E[e] <= k < M, else 0: block (kb, p) of X lies at V[p][64 kb ..][64] (k_traits.hip)
        const auto E = pb.miss_tab + MissTab::e;
        for (int i = tid; i < NB * E16; i += 256) {
            const int k = blk * NB + i / E16, e = i % E16;
            const int d = E[e];                                         // -1 beyond miss_E
            double x = 0.0;
            if (d >= 0 && d <= k && k < M) x = pb.V[((size_t)(d >> 6) * ld + k) * NR + (d & 63)];      // panel d / 64 <= blk < npi, k < Mld
            pb.miss_YE[(size_t)k * E16 + e] = x;
        }
        return;
    }
    for (int c0 = 0; c0 < E16; c0 += NB) {                              // column groups of at most 64
        const int ncols = min(NB, E16 - c0), nt = ncols / 16;
        f64x4 acc[4];
#pragma unroll
        for (int n = 0; n < 4; n++) acc[n] = f64x4{0.0, 0.0, 0.0, 0.0};
        traits_xt_y(acc, pb.V, pb.miss_YE + c0, blk, M, ld, E16, ncols, TA, TB, tid, wave, lane);
#pragma unroll
        for (int n = 0; n < 4; n++) {
            if (n >= nt) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = blk * NB + 16 * wave + (lane >> 4) + 4 * r;     // the f64 shape's C/D map; row < Mld
                pb.miss_AE[(size_t)row * E16 + c0 + 16 * n + (lane & 15)] = acc[n][r];
            }
        }
    }
}

constexpr int MLS = MISS_K + 1;        // LDS leading dimension of the k x k matrices of the solve

// one wave per (window, trait that lacks some SNPs); lane j < k owns row / column j
__global__ __launch_bounds__(64) void traits_miss_solve_kernel(const Prob* __restrict__ probs, const int2* __restrict__ tmap)
{
    __shared__ double L[MISS_K * MLS];         // A_DD, then its Cholesky factor (lower triangle)
    __shared__ double Li[MISS_K * MLS];        // L^-1 (lower triangle), column j written and read by lane j alone
    __shared__ double rhs[MISS_K], sol[MISS_K];
    const int2 wt = tmap[blockIdx.x];
    const Prob& pb = probs[wt.x];
    const auto tab = pb.miss_tab;
    const int t = tab[MissTab::masked + wt.y];
    const int k = tab[MissTab::k + t];                                  // 1 .. MISS_K
    const auto idx = tab + MissTab::idx + t * MISS_K;
    const auto pos = tab + MissTab::pos + t * MISS_K;
    const int tid = threadIdx.x;
    const int ld = pb.Mld, E16 = traits_t16(pb.miss_E), T16 = traits_t16(pb.traits_T);
    for (int e = tid; e < k * k; e += 64) {
        const int i = e / k, j = e % k;
        if (j <= i) L[i * MLS + j] = pb.miss_AE[(size_t)idx[i] * E16 + pos[j]];      // idx < M <= Mld, pos < miss_E <= E16
    }
    if (tid < k) rhs[tid] = pb.traits_G[(size_t)idx[tid] * T16 + t];    // g0_D
    __syncthreads();
    // Cholesky, right-looking, in place
    for (int j = 0; j < k; j++) {
        if (tid == j) L[j * MLS + j] = sqrt(L[j * MLS + j]);
        __syncthreads();
        if (tid > j && tid < k) L[tid * MLS + j] = L[tid * MLS + j] / L[j * MLS + j];
        __syncthreads();
        if (tid > j && tid < k)
            for (int c = j + 1; c <= tid; c++) L[tid * MLS + c] -= L[tid * MLS + j] * L[c * MLS + j];
        __syncthreads();
    }
    // L w = g0_D, then L^T x = w: c = -x
    for (int j = 0; j < k; j++) {
        if (tid == j) sol[j] = rhs[j] / L[j * MLS + j];
        __syncthreads();
        if (tid > j && tid < k) rhs[tid] -= L[tid * MLS + j] * sol[j];
        __syncthreads();
    }
    if (tid < k) rhs[tid] = sol[tid];
    __syncthreads();
    for (int j = k - 1; j >= 0; j--) {
        if (tid == j) sol[j] = rhs[j] / L[j * MLS + j];
        __syncthreads();
        if (tid < j) rhs[tid] -= L[j * MLS + tid] * sol[j];
        __syncthreads();
    }
    // column tid of L^-1 and its norm^2 = (A_DD^-1)_dd
    if (tid < k) {
        double dd = 0.0;
        for (int i = tid; i < k; i++) {
            double s = i == tid ? 1.0 : 0.0;
            for (int m = tid; m < i; m++) s -= L[i * MLS + m] * Li[m * MLS + tid];
            const double x = s / L[i * MLS + i];
            Li[i * MLS + tid] = x;
            dd += x * x;
        }
        const int d = idx[tid];
        const double c = -sol[tid];
        const double info = fabs(pb.A[(size_t)d * ld + d] - dd);        // A[0] = B11 stays intact through the factorisation; dist.cpp:198
        pb.out_traits_miss[tab[MissTab::off + t] + tid] = c / sqrt(info);           // dist.cpp:200
        pb.out_traits_miss[(size_t)pb.miss_n + tab[MissTab::off + t] + tid] = info;
        const auto keep = pb.miss_LD + (size_t)wt.y * MISS_LD;
        for (int j = 0; j <= tid; j++) keep[tid * MISS_K + j] = L[tid * MLS + j];
        keep[MISS_K * MISS_K + tid] = c;
    }
}

__global__ __launch_bounds__(256) void traits_miss_product_kernel(const Prob* __restrict__ probs, const int2* __restrict__ umap)
{
    __shared__ __attribute__((aligned(16))) double TA[NB * TLO];      // the A tile [64][TLA] of a stage, then the output tile [64][TLO]
    __shared__ __attribute__((aligned(16))) double TB[TK * TLB];
    const int2 wu = umap[blockIdx.x];
    const Prob& pb = probs[wu.x];
    if (pb.miss_nm == 0) return;                                       // (a mask without a set bit: nothing to multiply; block-uniform)
    const int u0 = wu.y * NB;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = pb.M, U = pb.U, ld = pb.Mld;
    const int E16 = traits_t16(pb.miss_E);
    for (int c0 = 0; c0 < E16; c0 += NB) {
        const int ncols = min(NB, E16 - c0);
        f64x4 acc[4];
#pragma unroll
        for (int n = 0; n < 4; n++) acc[n] = f64x4{0.0, 0.0, 0.0, 0.0};
        traits_b21_g(acc, pb.B21, pb.miss_AE + c0, u0, U, M, ld, E16, ncols, TA, TB, tid, wave, lane);
        traits_acc_to_lds(acc, TA, ncols / 16, wave, lane);
        __syncthreads();
        for (int e = tid; e < NB * NB; e += 256) {
            const int c = e >> 6, r = e & 63;
            const int u = u0 + r;
            if (c < ncols && u < U) pb.miss_YU[(size_t)(c0 + c) * U + u] = TA[c * TLO + r];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void traits_miss_apply_kernel(const Prob* __restrict__ probs, const int2* __restrict__ umap)
{
    __shared__ double Lw[4][MISS_K * MISS_K];       // per wave: the trait's L_D, row-major lower triangle
    __shared__ double cw[4][MISS_K];
    __shared__ int pw[4][MISS_K];
    const int2 wu = umap[blockIdx.x];
    const Prob& pb = probs[wu.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int U = pb.U, T = pb.traits_T, nm = pb.miss_nm;
    const int u = wu.y * NB + lane;
    const auto tab = pb.miss_tab;
    // every wave walks the same number of rounds (the barriers are the workgroup's); wave w takes the round's trait s0 + w
    for (int s0 = 0; s0 < nm; s0 += 4) {
        const int s = s0 + wave;
        const bool live = s < nm;                                      // wave-uniform
        int t = 0, k = 0;
        if (live) {
            t = tab[MissTab::masked + s];
            k = tab[MissTab::k + t];
            const auto keep = pb.miss_LD + (size_t)s * MISS_LD;
            for (int e = lane; e < k * MISS_K; e += 64) Lw[wave][e] = keep[e];      // (above the diagonal: never read)
            if (lane < k) { cw[wave][lane] = keep[MISS_K * MISS_K + lane]; pw[wave][lane] = tab[MissTab::pos + t * MISS_K + lane]; }
        }
        __syncthreads();
        if (live && u < U) {
            const double* __restrict__ Lt = Lw[wave];
            double v[MISS_K];
            double ss = 0.0, corr = 0.0;
#pragma unroll
            for (int j = 0; j < MISS_K; j++) {
                if (j < k) {                                           // wave-uniform
                    const double y = pb.miss_YU[(size_t)pw[wave][j] * U + u];       // y_u[d_j]; consecutive lanes, consecutive addresses
                    double a = y;
#pragma unroll
                    for (int i = 0; i < j; i++) a -= Lt[j * MISS_K + i] * v[i];
                    v[j] = a / Lt[j * MISS_K + j];
                    ss += v[j] * v[j];
                    corr += y * cw[wave][j];
                }
            }
            const double mean = pb.out_traits[(size_t)t * U + u] + corr;             // the raw mean b_u . g0 (traits_impute_kernel)
            const double info = fabs(pb.out_info[u] - ss);                            // dist.cpp:198
            pb.out_traits[(size_t)t * U + u] = mean / sqrt(info);                    // dist.cpp:200
            pb.out_traits_info[(size_t)t * U + u] = info;
        }
        __syncthreads();
    }
    // a trait that lacks nothing: the window's own info
    for (int e = tid; e < T * NB; e += 256) {
        const int t = e >> 6, uu = wu.y * NB + (e & 63);
        if (uu < U && tab[MissTab::k + t] == 0) pb.out_traits_info[(size_t)t * U + uu] = pb.out_info[uu];
    }
}

void launch_traits_miss_solve(const Prob* d_probs, const int2* d_map, int n_blocks, const int2* d_tmap, int n_traits, hipStream_t s)
{
    if (n_blocks <= 0 || n_traits <= 0) return;
    hipLaunchKernelGGL(traits_miss_cols_kernel, dim3(n_blocks), dim3(256), 0, s, d_probs, d_map, 0);
    hipLaunchKernelGGL(traits_miss_cols_kernel, dim3(n_blocks), dim3(256), 0, s, d_probs, d_map, 1);
    hipLaunchKernelGGL(traits_miss_solve_kernel, dim3(n_traits), dim3(64), 0, s, d_probs, d_tmap);
}

void launch_traits_miss_apply(const Prob* d_probs, const int2* d_umap, int n_strips, hipStream_t s)
{
    if (n_strips <= 0) return;
    hipLaunchKernelGGL(traits_miss_product_kernel, dim3(n_strips), dim3(256), 0, s, d_probs, d_umap);
    hipLaunchKernelGGL(traits_miss_apply_kernel, dim3(n_strips), dim3(256), 0, s, d_probs, d_umap);
}

}  // namespace gauss
