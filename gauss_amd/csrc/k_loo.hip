// Leave-one-out re-imputation of the measured SNPs of a window (the input check of summary-statistics imputation): what
// run_dist / run_distmix (dist.cpp:129-227, distmix.cpp:138-253) return for measured SNP i when it is presented as the only
// unmeasured SNP and the other M - 1 are the measured set.  With B = B11 (lambda on the diagonal, MakePosDef's repair included),
// b = B[i, -i], B' = B[-i, -i], and the rank-one downdate of B^-1:
//     d_i = (B^-1)_ii,  g_i = (B^-1 z1)_i
//     mean_i     = b B'^-1 z1[-i]        = z1_i - g_i / d_i
//     loo_info_i = |b B'^-1 b^T|         = |B_ii - 1 / d_i|          dist.cpp:198
//     loo_z_i    = mean_i / sqrt(loo_info_i)                        dist.cpp:200
//     loo_t_i    = (z1_i - mean_i) sqrt(d_i) = g_i / sqrt(d_i)      the standardised residual, N(0, 1) under z1 ~ N(0, B)
// The fused solve has left [X | y] = L^-1 [I | z1] in pb.V (k_solve.hip): d = column norms^2 of X, g = X^T y -- one triangular
// pass over X, no factorisation per SNP.
//
// One workgroup = one 64-column panel of X of one window that asked: 256 threads = 64 columns x 4 row groups.  Thread (c, r)
// walks rows k = 64 p + r, + 4, ... < M of V[p][k][c] (a row of the panel is 512 contiguous bytes across the 64 lanes; y[k]
// is one address per wave).  X is lower triangular: entries above the diagonal of the panel's first block are structural
// zeros and are not read (whether ride_fin stored them or not does not matter), blocks above the panel do not exist.  The four
// row groups meet in LDS and are added in group order: no atomics, the bits do not depend on the run.  Compiled with
// -ffp-contract=off like the other fp64 tails.
#include "gauss_internal.h"

namespace gauss {

constexpr int LOO_RG = 256 / NR;      // row groups
constexpr int LOO_UNR = 8;            // rows a thread requests before it adds them up (in row order)

__global__ __launch_bounds__(256) void loo_kernel(const Prob* __restrict__ probs, const int2* __restrict__ loomap)
{
    __shared__ double red[2][LOO_RG][NR];
    const int2 wp = loomap[blockIdx.x];
    const Prob& pb = probs[wp.x];
    const int p = wp.y;
    const int tid = threadIdx.x, c = tid % NR, rg = tid / NR;
    const int M = pb.M, ld = pb.Mld;
    const int g = p * NR + c;                                          // the SNP: column g of X
    const bool live = g < M;                                           // (the last panel also holds the z1 column and padding)
    const auto X = pb.V + (size_t)p * ld * NR + c;
    const auto Y = pb.V + (size_t)(M / NR) * ld * NR + (M % NR);       // y = L^-1 z1: column M of [X | y], every row stored
    double sxx = 0.0, sxy = 0.0;
    if (live) {
        for (int k0 = p * NR + rg; k0 < M; k0 += LOO_RG * LOO_UNR) {
            double x[LOO_UNR], y[LOO_UNR];
#pragma unroll
            for (int u = 0; u < LOO_UNR; u++) {
                const int k = k0 + LOO_RG * u;
                const bool in = k < M && k >= g;
                x[u] = in ? X[(size_t)k * NR] : 0.0;
                y[u] = in ? Y[(size_t)k * NR] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < LOO_UNR; u++) { sxx += x[u] * x[u]; sxy += x[u] * y[u]; }
        }
    }
    red[0][rg][c] = sxx;
    red[1][rg][c] = sxy;
    __syncthreads();
    if (rg != 0 || !live) return;
    double d = 0.0, gg = 0.0;
#pragma unroll
    for (int r = 0; r < LOO_RG; r++) { d += red[0][r][c]; gg += red[1][r][c]; }
    const double bii = pb.A[(size_t)g * ld + g];                       // A[0] = B11 stays intact through the factorisation
    const double mean = pb.z1[g] - gg / d;
    double info = fabs(bii - 1.0 / d);                                 // dist.cpp:198
    double z = mean / sqrt(info);                                      // dist.cpp:200
    const double t = gg / sqrt(d);
    if (M == 1) { info = 0.0; z = __builtin_nan(""); }                 // nothing to impute from: b is empty, 0 / sqrt(0)
    pb.out_loo[g] = z;
    pb.out_loo[(size_t)M + g] = info;
    pb.out_loo[(size_t)2 * M + g] = t;
}

void launch_loo(const Prob* d_probs, const int2* d_loomap, int n_panels, hipStream_t s)
{
    if (n_panels <= 0) return;
    hipLaunchKernelGGL(loo_kernel, dim3(n_panels), dim3(256), 0, s, d_probs, d_loomap);
}

}  // namespace gauss
