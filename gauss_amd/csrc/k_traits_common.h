// Pieces shared by the further traits' kernels (k_traits.hip) and the kernels of the traits that lack some measured SNPs
// (k_traits_miss.hip): both run column groups of at most 64 through the same two products, X^T Y over the rows of X = L^-1 and
// B21 G, and must sum in the same order -- the tiles, the MFMA chain and the two K loops live here.
#pragma once
#include "gauss_internal.h"
#include "k_solve_common.h"

namespace gauss {

constexpr int TK = 32;                 // K per stage
constexpr int TLA = TK + 2;            // LDS leading dimension of the [64 rows][TK] A tile
constexpr int TLB = NB + 2;            // LDS leading dimension of the [TK][64 columns] B tile
constexpr int TLO = NB + 2;            // ... of the [64 columns][64 SNPs] output tile of the B21 product (it reuses the A tile's place)

#if defined(__HIPCC__)
// acc[n] += A (rows 16 wave .., [row][k], TLA) * B ([k][column], TLB) over one stage; nt = live 16-column tiles (wave-uniform)
__device__ __forceinline__ void traits_mma(f64x4 (&acc)[4], const double* __restrict__ A, const double* __restrict__ B, int wave, int lane, int nt)
{
    const double* ap = A + (16 * wave + (lane & 15)) * TLA + (lane >> 4);
    const double* bp = B + (lane >> 4) * TLB + (lane & 15);
#pragma unroll
    for (int k0 = 0; k0 < TK; k0 += 4) {
        const double a = ap[k0];
#pragma unroll
        for (int n = 0; n < 4; n++)
            if (n < nt) acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bp[k0 * TLB + 16 * n], acc[n], 0, 0, 0);
    }
}

// rows [k0, k0 + TK) and `ncols` columns (a multiple of 16, at most 64) of a matrix of leading dimension `ld` into the B tile; the
// tile's columns from ncols on are never read by traits_mma
template <typename P>
__device__ __forceinline__ void traits_load_b(double* __restrict__ TB, P src, int k0, int ld, int ncols, int tid)
{
    for (int e = tid; e < TK * NB; e += 256) {
        const int r = e >> 6, c = e & 63;
        if (c < ncols) TB[r * TLB + c] = src[(size_t)(k0 + r) * ld + c];
    }
}

// acc += X^T Y for the 64 columns g = 64 blk .. of X: G[g][c] = sum over k >= g of X[k][g] Y[k][c], stages of 32 rows k from the diagonal
// block down to row M.  V holds X by panels (k_traits.hip); Y = the group's first column, leading dimension yld.
template <typename PV, typename PY>
__device__ __forceinline__ void traits_xt_y(f64x4 (&acc)[4], PV V, PY Y, int blk, int M, int ld, int yld, int ncols, double* __restrict__ TA,
                                            double* __restrict__ TB, int tid, int wave, int lane)
{
    const auto xp = V + (size_t)blk * ld * NR;
    for (int k0 = blk * NB; k0 < M; k0 += TK) {
        for (int e = tid; e < TK * NB; e += 256) {
            const int r = e >> 6, c = e & 63;                  // c fastest: a row of the panel is 512 contiguous bytes
            const int k = k0 + r, g = blk * NB + c;
            const double x = xp[(size_t)k * NR + c];           // in range: k < Mld
            TA[c * TLA + r] = (g <= k && k < M) ? x : 0.0;
        }
        traits_load_b(TB, Y, k0, yld, ncols, tid);
        __syncthreads();
        traits_mma(acc, TA, TB, wave, lane, ncols / 16);
        __syncthreads();
    }
}

// acc += B21 G for the strip of 64 unmeasured SNPs from u0 on: every B21 entry read once; G = the group's first column, leading dimension gld
template <typename PB, typename PG>
__device__ __forceinline__ void traits_b21_g(f64x4 (&acc)[4], PB B21, PG G, int u0, int U, int M, int ld, int gld, int ncols,
                                             double* __restrict__ TA, double* __restrict__ TB, int tid, int wave, int lane)
{
    for (int m0 = 0; m0 < M; m0 += TK) {
        for (int e = tid; e < NB * TK; e += 256) {
            const int r = e / TK, c = e % TK;
            const int u = u0 + r, m = m0 + c;
            const double b = B21[(size_t)min(u, U - 1) * ld + m];       // m < Mld
            TA[r * TLA + c] = (u < U && m < M) ? b : 0.0;
        }
        traits_load_b(TB, G, m0, gld, ncols, tid);
        __syncthreads();
        traits_mma(acc, TA, TB, wave, lane, ncols / 16);
        __syncthreads();
    }
}

// a wave's accumulators (16 SNPs x 16 columns a tile) into the LDS output tile, column-major: [column][SNP of the strip], TLO
__device__ __forceinline__ void traits_acc_to_lds(const f64x4 (&acc)[4], double* __restrict__ TO, int nt, int wave, int lane)
{
#pragma unroll
    for (int n = 0; n < 4; n++) {
        if (n >= nt) continue;
#pragma unroll
        for (int r = 0; r < 4; r++)
            TO[(16 * n + (lane & 15)) * TLO + 16 * wave + (lane >> 4) + 4 * r] = acc[n][r];
    }
}
#endif

}  // namespace gauss
