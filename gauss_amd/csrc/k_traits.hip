// Further traits on one window's LD: T more Z-score vectors measured at the window's SNPs, imputed from the B11 / B21 and the
// factorisation the window's job holds anyway.  With B = B11 (lambda on the diagonal, MakePosDef's repair included), Z the
// [M x T] matrix whose column t is trait t, and X = L^-1 (B = L L^T):
//     G    = B^-1 Z = X^T (X Z)                          [M x T]
//     Zraw = B21 G                                       [U x T]   mean_ut = b21_u . g_t          dist.cpp:193-194
//     out_traits[t][u] = Zraw[u][t] / sqrt(out_info[u])            info depends on the LD only    dist.cpp:198-202
// The fused solve has left X in pb.V (k_solve.hip): block (kb, p) of X at V[p][64 kb ..][64], lower block triangle, the diagonal
// blocks lower triangular.  What lies above the diagonal is a structural zero that may or may not have been stored, rows from M on
// are padding, and column M of [X | y] is z1's own right-hand side: none of it is read as a value -- an entry X[k][g] counts
// only for g <= k < M, everything else enters the products as an exact zero.
//
// Three launches of one shape: a workgroup of 4 waves owns 64 rows x T16 columns (T rounded up to 16) of its output, wave w the
// rows 16 w .. 16 w + 15; K runs in stages of 32 through LDS; the products run on v_mfma_f64_16x16x4_f64 (A one value per lane:
// row lane & 15, k lane >> 4; B: k lane >> 4, column lane & 15; C/D: column lane & 15, row (lane >> 4) + 4 reg -- NOT the f32
// shapes' map).
//   traits_weights_kernel, pass 0:  Y = X Z      block row kb of Y from the blocks (kb, 0 .. kb) of X
//   traits_weights_kernel, pass 1:  G = X^T Y    block row p of G from the blocks (p .. nblk - 1, p) of X, read transposed
//   traits_impute_kernel:           B21 G, divided by sqrt(out_info): a strip of 64 unmeasured SNPs, every B21 entry read once
//                                   (a trait that lacks some measured SNPs keeps its raw mean for k_traits_miss.hip, undivided)
// Pass 1 needs all of Y: the two passes are two launches, no atomics, no parked sums.  A column of the output is a chain of
// MFMAs over k in ascending order whose B operand is that column alone: trait t depends on its own Z-scores only -- not on T,
// not on the traits beside it -- and every launch form returns the same bits.  No scratch memory; 34 KB (weights) and 50 KB (product) of LDS.
#include "k_traits_common.h"      // the tiles, the MFMA chain and the two K loops, shared with k_traits_miss.hip

namespace gauss {

__global__ __launch_bounds__(256) void traits_weights_kernel(const Prob* __restrict__ probs, const int2* __restrict__ map, int pass)
{
    __shared__ __attribute__((aligned(16))) double TA[NB * TLA];
    __shared__ __attribute__((aligned(16))) double TB[TK * TLB];
    const int2 wb = map[blockIdx.x];
    const Prob& pb = probs[wb.x];
    const int blk = wb.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = pb.M, ld = pb.Mld;
    const int T16 = traits_t16(pb.traits_T), nt = T16 / 16;
    f64x4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; n++) acc[n] = f64x4{0.0, 0.0, 0.0, 0.0};

    if (pass == 0) {
        // Y[64 blk + r][t] = sum over g <= k of X[k][g] Z[g][t]: stages of 32 columns g, up to the diagonal block's last and below M
        const int n_stage = min(2 * (blk + 1), (M + TK - 1) / TK);
        for (int st = 0; st < n_stage; st++) {
            const int g0 = st * TK;
            const auto xp = pb.V + (size_t)(g0 >> 6) * ld * NR + (g0 & 63);
            for (int e = tid; e < NB * TK; e += 256) {
                const int r = e / TK, c = e % TK;
                const int k = blk * NB + r, g = g0 + c;
                const double x = xp[(size_t)k * NR + c];           // in range whatever it holds: panel <= blk < npi, k < Mld, column < NR
                TA[r * TLA + c] = (g <= k && k < M) ? x : 0.0;
            }
            traits_load_b(TB, pb.traits_Z, g0, T16, T16, tid);
            __syncthreads();
            traits_mma(acc, TA, TB, wave, lane, nt);
            __syncthreads();
        }
    } else {
        // G[64 blk + c][t] = sum over k >= g of X[k][g] Y[k][t]: stages of 32 rows k from the diagonal block down to row M
        traits_xt_y(acc, pb.V, pb.traits_Y, blk, M, ld, T16, T16, TA, TB, tid, wave, lane);
    }
    const auto out = pass == 0 ? pb.traits_Y : pb.traits_G;
#pragma unroll
    for (int n = 0; n < 4; n++) {
        if (n >= nt) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = blk * NB + 16 * wave + (lane >> 4) + 4 * r;     // the f64 shape's C/D map
            out[(size_t)row * T16 + 16 * n + (lane & 15)] = acc[n][r];
        }
    }
}

__global__ __launch_bounds__(256) void traits_impute_kernel(const Prob* __restrict__ probs, const int2* __restrict__ umap)
{
    __shared__ __attribute__((aligned(16))) double TA[NB * TLO];      // the A tile [64][TLA] of a stage, then the output tile [64][TLO]
    __shared__ __attribute__((aligned(16))) double TB[TK * TLB];
    const int2 wu = umap[blockIdx.x];
    const Prob& pb = probs[wu.x];
    const int u0 = wu.y * NB;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = pb.M, U = pb.U, ld = pb.Mld, T = pb.traits_T;
    const int T16 = traits_t16(T), nt = T16 / 16;
    f64x4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; n++) acc[n] = f64x4{0.0, 0.0, 0.0, 0.0};

    traits_b21_g(acc, pb.B21, pb.traits_G, u0, U, M, ld, T16, T16, TA, TB, tid, wave, lane);
    // through LDS, trait-major: the result block holds [T][U], a wave's accumulators hold 16 SNPs x 16 traits
    traits_acc_to_lds(acc, TA, nt, wave, lane);
    __syncthreads();
    // a trait that lacks some measured SNPs keeps its raw mean: traits_miss_apply_kernel adds its correction and divides by its own info
    const auto miss_k = pb.miss_tab ? pb.miss_tab + MissTab::k : pb.miss_tab;
    for (int e = tid; e < NB * NB; e += 256) {
        const int t = e >> 6, r = e & 63;
        const int u = u0 + r;
        if (t < T && u < U) {
            const double raw = TA[t * TLO + r];
            pb.out_traits[(size_t)t * U + u] = (miss_k && miss_k[t] > 0) ? raw : raw / sqrt(pb.out_info[u]);      // dist.cpp:200
        }
    }
}

void launch_traits_weights(const Prob* d_probs, const int2* d_map, int n_blocks, hipStream_t s)
{
    if (n_blocks <= 0) return;
    hipLaunchKernelGGL(traits_weights_kernel, dim3(n_blocks), dim3(256), 0, s, d_probs, d_map, 0);
    hipLaunchKernelGGL(traits_weights_kernel, dim3(n_blocks), dim3(256), 0, s, d_probs, d_map, 1);
}

void launch_traits_impute(const Prob* d_probs, const int2* d_umap, int n_strips, hipStream_t s)
{
    if (n_strips <= 0) return;
    hipLaunchKernelGGL(traits_impute_kernel, dim3(n_strips), dim3(256), 0, s, d_probs, d_umap);
}

}  // namespace gauss
