// Normal equations of the zmix regression (zmix(), zmix.R): over every SNP pair i < j of a problem, the row
// [y, x_1 .. x_G] = [z_i z_j, r_1(i, j) .. r_G(i, j)], r_g the genotype correlation of the pair inside group g of populations;
// rows with a non-finite entry are dropped (is.finite(rowSums(mat))); the kept rows give X^T X, X^T y, y^T y and their count.
// The per-pair correlations are never written to memory: they are formed from the per-population Gram partials that the pack
// and Gram kernels leave in the problem's slab, exactly as pop_cor_kernel / pair_cor_kernel (k_pack_epilogue.hip) form them.
//
//   zm_partial_kernel  one workgroup per Gram tile pair: the tile's entries are taken in chunks of ZM_ROWS (entry e of the
//                      128 x 128 tile, ascending); every thread forms one row of the chunk in LDS (zeros when the entry is not
//                      a pair i < j or the row is not finite), then thread k adds sum_rows x_a x_b of its upper-triangle
//                      entries (a, b) of the (G + 1) x (G + 1) cross-product over the chunk's rows in row order.  Out: one
//                      partial of (G + 1)(G + 2) / 2 doubles and one kept-row count per tile pair.
//   zm_final_kernel    the partials in tile-pair order: slice s of ZM_SLICES sums a contiguous quarter of the tile pairs in
//                      order, the slices are then added in slice order.
//
// Every sum has a fixed order and nothing is atomic: the bits do not depend on the run (the rule of k_popwgt.hip).
// Compiled with -ffp-contract=off: the correlation tails must round as pop_cor_kernel's do.
#include "gauss_internal.h"

namespace gauss {

constexpr int ZM_THREADS = 256;
constexpr int ZM_ROWS = ZM_THREADS;                    // rows of a chunk: one per thread
constexpr int ZM_MAXG = 64;                            // groups (the cap of gauss_pop_weights)
constexpr int ZM_MAXE = 9;                             // ceil(65 * 66 / 2 / 256) cross-product entries per thread
constexpr int ZM_SLICES = 4;
static_assert((TILE * TILE) % ZM_ROWS == 0, "chunks cover a tile exactly");

__device__ __forceinline__ double zm_slab_val(float v, int is_int) { return is_int ? (double)__float_as_int(v) : (double)v; }

// entry k -> (a, b), a <= b, upper triangle in row order over nc columns (column 0 is y)
__device__ __forceinline__ void zm_entry(int k, int nc, int& a, int& b)
{
    a = 0;
    while (k >= nc - a) { k -= nc - a; a++; }
    b = a + k;
}

__global__ __launch_bounds__(ZM_THREADS) void zm_partial_kernel(const Prob* __restrict__ probs, int prob, const int* __restrict__ pop_group,
                                                               int n_group, const double* __restrict__ z, double* __restrict__ part,
                                                               long long* __restrict__ part_n)
{
    extern __shared__ double rows[];                   // [ZM_ROWS][nc]
    __shared__ int s_cnt[ZM_THREADS];
    const Prob& pb = probs[prob];
    const int pair = blockIdx.x, t = threadIdx.x;
    const int ti = pb.pair_ti[pair], tj = pb.pair_tj[pair];
    const int P = pb.P, S = pb.M;
    const int nc = n_group + 1, ne = nc * (nc + 1) / 2;
    const float* tile_slab = pb.slab + (size_t)pair * pb.nseg * TILE * TILE;
    int ea[ZM_MAXE], eb[ZM_MAXE];
    double acc[ZM_MAXE];
#pragma unroll
    for (int j = 0; j < ZM_MAXE; j++) {
        ea[j] = eb[j] = 0;
        const int k = t + j * ZM_THREADS;
        if (k < ne) zm_entry(k, nc, ea[j], eb[j]);
        acc[j] = 0.0;
    }
    int kept = 0;
    double* row = rows + (size_t)t * nc;
    for (int e0 = 0; e0 < TILE * TILE; e0 += ZM_ROWS) {
        const int e = e0 + t;
        const int ri = ti * TILE + e / TILE, rj = tj * TILE + e % TILE;
        bool ok = ri < S && rj < S && ri < rj;          // i < j only; diagonal tiles hold the upper part
        if (!__syncthreads_or(ok)) continue;            // a chunk without pairs (below the diagonal, past the last row)
        if (ok) {
            const double y = z[ri] * z[rj];             // zmix.cpp:165
            row[0] = y;
            ok = isfinite(y);
            const int* sxi = pb.sx + (size_t)ri * P;
            const int* sxj = pb.sx + (size_t)rj * P;
            const int* sxxi = pb.sxx + (size_t)ri * P;
            const int* sxxj = pb.sxx + (size_t)rj * P;
            for (int g = 0; g < n_group; g++) {
                // pair_cor_kernel's expression, term by term; with one population per group it has pop_cor_kernel's bits
                // (every sum is an exact integer in fp64 and 0 + x = x, so the tails see the same operands)
                double n = 0, sumxy = 0, sumx = 0, sumy = 0, sumxsq = 0, sumysq = 0;
                for (int p = 0; p < P; p++) {
                    if ((pop_group ? pop_group[p] : p) != g) continue;
                    for (int s = pb.pop_seg0[p]; s < pb.pop_seg0[p + 1]; s++)
                        sumxy += zm_slab_val(tile_slab[(size_t)s * TILE * TILE + e], pb.gram_i8);
                    n += (double)(pb.pop_raw_off[p + 1] - pb.pop_raw_off[p]);
                    sumx += (double)sxi[p]; sumy += (double)sxj[p];
                    sumxsq += (double)sxxi[p]; sumysq += (double)sxxj[p];
                }
                const double numer = n * sumxy - sumx * sumy;                                 // util.cpp:165
                const double denor = sqrt(n * sumxsq - sumx * sumx) * sqrt(n * sumysq - sumy * sumy);   // util.cpp:166
                const double r = numer / denor;
                row[1 + g] = r;
                ok = ok && isfinite(r);
            }
        }
        if (!ok)
            for (int c = 0; c < nc; c++) row[c] = 0.0;   // a dropped row adds nothing
        kept += ok ? 1 : 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < ZM_MAXE; j++) {
            if (t + j * ZM_THREADS < ne) {
                const double* ca = rows + ea[j];
                const double* cb = rows + eb[j];
                double s = acc[j];
#pragma unroll 8
                for (int rr = 0; rr < ZM_ROWS; rr++) s = fma(ca[(size_t)rr * nc], cb[(size_t)rr * nc], s);
                acc[j] = s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < ZM_MAXE; j++) {
        const int k = t + j * ZM_THREADS;
        if (k < ne) part[(size_t)pair * ne + k] = acc[j];
    }
    s_cnt[t] = kept;
    __syncthreads();
    for (int s = ZM_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) s_cnt[t] += s_cnt[t + s];
        __syncthreads();
    }
    if (t == 0) part_n[pair] = s_cnt[0];
}

// block x: entries [64 x, 64 x + 64); wave s sums tile pairs [s n / 4, (s + 1) n / 4) in order, then the slices in order
__global__ __launch_bounds__(ZM_THREADS) void zm_final_kernel(const double* __restrict__ part, const long long* __restrict__ part_n,
                                                             int n_part, int ne, double* __restrict__ out, long long* __restrict__ out_n)
{
    __shared__ double red[ZM_SLICES][64];
    __shared__ long long red_n[ZM_SLICES];
    const int lane = threadIdx.x % 64, sl = threadIdx.x / 64;
    const int k = blockIdx.x * 64 + lane;
    const int p0 = (int)((long long)n_part * sl / ZM_SLICES), p1 = (int)((long long)n_part * (sl + 1) / ZM_SLICES);
    double s = 0.0;
    if (k < ne)
        for (int p = p0; p < p1; p++) s += part[(size_t)p * ne + k];
    red[sl][lane] = s;
    if (blockIdx.x == 0 && lane == 0) {
        long long c = 0;
        for (int p = p0; p < p1; p++) c += part_n[p];
        red_n[sl] = c;
    }
    __syncthreads();
    if (sl == 0) {
        double v = red[0][lane];
        for (int q = 1; q < ZM_SLICES; q++) v += red[q][lane];
        if (k < ne) out[k] = v;
        if (blockIdx.x == 0 && lane == 0) {
            long long c = 0;
            for (int q = 0; q < ZM_SLICES; q++) c += red_n[q];
            *out_n = c;
        }
    }
}

size_t zmix_lds_bytes(int n_group) { return sizeof(double) * (size_t)ZM_ROWS * (n_group + 1); }

void launch_zmix_normal_eq(const Prob* d_probs, int prob, int npair, const int* d_pop_group, int n_group, const double* d_z,
                           double* d_part, long long* d_part_n, double* d_out, long long* d_out_n, hipStream_t s)
{
    static DeviceOnce attr_once;
    attr_once.run([&]() {
        hipFuncSetAttribute(reinterpret_cast<const void*>(zm_partial_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)zmix_lds_bytes(ZM_MAXG));
    });
    const int ne = (n_group + 1) * (n_group + 2) / 2;
    if (npair > 0)
        hipLaunchKernelGGL(zm_partial_kernel, dim3(npair), dim3(ZM_THREADS), zmix_lds_bytes(n_group), s, d_probs, prob, d_pop_group,
                           n_group, d_z, d_part, d_part_n);
    hipLaunchKernelGGL(zm_final_kernel, dim3((ne + 63) / 64), dim3(ZM_THREADS), 0, s, d_part, d_part_n, npair, ne, d_out, d_out_n);
}

}  // namespace gauss
