// LD scores of the measured SNPs of an LD window, reduced where the LD step leaves its matrices: l_j = sum_k r_kj^2 over the window's
// SNPs within a radius of SNP j, the input of LD-score regression.  The M measured rows are the TARGETS (the SNPs being scored); rows
// k = 0 .. M - 1 of the concatenated row space are the measured rows (r_kj = B11[k][j], A[0], stored in full), rows M .. M + U - 1 the
// geno_u rows (r_kj = B21[k - M][j]); bp(k) = lds_bp[k].  Row k contributes to target j iff |bp(k) - bp(j)| <= lds_radius.  With
// a_0(k) = 1 and a_c(k) = lds_annot[c - 1][k] for the categories c = 1 .. C:
//     raw[c][j] = sum_k a_c(k) r_kj^2,   mass[c][j] = sum_k a_c(k),   l2 = raw (1 + 1 / (n - 2)) - mass / (n - 2)
// The definition, the outputs and the refusals: include/gauss_hip.h.
//
// The order of summation (DESIGN.md section 4 states it for a numpy restatement to replay): rows are cut into chunks of LDS_CHUNK,
// the measured rows from row 0 and the geno_u rows from row M -- a chunk never holds rows of both matrices.  A chunk's partial starts
// at 0 and takes the chunk's contributing rows in ascending order: t = r r, raw += a t, mass += a (one product each, not contracted;
// for category 0 a = 1 and a t = t exactly).  ldscore_finish_kernel starts every total at 0, adds the chunks' partials in ascending
// chunk order and forms l2 from the two totals.  Nothing here depends on the window's place in the job, on the other windows, on the
// source format of the genotype rows or on the queue the run took.  No atomics; nothing waits for another workgroup.
//
// ldscore_kernel: one wave = (LDS_COLS consecutive targets, one chunk, one category, one asking window): grid (target blocks of the
// widest window, chunks of the longest, (1 + most categories) x asking windows); a wave beyond its window's ranges leaves at once.
// Lanes run along the targets: row k of either matrix is row-major with pitch Mld, a wave reads 64 consecutive doubles of it.  A row
// outside a lane's band is not loaded by that lane (a select on the load and on the sum, never a product with 0): a non-finite r
// outside a target's band cannot reach it.  The positions are sorted inside the measured rows and inside the geno_u rows, so the band
// of the wave's targets is [bp(first) - radius, bp(last) + radius] and a chunk whose first .. last position misses it is skipped
// without reading a row; it parks zeros, which is what its partial is.  The category's weight of a row is one broadcast load.
// Memory-bound: every category reads the in-band part of B11 and B21 once (the matrices of one window stay in the 256 MB L3).
#include "gauss_internal.h"
#include <algorithm>

namespace gauss {

static_assert(LDS_COLS == 64, "a workgroup of ldscore_kernel is one wave: a lane per target");

constexpr int LDS_UNR = 8;                   // rows whose entries a lane has in flight before it sums them
constexpr int LDS_FIN_T = 256;               // threads of ldscore_finish_kernel: one per target

__global__ __launch_bounds__(LDS_COLS) void ldscore_kernel(const Prob* __restrict__ probs, const int* __restrict__ ldsmap, int max_c1)
{
    const Prob& pb = probs[ldsmap[blockIdx.z / max_c1]];
    const int cat = blockIdx.z % max_c1, chunk = blockIdx.y, j0 = blockIdx.x * LDS_COLS;
    const int M = pb.M, U = pb.U, ld = pb.Mld;
    const int cm = (M + LDS_CHUNK - 1) / LDS_CHUNK, nch = lds_chunks(M, U);
    if (cat > pb.lds_C || chunk >= nch || j0 >= M) return;          // (uniform: the whole wave leaves)
    const bool meas = chunk < cm;
    const int k0 = meas ? chunk * LDS_CHUNK : M + (chunk - cm) * LDS_CHUNK;      // rows [k0, k1) of the concatenated row space
    const int k1 = min(k0 + LDS_CHUNK, meas ? M : M + U);
    const auto bp = pb.lds_bp;
    const long long rad = pb.lds_radius;
    const int j = j0 + (int)threadIdx.x, jl = min(j0 + LDS_COLS, M) - 1;
    double raw = 0.0, mass = 0.0;
    // the chunk's positions [bp(k0), bp(k1 - 1)] against the band of the wave's targets [bp(j0) - rad, bp(jl) + rad]
    const bool touches = (long long)bp[k1 - 1] >= (long long)bp[j0] - rad && (long long)bp[k0] <= (long long)bp[jl] + rad;
    if (touches && j < M) {
        const long long bj = bp[j];
        const auto col = (meas ? pb.A + (size_t)k0 * ld : pb.B21 + (size_t)(k0 - M) * ld) + j;      // entry (k0, j); row k is (k - k0) ld further on
        const size_t a0 = cat ? (size_t)(cat - 1) * (size_t)(M + U) : 0;
        for (int k = k0; k < k1; k += LDS_UNR) {
            double r[LDS_UNR];
            bool in[LDS_UNR];
#pragma unroll
            for (int u = 0; u < LDS_UNR; u++) {
                const int kk = min(k + u, k1 - 1);
                const long long d = (long long)bp[kk] - bj;
                in[u] = k + u < k1 && d >= -rad && d <= rad;
                r[u] = in[u] ? col[(size_t)(kk - k0) * ld] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < LDS_UNR; u++)
                if (in[u]) {
                    const double a = cat ? pb.lds_annot[a0 + (size_t)(k + u)] : 1.0;
                    const double t = r[u] * r[u];
                    raw += a * t;
                    mass += a;
                }
        }
    }
    if (j < M) {
        const auto part = pb.lds_part + ((size_t)cat * nch + chunk) * 2 * (size_t)ld;
        part[j] = raw;
        part[(size_t)ld + j] = mass;
    }
}

// One thread per (target, category, asking window): the chunks' partials in ascending order, then l2 from the two totals
__global__ __launch_bounds__(LDS_FIN_T) void ldscore_finish_kernel(const Prob* __restrict__ probs, const int* __restrict__ ldsmap)
{
    const Prob& pb = probs[ldsmap[blockIdx.z]];
    const int cat = blockIdx.y, j = blockIdx.x * LDS_FIN_T + (int)threadIdx.x;
    const int M = pb.M, ld = pb.Mld, nch = lds_chunks(M, pb.U);
    if (cat > pb.lds_C || j >= M) return;
    const auto part = pb.lds_part + (size_t)cat * nch * 2 * (size_t)ld + j;
    double raw = 0.0, mass = 0.0;
    for (int c = 0; c < nch; c++) {
        raw += part[(size_t)(2 * c) * ld];
        mass += part[(size_t)(2 * c + 1) * ld];
    }
    const double nm2 = pb.lds_n - 2.0;
    const LdsLayout o = lds_layout(M, pb.lds_C);
    const size_t at = (size_t)cat * M + j;
    pb.out_lds[o.raw + at] = raw;
    pb.out_lds[o.l2 + at] = raw * (1.0 + 1.0 / nm2) - mass / nm2;
    pb.out_lds[o.mass + at] = mass;
}

void launch_ldscore(const Prob* d_probs, const int* d_ldsmap, int n, int max_M, int max_chunks, int max_C, hipStream_t s)
{
    if (n <= 0 || max_M <= 0 || max_chunks <= 0) return;
    const int c1 = 1 + max_C, per = 65535 / c1;      // (a grid's z extent ends at 65 535: more asking windows than that take further launches)
    for (int w0 = 0; w0 < n; w0 += per) {
        const int nw = std::min(per, n - w0);
        hipLaunchKernelGGL(ldscore_kernel, dim3((max_M + LDS_COLS - 1) / LDS_COLS, max_chunks, c1 * nw), dim3(LDS_COLS), 0, s, d_probs, d_ldsmap + w0, c1);
        hipLaunchKernelGGL(ldscore_finish_kernel, dim3((max_M + LDS_FIN_T - 1) / LDS_FIN_T, c1, nw), dim3(LDS_FIN_T), 0, s, d_probs, d_ldsmap + w0);
    }
}

}  // namespace gauss
