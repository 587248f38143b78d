// Optimal LD-block boundaries on the LD matrix an LD-only job left in HBM: the split of a region's M SNPs into K contiguous blocks of
// min_size .. max_size SNPs that minimises the sum of r^2 over the pairs that land in different blocks, for every K = 1 .. max_K at
// once.  The rule, the outputs and the refusals: include/gauss_hip.h (gauss_ld_split_rows).  W = min(max_size, M).  Three kernels,
// queued behind the job on its stream; the launch boundary is the only synchronisation, nothing waits for another workgroup.
//
// ldsplit_band_kernel: the row suffix sums.  For i < j the pair is in the band iff j - i < W and bp_j - bp_i <= radius; its value is
// e = r * r (one rounded product), taken as 0 in the sum where e < thr_r2, and as 0 everywhere where r is not finite (counted).
//     S[i][b]  = S[i][b + 1] + e_ib       from one past the row's last band column down to b = i + 1, strictly in that order
//     SM[i][b] = max(SM[i][b + 1], e_ib)  over the un-thresholded e
// One workgroup = one wave = LDSPLIT_ROWS = 64 consecutive rows, lane = row.  The row's band is walked from its far end in chunks of
// LDSPLIT_OFFS = 64 offsets d = j - i: the chunk's parallelogram of the upper triangle -- row i0 + r, columns i0 + r + d0 .. + 63 -- is
// read once, one coalesced 512-byte run per row, into LDS at [r][d - d0] with a row pitch of 65 doubles (lane r reads [r][l]: bank
// 2 (r + l) mod 64 of ds_read_b64's 64, no two lanes of a 32-lane group on one bank; the stores are contiguous), 33 KB.  Then every lane
// steps through the chunk's offsets from the largest down with its S and SM in registers and stores them offset-major,
// Sd[d - 1][i] = S[i][i + d]: for one d the 64 lanes store 64 consecutive doubles.  An entry outside the row's band is neither loaded
// nor read from LDS (a select on d <= dmax_i, not a product with 0).  Non-finite entries: a count per lane, summed over the wave by
// cross-lane moves, one integer atomic per workgroup (the count does not depend on the order).
//
// ldsplit_cost_kernel: one thread per boundary b; T[b][k] = T[b][k - 1] + S[b - k][b], k = 1 .. min(W, b), sequential in k, stored
// size-major (Tk[k - 1][b]); Mx[b] = max over k of SM[b - k][b].  For one k consecutive threads read consecutive words of Sd[k - 1].
// It also sets C[0][.] (0 at b = 0, +inf elsewhere).
//
// ldsplit_dp_kernel, one launch per k = 1 .. max_K: C[k][b] = min over the block sizes s = min_size .. min(max_size, b) of
// C[k - 1][b - s] + T[b][s], ties to the smaller a = b - s; +inf (and P = -1) where no candidate is finite or where b < M is not
// admissible (Mx[b] > max_r2).  A workgroup takes LDSPLIT_DP_B = 64 consecutive b, lane = b; its LDSPLIT_DP_NW = 16 waves share the
// sizes (wave w: the w-th, w + 16-th, ... of the sizes that k - 1 blocks can precede), so both C[k - 1][b - s] and Tk[s - 1][b] are 64
// consecutive doubles per wave and step; the waves' (value, a) pairs meet in LDS.  One addition per candidate and an exact min under a total order: C and P do not depend on how
// the candidates are shared.  Compiled with -ffp-contract=off: S + r * r stays a product and a sum.
#include "gauss_internal.h"

namespace gauss {

constexpr int LDSPLIT_PITCH = LDSPLIT_OFFS + 1;
constexpr int LDSPLIT_NONE = 0x7fffffff;
static_assert(LDSPLIT_ROWS == 64, "ldsplit_band_kernel: one row per lane of one wave");
static_assert(LDSPLIT_DP_B == 64, "ldsplit_dp_kernel: one boundary per lane");
static_assert((LDSPLIT_PITCH & 1) == 1, "an odd pitch in doubles keeps a wave's column reads off one bank");

__global__ __launch_bounds__(LDSPLIT_ROWS) void ldsplit_band_kernel(const LdSplitArgs a)
{
    __shared__ double s_tile[LDSPLIT_ROWS * LDSPLIT_PITCH];
    __shared__ int s_dmax[LDSPLIT_ROWS];
    const int lane = threadIdx.x, M = a.M, W = a.W;
    const int i0 = blockIdx.x * LDSPLIT_ROWS, i = i0 + lane;
    const int D = W - 1;                                    // the largest offset of any band (j - i < W; W <= M)
    const auto R = G(a.R);
    const auto bp = G(a.bp);
    const auto Sd = G(a.Sd);
    const auto SMd = G(a.SMd);
    const double thr = a.thr_r2;
    const size_t Ms = (size_t)M;

    int dmax = 0;                                           // the largest offset of row i's band: one past its last column is i + dmax + 1
    if (i < M) {
        const long long lim = (long long)bp[i] + a.radius;
        int lo = i + 1, hi = min(i + W, M);
        while (lo < hi) { const int m = (lo + hi) >> 1; if ((long long)bp[m] <= lim) lo = m + 1; else hi = m; }
        dmax = lo - i - 1;
        Sd[(size_t)(W - 1) * Ms + i] = 0.0;                 // offset W is outside every band
        SMd[(size_t)(W - 1) * Ms + i] = 0.0;
    }
    s_dmax[lane] = dmax;
    double s = 0.0, mx = 0.0;
    unsigned cnt = 0;
    __syncthreads();
    for (int c = (D + LDSPLIT_OFFS - 1) / LDSPLIT_OFFS - 1; c >= 0; c--) {
        const int d0 = 1 + c * LDSPLIT_OFFS;
        const int dl = d0 + lane;
#pragma unroll 8
        for (int r = 0; r < LDSPLIT_ROWS; r++) {
            const int ir = i0 + r;
            if (ir < M && dl <= s_dmax[r])                  // (dmax <= M - 1 - ir: the column is inside the matrix)
                s_tile[r * LDSPLIT_PITCH + lane] = R[(size_t)ir * Ms + (size_t)(ir + dl)];
        }
        __syncthreads();
        for (int l = min(LDSPLIT_OFFS, D - d0 + 1) - 1; l >= 0; l--) {
            const int d = d0 + l;
            if (d <= dmax) {
                const double r = s_tile[lane * LDSPLIT_PITCH + l];
                if (isfinite(r)) {
                    const double e = r * r;
                    s = s + (e < thr ? 0.0 : e);
                    mx = e > mx ? e : mx;
                } else cnt++;
            }
            if (i < M) {
                Sd[(size_t)(d - 1) * Ms + i] = s;
                SMd[(size_t)(d - 1) * Ms + i] = mx;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0 && cnt) atomicAdd(a.n_nonfinite, (unsigned long long)cnt);
}

__global__ __launch_bounds__(LDSPLIT_COST_T) void ldsplit_cost_kernel(const LdSplitArgs a)
{
    const int M = a.M, W = a.W;
    const int b = blockIdx.x * LDSPLIT_COST_T + threadIdx.x;
    if (b > M) return;
    const auto Sd = G(a.Sd);
    const auto SMd = G(a.SMd);
    const auto Tk = G(a.Tk);
    if (b == 0) { G(a.mx)[0] = 0.0; G(a.C0)[0] = 0.0; return; }
    G(a.C0)[b] = __builtin_inf();
    const size_t Ms = (size_t)M, Mp = (size_t)M + 1;
    const int kmax = min(W, b);
    double t = 0.0, mx = 0.0;
#pragma unroll 8
    for (int k = 1; k <= kmax; k++) {
        const size_t at = (size_t)(k - 1) * Ms + (size_t)(b - k);
        t = t + Sd[at];
        const double m = SMd[at];
        mx = m > mx ? m : mx;
        Tk[(size_t)(k - 1) * Mp + b] = t;
    }
    G(a.mx)[b] = mx;
}

// the order of the min: the smaller value first, then the smaller a
__device__ __forceinline__ bool ldsplit_better(double v, int p, double v2, int p2) { return v < v2 || (v == v2 && p < p2); }

__global__ __launch_bounds__(LDSPLIT_DP_B * LDSPLIT_DP_NW) void ldsplit_dp_kernel(const LdSplitArgs a, const int k, const double* c_prev, double* c_cur)
{
    __shared__ double s_v[LDSPLIT_DP_NW][LDSPLIT_DP_B];
    __shared__ int s_a[LDSPLIT_DP_NW][LDSPLIT_DP_B];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, M = a.M;
    const int b = 1 + blockIdx.x * LDSPLIT_DP_B + lane;
    const size_t Mp = (size_t)M + 1;
    const auto Cp = G(c_prev);
    const auto Tk = G(a.Tk);
    double bv = __builtin_inf();
    int ba = LDSPLIT_NONE;
    if (b <= M) {
        // a = b - s >= 0, and no block holds more than M SNPs; C[k - 1][a] is finite only where k - 1 blocks can end, a in
        // [(k - 1) min_size, (k - 1) max_size]: the sizes outside that are not read (they are +inf, which never wins and never ties a
        // finite value, and where every candidate is +inf the outcome is +inf and -1 whichever was looked at)
        const int s_lo = max(a.min_size, b - (k - 1) * a.max_size), s_hi = min(min(a.W, b), b - (k - 1) * a.min_size);
#pragma unroll 4
        for (int s = s_lo + w; s <= s_hi; s += LDSPLIT_DP_NW) {
            const double v = Cp[b - s] + Tk[(size_t)(s - 1) * Mp + b];
            if (ldsplit_better(v, b - s, bv, ba)) { bv = v; ba = b - s; }
        }
    }
    s_v[w][lane] = bv; s_a[w][lane] = ba;
    __syncthreads();
    if (w != 0 || b > M) return;
#pragma unroll
    for (int q = 1; q < LDSPLIT_DP_NW; q++)
        if (ldsplit_better(s_v[q][lane], s_a[q][lane], bv, ba)) { bv = s_v[q][lane]; ba = s_a[q][lane]; }
    const bool open = b == M || G(a.mx)[b] <= a.max_r2;     // a boundary inside the region that no band pair above max_r2 spans
    if (!open || !(bv < __builtin_inf())) { bv = __builtin_inf(); ba = -1; }
    G(c_cur)[b] = bv;
    G(a.prev)[(size_t)(k - 1) * Mp + b] = ba;
    if (b == M) G(a.cfin)[k - 1] = bv;
    if (b == 1) { G(c_cur)[0] = __builtin_inf(); G(a.prev)[(size_t)(k - 1) * Mp] = -1; }      // no block ends at 0
}

void launch_ldsplit(const LdSplitArgs& a, hipStream_t s)
{
    if (a.M <= 0 || a.W <= 0 || a.max_K <= 0) return;
    hipLaunchKernelGGL(ldsplit_band_kernel, dim3((a.M + LDSPLIT_ROWS - 1) / LDSPLIT_ROWS), dim3(LDSPLIT_ROWS), 0, s, a);
    hipLaunchKernelGGL(ldsplit_cost_kernel, dim3((a.M + 1 + LDSPLIT_COST_T - 1) / LDSPLIT_COST_T), dim3(LDSPLIT_COST_T), 0, s, a);
    const double* prev = a.C0;
    double* cur = a.C1;
    for (int k = 1; k <= a.max_K; k++) {
        hipLaunchKernelGGL(ldsplit_dp_kernel, dim3((a.M + LDSPLIT_DP_B - 1) / LDSPLIT_DP_B), dim3(LDSPLIT_DP_B * LDSPLIT_DP_NW), 0, s, a, k, prev, cur);
        double* const t = const_cast<double*>(prev);
        prev = cur;
        cur = t;
    }
}

}  // namespace gauss
