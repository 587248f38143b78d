// Stepwise conditional signal selection among the measured SNPs of an imputation window: how many independent signals the window
// holds.  With B = B11 (lambda on the diagonal, MakePosDef's repair included), z = z1 and S the ordered set of selected SNPs,
//     zc_i = (z_i - B_iS B_SS^-1 z_S) / sqrt(B_ii - B_iS B_SS^-1 B_Si)
// is the statistic of SNP i given S.  Greedy: the admissible SNP with the largest zc_i^2 enters, until the largest falls below
// chi2_stop or K SNPs are in -- a partial Cholesky factorisation of B whose pivot is the largest conditional chi^2:
//     r = z;  v = diag(B);  W = []
//     step t = 0, 1, ... < K:
//         admissible(i):  i not in S  and  v_i > min_var_frac * B_ii
//         t < n_forced:   j = forced[t]; not admissible: raise the skipped flag, next step
//         else:           j = argmax over admissible i of r_i^2 / v_i (ties: smallest i; NaN never wins); stop if none or below chi2_stop
//         sel[n] = j;  zin[n] = r_j / sqrt(v_j);  n += 1
//         w_i = (B_ji - sum_{s < n - 1, ascending} W[s][i] W[s][j]) / sqrt(v_j)      every i < M
//         r_i -= w_i zin;  v_i -= w_i w_i;  W[n - 1] = w
//     end:  zc_i = r_i / sqrt(v_i) for admissible i, NaN otherwise;  var_left_i = v_i / B_ii for every i
//           L = [W[b][sel[a]]], b <= a: the Cholesky factor of B_SS;  joint_a = (B_SS^-1 z_S)_a / sqrt((B_SS^-1)_aa)
// The collinearity guard: the ridge caps what a duplicate SNP can explain -- for two identical rows B_ij = 1 and B_ii = 1 + lambda,
// so 1 - v_i / B_ii = 1 / (1 + lambda)^2 = 0.826 at lambda = 0.1 and a plain "r^2 >= 0.9" test on that ratio would never fire.  The
// host passes min_var_frac = 1 - collin / (1 + lambda)^2: for |S| = 1 exactly "the pair's un-ridged r^2 >= collin", for larger S
// the same rule applied to the explained share.
//
// One workgroup = one window that asked; thread tid owns SNPs tid, tid + SLCT_T, ...: it alone writes their r, v and entries of W,
// and keeps their "selected" flags in one 64-bit word (M <= 64 SLCT_T, gauss_plan.cpp).  r, v and diag(B) live in LDS while
// M <= SLCT_LDS_M; beyond that r and v live in the window's zc / var_left slots of the result block and the diagonal is read
// from A[0].  Row j of A[0] (= column j: B11 is stored in full, and the factorisation leaves A[0] alone) and the rows of W are read
// coalesced over i; the n values W[s][j] go through LDS.  The argmax is a reduction of (chi^2, index) pairs by cross-lane moves
// inside a wave, then through LDS across the waves; ties go to the smaller index: no atomics, the bits and the choice do not
// depend on the run.  Wave 0 does the n x n substitutions at the end: lane a forms column a of L^-1, whose squared norm is
// (B_SS^-1)_aa and whose product with y = L^-1 z_S is (B_SS^-1 z_S)_a -- and y is zin, the forward substitution the selection
// has already done.  Every branch on j, n or the stopping rule is uniform: all threads read the same values.
// Latency-bound (K dependent steps of a few loads each); compiled with -ffp-contract=off like the other fp64 tails.
#include "gauss_internal.h"

namespace gauss {

constexpr int SLCT_LDS_M = 2048;             // r, v, diag(B) of a window of up to this many measured SNPs: 48 KB of LDS
constexpr int SLCT_NW = SLCT_T / 64;
constexpr int SLCT_LP = SLCT_K + 1;          // row pitch of the two K x K matrices of the end phase (they reuse the r / v space)
constexpr int SLCT_NONE = 0x7fffffff;
static_assert(2 * SLCT_K * SLCT_LP <= 3 * SLCT_LDS_M, "L and L^-1 fit into the space of r, v and diag(B)");
static_assert(SLCT_K <= 64 && SLCT_K <= SLCT_T, "one lane per selected SNP");

// the order of the argmax: larger chi^2 first, then the smaller index; a NaN chi^2 is never better
__device__ __forceinline__ bool slct_better(double c, int i, double c2, int i2) { return c > c2 || (c == c2 && i < i2); }

__global__ __launch_bounds__(SLCT_T) void slct_kernel(const Prob* __restrict__ probs, const int* __restrict__ slctmap)
{
    __shared__ double s_rv[3 * SLCT_LDS_M];
    __shared__ double s_wj[SLCT_K], s_zin[SLCT_K], s_redc[SLCT_NW];
    __shared__ int s_redi[SLCT_NW], s_sel[SLCT_K];
    const Prob& pb = probs[slctmap ? slctmap[blockIdx.x] : (int)blockIdx.x];
    const int tid = threadIdx.x;
    const int M = pb.M, ld = pb.Mld, K = pb.slct_max, nf = pb.n_slct_forced;
    const double stop = pb.slct_chi2_stop, mvf = pb.slct_min_var_frac;
    const auto A = pb.A;                                    // A[0] = B11
    const auto W = pb.slct_W;
    const auto out = pb.out_slct;
    const SlctLayout o = slct_layout(M, K);
    const auto o_idx = out + o.idx, o_zin = out + o.zin, o_joint = out + o.joint, o_zc = out + o.zc, o_var = out + o.var;
    const bool in_lds = M <= SLCT_LDS_M;
    double* const r = in_lds ? s_rv : (double*)o_zc;
    double* const v = in_lds ? s_rv + SLCT_LDS_M : (double*)o_var;
    double* const s_b = s_rv + 2 * SLCT_LDS_M;
    auto bii = [&](int i) { return in_lds ? s_b[i] : A[(size_t)i * ld + i]; };

    for (int i = tid; i < M; i += SLCT_T) {
        const double b = A[(size_t)i * ld + i];
        r[i] = pb.z1[i];
        v[i] = b;
        if (in_lds) s_b[i] = b;
    }
    unsigned long long mine = 0;                            // bit k: SNP tid + k SLCT_T is selected
    int n = 0, skipped = 0;
    __syncthreads();
    for (int t = 0; t < K; t++) {
        int j;
        if (t < nf) {
            j = pb.slct_forced[t];                          // (distinct and all ahead of the free steps: not selected yet)
            if (!(v[j] > mvf * bii(j))) { skipped = 1; continue; }
        } else {
            double bc = -1.0;
            int bi = SLCT_NONE;
            for (int i = tid, k = 0; i < M; i += SLCT_T, k++) {
                const double vi = v[i];
                if (((mine >> k) & 1ull) || !(vi > mvf * bii(i))) continue;
                const double c = r[i] * r[i] / vi;
                if (slct_better(c, i, bc, bi)) { bc = c; bi = i; }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double c2 = __shfl_xor(bc, off, 64);
                const int i2 = __shfl_xor(bi, off, 64);
                if (slct_better(c2, i2, bc, bi)) { bc = c2; bi = i2; }
            }
            if ((tid & 63) == 0) { s_redc[tid >> 6] = bc; s_redi[tid >> 6] = bi; }
            __syncthreads();
            bc = s_redc[0]; bi = s_redi[0];
#pragma unroll
            for (int w = 1; w < SLCT_NW; w++)
                if (slct_better(s_redc[w], s_redi[w], bc, bi)) { bc = s_redc[w]; bi = s_redi[w]; }
            if (bi == SLCT_NONE || bc < stop) break;
            j = bi;
        }
        // SNP j enters: every thread reads the pivot's r and v before the barrier, its owner rewrites them after it
        const double sq = sqrt(v[j]);
        const double zin = r[j] / sq;
        if (tid < n) s_wj[tid] = W[(size_t)tid * ld + j];
        if (tid == 0) { s_sel[n] = j; s_zin[n] = zin; o_idx[n] = (double)j; o_zin[n] = zin; }
        if (j % SLCT_T == tid) mine |= 1ull << (j / SLCT_T);
        __syncthreads();
        const auto row = A + (size_t)j * ld;
        const auto Wn = W + (size_t)n * ld;
        for (int i = tid; i < M; i += SLCT_T) {
            double sum = 0.0;
#pragma unroll 4
            for (int s = 0; s < n; s++) sum += W[(size_t)s * ld + i] * s_wj[s];
            const double w = (row[i] - sum) / sq;
            r[i] -= w * zin;
            v[i] -= w * w;
            Wn[i] = w;
        }
        n++;
        __syncthreads();
    }
    // what is left: conditional z of the admissible SNPs, the variance left of all (r and v may BE these slots: read, then written)
    for (int i = tid, k = 0; i < M; i += SLCT_T, k++) {
        const double vi = v[i], ri = r[i], b = bii(i);
        const bool adm = !((mine >> k) & 1ull) && vi > mvf * b;
        o_zc[i] = adm ? ri / sqrt(vi) : __builtin_nan("");
        o_var[i] = vi / b;
    }
    if (tid == 0) { out[o.n] = (double)n; out[o.skipped] = (double)skipped; }
    if (tid >= n && tid < K) { o_idx[tid] = -1.0; o_zin[tid] = __builtin_nan(""); o_joint[tid] = __builtin_nan(""); }
    __syncthreads();                                        // r, v and diag(B) are done with: their LDS holds L and L^-1 now
    double* const L = s_rv;                                 // L[a][b] = W[b][sel[a]], b <= a: the Cholesky factor of B_SS
    double* const X = s_rv + SLCT_K * SLCT_LP;              // X[b][a] = (L^-1)[b][a], b >= a: column a is lane a's
    for (int e = tid; e < n * n; e += SLCT_T) {
        const int a = e / n, b = e % n;
        if (b <= a) L[a * SLCT_LP + b] = W[(size_t)b * ld + s_sel[a]];
    }
    __syncthreads();
    if (tid >= n) return;
    const int a = tid;
    double x = 1.0 / L[a * SLCT_LP + a];
    double d = x * x, g = x * s_zin[a];
    X[a * SLCT_LP + a] = x;
    for (int b = a + 1; b < n; b++) {
        double sum = 0.0;
        for (int c = a; c < b; c++) sum += L[b * SLCT_LP + c] * X[c * SLCT_LP + a];
        x = -sum / L[b * SLCT_LP + b];
        X[b * SLCT_LP + a] = x;
        d += x * x;
        g += x * s_zin[b];
    }
    o_joint[a] = g / sqrt(d);
}

void launch_slct(const Prob* d_probs, const int* d_slctmap, int n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(slct_kernel, dim3(n), dim3(SLCT_T), 0, s, d_probs, d_slctmap);
}

}  // namespace gauss
