// The imputed SNPs of a window conditioned on the signals its selection found (k_slct.hip): is an imputed hit a signal of its own or
// the shadow of a selected SNP?  With B = B11 (lambda on the diagonal, MakePosDef's repair included), z = z1, S the ordered selected
// set (n = |S| <= SLCT_K), L the Cholesky factor of B_SS, y = L^-1 z_S (the selection's zin), b_u row u of B21,
// m_u = b_u B^-1 z and info_u = |b_u B^-1 b_u^T|:
//     w_u[s]     = (B21[u][sel[s]] - sum_{t < s, ascending} w_u[t] L[s][t]) / L[s][s],      L[s][t] = W[t][sel[s]]
//     cond_z_u   = (m_u - w_u . y) / sqrt(info_u - w_u . w_u)        where info_u - w_u . w_u > min_var_frac * info_u, else NaN
//     cond_var_u = (info_u - w_u . w_u) / info_u                     always
// cov(m_u, z_S) = b_u[S] under z ~ N(0, B), so the numerator's variance is info_u - b_u[S] B_SS^-1 b_u[S]^T: not 1, which is what
// conditioning an imputed z like a measured one would assume.  n = 0: cond_z_u has the bits of z_u and cond_var_u is 1.
//
// m_u = out_z[u] sqrt(out_info[u]) and info_u = out_info[u]: the kernel reads what the closing step has written, not its sums, so it
// runs unchanged behind the fused closing product and behind the stand-alone solve.  Grid = (blocks of COND_T unmeasured SNPs) x (the
// windows that asked); one thread per u.  The workgroup reads n, the indices (exact doubles) and y from the window's selection
// section, and L from the selection's W, into LDS (SLCT_K (SLCT_K + 1) + SLCT_K doubles); every lane reads the same LDS word at a
// time (a broadcast).  A thread gathers its n entries of B21 (uncoalesced 8-byte reads, U n of them), and keeps w_u in registers: the
// loops over s and t are unrolled to SLCT_K and guarded by s < n, which is the same in every lane (n sits in a scalar register), so
// no array is indexed at run time and nothing goes to scratch.  Sums in a fixed order, no atomics: the bits do not depend on the run
// or on the launch form.  Compiled with -ffp-contract=off like the other fp64 tails.
#include "gauss_internal.h"

namespace gauss {

constexpr int COND_LP = SLCT_K + 1;          // row pitch of L in LDS

__global__ __launch_bounds__(COND_T) void cond_kernel(const Prob* __restrict__ probs, const int* __restrict__ condmap)
{
    __shared__ double s_L[SLCT_K * COND_LP], s_y[SLCT_K];
    __shared__ int s_sel[SLCT_K];
    const Prob& pb = probs[condmap ? condmap[blockIdx.y] : (int)blockIdx.y];
    const int tid = threadIdx.x;
    const int M = pb.M, U = pb.U, ld = pb.Mld, K = pb.slct_max;
    if ((int)blockIdx.x * COND_T >= U) return;              // (the grid is as wide as the job's largest asking window)
    const SlctLayout o = slct_layout(M, K);
    const auto sel_out = pb.out_slct;
    const auto W = pb.slct_W;
    // n and the indices are the selection's own: whatever a run that is being replaced may have left there, nothing is read
    // outside the window's matrices
    const double nd = sel_out[o.n];
    const int n = __builtin_amdgcn_readfirstlane((nd >= 0.0 && nd <= (double)K) ? (int)nd : 0);
    if (tid < n) {
        const double jd = sel_out[o.idx + tid];
        s_sel[tid] = (jd >= 0.0 && jd < (double)M) ? (int)jd : 0;
        s_y[tid] = sel_out[o.zin + tid];
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += COND_T) {
        const int a = e / n, b = e % n;
        if (b <= a) s_L[a * COND_LP + b] = W[(size_t)b * ld + s_sel[a]];
    }
    __syncthreads();
    const int u = blockIdx.x * COND_T + tid;
    if (u >= U) return;
    const double zu = pb.out_z[u], info = pb.out_info[u];
    double cz = zu, cv = 1.0;
    if (n > 0) {
        const auto brow = pb.B21 + (size_t)u * ld;
        double b[SLCT_K], w[SLCT_K];
#pragma unroll
        for (int s = 0; s < SLCT_K; s++)
            if (s < n) b[s] = brow[s_sel[s]];
        double ww = 0.0, wy = 0.0;
#pragma unroll
        for (int s = 0; s < SLCT_K; s++)
            if (s < n) {
                double sum = 0.0;
#pragma unroll
                for (int t = 0; t < s; t++) sum += w[t] * s_L[s * COND_LP + t];
                w[s] = (b[s] - sum) / s_L[s * COND_LP + s];
                ww += w[s] * w[s];
                wy += w[s] * s_y[s];
            }
        const double left = info - ww;
        const double m = zu * sqrt(info);
        cz = left > pb.cond_min_var_frac * info ? (m - wy) / sqrt(left) : __builtin_nan("");
        cv = left / info;
    }
    pb.out_cond[u] = cz;
    pb.out_cond[(size_t)U + u] = cv;
}

void launch_cond(const Prob* d_probs, const int* d_condmap, int n, int max_U, hipStream_t s)
{
    if (n <= 0 || max_U <= 0) return;
    hipLaunchKernelGGL(cond_kernel, dim3((max_U + COND_T - 1) / COND_T, n), dim3(COND_T), 0, s, d_probs, d_condmap);
}

}  // namespace gauss
