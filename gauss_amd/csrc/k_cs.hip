// Credible sets of the signals a window's selection found (k_slct.hip): for each signal, which SNPs could be the causal one?  The
// candidates are the M measured SNPs (index 0 .. M - 1) and the U unmeasured ones (M .. M + U - 1), the latter with the variance an
// imputed SNP really has (k_cond.hip).  Notation of k_slct.hip / k_cond.hip: B = B11, z = z1, S the ordered selected set, n = |S|,
// L the Cholesky factor of B_SS (L[s][t] = W[t][sel[s]]), y = L^-1 z_S (zin), X = L^-1, P = B_SS^-1 = X^T X, beta = P z_S = X^T y.
//     measured i:    w_i = W[.][i],                       r_i = z_i - w_i . y,   v_i = B_ii - w_i . w_i,      d_i = B_ii
//     unmeasured u:  w_u = L^-1 b_u[S]^T (cond_kernel's),  r_u = m_u - w_u . y,   v_u = info_u - w_u . w_u,    d_u = 1
// are the statistics given all of S.  Signal a left out (S' = S \ {a}) is a rank-one update, with g = X^T w (g_a = (B_iS B_SS^-1)_a):
//     r' = r + g_a beta_a / P_aa,   v' = v + g_a^2 / P_aa,   zc = r' / sqrt(v'),   s = v' / d
// SNP sel[a] in its own set has zc = joint_a (the selection's bits) and v' = 1 / P_aa and is always a candidate; sel[b], b != a, is
// no candidate of set a.  Any other SNP is a candidate while v' > slct_min_var_frac B_ii and z_i finite (measured) or
// v' > cond_min_var_frac info_u, info_u > 0 and z_u finite (unmeasured).  With the causal SNP's non-centrality ~ N(0, omega),
// zc ~ N(0, 1 + omega s):
//     lbf = ( zc^2 omega s / (1 + omega s) - log1p(omega s) ) / 2            -inf for a non-candidate
//     lse_a = log sum_i exp(lbf_ia)   (max first),   pip_ia = exp(lbf_ia - lse_a)
// Candidate i is in set a iff pip_ia > 0 and the mass ranked ahead of it (larger pip; ties: smaller index) is below rho: the
// shortest prefix that reaches rho (rho = 1: every candidate with pip_ia > 0).  Per candidate: pip = 1 - prod_a (1 - pip_ia),
// set = the a of largest pip_ia among the sets that hold it (ties: smaller a; -1: none), set_pip = that pip_ia (0: none).  Per
// signal: size, mass = sum of the members' pip, lse;
// slots a >= n: size 0, mass and lse NaN.
//
// Three launches behind cond_kernel's place in the tail (they read z and info of the closing step, the selection and B21):
//   cs_lbf_kernel   grid = (blocks of CS_T candidates) x (asking windows), one thread per candidate.  The workgroup rebuilds n, the
//                   indices, y and L as cond_kernel does (same range checks), and X, beta / P_aa and P_aa in LDS; a thread keeps w in
//                   registers (loops unrolled to SLCT_K and guarded by the uniform s < n: no array indexed at run time, no scratch)
//                   and writes lbf_ia, a < n, to the window's workspace cs_lbf [K][cs_tld(T)].
//   cs_set_kernel   one workgroup per (signal, asking window): max and sum by an in-wave, then cross-wave reduction (a NaN never
//                   wins the max), pip in place, then the mass ranked ahead of every candidate counted directly, j ascending
//                   (O(T^2) compare-adds).  The row of pips sits in LDS while T <= CS_LDS_T and is read from the workspace beyond.
//                   Membership goes to the byte plane cs_mem.
//   cs_fold_kernel  one thread per candidate: pip, set, set_pip over a ascending.
// No atomics, every sum in a fixed order: the bits do not depend on the run or on the launch form.  Compiled with
// -ffp-contract=off like the other fp64 tails.
#include "gauss_internal.h"
#include "k_cs_common.h"      // the membership step of one row, shared with k_susie.hip

namespace gauss {

constexpr int CS_LP = SLCT_K + 1;            // row pitch of L and X in LDS
static_assert(SLCT_K <= CS_T && SLCT_K <= 64, "one lane per selected SNP");

// n and the indices are the selection's own; whatever a run that is being replaced may have left there, nothing is indexed outside
// the window's matrices
__device__ __forceinline__ int cs_n_of(const Prob& pb)
{
    const double nd = pb.out_slct[slct_layout(pb.M, pb.slct_max).n];
    return __builtin_amdgcn_readfirstlane((nd >= 0.0 && nd <= (double)pb.slct_max) ? (int)nd : 0);
}

__global__ __launch_bounds__(CS_T) void cs_lbf_kernel(const Prob* __restrict__ probs, const int* __restrict__ csmap)
{
    __shared__ double s_L[SLCT_K * CS_LP], s_X[SLCT_K * CS_LP], s_y[SLCT_K], s_bp[SLCT_K], s_paa[SLCT_K], s_joint[SLCT_K];
    __shared__ int s_sel[SLCT_K];
    const Prob& pb = probs[csmap ? csmap[blockIdx.y] : (int)blockIdx.y];
    const int tid = threadIdx.x;
    const int M = pb.M, U = pb.U, T = M + U, ld = pb.Mld, K = pb.slct_max;
    if ((int)blockIdx.x * CS_T >= T) return;                // (the grid is as wide as the job's largest asking window)
    const SlctLayout o = slct_layout(M, K);
    const auto sel_out = pb.out_slct;
    const auto W = pb.slct_W;
    const int n = cs_n_of(pb);
    if (n == 0) return;                                     // nothing selected: no row of lbf is read
    if (tid < n) {
        const double jd = sel_out[o.idx + tid];
        s_sel[tid] = (jd >= 0.0 && jd < (double)M) ? (int)jd : 0;
        s_y[tid] = sel_out[o.zin + tid];
        s_joint[tid] = sel_out[o.joint + tid];
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += CS_T) {
        const int a = e / n, b = e % n;
        if (b <= a) s_L[a * CS_LP + b] = W[(size_t)b * ld + s_sel[a]];
        else s_X[a * CS_LP + b] = 0.0;                      // X is lower triangular; the zeros let g run over every b < n
    }
    __syncthreads();
    if (tid < n) {
        // lane a forms column a of X = L^-1 (slct_kernel's end phase): beta_a = X[., a] . y and P_aa = |X[., a]|^2
        const int a = tid;
        double x = 1.0 / s_L[a * CS_LP + a];
        double d = x * x, g = x * s_y[a];
        s_X[a * CS_LP + a] = x;
        for (int b = a + 1; b < n; b++) {
            double sum = 0.0;
            for (int c = a; c < b; c++) sum += s_L[b * CS_LP + c] * s_X[c * CS_LP + a];
            x = -sum / s_L[b * CS_LP + b];
            s_X[b * CS_LP + a] = x;
            d += x * x;
            g += x * s_y[b];
        }
        s_bp[a] = g / d;
        s_paa[a] = d;
    }
    __syncthreads();
    const int c = blockIdx.x * CS_T + tid;
    if (c >= T) return;
    const bool meas = c < M;
    double w[SLCT_K];
    double num, var, den, floor_v;                          // r, v, d and the guard's threshold of this candidate
    bool ok = true;
    int mine = -1;                                          // measured: its place in S, -1: not selected
    if (meas) {
#pragma unroll
        for (int s = 0; s < SLCT_K; s++)
            if (s < n) w[s] = W[(size_t)s * ld + c];
        for (int s = 0; s < n; s++)
            if (s_sel[s] == c) mine = s;
        const double bii = pb.A[(size_t)c * ld + c];        // A[0] = B11 stays intact through the factorisation
        num = pb.z1[c]; var = bii; den = bii; floor_v = pb.slct_min_var_frac * bii;
        ok = isfinite(num);
    } else {
        const int u = c - M;
        const auto brow = pb.B21 + (size_t)u * ld;
        double b[SLCT_K];
#pragma unroll
        for (int s = 0; s < SLCT_K; s++)
            if (s < n) b[s] = brow[s_sel[s]];
#pragma unroll
        for (int s = 0; s < SLCT_K; s++)
            if (s < n) {
                double sum = 0.0;
#pragma unroll
                for (int t = 0; t < s; t++) sum += w[t] * s_L[s * CS_LP + t];
                w[s] = (b[s] - sum) / s_L[s * CS_LP + s];
            }
        const double zu = pb.out_z[u], info = pb.out_info[u];
        num = zu * sqrt(info); var = info; den = 1.0; floor_v = pb.cond_min_var_frac * info;
        ok = info > 0.0 && isfinite(zu);
    }
    double ww = 0.0, wy = 0.0;
#pragma unroll
    for (int s = 0; s < SLCT_K; s++)
        if (s < n) { ww += w[s] * w[s]; wy += w[s] * s_y[s]; }
    const double r = num - wy, v = var - ww;
    const double omega = pb.cs_prior_var;
    const double ninf = -__builtin_inf();
    double* const lbf = pb.cs_lbf + c;
    const size_t tld = (size_t)cs_tld(T);
    for (int a = 0; a < n; a++) {
        double g = 0.0;
#pragma unroll
        for (int b = 0; b < SLCT_K; b++)
            if (b < n) g += s_X[b * CS_LP + a] * w[b];
        const double paa = s_paa[a];
        double v1 = v + g * g / paa;
        double zc = (r + g * s_bp[a]) / sqrt(v1);
        bool cand = ok && v1 > floor_v;
        if (mine >= 0) {
            cand = mine == a;
            v1 = 1.0 / paa;
            zc = s_joint[a];
        }
        const double os = omega * (v1 / den);
        lbf[(size_t)a * tld] = cand ? 0.5 * (zc * zc * os / (1.0 + os) - log1p(os)) : ninf;
    }
}

__global__ __launch_bounds__(CS_SET_T) void cs_set_kernel(const Prob* __restrict__ probs, const int* __restrict__ csmap)
{
    __shared__ double s_row[CS_LDS_T], s_red[CS_SET_NW];
    const Prob& pb = probs[csmap ? csmap[blockIdx.y] : (int)blockIdx.y];
    const int tid = threadIdx.x, a = blockIdx.x;
    const int T = pb.M + pb.U, K = pb.slct_max;
    if (a >= K) return;
    const CsLayout o = cs_layout(T, K);
    const auto out = pb.out_cs;
    const int n = cs_n_of(pb);
    if (a >= n) {
        if (tid == 0) { out[o.size + a] = 0.0; out[o.mass + a] = __builtin_nan(""); out[o.lse + a] = __builtin_nan(""); }
        return;
    }
    const size_t tld = (size_t)cs_tld(T);
    double* const g_row = pb.cs_lbf + (size_t)a * tld;
    uint8_t* const mem = pb.cs_mem + (size_t)a * tld;
    double size, mass, lse;
    cs_set_row(g_row, mem, T, pb.cs_coverage, s_row, s_red, tid, size, mass, lse);
    if (tid == 0) { out[o.size + a] = size; out[o.mass + a] = mass; out[o.lse + a] = lse; }
}

__global__ __launch_bounds__(CS_T) void cs_fold_kernel(const Prob* __restrict__ probs, const int* __restrict__ csmap)
{
    const Prob& pb = probs[csmap ? csmap[blockIdx.y] : (int)blockIdx.y];
    const int T = pb.M + pb.U, K = pb.slct_max;
    const int c = blockIdx.x * CS_T + threadIdx.x;
    if (c >= T) return;
    const CsLayout o = cs_layout(T, K);
    const auto out = pb.out_cs;
    const int n = cs_n_of(pb);
    const size_t tld = (size_t)cs_tld(T);
    double keep = 1.0, best = 0.0;
    int set = -1;
    for (int a = 0; a < n; a++) {
        const double p = pb.cs_lbf[(size_t)a * tld + c];
        keep *= 1.0 - p;
        if (pb.cs_mem[(size_t)a * tld + c] && (set < 0 || p > best)) { set = a; best = p; }
    }
    out[o.pip + c] = n > 0 ? 1.0 - keep : 0.0;
    out[o.set + c] = (double)set;
    out[o.set_pip + c] = best;
}

void launch_cs(const Prob* d_probs, const int* d_csmap, int n, int max_T, hipStream_t s)
{
    if (n <= 0 || max_T <= 0) return;
    const dim3 cand((max_T + CS_T - 1) / CS_T, n);
    hipLaunchKernelGGL(cs_lbf_kernel, cand, dim3(CS_T), 0, s, d_probs, d_csmap);
    hipLaunchKernelGGL(cs_set_kernel, dim3(SLCT_K, n), dim3(CS_SET_T), 0, s, d_probs, d_csmap);
    hipLaunchKernelGGL(cs_fold_kernel, cand, dim3(CS_T), 0, s, d_probs, d_csmap);
}

}  // namespace gauss
