// Population weights from allele frequencies (afmix() / cpw2(), afmix.cpp:114-215 / cpw2.cpp:110-211): for every interval
// of SNPs, the sample covariance of the columns [af1study, AF_pop0 .. AF_pop(P-1)], MakePosDef on the P x P block Cxx
// (util.cpp:302-318) and W_i = Cxx^-1 Cxy.  fp64 throughout, plain FMA code (the work is ~(P+1)^2 S flops).
//
//   pw_colsum_kernel   one workgroup per chunk: column sums of the chunk's rows
//   pw_mean_kernel     one workgroup per interval: the chunks' sums in chunk order / n  (CalCov's x.mean())
//   pw_cross_kernel    one workgroup per chunk: sum over rows of (x_a - mean_a)(x_b - mean_b), a <= b  (two-pass, util.cpp:205-213)
//   pw_solve_kernel    one workgroup per interval: the chunks' cross sums in chunk order / (n - 1), a parallel cyclic Jacobi
//                      eigen-clamp of Cxx in LDS, a Cholesky solve
//
// A chunk is at most PW_CHUNK rows of ONE interval: an interval of 10^6 rows (interval = 1) spreads its reductions over ~2000
// workgroups, an interval of 1000 rows takes two.  The split is a function of the interval sizes alone, every reduction has a
// fixed order and nothing is atomic, so the bits are the same on every run.
#include "gauss_internal.h"
#include "../../include/gauss_hip.h"

namespace gauss {

constexpr int PW_THREADS = 256;
constexpr int PW_TR = 32;                              // rows per LDS tile of pw_cross_kernel
constexpr int PW_MAXP = 64;                            // populations (Cxx and V: 2 x 64 x 65 doubles in LDS)
constexpr int PW_MAXPAIR = 9;                          // ceil(65 * 66 / 2 / 256) column pairs per thread
constexpr int PW_MAX_SWEEPS = 40;                      // Jacobi sweeps before GAUSS_ST_NOCONV (fp64 Jacobi needs ~10)

// column pair k -> (a, b), a <= b, upper triangle in row order (a = 0 is the study column)
__device__ __forceinline__ void pw_pair(int k, int nc, int& a, int& b)
{
    a = 0;
    while (k >= nc - a) { k -= nc - a; a++; }
    b = a + k;
}

__global__ __launch_bounds__(PW_THREADS) void pw_colsum_kernel(const double* __restrict__ x, int nc, const PwChunk* __restrict__ chunks,
                                                              double* __restrict__ part)
{
    __shared__ double red[PW_THREADS];
    const PwChunk ch = chunks[blockIdx.x];
    const int t = threadIdx.x;
    const int G = PW_THREADS / nc;                     // row lanes; thread (g, c) sums rows g, g + G, ... of column c
    const int c = t % nc, g = t / nc;
    double s = 0.0;
    if (g < G)
        for (long long r = ch.r0 + g; r < ch.r1; r += G) s += x[r * nc + c];
    red[t] = s;
    __syncthreads();
    if (t < nc) {
        double a = 0.0;
        for (int k = 0; k < G; k++) a += red[k * nc + t];
        part[(size_t)blockIdx.x * nc + t] = a;
    }
}

__global__ __launch_bounds__(128) void pw_mean_kernel(const double* __restrict__ part, int nc, const int* __restrict__ chunk_off,
                                                      const long long* __restrict__ off, double* __restrict__ mean)
{
    const int iv = blockIdx.x, t = threadIdx.x;
    if (t >= nc) return;
    double s = 0.0;
    for (int k = chunk_off[iv]; k < chunk_off[iv + 1]; k++) s += part[(size_t)k * nc + t];
    mean[(size_t)iv * nc + t] = s / (double)(off[iv + 1] - off[iv]);      // n = 0: 0 / 0 = NaN
}

__global__ __launch_bounds__(PW_THREADS) void pw_cross_kernel(const double* __restrict__ x, int nc, const PwChunk* __restrict__ chunks,
                                                             const double* __restrict__ mean, double* __restrict__ part)
{
    __shared__ double tile[PW_TR * (PW_MAXP + 1)];
    __shared__ double mu[PW_MAXP + 1];
    const PwChunk ch = chunks[blockIdx.x];
    const int t = threadIdx.x;
    const int npair = nc * (nc + 1) / 2;
    if (t < nc) mu[t] = mean[(size_t)ch.iv * nc + t];
    int pa[PW_MAXPAIR], pb[PW_MAXPAIR];
    double acc[PW_MAXPAIR];
#pragma unroll
    for (int j = 0; j < PW_MAXPAIR; j++) {
        const int k = t + j * PW_THREADS;
        pa[j] = pb[j] = 0;
        if (k < npair) pw_pair(k, nc, pa[j], pb[j]);
        acc[j] = 0.0;
    }
    __syncthreads();
    for (long long r0 = ch.r0; r0 < ch.r1; r0 += PW_TR) {
        const int nr = (int)min((long long)PW_TR, ch.r1 - r0);
        for (int e = t; e < nr * nc; e += PW_THREADS) tile[e] = x[r0 * nc + e] - mu[e % nc];     // rows are contiguous: one coalesced run
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PW_MAXPAIR; j++) {
            if (t + j * PW_THREADS < npair)
                for (int rr = 0; rr < nr; rr++) acc[j] = fma(tile[rr * nc + pa[j]], tile[rr * nc + pb[j]], acc[j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < PW_MAXPAIR; j++) {
        const int k = t + j * PW_THREADS;
        if (k < npair) part[(size_t)blockIdx.x * npair + k] = acc[j];
    }
}

// LDS of pw_solve_kernel, in doubles: A, V, C (m x (m + 1) each), cxy, lam, rotation cosines / sines, a reduction buffer
__host__ __device__ constexpr size_t pw_solve_lds_doubles(int m) { return 3 * (size_t)m * (m + 1) + 2 * PW_MAXP + PW_MAXP + PW_THREADS; }

__global__ __launch_bounds__(PW_THREADS) void pw_solve_kernel(const double* __restrict__ part, int P, const int* __restrict__ chunk_off,
                                                             const long long* __restrict__ off, double eps, double* __restrict__ w_out,
                                                             int* __restrict__ status)
{
    extern __shared__ double lds[];
    __shared__ int s_flag, s_rot;
    __shared__ int s_p[PW_MAXP / 2], s_q[PW_MAXP / 2];
    const int iv = blockIdx.x, t = threadIdx.x;
    const int nc = P + 1, npair = nc * (nc + 1) / 2;
    const int m = P + (P & 1);                         // even order for the round-robin; index P (P odd) is a dummy, never rotated
    const int ld = m + 1;
    double* A = lds;                                   // Jacobi working copy of Cxx
    double* V = A + (size_t)m * ld;                    // eigenvectors (columns)
    double* C = V + (size_t)m * ld;                    // Cxx itself, then its Cholesky factor
    double* cxy = C + (size_t)m * ld;
    double* lam = cxy + PW_MAXP;
    double* cs_c = lam + PW_MAXP;
    double* cs_s = cs_c + PW_MAXP / 2;
    double* red = cs_s + PW_MAXP / 2;

    // ---- covariance: the chunks' cross sums in chunk order, / (n - 1) (n = 1: 0 / 0 = NaN, as in the reference)
    const double denom = (double)(off[iv + 1] - off[iv] - 1);
    if (t == 0) s_flag = 0;
    for (int e = t; e < m * ld; e += PW_THREADS) { A[e] = 0.0; V[e] = 0.0; C[e] = 0.0; }
    __syncthreads();
    for (int k = t; k < npair; k += PW_THREADS) {
        double s = 0.0;
        for (int c = chunk_off[iv]; c < chunk_off[iv + 1]; c++) s += part[(size_t)c * npair + k];
        const double cov = s / denom;
        int a, b;
        pw_pair(k, nc, a, b);
        if (a == 0) { if (b > 0) cxy[b - 1] = cov; }
        else { C[(a - 1) * ld + (b - 1)] = cov; C[(b - 1) * ld + (a - 1)] = cov; }
        if (!isfinite(cov) && !(a == 0 && b == 0)) s_flag = 1;
    }
    if (t == 0 && chunk_off[iv + 1] == chunk_off[iv]) s_flag = 1;     // no rows at all
    __syncthreads();
    if (s_flag) {                                      // NaN in, NaN out: no eigen-solve on non-finite input
        for (int j = t; j < P; j += PW_THREADS) w_out[(size_t)iv * P + j] = NAN;
        if (t == 0) status[iv] = GAUSS_ST_NONFINITE;
        return;
    }

    // ---- MakePosDef (util.cpp:302-318): eigenvalues by cyclic Jacobi, m / 2 disjoint rotations per round (round-robin order);
    // a rotation is skipped when its off-diagonal entry is below 4 eps_mach ||Cxx||_F
    double fs = 0.0;
    for (int e = t; e < P * P; e += PW_THREADS) { const double v = C[(e / P) * ld + e % P]; fs = fma(v, v, fs); }
    red[t] = fs;
    __syncthreads();
    for (int s = PW_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double tol = 4.0 * 2.220446049250313e-16 * sqrt(red[0]);
    for (int e = t; e < m * ld; e += PW_THREADS) A[e] = C[e];
    for (int i = t; i < m; i += PW_THREADS) V[i * ld + i] = 1.0;
    __syncthreads();
    bool converged = false;
    for (int sweep = 0; sweep < PW_MAX_SWEEPS; sweep++) {
        if (t == 0) s_rot = 0;
        __syncthreads();
        for (int round = 0; round < m - 1; round++) {
            if (t < m / 2) {
                int p, q;
                if (t == 0) { p = m - 1; q = round; }
                else { p = (round + t) % (m - 1); q = (round - t + m - 1) % (m - 1); }
                if (p > q) { const int x = p; p = q; q = x; }
                double c = 1.0, s = 0.0;
                if (q < P) {
                    const double apq = A[p * ld + q];
                    if (fabs(apq) > tol) {
                        const double tau = (A[q * ld + q] - A[p * ld + p]) / (2.0 * apq);
                        const double tt = fabs(tau) > 1e150 ? 0.5 / tau
                                                            : (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + tt * tt);
                        s = tt * c;
                        s_rot = 1;
                    }
                }
                s_p[t] = p; s_q[t] = q; cs_c[t] = c; cs_s[t] = s;
            }
            __syncthreads();
            for (int e = t; e < (m / 2) * m; e += PW_THREADS) {          // rows p, q <- J^T A
                const int k = e / m, j = e % m;
                const double c = cs_c[k], s = cs_s[k];
                if (s == 0.0) continue;
                double* rp = A + s_p[k] * ld;
                double* rq = A + s_q[k] * ld;
                const double x = rp[j], y = rq[j];
                rp[j] = c * x - s * y;
                rq[j] = s * x + c * y;
            }
            __syncthreads();
            for (int e = t; e < (m / 2) * m; e += PW_THREADS) {          // columns p, q <- A J, V J
                const int k = e / m, i = e % m;
                const double c = cs_c[k], s = cs_s[k];
                if (s == 0.0) continue;
                const int p = s_p[k], q = s_q[k];
                double x = A[i * ld + p], y = A[i * ld + q];
                A[i * ld + p] = c * x - s * y;
                A[i * ld + q] = s * x + c * y;
                x = V[i * ld + p]; y = V[i * ld + q];
                V[i * ld + p] = c * x - s * y;
                V[i * ld + q] = s * x + c * y;
            }
            __syncthreads();
        }
        const int any = s_rot;
        __syncthreads();
        if (!any) { converged = true; break; }
    }
    if (!converged) {
        for (int j = t; j < P; j += PW_THREADS) w_out[(size_t)iv * P + j] = NAN;
        if (t == 0) status[iv] = GAUSS_ST_NOCONV | GAUSS_ST_NONFINITE;
        return;
    }
    double lmin = A[0];
    for (int i = 1; i < P; i++) lmin = fmin(lmin, A[i * ld + i]);
    const bool clamped = lmin < eps;                   // the reference rebuilds Cxx only in this case
    if (clamped) {
        for (int i = t; i < P; i += PW_THREADS) lam[i] = fmax(A[i * ld + i], eps);
        __syncthreads();
        for (int e = t; e < P * P; e += PW_THREADS) {  // Cxx <- V diag(max(lambda, eps)) V^T
            const int i = e / P, j = e % P;
            double s = 0.0;
            for (int k = 0; k < P; k++) s = fma(V[i * ld + k] * lam[k], V[j * ld + k], s);
            C[i * ld + j] = s;
        }
        __syncthreads();
    }

    // ---- W_i = Cxx^-1 Cxy by Cholesky (Cxx is symmetric positive definite here: lambda_min >= eps, or clamped to it)
    for (int k = 0; k < P; k++) {
        if (t == 0) {
            const double d = C[k * ld + k];
            if (!(d > 0.0) || !isfinite(d)) s_flag = 1;
            else C[k * ld + k] = sqrt(d);
        }
        __syncthreads();
        if (s_flag) break;
        const double dk = C[k * ld + k];
        for (int i = k + 1 + t; i < P; i += PW_THREADS) C[i * ld + k] /= dk;
        __syncthreads();
        const int r = P - k - 1;
        for (int e = t; e < r * r; e += PW_THREADS) {
            const int i = k + 1 + e / r, j = k + 1 + e % r;
            if (j <= i) C[i * ld + j] -= C[i * ld + k] * C[j * ld + k];
        }
        __syncthreads();
    }
    if (!s_flag) {
        for (int k = 0; k < P; k++) {                  // L y = cxy
            if (t == 0) cxy[k] /= C[k * ld + k];
            __syncthreads();
            for (int i = k + 1 + t; i < P; i += PW_THREADS) cxy[i] -= C[i * ld + k] * cxy[k];
            __syncthreads();
        }
        for (int k = P - 1; k >= 0; k--) {             // L^T w = y
            if (t == 0) cxy[k] /= C[k * ld + k];
            __syncthreads();
            for (int i = t; i < k; i += PW_THREADS) cxy[i] -= C[k * ld + i] * cxy[k];
            __syncthreads();
        }
    }
    int st = clamped ? GAUSS_ST_CLAMPED : 0;
    if (s_flag) st |= GAUSS_ST_NONFINITE;
    for (int j = t; j < P; j += PW_THREADS) {
        const double w = s_flag ? NAN : cxy[j];
        w_out[(size_t)iv * P + j] = w;
    }
    if (t == 0) status[iv] = st;
}

void launch_pop_weights(const double* d_x, int n_pop, const PwChunk* d_chunks, int n_chunk, const int* d_chunk_off,
                        const long long* d_off, int n_interval, double eps, double* d_part1, double* d_mean, double* d_part2,
                        double* d_w, int* d_status, hipStream_t s)
{
    const int nc = n_pop + 1;
    const int m = n_pop + (n_pop & 1);
    const size_t smem = sizeof(double) * pw_solve_lds_doubles(m);
    static DeviceOnce attr_once;
    attr_once.run([&]() {
        hipFuncSetAttribute(reinterpret_cast<const void*>(pw_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(double) * pw_solve_lds_doubles(PW_MAXP)));
    });
    if (n_chunk > 0) hipLaunchKernelGGL(pw_colsum_kernel, dim3(n_chunk), dim3(PW_THREADS), 0, s, d_x, nc, d_chunks, d_part1);
    hipLaunchKernelGGL(pw_mean_kernel, dim3(n_interval), dim3(128), 0, s, d_part1, nc, d_chunk_off, d_off, d_mean);
    if (n_chunk > 0) hipLaunchKernelGGL(pw_cross_kernel, dim3(n_chunk), dim3(PW_THREADS), 0, s, d_x, nc, d_chunks, d_mean, d_part2);
    hipLaunchKernelGGL(pw_solve_kernel, dim3(n_interval), dim3(PW_THREADS), smem, s, d_part2, n_pop, d_chunk_off, d_off, eps, d_w, d_status);
}

}  // namespace gauss
