// Gene-based sum-of-chi2 test (the statistic of fastBAT, VEGAS and MAGMA's SNP-wise mean model) on the LD blocks a gene job left in
// HBM: per gene the position-order LD pruning, the eigenvalues of the kept block, and per trait Q = sum z^2 over the kept SNPs and
// the gene's top SNP.  The definition, the outputs and the refusals: include/gauss_hip.h (gauss_gene_sumchi2).  For one gene of n
// rows with block R (n x n, both triangles, diagonal 1):
//   (a) nanrow[i] = n > 1 and R_ij is NaN for every j != i (a monomorphic SNP)
//       for i = 0 .. n-1:  nanrow[i] or dropped[i]: pass;  else i is kept and every j > i with R_ij * R_ij > prune_r2 is dropped
//   (b) k = kept rows.  k = 0: GAUSS_ST_SUMCHI2_EMPTY;  k > SC2_K_MAX: GAUSS_ST_SUMCHI2_TOOLARGE;  both: every lambda NaN
//   (c) A = R[kept][kept], order m = k + (k & 1) (index k of an odd k is a dummy, never rotated), row pitch m + 1 doubles.
//       tol = 4 * 2^-52 * sqrt(F), F = sum of A_ab^2: thread t adds, in this order, the squares of the entries e = t, t + 256, ... of
//       the k x k block in row-major order (one product, one add each); then 8 halving steps part[t] += part[t + s], s = 128 .. 1.
//       Sweeps of m - 1 rounds, round r rotating the m / 2 disjoint pairs of the round-robin order (pair 0: (m - 1, r); pair t:
//       ((r + t) mod (m - 1), (r - t) mod (m - 1)); the smaller index is p).  A pair with q >= k or |A_pq| <= tol is skipped; else
//       tau = (A_qq - A_pp) / (2 A_pq), t = sign(tau) / (|tau| + sqrt(1 + tau^2)) (0.5 / tau beyond 1e150), c = 1 / sqrt(1 + t^2),
//       s = t c; rows p, q <- J^T A (x' = c x - s y, y' = s x + c y), then columns p, q <- A J.  A sweep without a rotation ends the
//       solve; SC2_MAX_SWEEPS sweeps without one: GAUSS_ST_NOCONV and NaN.  The diagonal sorted descending by rank counting
//       (ties: the smaller index first).  sweeps counts the last, rotation-free sweep too.
//   (d) per trait: Q = the kept rows' z^2 added in ascending row order by one thread (one product, one add each);  top = the row
//       with the largest z^2 among all n rows whose z is finite (ties: the smaller row; none: -1)
// Compiled with -ffp-contract=off: every product and sum above is rounded as written, fp64 division and square root round
// correctly, and no sum depends on the thread mapping -- the numpy replay of tests/sumchi2_ref.py gives the same bits.
//
// One workgroup of SC2_T = 256 threads = one gene (blockIdx.x).  (a) reads the block twice at the most: wave w tests rows w, w + 4,
// ... for NaN with coalesced reads and a ballot, then the loop reads the part j > i of every kept row i coalesced; the flags are
// ints in LDS; every branch on i is uniform (all threads read the same LDS word); one barrier per kept row.  The kept list comes
// from a count per thread (4 consecutive rows each) and a prefix over the 256 counts.  (c) runs in LDS alone: 129 x 128 doubles at
// k = 128 (the odd pitch spreads a column walk over the banks), one thread per rotation, 32 entries a thread per update, 3 barriers
// a round.  All LDS is carved from the dynamic region, tables first (a multiple of 16 bytes), the block last: 13 840 + 132 096
// bytes at k = 128 of gfx950's 160 KB, so one workgroup per CU; the launch asks for what its largest gene can need.  Vector loads
// and stores only, no atomics; nothing waits for another workgroup.  Latency-bound: (m - 1) rounds x sweeps x 3 barriers.
#include "gauss_internal.h"
#include "../../include/gauss_hip.h"

namespace gauss {

constexpr int SC2_NW = SC2_T / 64;
constexpr int SC2_PER = SC2_N_MAX / SC2_T;             // consecutive rows of a thread in the kept list's count
constexpr int SC2_NONE = 0x7fffffff;
// the tables in front of the block, in bytes: cosines, sines [K_MAX / 2], the reduction buffer [T], the sorted diagonal [K_MAX] as
// doubles; then p, q [K_MAX / 2], counts [T], the kept list [N_MAX], the flags [N_MAX], control words [4] as ints
constexpr size_t SC2_TAB_DOUBLES = SC2_K_MAX / 2 * 2 + SC2_T + SC2_K_MAX;
constexpr size_t SC2_TAB_INTS = SC2_K_MAX / 2 * 2 + SC2_T + SC2_N_MAX * 2 + 4;
constexpr size_t SC2_TAB_BYTES = SC2_TAB_DOUBLES * 8 + SC2_TAB_INTS * 4;
__host__ __device__ constexpr size_t sc2_lds_bytes(int m) { return SC2_TAB_BYTES + (size_t)m * (size_t)(m + 1) * 8; }
static_assert(SC2_TAB_BYTES % 16 == 0, "the block behind the tables starts on a 16-byte boundary");
static_assert(sc2_lds_bytes(SC2_K_MAX) <= (size_t)160 << 10, "the tables and the largest kept block fit gfx950's LDS");
static_assert(SC2_N_MAX % SC2_T == 0 && SC2_TRAITS_MAX <= SC2_T && SC2_K_MAX <= SC2_T, "one thread per trait and per eigenvalue");

// the order of the top SNP: the larger z^2 first, then the smaller row
__device__ __forceinline__ bool sc2_better(double c, int i, double c2, int i2) { return c > c2 || (c == c2 && i < i2); }

__global__ __launch_bounds__(SC2_T) void sumchi2_kernel(const Sumchi2Args a)
{
    extern __shared__ __attribute__((aligned(16))) double sc2_smem[];
    double* const cs_c = sc2_smem;
    double* const cs_s = cs_c + SC2_K_MAX / 2;
    double* const red = cs_s + SC2_K_MAX / 2;
    double* const s_lam = red + SC2_T;
    int* const s_p = (int*)(s_lam + SC2_K_MAX);
    int* const s_q = s_p + SC2_K_MAX / 2;
    int* const s_cnt = s_q + SC2_K_MAX / 2;
    int* const s_kidx = s_cnt + SC2_T;
    int* const s_drop = s_kidx + SC2_N_MAX;            // 0 kept (so far), 1 pruned, 2 a NaN row
    int* const s_ctl = s_drop + SC2_N_MAX;             // [0] k, [1] a rotation was made in this sweep
    double* const A = (double*)(s_ctl + 4);

    const int tid = threadIdx.x, g = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = G(a.gene_off)[g];
    const int n = G(a.gene_off)[g + 1] - r0;
    if (n < 0 || n > SC2_N_MAX) return;                // (the entry point refuses such a gene before anything runs)
    const auto R = G(a.R) + G(a.gene_out_off)[g];
    const auto z = G(a.z);
    const auto o_lam = G(a.lam) + (size_t)g * SC2_K_MAX;
    const double prune_r2 = a.prune_r2;
    const double nan = __builtin_nan("");

    // ---- (a) the NaN rows, then the pruning in row order
    for (int i = wave; i < n; i += SC2_NW) {
        const auto row = R + (size_t)i * (size_t)n;
        bool some = false;
        for (int j = lane; j < n; j += 64) some = some || (j != i && !isnan(row[j]));
        const bool any = __ballot(some) != 0ull;
        if (lane == 0) s_drop[i] = (n > 1 && !any) ? 2 : 0;
    }
    __syncthreads();
    for (int i = 0; i < n; i++) {
        if (s_drop[i]) continue;                       // uniform; flag i was last written before the previous barrier
        const auto row = R + (size_t)i * (size_t)n;
        for (int j = i + 1 + tid; j < n; j += SC2_T) {
            const double r = row[j];
            const double t2 = r * r;
            if (t2 > prune_r2) s_drop[j] = 1;          // (a NaN compares false: a NaN row keeps its 2)
        }
        __syncthreads();
    }

    // ---- the kept list, in row order
    {
        const int base = tid * SC2_PER;
        int cnt = 0;
#pragma unroll
        for (int u = 0; u < SC2_PER; u++) cnt += (base + u < n && s_drop[base + u] == 0) ? 1 : 0;
        s_cnt[tid] = cnt;
        __syncthreads();
        int off = 0;
        for (int u = 0; u < tid; u++) off += s_cnt[u];
        if (tid == SC2_T - 1) s_ctl[0] = off + cnt;
#pragma unroll
        for (int u = 0; u < SC2_PER; u++) {
            const int i = base + u;
            if (i >= n) break;
            const int keep = s_drop[i] == 0;
            if (keep) s_kidx[off++] = i;
            G(a.kept)[r0 + i] = keep;
        }
        if (tid < SC2_K_MAX) s_lam[tid] = nan;
        __syncthreads();
    }
    const int k = s_ctl[0];

    // ---- (d) per trait: Q by one thread over the kept rows in ascending order; the top row by one wave
    if (tid < a.n_trait) {
        const auto zt = z + (size_t)tid * (size_t)a.n_snp + r0;
        double q = 0.0;
        for (int u = 0; u < k; u++) {
            const double v = zt[s_kidx[u]];
            const double v2 = v * v;
            q = q + v2;
        }
        G(a.q)[(size_t)tid * (size_t)a.n_gene + g] = q;
    }
    for (int t = wave; t < a.n_trait; t += SC2_NW) {
        const auto zt = z + (size_t)t * (size_t)a.n_snp + r0;
        double bc = -1.0;
        int bi = SC2_NONE;
        for (int i = lane; i < n; i += 64) {
            const double v = zt[i];
            const double v2 = v * v;
            if (isfinite(v) && sc2_better(v2, i, bc, bi)) { bc = v2; bi = i; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double c2 = __shfl_xor(bc, off, 64);
            const int i2 = __shfl_xor(bi, off, 64);
            if (sc2_better(c2, i2, bc, bi)) { bc = c2; bi = i2; }
        }
        if (lane == 0) G(a.top)[(size_t)t * (size_t)a.n_gene + g] = bi == SC2_NONE ? -1 : bi;
    }

    // ---- (b) nothing to solve, or too much
    const int m = k + (k & 1), ld = m + 1;
    if (k == 0 || k > SC2_K_MAX || m > a.m_lds) {      // (m <= m_lds always holds where k <= SC2_K_MAX: the launch sizes it by the largest gene)
        if (tid < SC2_K_MAX) o_lam[tid] = nan;
        if (tid == 0) {
            G(a.n_kept)[g] = k;
            G(a.status)[g] = k == 0 ? GAUSS_ST_SUMCHI2_EMPTY : GAUSS_ST_SUMCHI2_TOOLARGE;
            G(a.sweeps)[g] = 0;
        }
        return;
    }

    // ---- (c) the kept block into LDS, its Frobenius norm, the Jacobi sweeps
    for (int e = tid; e < m * ld; e += SC2_T) {
        const int p = e / ld, q = e % ld;
        A[e] = (p < k && q < k) ? R[(size_t)s_kidx[p] * (size_t)n + (size_t)s_kidx[q]] : 0.0;
    }
    __syncthreads();
    {
        double fs = 0.0;
        for (int e = tid; e < k * k; e += SC2_T) {
            const double v = A[(e / k) * ld + e % k];
            const double v2 = v * v;
            fs = fs + v2;
        }
        red[tid] = fs;
        __syncthreads();
        for (int s = SC2_T / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] = red[tid] + red[tid + s];
            __syncthreads();
        }
    }
    const double tol = 8.881784197001252e-16 * sqrt(red[0]);            // 4 * 2^-52 ||A||_F
    bool converged = false;
    int sweeps = 0;
    for (int sweep = 0; sweep < SC2_MAX_SWEEPS; sweep++) {
        if (tid == 0) s_ctl[1] = 0;
        __syncthreads();
        for (int round = 0; round < m - 1; round++) {
            if (tid < m / 2) {
                int p, q;
                if (tid == 0) { p = m - 1; q = round; }
                else { p = (round + tid) % (m - 1); q = (round - tid + m - 1) % (m - 1); }
                if (p > q) { const int x = p; p = q; q = x; }
                double c = 1.0, s = 0.0;
                if (q < k) {
                    const double apq = A[p * ld + q];
                    if (fabs(apq) > tol) {
                        const double tau = (A[q * ld + q] - A[p * ld + p]) / (2.0 * apq);
                        const double tt = fabs(tau) > 1e150 ? 0.5 / tau
                                                            : (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + tt * tt);
                        s = tt * c;
                        s_ctl[1] = 1;
                    }
                }
                s_p[tid] = p; s_q[tid] = q; cs_c[tid] = c; cs_s[tid] = s;
            }
            __syncthreads();
            for (int e = tid; e < (m / 2) * m; e += SC2_T) {            // rows p, q <- J^T A
                const int r = e / m, j = e % m;
                const double c = cs_c[r], s = cs_s[r];
                if (s == 0.0) continue;
                double* rp = A + s_p[r] * ld;
                double* rq = A + s_q[r] * ld;
                const double x = rp[j], y = rq[j];
                rp[j] = c * x - s * y;
                rq[j] = s * x + c * y;
            }
            __syncthreads();
            for (int e = tid; e < (m / 2) * m; e += SC2_T) {            // columns p, q <- A J
                const int r = e / m, i = e % m;
                const double c = cs_c[r], s = cs_s[r];
                if (s == 0.0) continue;
                const int p = s_p[r], q = s_q[r];
                const double x = A[i * ld + p], y = A[i * ld + q];
                A[i * ld + p] = c * x - s * y;
                A[i * ld + q] = s * x + c * y;
            }
            __syncthreads();
        }
        sweeps = sweep + 1;
        const int any = s_ctl[1];
        __syncthreads();
        if (!any) { converged = true; break; }
    }

    // ---- the diagonal, descending (rank counting; ties: the smaller index first); NaN beyond k and where the solve gave up
    if (converged && tid < k) {
        const double d = A[tid * ld + tid];
        int rank = 0;
        for (int j = 0; j < k; j++) {
            const double dj = A[j * ld + j];
            rank += (dj > d || (dj == d && j < tid)) ? 1 : 0;
        }
        s_lam[rank] = d;
    }
    __syncthreads();
    if (tid < SC2_K_MAX) o_lam[tid] = s_lam[tid];
    if (tid == 0) {
        G(a.n_kept)[g] = k;
        G(a.status)[g] = converged ? 0 : GAUSS_ST_NOCONV;
        G(a.sweeps)[g] = sweeps;
    }
}

void launch_sumchi2(Sumchi2Args a, int max_n, hipStream_t s)
{
    if (a.n_gene <= 0) return;
    static DeviceOnce attr_once;
    attr_once.run([&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(sumchi2_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)sc2_lds_bytes(SC2_K_MAX));
    });
    const int kmax = max_n < SC2_K_MAX ? (max_n < 0 ? 0 : max_n) : SC2_K_MAX;
    a.m_lds = kmax + (kmax & 1);
    hipLaunchKernelGGL(sumchi2_kernel, dim3(a.n_gene), dim3(SC2_T), sc2_lds_bytes(a.m_lds), s, a);
}

}  // namespace gauss
