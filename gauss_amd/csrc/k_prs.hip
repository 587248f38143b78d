// Polygenic score weights of an imputation window: lassosum's model (Mak et al. 2017), elastic-net-penalised regression on summary
// statistics by cyclic coordinate descent, on the window's own LD.  With B = B11 in A[0] (lambda on the diagonal, MakePosDef's repair
// included), z = z1 and r_j = z_j / sqrt(n - 2 + z_j^2), a chain at shrinkage s takes the penalties lam in the caller's order, each
// from the solution of the one before it, from beta = 0 and g = B beta = 0.  One sweep, j = 0 .. M - 1 in order, frozen j (z_j not
// finite) skipped:
//     den = (1 - s) B_jj + s
//     u   = r_j - (1 - s) (g_j - B_jj beta_j)
//     b'  = sign(u) (|u| - lam) / den  if |u| > lam, else 0
//     D   = b' - beta_j;  D != 0:  g_i += D * B_ji for every i < M,  beta_j = b'
// delta = max |D| of the sweep; the penalty is left when delta < tol * r_max (or r_max = 0), or after max_sweeps sweeps (the cell's
// flag is raised, gauss_job_fetch turns it into GAUSS_ST_PRS_NOCONV).  The definition, the outputs and the refusals: include/gauss_hip.h.
//
// One workgroup = one chain = one (s, asking window): grid (most chains of a window, asking windows); a workgroup beyond its window's
// chains leaves at once.  A chain is strictly sequential in j; the parallelism inside it is over i in the update of g, across chains
// it is chains x windows.  beta, g, r and diag(B) of the chain live in LDS, 4 M doubles (the launch passes the largest M among the
// asking windows; PRS_M_MAX = 4096 takes 128 KB of gfx950's 160).  r holds a NaN for a frozen SNP: that is the flag.
// EVERY lane computes the same D from the same four LDS words (broadcast reads), so every branch below is uniform over the workgroup:
//   - D == 0 (with sparse solutions most coordinates): no row read, no barrier, nothing written;
//   - D != 0: a barrier (every wave has read coordinate j's words), lane t adds D * B_ji to g_i for i = t, t + T, .. from row j of
//     A[0] (B is symmetric and stored in full: the row is contiguous, the read coalesced), lane 0 stores beta_j, a barrier.
// Between two such barrier pairs nothing in LDS changes, so a wave that runs ahead over coordinates with D == 0 reads what every other
// wave reads, and reaches the same next coordinate with D != 0: the barriers always pair up.  The algorithm has no reductions: g_i
// is a fixed sequence of "one multiply, one add" (compiled with -ffp-contract=off), so beta does not depend on T; the two maxima
// that are reduced across lanes (r_max, the KKT residual) are exact whatever the order.  br = beta' r and bg = beta' g are summed in
// index order by every lane alike.  Every loop is bounded: n_lam <= 32, max_sweeps <= 1000, M <= 4096.  No atomics, nothing waits
// for another workgroup.  Latency-bound: a coordinate that does not move costs four LDS reads and some ten dependent fp64
// operations, one that moves a row of B from L2 / HBM and two barriers.
// T = 256 (a workgroup per chain) is the form the library runs; T = 64 (a wave per chain) is built beside it and chosen with
// GAUSS_PRS_T=64 for measurements: same bits.
#include "gauss_internal.h"
#include <algorithm>
#include <cstdlib>

namespace gauss {

static_assert(PRS_S == 8 && PRS_LAM == 32, "Prob::prs_s / prs_lam are declared with these sizes");
static_assert(4 * (size_t)PRS_M_MAX * sizeof(double) + 1024 <= 160 * 1024, "beta, g, r and diag(B) of the largest window fit into LDS");

constexpr int PRS_U = 8;                     // entries of a row a lane loads before it updates g with them

template <int T>
__global__ __launch_bounds__(T) void prs_kernel(const Prob* __restrict__ probs, const int* __restrict__ prsmap)
{
    extern __shared__ __attribute__((aligned(16))) double prs_smem[];
    __shared__ double s_red[T / 64];
    const Prob& pb = probs[prsmap ? prsmap[blockIdx.y] : (int)blockIdx.y];
    const int is = blockIdx.x;
    if (is >= pb.prs_n_s) return;                           // (uniform: the whole workgroup leaves)
    const int tid = threadIdx.x;
    const int M = pb.M, ld = pb.Mld, n_lam = pb.prs_n_lam, cap = pb.prs_max_sweeps;
    const auto A = pb.A;                                    // A[0] = B11
    double* const beta = prs_smem;
    double* const g = prs_smem + M;
    double* const r = prs_smem + 2 * (size_t)M;
    double* const bd = prs_smem + 3 * (size_t)M;
    const PrsLayout o = prs_layout(M, pb.prs_n_s, n_lam);
    const auto out = pb.out_prs;

    // a maximum over the workgroup of a value that is never NaN: exact in any order
    auto wg_max = [&](double v) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
        if ((tid & 63) == 0) s_red[tid >> 6] = v;
        __syncthreads();
        v = s_red[0];
#pragma unroll
        for (int w = 1; w < T / 64; w++) v = fmax(v, s_red[w]);
        __syncthreads();                                    // (s_red is free again)
        return v;
    };

    const double nm2 = pb.prs_n - 2.0;
    double rmax = 0.0;
    for (int i = tid; i < M; i += T) {
        const double z = pb.z1[i];
        const bool fin = z - z == 0.0;                      // finite
        const double ri = z / sqrt(nm2 + z * z);
        beta[i] = 0.0;
        g[i] = 0.0;
        r[i] = fin ? ri : __builtin_nan("");
        bd[i] = A[(size_t)i * ld + i];
        if (fin) rmax = fmax(rmax, fabs(ri));
    }
    rmax = wg_max(rmax);                                    // (its barriers also publish the four arrays)
    const double s = pb.prs_s[is], oms = 1.0 - s;
    const double thr = pb.prs_tol * rmax;

    for (int il = 0; il < n_lam; il++) {
        const double lam = pb.prs_lam[il];
        int sweeps = 0;
        double delta = 0.0;
        for (int sw = 0; sw < cap; sw++) {
            delta = 0.0;
            for (int j = 0; j < M; j++) {
                const double rj = r[j];
                if (rj != rj) continue;                     // frozen
                const double bj = beta[j], bjj = bd[j], gj = g[j];
                const double u = rj - oms * (gj - bjj * bj);
                const double au = fabs(u);
                double bn = 0.0;
                if (au > lam) {
                    const double den = oms * bjj + s;
                    bn = copysign(au - lam, u) / den;
                }
                const double d = bn - bj;
                if (d != 0.0) {
                    __syncthreads();                        // every wave has read coordinate j's words
                    const auto row = A + (size_t)j * ld;
                    // (PRS_U loads of the row in flight before the first of them is used: the loop is bound by their latency)
                    for (int i0 = tid; i0 < M; i0 += PRS_U * T) {
                        double v[PRS_U];
#pragma unroll
                        for (int k = 0; k < PRS_U; k++) v[k] = i0 + k * T < M ? row[i0 + k * T] : 0.0;
#pragma unroll
                        for (int k = 0; k < PRS_U; k++)
                            if (i0 + k * T < M) g[i0 + k * T] += d * v[k];
                    }
                    if (tid == 0) beta[j] = bn;
                    __syncthreads();
                    delta = fmax(delta, fabs(d));
                }
            }
            sweeps = sw + 1;
            if (delta < thr || rmax == 0.0) break;
        }
        // the cell's outputs, from the state the last sweep left
        const size_t c = (size_t)is * n_lam + il;
        double br = 0.0, bg = 0.0;
        int nnz = 0;
        for (int j = 0; j < M; j++) {
            const double bj = beta[j], rj = r[j];
            br += bj * (rj != rj ? 0.0 : rj);
            bg += bj * g[j];
            nnz += bj != 0.0 ? 1 : 0;
        }
        double kkt = 0.0;
        const auto ob = out + o.beta + c * (size_t)M;
        for (int i = tid; i < M; i += T) {
            const double bi = beta[i], ri = r[i];
            ob[i] = bi;
            if (ri != ri) continue;
            const double q = ri - oms * g[i] - s * bi;
            const double res = bi != 0.0 ? fabs(q - copysign(lam, bi)) : fmax(0.0, fabs(q) - lam);
            kkt = fmax(kkt, res);
        }
        kkt = wg_max(kkt);
        if (tid == 0) {
            const auto cell = out + o.cell + c * PRS_CELL;
            cell[PRS_NNZ] = (double)nnz;
            cell[PRS_SWEEPS] = (double)sweeps;
            cell[PRS_DELTA] = delta;
            cell[PRS_BR] = br;
            cell[PRS_BG] = bg;
            cell[PRS_KKT] = kkt;
            cell[PRS_NOCONV] = (delta < thr || rmax == 0.0) ? 0.0 : 1.0;
            cell[PRS_NOCONV + 1] = 0.0;
        }
    }
}

void launch_prs(const Prob* d_probs, const int* d_prsmap, int n, int max_s, int max_M, hipStream_t s)
{
    if (n <= 0 || max_s <= 0 || max_M <= 0) return;
    constexpr int SMEM_MAX = (int)(4 * (size_t)PRS_M_MAX * sizeof(double));
    static DeviceOnce attr_once;
    attr_once.run([&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(prs_kernel<PRS_T>), hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_MAX);
        hipFuncSetAttribute(reinterpret_cast<const void*>(prs_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_MAX);
    });
    const size_t smem = 4 * (size_t)std::min(max_M, PRS_M_MAX) * sizeof(double);
    const char* const e = getenv("GAUSS_PRS_T");
    if (e && atoi(e) == 64)                // a wave per chain: for measurements (read per launch), same bits
        hipLaunchKernelGGL(prs_kernel<64>, dim3(max_s, n), dim3(64), smem, s, d_probs, d_prsmap);
    else
        hipLaunchKernelGGL(prs_kernel<PRS_T>, dim3(max_s, n), dim3(PRS_T), smem, s, d_probs, d_prsmap);
}

}  // namespace gauss
