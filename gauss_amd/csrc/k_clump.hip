// LD clumping (PLINK's --clump rule) on the LD matrix an LD-only job left in HBM: which SNPs of a region lead a clump, and which clump
// every other SNP belongs to.  The definition, the outputs and the refusals: include/gauss_hip.h (gauss_ld_clump_rows).  For one trait:
//     owner = -1, rank = 0, r2 = NaN everywhere;  n = 0
//     repeat:  i = the unowned row with the largest key >= key_index (ties: the smaller row; a NaN key never leads); none: stop
//              n += 1;  owner[i] = i;  rank[i] = n;  r2[i] = 1
//              every j != i with |bp_j - bp_i| <= radius, owner[j] == -1, key_j >= key_member:
//                  t2 = R[i][j] * R[i][j];  t2 >= r2_min (false for a NaN):  owner[j] = i;  r2[j] = t2
// which is the sorted walk of the header: the rows in (key descending, row ascending) order, a row that is owned when its turn comes
// is passed over.  No sum is formed anywhere: t2 is one rounded product, so the outputs do not depend on the thread mapping.
//
// One workgroup = one trait (blockIdx.x); the traits share R and bp.  The trait's keys [M] doubles, owner [M] ints and bp [M] ints live
// in LDS: 16 M bytes, 128 KB at CLUMP_M_MAX = 8 192 of gfx950's 160.  Per clump: the argmax of (key, row) over the unowned rows --
// thread tid looks at rows tid, tid + CLUMP_T, ..., then cross-lane moves inside a wave, then through LDS across the waves, as
// slct_kernel does (k_slct.hip) -- then the band [lo, hi) of the lead by two binary searches on bp in LDS, then the band's part of row i
// of R, read coalesced over j (the LD-only epilogue stores both triangles: row i is column i).  A row outside the band is not read.
// Every branch on the lead, the band or the stopping rule is uniform: all threads read the same LDS words.  Two barriers per clump.
// owner is written out once at the end; rank, r2 and n_clumps are written once each, by whoever decides them.  Vector loads and
// stores only, no atomics; nothing waits for another workgroup.  Latency-bound: at most M dependent steps of a scan of 16 M bytes of
// LDS and a band of one row.  Compiled with -ffp-contract=off like the other fp64 tails (there is nothing to contract).
#include "gauss_internal.h"

namespace gauss {

constexpr int CLUMP_NW = CLUMP_T / 64;
constexpr int CLUMP_NONE = 0x7fffffff;
static_assert((size_t)CLUMP_M_MAX * 16 + 1024 <= (size_t)160 << 10, "keys, owner and bp of the largest region fit gfx950's LDS");

// the order of the argmax: the larger key first, then the smaller row
__device__ __forceinline__ bool clump_better(double c, int i, double c2, int i2) { return c > c2 || (c == c2 && i < i2); }

__global__ __launch_bounds__(CLUMP_T) void clump_kernel(const ClumpArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double clump_smem[];
    __shared__ double s_redc[CLUMP_NW];
    __shared__ int s_redi[CLUMP_NW];
    const int tid = threadIdx.x, M = a.M;
    const size_t t0 = (size_t)blockIdx.x * (size_t)M;       // this trait's rows of key and of the outputs
    double* const s_key = clump_smem;
    int* const s_owner = (int*)(clump_smem + M);
    int* const s_bp = s_owner + M;
    const auto R = G(a.R);
    const auto key = G(a.key) + t0;
    const auto bp = G(a.bp);
    const auto o_owner = G(a.owner) + t0;
    const auto o_rank = a.rank ? G(a.rank) + t0 : nullptr;
    const auto o_r2 = a.r2 ? G(a.r2) + t0 : nullptr;
    const long long radius = a.radius;
    const double r2_min = a.r2_min, k_index = a.key_index, k_member = a.key_member;

    for (int i = tid; i < M; i += CLUMP_T) { s_key[i] = key[i]; s_owner[i] = -1; s_bp[i] = bp[i]; }
    int n = 0;
    __syncthreads();
    for (int step = 0; step < M; step++) {                  // (every step but the last gives one more row an owner)
        double bc = k_index;                                // nothing below key_index leads; a NaN key fails the comparison
        int bi = CLUMP_NONE;
        for (int i = tid; i < M; i += CLUMP_T) {
            const double c = s_key[i];
            if (s_owner[i] == -1 && c >= k_index && clump_better(c, i, bc, bi)) { bc = c; bi = i; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double c2 = __shfl_xor(bc, off, 64);
            const int i2 = __shfl_xor(bi, off, 64);
            if (clump_better(c2, i2, bc, bi)) { bc = c2; bi = i2; }
        }
        if ((tid & 63) == 0) { s_redc[tid >> 6] = bc; s_redi[tid >> 6] = bi; }
        __syncthreads();
        bc = s_redc[0]; bi = s_redi[0];
#pragma unroll
        for (int w = 1; w < CLUMP_NW; w++)
            if (clump_better(s_redc[w], s_redi[w], bc, bi)) { bc = s_redc[w]; bi = s_redi[w]; }
        if (bi == CLUMP_NONE) break;
        const int i = bi;
        n++;
        // the band of the lead: [lo, hi) = the rows with bp_i - radius <= bp <= bp_i + radius (bp never decreases)
        const long long b_lo = (long long)s_bp[i] - radius, b_hi = (long long)s_bp[i] + radius;
        int lo = 0, hi = M;
        for (int r = i; lo < r;) { const int m = (lo + r) >> 1; if ((long long)s_bp[m] < b_lo) lo = m + 1; else r = m; }
        for (int l = i + 1; l < hi;) { const int m = (l + hi) >> 1; if ((long long)s_bp[m] <= b_hi) l = m + 1; else hi = m; }
        if (tid == 0) {
            s_owner[i] = i;
            if (o_rank) o_rank[i] = n;
            if (o_r2) o_r2[i] = 1.0;
        }
        const auto row = R + (size_t)i * (size_t)M;
        for (int j = lo + tid; j < hi; j += CLUMP_T) {
            if (j == i || s_owner[j] != -1 || !(s_key[j] >= k_member)) continue;
            const double r = row[j];
            const double t2 = r * r;
            if (t2 >= r2_min) {
                s_owner[j] = i;
                if (o_r2) o_r2[j] = t2;
            }
        }
        __syncthreads();
    }
    // (a thread that left the loop at `break` did so behind the barrier that follows the last clump's writes)
    for (int i = tid; i < M; i += CLUMP_T) {
        const int o = s_owner[i];
        o_owner[i] = o;
        if (o_rank && o != i) o_rank[i] = 0;
        if (o_r2 && o == -1) o_r2[i] = __builtin_nan("");
    }
    if (tid == 0 && a.n_clumps) G(a.n_clumps)[blockIdx.x] = n;
}

void launch_clump(const ClumpArgs& a, int n_key, hipStream_t s)
{
    if (n_key <= 0 || a.M <= 0) return;
    static DeviceOnce attr_once;
    attr_once.run([&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(clump_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CLUMP_M_MAX * 16);
    });
    hipLaunchKernelGGL(clump_kernel, dim3(n_key), dim3(CLUMP_T), (size_t)a.M * 16, s, a);
}

}  // namespace gauss
