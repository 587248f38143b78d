// What the multi-causal fit (k_susie.hip) and the colocalisation of its traits (k_coloc.hip) share: the window and the fitted trait a
// workgroup works on, and the workgroup's reductions in their fixed order.
#pragma once
#include "k_cs_common.h"

namespace gauss {

constexpr int SUSIE_NW = SUSIE_T / 64;

#if defined(__HIPCC__)
__device__ __forceinline__ const Prob& susie_prob(const Prob* probs, const int* map, int y) { return probs[map ? map[y] : y]; }
__device__ __forceinline__ SusieWs susie_ws_of(const Prob& pb) { return susie_ws(pb.M, pb.U, pb.Mld, pb.susie_L, !pb.susie_measured_only); }

// One fitted trait of a window, t = 0 .. susie_k.  Trait 0 is z1 with out_z, the state at the offsets of SusieWs, susie_mem and
// out_susie as they are; further trait t reads row t - 1 of the further traits' scores (traits_Z, SNP-major) and of their imputed
// Z-scores (out_traits), and has its own block of the workspace, its own membership bytes and its own block of out_susie_more.
struct SusieTrait {
    GP(double) st;             // the trait's state: st + SusieWs::zhat .. keep (W and Y stay at susie_ws + their offsets)
    GP(const double) z;        // measured score of SNP j: z[j * zs]
    int zs;
    GP(const double) zu;       // [U] imputed Z-scores (z / sqrt(info)) of the unmeasured SNPs
    GP(uint8_t) mem;           // [L][tld]
    GP(double) out;            // [susie_layout.count]
    GP(double) out_lbf;        // [L][T] where the section holds the lbf rows (Prob::susie_lbf)
};
__device__ __forceinline__ SusieTrait susie_trait(const Prob& pb, const SusieWs& o, int t)
{
    const int T = pb.M + pb.U, L = pb.susie_L;
    const SusieMoreLayout m = susie_more_layout(T, L, pb.susie_am != 0, pb.susie_lbf != 0, pb.susie_k, pb.coloc != 0);
    if (t == 0) return {pb.susie_ws, pb.z1, 1, pb.out_z, pb.susie_mem, pb.out_susie, pb.out_susie_more + m.lbf};
    const auto blk = pb.out_susie_more + m.trait + (size_t)(t - 1) * m.one;
    return {pb.susie_ws + (size_t)t * o.trait, pb.traits_Z + (t - 1), traits_t16(pb.traits_T), pb.out_traits + (size_t)(t - 1) * pb.U,
            pb.susie_mem + (size_t)t * L * cs_tld(T), blk, blk + m.tlbf};
}

// log Bayes factor of a single effect of prior variance V at a candidate of residual score r and variance d
__device__ __forceinline__ double susie_lbf(double r, double d, double V)
{
    if (V == 0.0) return 0.0;
    const double vd = V * d;
    return 0.5 * (r * r * V / (1.0 + vd) - log1p(vd));
}

// the sweeps the fit ran: what the step that saw it converge wrote down, else all of them
__device__ __forceinline__ int susie_sweeps_of(const Prob& pb, GP(const double) ctl)
{
    const double s = ctl[SUSIE_CTL_SWEEPS];
    const int n = ctl[SUSIE_CTL_DONE] != 0.0 && s >= 0.0 && s <= (double)pb.susie_max_sweeps ? (int)s : pb.susie_max_sweeps;
    return __builtin_amdgcn_readfirstlane(n);
}

// max and sum over the workgroup (SUSIE_T threads) in a fixed order: lanes by xor moves, then the waves ascending
__device__ __forceinline__ double susie_block_max(double x, double* s_red, int tid)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = cs_max(x, __shfl_xor(x, off, 64));
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = x;
    __syncthreads();
    double t = s_red[0];
#pragma unroll
    for (int w = 1; w < SUSIE_NW; w++) t = cs_max(t, s_red[w]);
    return t;
}
__device__ __forceinline__ double susie_block_sum(double x, double* s_red, int tid)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = x;
    __syncthreads();
    double t = s_red[0];
#pragma unroll
    for (int w = 1; w < SUSIE_NW; w++) t += s_red[w];
    return t;
}
#endif

}  // namespace gauss
