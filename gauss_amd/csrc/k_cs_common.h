// The membership step of a credible set, shared by the credible sets of the selected signals (k_cs.hip) and the sets of the
// multi-causal fit (k_susie.hip): both turn one row of log Bayes factors into pips and count the mass ranked ahead of every
// candidate, and must do so with the same sums in the same order -- the reductions and the row's body live here.
#pragma once
#include "gauss_internal.h"

namespace gauss {

constexpr int CS_LDS_T = 4096;               // a row of up to this many pips sits in LDS: 32 KB
constexpr int CS_SET_NW = CS_SET_T / 64;

#if defined(__HIPCC__)
// the order of the max: a NaN is never better
__device__ __forceinline__ double cs_max(double a, double b) { return b > a ? b : a; }

// sum over the workgroup in a fixed order: the lanes of a wave by xor moves, then the waves ascending
__device__ __forceinline__ double cs_block_sum(double x, double* s_red, int tid)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    __syncthreads();                                        // (s_red may still be read from the reduction before)
    if ((tid & 63) == 0) s_red[tid >> 6] = x;
    __syncthreads();
    double t = s_red[0];
#pragma unroll
    for (int w = 1; w < CS_SET_NW; w++) t += s_red[w];
    return t;
}

// One row of T log Bayes factors (g_row, -inf for a non-candidate) by one workgroup of CS_SET_T threads: lse, pip in place, then the
// mass ranked ahead of every candidate counted directly, j ascending, and the membership bytes (mem).  s_row [CS_LDS_T] and
// s_red [CS_SET_NW] are the workgroup's LDS.  Every thread returns the same size, mass and lse.
__device__ __forceinline__ void cs_set_row(double* const g_row, uint8_t* const mem, const int T, const double rho, double* const s_row,
                                           double* const s_red, const int tid, double& size_out, double& mass_out, double& lse_out)
{
    const bool in_lds = T <= CS_LDS_T;
    double* const row = in_lds ? s_row : g_row;
    // the row's max (sel[a] is always a candidate: it is finite unless a NaN has come in), then lse
    double mx = -__builtin_inf();
    for (int i = tid; i < T; i += CS_SET_T) mx = cs_max(mx, g_row[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = cs_max(mx, __shfl_xor(mx, off, 64));
    if ((tid & 63) == 0) s_red[tid >> 6] = mx;
    __syncthreads();
    mx = s_red[0];
#pragma unroll
    for (int w = 1; w < CS_SET_NW; w++) mx = cs_max(mx, s_red[w]);
    double sum = 0.0;
    for (int i = tid; i < T; i += CS_SET_T) sum += exp(g_row[i] - mx);
    sum = cs_block_sum(sum, s_red, tid);
    const double lse = mx + log(sum);
    // pip in place: a thread rewrites the entries it alone has read
    for (int i = tid; i < T; i += CS_SET_T) {
        const double p = exp(g_row[i] - lse);
        g_row[i] = p;
        if (in_lds) s_row[i] = p;
    }
    __syncthreads();                                        // (workgroup scope covers the global row too: this workgroup alone reads it)
    // membership: the mass ranked ahead of i, j ascending; every lane reads the same row[j] at a time
    double mass = 0.0, size = 0.0;
    for (int i = tid; i < T; i += CS_SET_T) {
        const double p = row[i];
        double ahead = 0.0;
        for (int j = 0; j < T; j++) {
            const double q = row[j];
            if (q > p || (q == p && j < i)) ahead += q;
        }
        const bool in = p > 0.0 && (ahead < rho || rho >= 1.0);      // (rho = 1: the rounded mass ahead may reach 1, the exact one cannot)
        mem[i] = in ? 1 : 0;
        if (in) { mass += p; size += 1.0; }
    }
    mass_out = cs_block_sum(mass, s_red, tid);
    size_out = cs_block_sum(size, s_red, tid);
    lse_out = lse;
}
#endif

}  // namespace gauss
