// K1r: resample-pack for simulateLD (simulateLD.cpp:161-199).  The reference builds geno_mat [M x sim_size] from drawn panel
// samples, leaves the columns past the draws at 0 and runs CalCor (n = sim_size) over every row pair.  Here the drawn columns
// of one measured row are written as the Gram operand -- the encoding of pack_stats_kernel (k_pack_epilogue.hip) -- with the
// row's pooled integer sums; the Gram kernel and the pooled LD epilogue then run unchanged with Prob::N = sim_size.  The zero
// columns add nothing to any sum: they only enter through n.
//
// Compiled with -ffp-contract=off: rt_sd follows CalCor's sqrt(n*sumxsq - sumx*sumx) (util.cpp:66-67) operation by operation,
// as pack_stats_kernel does.
#include "gauss_internal.h"

namespace gauss {

struct __attribute__((packed)) SimU32 { uint32_t v; };

// Prob::draw_col holds the source column of every packed column [0, Kp), sorted ascending, -1 past the draws.  A column is
// a byte index into a one-byte row (code = byte & 0x0F), or a 2-bit sample index into a packed row (sample c at bits 2 (c % 4)
// of byte c / 4).  STAGED: the whole source row (Prob::row_src_bytes, <= SIMLD_LDS_MAX) is first copied into LDS with dword
// loads -- the sorted columns then read it nearly in order there instead of as single-byte gathers from HBM; a row too long for
// LDS is read from global memory directly (sorted columns: neighbouring lanes still share cache lines).
template <bool STAGED>
__global__ __launch_bounds__(256) void resample_pack_kernel(const Prob* __restrict__ probs, const int2* __restrict__ rowmap)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_row[];
    __shared__ int s_sum[2][4];
    const int2 rm = rowmap[blockIdx.x];
    const Prob& pb = probs[rm.x];
    const int r = rm.y;                                   // a measured row (resampled windows have no unmeasured part)
    const long long srow = pb.rows_m ? pb.rows_m[r] : r;
    const uint8_t* src = pb.raw_m + (size_t)srow * pb.ld_raw;
    const bool fmt2 = pb.geno_fmt != 0;
    if (STAGED) {
        const int nb = pb.row_src_bytes;
        const int nd = nb >> 2;
        uint32_t* s32 = reinterpret_cast<uint32_t*>(s_row);
        // four dword loads in flight per lane before the first LDS store (a row is 8-33 KB: latency, not bandwidth)
        for (int d0 = threadIdx.x; d0 < nd; d0 += 4 * 256) {
            uint32_t v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int d = d0 + 256 * j;
                v[j] = d < nd ? reinterpret_cast<const SimU32*>(src + 4 * (size_t)d)->v : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (d0 + 256 * j < nd) s32[d0 + 256 * j] = v[j];
        }
        for (int b = (nd << 2) + threadIdx.x; b < nb; b += 256) s_row[b] = src[b];
        __syncthreads();
    }
    auto code = [&](int c) -> uint32_t {
        if (c < 0) return 0u;
        if (fmt2) {
            const uint32_t byte = STAGED ? s_row[c >> 2] : src[c >> 2];
            return (byte >> (2 * (c & 3))) & 3u;
        }
        return (uint32_t)(STAGED ? s_row[c] : src[c]) & 0x0Fu;      // '0'..'9' and 0..15 both decode as byte & 0x0F
    };

    const int nwords = pb.Kp >> 4;                        // a multiple of 4 (Kp is a multiple of 64)
    const int nloop = (nwords + 255) & ~255;
    uint4* dst = reinterpret_cast<uint4*>(pb.packed + (size_t)r * pb.Kp);
    const int4* cols = reinterpret_cast<const int4*>(pb.draw_col);
    int sx = 0, sxx = 0;
    for (int w0 = threadIdx.x; w0 < nloop; w0 += 256) {
        const bool live = w0 < nwords;                    // whole waves stay in the loop for the lane exchange below
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (live) {
            int4 c[4];
#pragma unroll
            for (int q = 0; q < 4; q++) c[q] = cols[4 * w0 + q];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = code(c[q].x) | code(c[q].y) << 8 | code(c[q].z) << 16 | code(c[q].w) << 24;
        }
        // pack_stats_kernel's finish_word for one pseudo-population: sums, operand encoding, chunk_unit_layout store
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t x = v[q];
            sx = __builtin_amdgcn_udot4(x, 0x01010101u, sx, false);
            sxx = __builtin_amdgcn_udot4(x, x, sxx, false);
            uint32_t c;
            if (pb.gram_i8) {
                c = x;
            } else if (fmt2 || (x & 0x08080808u) == 0) {
                c = __builtin_amdgcn_perm(0x4E4C4A48u, 0x44403800u, x);        // e4m3 of 0..7 as an eight-entry byte table
            } else {
                c = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const uint32_t t = (x >> (8 * b)) & 0xFu;
                    const uint32_t e = t == 0 ? 0u : t == 1 ? 0x38u : t < 4 ? 0x40u + 4u * (t - 2) : t < 8 ? 0x48u + 2u * (t - 4) : 0x50u + (t - 8);
                    c |= e << (8 * b);
                }
            }
            v[q] = c;
        }
        const bool odd = (w0 & 1) != 0;
        const uint32_t s0 = odd ? v[0] : v[1], s1 = odd ? v[2] : v[3];
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s0, 0xB1, 0xF, 0xF, true);    // lane ^ 1
        const uint32_t r1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s1, 0xB1, 0xF, 0xF, true);
        if (live) dst[w0] = odd ? make_uint4(r0, r1, v[1], v[3]) : make_uint4(v[0], v[2], r0, r1);
    }
    // exact integer sums: the order of the adds changes no bit
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sx += __shfl_xor(sx, off);
        sxx += __shfl_xor(sxx, off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_sum[0][wave] = sx; s_sum[1][wave] = sxx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int isx = s_sum[0][0] + s_sum[0][1] + s_sum[0][2] + s_sum[0][3];
        const int isxx = s_sum[1][0] + s_sum[1][1] + s_sum[1][2] + s_sum[1][3];
        pb.sx[r] = isx;
        pb.sxx[r] = isxx;
        // pooled row tables of pack_stats_kernel with num_samples = N = sim_size (CalCor's n, simulateLD.cpp:258)
        const double sumx = (double)isx, sumxsq = (double)isxx;
        pb.rt_wm[r] = sumx;
        pb.rt_sd[r] = sqrt((pb.N) * sumxsq - sumx * sumx);
    }
}

int resample_pack_lds_bytes(long long row_src_bytes)
{
    const long long b = (row_src_bytes + 15) / 16 * 16;
    return (b > 0 && b <= SIMLD_LDS_MAX) ? (int)b : 0;
}

void launch_resample_pack(const Prob* d_probs, const int2* d_rowmap, int n_rows, int lds_bytes, hipStream_t s)
{
    if (n_rows <= 0) return;
    if (lds_bytes > 0)
        hipLaunchKernelGGL(resample_pack_kernel<true>, dim3(n_rows), dim3(256), lds_bytes, s, d_probs, d_rowmap);
    else
        hipLaunchKernelGGL(resample_pack_kernel<false>, dim3(n_rows), dim3(256), 0, s, d_probs, d_rowmap);
}

}  // namespace gauss
