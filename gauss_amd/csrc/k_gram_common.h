// Pieces shared by the Gram kernels (k_gram.hip: e4m3 / int8 operands, k_gram_fp6.hip: e2m3 operands): how a wave's
// exact partial sums leave for the partial slabs.
#pragma once
#include "gauss_internal.h"

namespace gauss {

// ---- wave roles: which block of the 128 x 128 tile a workgroup's wave multiplies (host and device) ----------------------
// Item::flags bits 6-7 hold the tile's layout, chosen per item by the planner (tile_layout below; 0 unless the planner
// set it).  QUAD: wave w owns the 64 x 64 quadrant (w >> 1, w & 1).  A tile whose live B rows (output columns) or live A rows
// end in the first 64 leaves two of those quadrants empty, and the waves of a workgroup meet at a barrier every chunk: the narrow
// layouts cut the live half into four blocks instead, 64 rows x 32 columns each (both halves empty, one A row per lane: 32 x 32), so that every
// wave issues half the MFMAs per K step.  Same operand images, same slab addresses, the same sums: only the origins move.
constexpr int LAYOUT_SHIFT = 6;
constexpr int LAYOUT_QUAD = 0, LAYOUT_NARROW_B = 1, LAYOUT_NARROW_A = 2, LAYOUT_NARROW_AB = 3;
struct WaveRole { int r0, c0, rows, cols; };          // origin and extent of the wave's block inside the tile
constexpr WaveRole wave_role(int wave, int layout)
{
    return layout == LAYOUT_NARROW_B    ? WaveRole{(wave >> 1) * 64, (wave & 1) * 32, 64, 32}
           : layout == LAYOUT_NARROW_A  ? WaveRole{0, wave * 32, 64, 32}
           : layout == LAYOUT_NARROW_AB ? WaveRole{(wave >> 1) * 32, (wave & 1) * 32, 32, 32}
                                        : WaveRole{(wave >> 1) * 64, (wave & 1) * 64, 64, 64};
}
// the planner's choice.  Both halves empty: an unpacked item takes the four 32 x 32 blocks; a packed item (two A rows per lane) keeps
// its two 64 x 32 blocks -- one MFMA per wave and K step either way, and 32-row blocks would not pack: twice the MFMAs
constexpr int tile_layout(int rows_a, int rows_b, bool packed)
{
    if (rows_a <= 64 && rows_b <= 64) return packed ? LAYOUT_NARROW_B : LAYOUT_NARROW_AB;
    return rows_b <= 64 ? LAYOUT_NARROW_B : (rows_a <= 64 ? LAYOUT_NARROW_A : LAYOUT_QUAD);
}

// What a wave multiplies of an item: na / nb = live 32-row halves of A / of B inside its block; nc > 0 (f32 path): its live B rows
// are nc groups of 16 with the last 32-row half at most half full -- 1 or 3 groups -- and go through the 16-column edge routine.
// sk10: the unpacked 64 x 64 block on the diagonal of a diagonal tile, whose lower-left 32 x 32 sub-block is neither multiplied nor
// stored.  na = 0: the wave only stages.  (A diagonal tile's blocks below the diagonal mirror those above it and no reader of the
// slab looks at them; a packed 64-row block on the diagonal holds one at no cost.)
struct WaveWork { int na, nb, nc; bool sk10; };
constexpr WaveWork wave_work(int rows_a, int rows_b, bool diag, bool packed, bool edge16, int wave, int layout)
{
    const WaveRole ro = wave_role(wave, layout);
    int na = (rows_a - ro.r0 + 31) / 32, nb = (rows_b - ro.c0 + 31) / 32, nb16 = (rows_b - ro.c0 + 15) / 16;
    na = na < 0 ? 0 : (na > ro.rows / 32 ? ro.rows / 32 : na);
    nb = nb < 0 ? 0 : (nb > ro.cols / 32 ? ro.cols / 32 : nb);
    nb16 = nb16 < 0 ? 0 : (nb16 > ro.cols / 16 ? ro.cols / 16 : nb16);
    if (diag && ro.r0 >= ro.c0 + ro.cols) na = 0;
    const int nc = (edge16 && na > 0 && (nb16 & 1)) ? nb16 : 0;
    return WaveWork{na, nb, nc, diag && !packed && ro.r0 == ro.c0 && na == 2 && nb == 2};
}
// the wave's MFMA issue per K step as a share of a full wave's (what the barrier makes the tile's pace: the largest of the four)
constexpr double wave_load(const WaveWork& w, bool packed)
{
    const int g = w.nc ? w.nc : 2 * w.nb;                  // groups of 16 columns
    return packed ? (w.na > 0 ? g / 4.0 : 0.0) : w.na * g / 8.0;
}

// every layout covers a tile's live entries exactly once, whatever the live extents are (a diagonal tile: those on or above
// the diagonal, at the granularity of the blocks)
constexpr bool layouts_cover()
{
    for (int layout = 0; layout < 4; layout++)
        for (int r = 0; r < 128; r += 8)
            for (int c = 0; c < 128; c += 8) {
                int n = 0;
                for (int w = 0; w < 4; w++) {
                    const WaveRole ro = wave_role(w, layout);
                    n += (r >= ro.r0 && r < ro.r0 + ro.rows && c >= ro.c0 && c < ro.c0 + ro.cols) ? 1 : 0;
                }
                const bool in = ((layout & LAYOUT_NARROW_B) ? c < 64 : true) && ((layout & LAYOUT_NARROW_A) ? r < 64 : true);
                if (n != (in ? 1 : 0)) return false;
            }
    return true;
}
static_assert(layouts_cover(), "a layout's four blocks tile its live part exactly once");

#if defined(__HIPCC__)
__device__ __forceinline__ float slab_bits(float v) { return v; }
__device__ __forceinline__ float slab_bits(int v) { return __int_as_float(v); }
// 16-bit slabs: the exact sum as an unsigned integer; rows 2k and 2k + 1 of a column share one dword
__device__ __forceinline__ uint32_t slab_u(float v) { return (uint32_t)v; }
__device__ __forceinline__ uint32_t slab_u(int v) { return (uint32_t)v; }
__device__ __forceinline__ float slab_pair(uint32_t lo, uint32_t hi) { return __uint_as_float((lo & 0xFFFFu) | (hi << 16)); }

// End of a K segment: the wave's four 32 x 32 accumulators go to that segment's slab.
// C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
// obase / obase16: the lane's first entry in a slab of f32 (int32) values / of uint16 row pairs.
template <int NA, int NB, bool SK10, typename OUT, typename ACC>
__device__ __forceinline__ void flush_acc(OUT out, bool slab16, int obase, int obase16, const ACC& acc00, const ACC& acc01,
                                          const ACC& acc10, const ACC& acc11)
{
    if (slab16) {
        // accumulator registers r and r + 1 (r even) are rows 2k and 2k + 1 of the same column: one dword
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const int o = obase16 + (((r & 3) + 8 * (r >> 2)) >> 1) * TILE;
            out[o] = slab_pair(slab_u(acc00[r]), slab_u(acc00[r + 1]));
            if (NB > 1) out[o + 32] = slab_pair(slab_u(acc01[r]), slab_u(acc01[r + 1]));
            if (NA > 1) {
                if (!SK10) out[o + 16 * TILE] = slab_pair(slab_u(acc10[r]), slab_u(acc10[r + 1]));
                if (NB > 1) out[o + 16 * TILE + 32] = slab_pair(slab_u(acc11[r]), slab_u(acc11[r + 1]));
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int o = obase + ((r & 3) + 8 * (r >> 2)) * TILE;
            out[o] = slab_bits(acc00[r]);
            if (NB > 1) out[o + 32] = slab_bits(acc01[r]);
            if (NA > 1) {
                if (!SK10) out[o + 32 * TILE] = slab_bits(acc10[r]);
                if (NB > 1) out[o + 32 * TILE + 32] = slab_bits(acc11[r]);
            }
        }
    }
}
#endif  // __HIPCC__

}  // namespace gauss
