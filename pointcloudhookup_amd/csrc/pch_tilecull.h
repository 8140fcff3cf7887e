// What every sweep of row tiles over a culled item table shares (pch_crop.hip over boxes, pch_clearance.hip and
// pch_treefall.hip over spans): the workgroup's bounding box out of the lanes' boxes, the bitmap of the items whose cull
// bounds meet it, and the wave-uniform walk of that bitmap.  The kernel fills the lane box itself - which rows it boxes
// is what differs between the sweeps - and declares the LDS arrays.
#pragma once
#include "pch_common.h"

#include <math.h>

namespace pch {

#ifdef __HIPCC__
// the workgroup's box out of every lane's: on return lo / hi hold it in every lane.  wlo / whi: one slot per wave (LDS).
// One barrier.
template <int WAVES>
__device__ __forceinline__ void cull_tile_box(double (&lo)[3], double (&hi)[3], double (&wlo)[WAVES][3],
                                              double (&whi)[WAVES][3]) {
    const int w = wave_id(), l = lane_id();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = wave_reduce_min(lo[a]);
        hi[a] = wave_reduce_max(hi[a]);
        if (l == 0) { wlo[w][a] = lo[a]; whi[w][a] = hi[a]; }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int w2 = 0; w2 < WAVES; ++w2) { lo[a] = fmin(lo[a], wlo[w2][a]); hi[a] = fmax(hi[a], whi[w2][a]); }
}

// the items this tile has to visit, as a bitmap in item order (active: (count + 63) / 64 words of LDS): those that take
// part and whose bounds are not all finite or meet the tile's box.  bounds(t, blo, bhi) says whether item t takes part
// and where its three lower and three upper bounds stand.  Bounds that are not all finite mean "could not be bounded"
// (-inf / +inf, or NaN, which fails every comparison): such an item is never culled.  An empty box (lo = +inf,
// hi = -inf) meets nothing.  Ends with a barrier: `active` may be read behind it.
template <int WAVES, class Bounds>
__device__ __forceinline__ void cull_tile_bitmap(uint64_t* active, int count, const double (&lo)[3],
                                                 const double (&hi)[3], Bounds bounds) {
    const int l = lane_id();
    const int nwords = (count + 63) >> 6;
    for (int c = wave_id(); c < nwords; c += WAVES) {
        const int t = c * 64 + l;
        bool on = false;
        const double *blo, *bhi;
        if (t < count && bounds(t, blo, bhi)) {
            bool finite = true, meets = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                finite = finite && isfinite(blo[a]) && isfinite(bhi[a]);
                meets = meets && lo[a] <= bhi[a] && hi[a] >= blo[a];
            }
            on = !finite || meets;
        }
        const uint64_t m = __ballot(on);
        if (l == 0) active[c] = m;
    }
    __syncthreads();
}

// next set bit of the tile's bitmap at or behind (word, bits): wave-uniform, so that the item's record behind it comes
// through scalar loads.  Start with word = -1, bits = 0; bits = what is left of word `word`.  Returns the item or -1.
__device__ __forceinline__ int cull_next_bit(const uint64_t* active, int nwords, int& word, uint64_t& bits) {
    while (bits == 0) {
        if (++word >= nwords) return -1;
        const uint64_t v = active[word];
        bits = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) |
               (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
    }
    const int t = word * 64 + (int)__builtin_ctzll(bits);
    bits &= bits - 1;
    return t;
}
#endif  // __HIPCC__

}  // namespace pch
