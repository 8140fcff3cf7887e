// What the sweeps over rows and span polylines share (pch_clearance.hip, pch_treefall.hip): the tile geometry, the
// per-span cull record that cl_bounds_k writes (its derivation stands in front of the kernel, in pch_clearance.hip) and
// the wave-uniform walk of a tile's span bitmap.
#pragma once
#include "pch_common.h"

namespace pch {

constexpr int CL_THREADS = 256;
constexpr int CL_ROUNDS  = 4;
constexpr int CL_TILE    = CL_THREADS * CL_ROUNDS;          // 1024 rows per workgroup
constexpr int CL_WAVES   = CL_THREADS / 64;
constexpr int CL_MAXSPAN = 4096;
constexpr int CL_MAXSEG  = 128;
constexpr int CL_WORDS   = CL_MAXSPAN / 64;                 // words of the active-span bitmap

// what the sweep knows of a span beside the caller's records: cull bounds (world), along-track and height intervals
// (span frame)
struct ClSpan { double lo[3], hi[3], flo, fhi, wlo, whi; };

// cl_bounds_k on the stream: per span the "takes part" flag and the cull record for `radius`, the largest radius any
// row of the sweep behind it is measured with (nspans > 0)
int cl_bounds_run(const double* curves5, const double* segs, int nspans, int nseg, double radius, ClSpan* out,
                  uint32_t* take, hipStream_t s);

#ifdef __HIPCC__
// next set bit of the tile's span bitmap at or behind (word, bits): wave-uniform (cb_next_box)
__device__ __forceinline__ int cl_next_span(const uint64_t* active, int nwords, int& word, uint64_t& bits) {
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
