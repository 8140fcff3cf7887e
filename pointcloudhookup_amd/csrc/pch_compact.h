// Order-preserving compaction in ONE sweep with the rows of a tile held in registers: a workgroup of 256 threads takes
// a tile of ROUNDS x 256 consecutive rows, every wave of it ROUNDS x 64, one ballot per round of 64 rows says which
// rows are kept, the tile's output offset comes from the decoupled look-back over the tiles in front of it
// (pch_lookback.h), and the kept rows are written in lane order.  The pieces, in the order a kernel calls them:
//   oc_take_tile -> (the kernel loads its rows and takes its ballots) -> oc_place -> oc_visit [-> oc_fold_box]
// Users: crop_aabb_k (pch_view.hip), pl_filter_k (pch_plane.hip).  The kept-row box at the end of the file is also what
// the height filter's sweeps emit through (gf_compact_k / gf_cand_k / gf_finalize_k, pch_filter.hip); their tile forms
// (masks in LDS, dense survivors, candidate slots) and their ending (two totals, the use_b decision) are their own.
#pragma once
#include "pch_common.h"
#include "pch_lookback.h"

namespace pch {

constexpr int OC_THREADS = 256;
constexpr int OC_WAVES   = OC_THREADS / 64;
constexpr int OC_SLOTS   = 64;                              // slot sets a sweep's box is spread over (see oc_fold_box)
constexpr uint32_t OC_NONE = 0xFFFFFFFFu;                   // oc_place: the tile keeps nothing (offsets stay below 2^32 - 1)

// the one carve-up of such a sweep's workspace (size query and call): its state, then one look-back word per tile
template <class State, int TILE>
struct OcWs {
    int64_t   nt;
    State*    st;
    uint64_t* status;
    OcWs(Arena& a, int64_t n) : nt(ceil_div(n > 0 ? n : 1, TILE)) {
        st = a.take<State>(1);
        status = a.take<uint64_t>(nt);
    }
    static size_t bytes(int64_t n) { Arena a; OcWs w(a, n); return a.off; }
};

// ---- take a tile (every thread of the workgroup calls; contains a barrier).
// FORWARD PROGRESS: the look-back waits for every tile in front of this one, so the tile order must be an order in
// which workgroups START: HIP promises nothing about blockIdx dispatch order, and a resident workgroup spinning on a
// tile that was never scheduled would hang the GPU.  The logical tile is therefore a ticket drawn on arrival (as
// rocPRIM's look-back scan does): every tile with a smaller ticket belongs to a workgroup that is already running.
// *ticket is zero before the launch.
__device__ __forceinline__ int64_t oc_take_tile(uint32_t* __restrict__ ticket) {
    __shared__ uint32_t tile_sh;
    if (threadIdx.x == 0) tile_sh = atomicAdd(ticket, 1u);
    __syncthreads();
    return tile_sh;
}

// ---- the count word of a sweep (ONE lane per tile calls).  It starts at 0: the last tile adds the total (< 2^62), a
// tile whose look-back wait ran out of its budget sets the sign bit - idempotent, so the word reads negative iff some
// tile failed, however many did (every tile behind a poisoned one fails too) and in whatever order the two happen.
__device__ __forceinline__ void oc_count_update(unsigned long long* __restrict__ count, bool lb_failed, bool last_tile,
                                                unsigned long long total) {
    if (lb_failed) atomicOr(count, 1ull << 63);
    else if (last_tile) atomicAdd(count, total);
}

// first output row of wave w: the tile's prefix plus the kept rows of the waves in front
__device__ __forceinline__ uint32_t oc_wave_offset(uint32_t excl, const uint32_t (&wtot)[OC_WAVES], int w) {
    uint32_t woff = excl;
    for (int w2 = 0; w2 < w; ++w2) woff += wtot[w2];
    return woff;
}

// ---- place a tile (every thread calls; two barriers).  m: the ballots of this wave's rounds.  The wave totals go to
// LDS, wave 0 obtains the tile's exclusive prefix by look-back and updates the count word.  Returns this wave's first
// output row, or OC_NONE when the tile keeps nothing (workgroup-uniform).
template <int ROUNDS>
__device__ __forceinline__ uint32_t oc_place(const unsigned long long (&m)[ROUNDS], uint64_t* __restrict__ status,
                                             int64_t tile, int64_t* __restrict__ out_count) {
    __shared__ uint32_t wtot[OC_WAVES];
    __shared__ uint32_t excl_sh;
    const int w = wave_id(), l = lane_id();
    uint32_t run = 0;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) run += (uint32_t)__popcll(m[r]);
    if (l == 0) wtot[w] = run;
    __syncthreads();
    const uint32_t T = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    if (w == 0) {
        const uint32_t e0 = gf_lookback(status, tile, T);
        const bool lb_failed = e0 == GF_LB_FAILED;
        const uint32_t e = lb_failed ? 0u : e0;              // prefix 0 keeps the writes of oc_visit inside the output
        if (l == 0) {
            excl_sh = e;
            oc_count_update(reinterpret_cast<unsigned long long*>(out_count), lb_failed,
                            tile == (int64_t)gridDim.x - 1, (unsigned long long)e + T);
        }
    }
    __syncthreads();
    return T == 0 ? OC_NONE : oc_wave_offset(excl_sh, wtot, w);
}
static_assert(OC_WAVES == 4, "oc_place sums four wave totals");

// ---- visit the kept rows of this lane in file order: f(round, output row); woff is what oc_place returned
template <int ROUNDS, class F>
__device__ __forceinline__ void oc_visit(const unsigned long long (&m)[ROUNDS], uint32_t woff, F&& f) {
    const int l = lane_id();
    const uint64_t lt = lanemask_lt();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        if ((m[r] >> l) & 1ull) f(r, (int64_t)woff + (uint32_t)__popcll(m[r] & lt));
        woff += (uint32_t)__popcll(m[r]);
    }
}

// ---- the centred float32 rows of stage B and the box of the finite ones.  Kept row (x, y, z) = input row `row`
// becomes output row o, centred; lo / hi collect the box as ordered uint32 (lo holds ~ordered(min)), so that
// everything folds with max and 0 is the neutral start
__device__ __forceinline__ void oc_emit(float x, float y, float z, const float (&c)[3], int64_t o, int64_t row,
                                        float* __restrict__ out_points, int32_t* __restrict__ out_index,
                                        uint32_t (&lo)[3], uint32_t (&hi)[3]) {
    const float v[3] = {x - c[0], y - c[1], z - c[2]};       // points = raw_points - centroid (float32)
    out_points[3 * o + 0] = v[0];
    out_points[3 * o + 1] = v[1];
    out_points[3 * o + 2] = v[2];
    if (out_index) out_index[o] = (int32_t)row;
    if (fabsf(v[0]) < INFINITY && fabsf(v[1]) < INFINITY && fabsf(v[2]) < INFINITY) {   // NaN/inf rows
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t kk = f32_ordered(v[a]);
            lo[a] = ~kk > lo[a] ? ~kk : lo[a];
            hi[a] = kk > hi[a] ? kk : hi[a];
        }
    }
}
// the tile's box: over the wave, over the waves, into one of the sweep's OC_SLOTS slot sets (zeroed before the launch;
// every thread calls, one barrier)
__device__ __forceinline__ void oc_fold_box(uint32_t (*__restrict__ slots)[6], int64_t tile, uint32_t (&lo)[3],
                                            uint32_t (&hi)[3], uint32_t (&box)[OC_WAVES][6]) {
    const int w = wave_id();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = wave_reduce_max(lo[a]);
        hi[a] = wave_reduce_max(hi[a]);
        if (lane_id() == 0) { box[w][a] = lo[a]; box[w][3 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        uint32_t v = box[0][a];
        for (int w2 = 1; w2 < OC_WAVES; ++w2) v = box[w2][a] > v ? box[w2][a] : v;
        if (v) atomicMax(&slots[tile % OC_SLOTS][a], v);
    }
}
// word a (0..2 min xyz, 3..5 max xyz) of the box the slot sets hold; zeros when no finite row was kept
__device__ __forceinline__ float oc_box_word(const uint32_t (*__restrict__ slots)[6], int a) {
    uint32_t v = 0u;
    for (int k = 0; k < OC_SLOTS; ++k) { const uint32_t u = slots[k][a]; v = u > v ? u : v; }
    return v == 0u ? 0.0f : f32_unordered(a < 3 ? ~v : v);
}

}  // namespace pch
