// Tree fall: for every row of a cloud its height above the terrain grid and, where that height makes it
// vegetation, the squared distance from its ground foot (X, Y, g) to the nearest fitted span curve within its own reach
// R = (H + grow) + limit; per span the rows attributed to it, those that strike, the smallest distance, the tallest row
// and their rows.  The rule is spelled out in include/pch_hip.h; every output is the rule's, bit for bit, whatever is
// culled here.
//   bounds  : cl_bounds_k (pch_clearance.hip) at radius = Rmax = (h_max + grow) + limit.  fl(.) is monotone, so every
//             row that takes part has reach <= fl(h_max + grow), R <= Rmax and R2 <= fl(Rmax * Rmax): whatever the
//             bounds' derivation excludes at Rmax no row can accept at its own R
//   sweep   : tiles of 1024 rows.  Its own: the loads (issued as cl_sweep_k's), the ground under every row
//             (tl_ground_at, the terrain rule's own function), its height, whether it takes part and its own R2, the
//             lane's box over the FEET of the rows that take part; dist2, span, height and class for every row of the
//             tile; per owning span the count and the strikes tallied in LDS, the smallest distance and the largest
//             height folded with integer atomics on cl_minkey and on the order-preserving key.  Shared
//             (pch_spancull.h, pch_tilecull.h): the tile's box and span bitmap (cl_tile_spans), the walk of the spans
//             with the row's own R2 in the tests in front of the segment loop (cl_walk_spans), the loop over a round's
//             owning spans (cl_fold_owners), the tallies added once per (tile, span) (cl_flush_hist)
//   finish  : one pass over dist2, span and height - the lowest rows that attain a span's two extremes; the table
// No inline assembly, no floating-point atomic, nothing waits on another workgroup; the same bits on every run.
#include "pch_common.h"
#include "pch_spancull.h"
#include "pch_terrain.h"

#include <math.h>

namespace pch {

// tally / strikes / maxinv: ClWs's tally / second / maxinv; maxkey: per span the largest f32_ordered(height) - the height
// of a row that takes part is finite, and only a NaN with every bit set has the key zero, so zero = no row yet.  All
// zeroed by the caller.  stats (4 words): the rows that took part, the uncovered rows, the (row, span) segment loops run
// and the (tile, span) pairs walked.
__global__ __launch_bounds__(CL_THREADS) void tf_sweep_k(
    const float* __restrict__ xyz, const uint8_t* __restrict__ skip, int64_t n, TlSub sub, TlGrid grid,
    const float* __restrict__ ground, const double* __restrict__ curves5, const double* __restrict__ segs, int nspans,
    int nseg, const ClSpan* __restrict__ sp, const uint32_t* __restrict__ take, double h_min, double h_max, double grow,
    double limit, double* __restrict__ out_dist2, int32_t* __restrict__ out_span, float* __restrict__ out_height,
    uint8_t* __restrict__ out_class, unsigned long long* __restrict__ tally, unsigned long long* __restrict__ strikes,
    unsigned long long* __restrict__ maxinv, uint32_t* __restrict__ maxkey, unsigned long long* __restrict__ stats) {
    __shared__ uint64_t active[CL_WORDS];
    __shared__ uint32_t hist[CL_MAXSPAN];                // count in the low half, strikes in the high half
    __shared__ double wlo[CL_WAVES][3], whi[CL_WAVES][3];
    const int w = wave_id(), l = lane_id();
    const int64_t base = (int64_t)blockIdx.x * CL_TILE + (int64_t)w * (64 * CL_ROUNDS);
    const TlRow* __restrict__ rows = reinterpret_cast<const TlRow*>(xyz);
    TlRow q[CL_ROUNDS];
    uint8_t sk[CL_ROUNDS];
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        q[r] = rows[i < n ? i : 0];
    }
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        sk[r] = skip ? skip[i < n ? i : 0] : (uint8_t)0;
    }
    for (int j = threadIdx.x; j < nspans; j += CL_THREADS) hist[j] = 0;
    // the ground under every row, once, before the cull: the foot (X, Y, g) is what is measured and what is boxed
    double gd[CL_ROUNDS];
    bool fin[CL_ROUNDS];
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) {
        q[r] = tl_frame(q[r], sub);
        fin[r] = isfinite(q[r].x) && isfinite(q[r].y) && isfinite(q[r].z);
        gd[r] = fin[r] ? tl_ground_at(grid, ground, (double)q[r].x, (double)q[r].y) : (double)tl_nan();
    }
    // height, participation, the row's own R2, and the tile's bounding box over the feet of the rows that take part
    // (no other row can be accepted)
    bool ok[CL_ROUNDS];
    float hf[CL_ROUNDS];
    double R2[CL_ROUNDS];
    uint32_t part = 0, bare = 0;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        const bool none = gd[r] != gd[r];
        const double H = (double)q[r].z - gd[r];
        hf[r] = none ? tl_nan() : (float)H;
        const bool alive = i < n && sk[r] == 0 && fin[r];
        ok[r] = alive && !none && h_min <= H && H <= h_max;
        const double reach = H + grow;
        const double R = reach + limit;
        R2[r] = R * R;
        part += ok[r] ? 1u : 0u;
        bare += (alive && none) ? 1u : 0u;
        if (ok[r]) {
            lo[0] = fmin(lo[0], (double)q[r].x); hi[0] = fmax(hi[0], (double)q[r].x);
            lo[1] = fmin(lo[1], (double)q[r].y); hi[1] = fmax(hi[1], (double)q[r].y);
            lo[2] = fmin(lo[2], gd[r]);          hi[2] = fmax(hi[2], gd[r]);
        }
    }
    cl_tile_spans(active, nspans, sp, take, lo, hi, wlo, whi);

    double best[CL_ROUNDS];
    int who[CL_ROUNDS];
    uint32_t ran, walked;
    cl_walk_spans(active, nspans, curves5, segs, nseg, sp, q, ok, [&](int r) { return gd[r]; },
                  [&](int r) { return R2[r]; }, best, who, ran, walked);

    // the four per-row outputs for every row of the tile; per span of a wave's round one LDS add and one fold of the
    // smallest distance and of the largest height
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        const double reach = ((double)q[r].z - gd[r]) + grow;
        const double s2 = reach * reach;
        const bool hit = who[r] >= 0 && best[r] <= s2;
        if (i < n) {
            out_dist2[i] = best[r];
            out_span[i] = who[r];
            out_height[i] = hf[r];
            out_class[i] = who[r] < 0 ? (uint8_t)PCH_TREEFALL_CLEAR : hit ? (uint8_t)PCH_TREEFALL_STRIKE
                                                                          : (uint8_t)PCH_TREEFALL_NEAR;
        }
        cl_fold_owners(who[r], [&](int k, bool same, uint32_t owned) {
            const uint32_t ns = (uint32_t)__popcll(__ballot(same && hit));
            const double v = wave_reduce_min(same ? best[r] : (double)INFINITY);
            const uint32_t top = wave_reduce_max(same ? f32_ordered(hf[r]) : 0u);
            if (l == 0) {
                atomicAdd(&hist[k], owned + (ns << 16));
                atomicMax(&maxinv[k], cl_minkey(v));
                atomicMax(&maxkey[k], top);
            }
        });
    }
    part = wave_reduce_add(part);
    bare = wave_reduce_add(bare);
    if (l == 0) {
        if (part) atomicAdd(&stats[0], (unsigned long long)part);
        if (bare) atomicAdd(&stats[1], (unsigned long long)bare);
        if (ran) atomicAdd(&stats[2], (unsigned long long)ran);
        if (w == 0 && walked) atomicAdd(&stats[3], (unsigned long long)walked);
    }
    __syncthreads();
    cl_flush_hist(hist, nspans, tally, strikes);
}

// the table, and the lowest rows that attain a span's smallest distance and its largest height (out_min_row and
// out_max_row arrive as all ones = -1)
__global__ __launch_bounds__(CL_THREADS) void tf_finish_k(
    const double* __restrict__ dist2, const int32_t* __restrict__ span, const float* __restrict__ height, int64_t n,
    int nspans, const unsigned long long* __restrict__ tally, const unsigned long long* __restrict__ strikes,
    const unsigned long long* __restrict__ maxinv, const uint32_t* __restrict__ maxkey,
    const unsigned long long* __restrict__ stats, int64_t* __restrict__ out_count, int64_t* __restrict__ out_strikes,
    double* __restrict__ out_min_dist2, unsigned long long* __restrict__ out_min_row, float* __restrict__ out_max_height,
    unsigned long long* __restrict__ out_max_row, int64_t* __restrict__ out_stats) {
    const int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
    if (i < nspans) {
        out_count[i] = (int64_t)tally[i];
        out_strikes[i] = (int64_t)strikes[i];
        out_min_dist2[i] = cl_minkey_value(maxinv[i]);
        const uint32_t key = maxkey[i];
        out_max_height[i] = key ? f32_unordered(key) : tl_nan();
    }
    if (out_stats && i < 4) out_stats[i] = (int64_t)stats[i];
    if (i >= n) return;
    const int32_t k = span[i];
    if (k < 0 || k >= nspans) return;
    if (cl_minkey(dist2[i]) == maxinv[k]) atomicMin(&out_min_row[k], (unsigned long long)i);
    if (f32_ordered(height[i]) == maxkey[k]) atomicMin(&out_max_row[k], (unsigned long long)i);
}

struct TfWs : ClWs { uint32_t* maxkey; };
static void tf_plan(Arena& a, int32_t nspans, TfWs& w) {
    cl_plan_front(a, nspans, 4, w);
    w.maxkey = a.take<uint32_t>(cl_slots(nspans));       // in front of sp: the one fill zeroes it too
    cl_plan_back(a, nspans, w);
}
static bool tf_sizes_ok(int64_t n, int32_t nspans, int32_t nseg) { return tl_rows_ok(n) && cl_spans_ok(nspans, nseg); }

}  // namespace pch

using namespace pch;

extern "C" size_t pch_treefall_ws_bytes(int64_t n, int32_t nspans, int32_t nsegments) {
    if (!tf_sizes_ok(n, nspans, nsegments)) return 0;
    Arena a;
    TfWs w;
    tf_plan(a, nspans, w);
    return a.off;
}

extern "C" int pch_treefall_f32(const float* xyz, const uint8_t* skip, int64_t n, const float* sub3_host,
                                const PchTerrainGrid* grid_host, const float* ground, const double* curves5,
                                const double* segs, int32_t nspans, int32_t nsegments, double h_min, double h_max,
                                double grow, double limit, double* out_dist2, int32_t* out_span, float* out_height,
                                uint8_t* out_class, int64_t* out_count, int64_t* out_strikes, double* out_min_dist2,
                                int64_t* out_min_row, float* out_max_height, int64_t* out_max_row, int64_t* out_stats,
                                void* ws, size_t ws_bytes, void* stream) {
    PCH_REQUIRE(tf_sizes_ok(n, nspans, nsegments), "0 <= n < 2^31, 0 <= nspans <= 4096, 1 <= nsegments <= 128");
    TlGrid g;
    PCH_REQUIRE(tl_grid_of(grid_host, g), "the grid needs cell > 0 and finite, nx, ny >= 1 and nx * ny <= 2^24");
    PCH_REQUIRE(isfinite(h_min) && isfinite(h_max) && isfinite(grow) && isfinite(limit) && 0.0 <= h_min &&
                    h_min <= h_max && grow >= 0.0 && limit >= 0.0,
                "h_min, h_max, grow and limit must be finite with 0 <= h_min <= h_max, grow >= 0 and limit >= 0");
    PCH_REQUIRE(ground, "null ground grid");
    PCH_REQUIRE(n == 0 || (xyz && out_dist2 && out_span && out_height && out_class), "null row buffer");
    PCH_REQUIRE(nspans == 0 || (curves5 && segs && out_count && out_strikes && out_min_dist2 && out_min_row &&
                                out_max_height && out_max_row),
                "null span buffer");
    PCH_REQUIRE(ws, "null workspace");
    PCH_DEVICE_GUARD(ws);
    {
        DeviceGuard in(ground);
        if (in.rc != PCH_OK) return in.rc;
    }
    hipStream_t s = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    TfWs w;
    tf_plan(a, nspans, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    // every row that takes part has H <= h_max, and rounding is monotone: reach = fl(H + grow) <= fl(h_max + grow) and
    // R = fl(reach + limit) <= Rmax
    const double rmax = (h_max + grow) + limit;
    PCH_HIP_TRY(hipMemsetAsync(ws, 0, cl_front_bytes(ws, w), s));
    if (nspans > 0) {
        PCH_HIP_TRY(hipMemsetAsync(out_min_row, 0xFF, sizeof(int64_t) * (size_t)nspans, s));
        PCH_HIP_TRY(hipMemsetAsync(out_max_row, 0xFF, sizeof(int64_t) * (size_t)nspans, s));
        PCH_TRY(cl_bounds_run(curves5, segs, (int)nspans, (int)nsegments, rmax, w.sp, w.take, s));
    }
    if (n > 0)
        PCH_LAUNCH("treefall_sweep", tf_sweep_k, dim3((unsigned)ceil_div(n, CL_TILE)), dim3(CL_THREADS), 0, s, xyz, skip,
                   n, tl_sub_of(sub3_host), g, ground, curves5, segs, (int)nspans, (int)nsegments, (const ClSpan*)w.sp,
                   (const uint32_t*)w.take, h_min, h_max, grow, limit, out_dist2, out_span, out_height, out_class,
                   w.tally, w.second, w.maxinv, w.maxkey, w.counters);
    // the finisher walks the rows only where a span can own one; its first threads write the table and the statistics
    const int64_t fin_n = nspans > 0 ? n : 0;
    int64_t most = fin_n > nspans ? fin_n : (int64_t)nspans;
    if (most < 4) most = 4;
    if (nspans > 0 || out_stats)
        PCH_LAUNCH("treefall_finish", tf_finish_k, dim3((unsigned)ceil_div(most, CL_THREADS)), dim3(CL_THREADS), 0, s,
                   (const double*)out_dist2, (const int32_t*)out_span, (const float*)out_height, fin_n, (int)nspans,
                   (const unsigned long long*)w.tally, (const unsigned long long*)w.second,
                   (const unsigned long long*)w.maxinv, (const uint32_t*)w.maxkey, (const unsigned long long*)w.counters,
                   out_count, out_strikes, out_min_dist2, reinterpret_cast<unsigned long long*>(out_min_row),
                   out_max_height, reinterpret_cast<unsigned long long*>(out_max_row), out_stats);
    return PCH_OK;
}
