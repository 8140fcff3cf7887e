// Tree fall: for every row of a cloud its height above the terrain grid and, where that height makes it
// vegetation, the squared distance from its ground foot (X, Y, g) to the nearest fitted span curve within its own reach
// R = (H + grow) + limit; per span the rows attributed to it, those that strike, the smallest distance, the tallest row
// and their rows.  The rule is spelled out in include/pch_hip.h; every output is the rule's, bit for bit, whatever is
// culled here.
//   bounds  : cl_bounds_k (pch_clearance.hip) at radius = Rmax = (h_max + grow) + limit.  fl(.) is monotone, so every
//             row that takes part has reach <= fl(h_max + grow), R <= Rmax and R2 <= fl(Rmax * Rmax): whatever the
//             bounds' derivation excludes at Rmax no row can accept at its own R
//   sweep   : tiles of 1024 rows (cl_sweep_k's structure): every row and skip load issued before anything is waited
//             for, then the ground under every row (tl_ground_at, the terrain rule's own function), its height and
//             whether it takes part; the tile's bounding box over the FEET of the rows that take part, a bitmap of the
//             spans whose bounds meet it, the spans walked wave-uniformly in ascending order with the segment records
//             through wave-uniform (scalar) loads and the row's own R2 in the tests in front of the segment loop;
//             dist2, span, height and class for every row of the tile, count and strikes tallied per span in LDS and
//             added once per (tile, span), the smallest distance and the largest height folded with integer atomics on
//             the bit pattern and on the order-preserving key
//   finish  : one pass over dist2, span and height - the lowest rows that attain a span's two extremes; the table
// No inline assembly, no floating-point atomic, nothing waits on another workgroup; the same bits on every run.
#include "pch_common.h"
#include "pch_spancull.h"
#include "pch_terrain.h"

#include <math.h>

namespace pch {

// tally / maxinv / maxkey: per span, zeroed by the caller.  maxinv holds the largest ~bits(d2) seen (cl_sweep_k's),
// maxkey the largest f32_ordered(height): the height of a row that takes part is finite, and only a NaN with every bit
// set has the key zero, so zero = no row yet.  stats (4 words): the rows that took part, the uncovered rows, the
// (row, span) segment loops run and the (tile, span) pairs walked.
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
    const int nwords = (nspans + 63) >> 6;
    const int64_t base = (int64_t)blockIdx.x * CL_TILE + (int64_t)w * (64 * CL_ROUNDS);
    const TlRow* __restrict__ rows = reinterpret_cast<const TlRow*>(xyz);
    // every load of the tile is issued before anything is waited for; none stands under a condition
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
        for (int w2 = 0; w2 < CL_WAVES; ++w2) { lo[a] = fmin(lo[a], wlo[w2][a]); hi[a] = fmax(hi[a], whi[w2][a]); }
    // the spans this tile has to walk, as a bitmap in span order: those that take part and whose bounds are not all
    // finite or meet the tile's box (a tile without a row that takes part has an empty box, which meets nothing)
    for (int c = w; c < nwords; c += CL_WAVES) {
        const int t = c * 64 + l;
        bool on = false;
        if (t < nspans && take[t]) {
            const ClSpan& b = sp[t];
            bool finite = true, meets = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                finite = finite && isfinite(b.lo[a]) && isfinite(b.hi[a]);
                meets = meets && lo[a] <= b.hi[a] && hi[a] >= b.lo[a];
            }
            on = !finite || meets;
        }
        const uint64_t m = __ballot(on);
        if (l == 0) active[c] = m;
    }
    __syncthreads();

    double best[CL_ROUNDS];
    int who[CL_ROUNDS];
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) { best[r] = INFINITY; who[r] = -1; }
    uint32_t ran = 0, walked = 0;
    int word = -1;
    uint64_t bits = 0;
    for (int k = cl_next_span(active, nwords, word, bits); k >= 0; k = cl_next_span(active, nwords, word, bits)) {
        const double* __restrict__ c = curves5 + 5 * (size_t)k;
        const double cx = c[0], cy = c[1], cz = c[2], ux = c[3], uy = c[4];
        const double flo = sp[k].flo, fhi = sp[k].fhi, hlo = sp[k].wlo, hhi = sp[k].whi;
        double m[CL_ROUNDS], h[CL_ROUNDS], tt[CL_ROUNDS], g[CL_ROUNDS];
        bool go[CL_ROUNDS];
        bool some = false;
#pragma unroll
        for (int r = 0; r < CL_ROUNDS; ++r) {
            const double dx = (double)q[r].x - cx, dy = (double)q[r].y - cy;
            h[r] = gd[r] - cz;
            m[r] = (dx * ux) + (dy * uy);
            const double t = (dy * ux) - (dx * uy);
            tt[r] = t * t;
            // d2 = g + t*t >= t*t (g >= 0), so a row with t*t > R2 or t*t >= best cannot be taken; nor can one with m
            // outside [flo, fhi] or w outside [wlo, whi]: cl_bounds_k's derivation at Rmax >= R.  A NaN fails every
            // comparison, as it does in the rule.
            go[r] = ok[r] && tt[r] <= R2[r] && tt[r] < best[r] && m[r] >= flo && m[r] <= fhi && h[r] >= hlo &&
                    h[r] <= hhi;
            g[r] = INFINITY;
            some = some || go[r];
        }
        ++walked;
        const uint64_t any = __ballot(some);
        if (any == 0) continue;                          // (wave-uniform)
#pragma unroll
        for (int r = 0; r < CL_ROUNDS; ++r) ran += (uint32_t)__popcll(__ballot(go[r]));
        const double* __restrict__ sg = segs + 5 * (size_t)k * nseg;
        for (int j = 0; j < nseg; ++j) {
            const double mj = sg[5 * j], zj = sg[5 * j + 1], dm = sg[5 * j + 2], dz = sg[5 * j + 3], inv = sg[5 * j + 4];
#pragma unroll
            for (int r = 0; r < CL_ROUNDS; ++r) {
                const double rm = m[r] - mj, rw = h[r] - zj;
                double qq = ((rm * dm) + (rw * dz)) * inv;
                if (qq < 0.0) qq = 0.0;
                if (qq > 1.0) qq = 1.0;
                const double em = rm - (qq * dm), ew = rw - (qq * dz);
                const double d = (em * em) + (ew * ew);
                if (d < g[r]) g[r] = d;
            }
        }
#pragma unroll
        for (int r = 0; r < CL_ROUNDS; ++r) {
            const double d2 = g[r] + tt[r];
            if (go[r] && d2 <= R2[r] && d2 < best[r]) { best[r] = d2; who[r] = k; }
        }
    }

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
        uint64_t pend = __ballot(who[r] >= 0);
        while (pend) {
            const int k = __builtin_amdgcn_readlane(who[r], (int)__builtin_ctzll(pend));
            const bool same = who[r] == k;
            const uint64_t mask = __ballot(same);
            const uint32_t ns = (uint32_t)__popcll(__ballot(same && hit));
            const double v = wave_reduce_min(same ? best[r] : (double)INFINITY);
            const uint32_t top = wave_reduce_max(same ? f32_ordered(hf[r]) : 0u);
            if (l == 0) {
                atomicAdd(&hist[k], (uint32_t)__popcll(mask) + (ns << 16));
                atomicMax(&maxinv[k], ~(unsigned long long)__double_as_longlong(v));
                atomicMax(&maxkey[k], top);
            }
            pend &= ~mask;
        }
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
    for (int j = threadIdx.x; j < nspans; j += CL_THREADS) {
        const uint32_t hv = hist[j];
        if (hv & 0xFFFFu) atomicAdd(&tally[j], (unsigned long long)(hv & 0xFFFFu));
        if (hv >> 16) atomicAdd(&strikes[j], (unsigned long long)(hv >> 16));
    }
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
        const unsigned long long v = maxinv[i];
        out_min_dist2[i] = v ? __longlong_as_double((long long)~v) : (double)INFINITY;
        const uint32_t key = maxkey[i];
        out_max_height[i] = key ? f32_unordered(key) : tl_nan();
    }
    if (out_stats && i < 4) out_stats[i] = (int64_t)stats[i];
    if (i >= n) return;
    const int32_t k = span[i];
    if (k < 0 || k >= nspans) return;
    if (~(unsigned long long)__double_as_longlong(dist2[i]) == maxinv[k]) atomicMin(&out_min_row[k], (unsigned long long)i);
    if (f32_ordered(height[i]) == maxkey[k]) atomicMin(&out_max_row[k], (unsigned long long)i);
}

struct TfWs {
    unsigned long long *tally, *strikes, *maxinv, *stats;
    uint32_t* maxkey;
    ClSpan* sp;
    uint32_t* take;
};
static void tf_plan(Arena& a, int32_t nspans, TfWs& w) {
    const size_t K = nspans > 0 ? (size_t)nspans : 1;
    // the tallies in front: one fill zeroes them
    w.tally = a.take<unsigned long long>(K);
    w.strikes = a.take<unsigned long long>(K);
    w.maxinv = a.take<unsigned long long>(K);
    w.stats = a.take<unsigned long long>(4);
    w.maxkey = a.take<uint32_t>(K);
    w.sp = a.take<ClSpan>(K);
    w.take = a.take<uint32_t>(K);
}
static bool tf_sizes_ok(int64_t n, int32_t nspans, int32_t nseg) {
    return tl_rows_ok(n) && nspans >= 0 && nspans <= CL_MAXSPAN && nseg >= 1 && nseg <= CL_MAXSEG;
}

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
    PCH_HIP_TRY(hipMemsetAsync(ws, 0, (size_t)(reinterpret_cast<char*>(w.sp) - static_cast<char*>(ws)), s));
    if (nspans > 0) {
        PCH_HIP_TRY(hipMemsetAsync(out_min_row, 0xFF, sizeof(int64_t) * (size_t)nspans, s));
        PCH_HIP_TRY(hipMemsetAsync(out_max_row, 0xFF, sizeof(int64_t) * (size_t)nspans, s));
        PCH_TRY(cl_bounds_run(curves5, segs, (int)nspans, (int)nsegments, rmax, w.sp, w.take, s));
    }
    if (n > 0)
        PCH_LAUNCH("treefall_sweep", tf_sweep_k, dim3((unsigned)ceil_div(n, CL_TILE)), dim3(CL_THREADS), 0, s, xyz, skip,
                   n, tl_sub_of(sub3_host), g, ground, curves5, segs, (int)nspans, (int)nsegments, (const ClSpan*)w.sp,
                   (const uint32_t*)w.take, h_min, h_max, grow, limit, out_dist2, out_span, out_height, out_class,
                   w.tally, w.strikes, w.maxinv, w.maxkey, w.stats);
    // the finisher walks the rows only where a span can own one; its first threads write the table and the statistics
    const int64_t fin_n = nspans > 0 ? n : 0;
    int64_t most = fin_n > nspans ? fin_n : (int64_t)nspans;
    if (most < 4) most = 4;
    if (nspans > 0 || out_stats)
        PCH_LAUNCH("treefall_finish", tf_finish_k, dim3((unsigned)ceil_div(most, CL_THREADS)), dim3(CL_THREADS), 0, s,
                   (const double*)out_dist2, (const int32_t*)out_span, (const float*)out_height, fin_n, (int)nspans,
                   (const unsigned long long*)w.tally, (const unsigned long long*)w.strikes,
                   (const unsigned long long*)w.maxinv, (const uint32_t*)w.maxkey, (const unsigned long long*)w.stats,
                   out_count, out_strikes, out_min_dist2, reinterpret_cast<unsigned long long*>(out_min_row),
                   out_max_height, reinterpret_cast<unsigned long long*>(out_max_row), out_stats);
    return PCH_OK;
}
