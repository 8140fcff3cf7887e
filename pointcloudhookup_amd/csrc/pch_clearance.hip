// Conductor clearance: for every row of a cloud the squared distance to the nearest fitted span curve
// within a radius, and per span the rows attributed to it, those inside a limit, the smallest distance and its row.  The
// rule is spelled out in include/pch_hip.h; every output is the rule's, bit for bit, whatever is culled here.
//   bounds  : one thread per span - the "takes part" flag (all 5 + 5 S values finite), the cull bounds of the polyline
//             and the along-track and height intervals outside which no row can lie within the radius
//   sweep   : tiles of 1024 rows.  Its own: the loads, the lane's box over its finite rows that are not skipped; dist2
//             and span for every row of the tile; per owning span the count and the violations tallied in LDS and the
//             smallest distance folded with a 64-bit integer atomic on cl_minkey.  Shared (pch_spancull.h,
//             pch_tilecull.h): the tile's box and the bitmap of the spans whose bounds meet it (cl_tile_spans), the
//             spans walked wave-uniformly in ascending order with the segment records through scalar loads
//             (cl_walk_spans), the loop over a round's owning spans (cl_fold_owners), the tallies added once per
//             (tile, span) (cl_flush_hist)
//   finish  : one pass over dist2 and span - the lowest row that attains a span's smallest distance; the table
//             (cl_finish_run: the launch pch_swing.hip shares, as pch_treefall.hip shares cl_bounds_run)
// No inline assembly, no floating-point atomic, nothing waits on another workgroup; the same bits on every run.
#include "pch_common.h"
#include "pch_spancull.h"

#include <math.h>

namespace pch {

struct ClRow { float x, y, z; };

// ---- the cull bounds.  The rule accepts row p for span k only if d2 = g + t*t <= r2, where g is the smallest of the
// d = em*em + ew*ew over the segments.  Write x_j = m_j + q*dm_j and y_j = z_j + q*dz_j for the point of segment j the
// rule measures to (q in [0,1], so x_j lies between the vertices m_j and m_j + dm_j, y_j between z_j and z_j + dz_j),
// [mlo, mhi] and [zlo, zhi] for the ranges of those vertices, A = max(|mlo|, |mhi|), Z = max(|zlo|, |zhi|) and
// B = max(A, Z) + radius.  With u = 2^-53:
//   (a) along the track.  em is (m - m_j) - q*dm_j with three roundings, and a row with m >= mhi + D has
//       m - x_j >= D - u*A exactly (the computed vertex m_j + dm_j is within u*A of the exact sum).  Each rounding is
//       relative to a term no larger than 3*(2A) when m - m_j < 2*dm_j, and relative to the result otherwise, so the
//       computed em >= (D - 8u*A)(1 - 4u).  With D = (radius + CL_EDGE*A)(1 + CL_EDGE), CL_EDGE = 2^-40 = 8192 u, that
//       is above radius*(1 + 2^-41), hence em*em > r2 (r2 <= radius^2 (1 + u)), d >= em*em, g > r2 and d2 >= g > r2:
//       not accepted.  The same below mlo - D.  [flo, fhi] = [mlo - D, mhi + D] is the interval the sweep tests m
//       against before it runs the segment loop; it needs no unit direction, only the rule's own m.
//   (b) height.  The same argument on ew = (w - z_j) - q*dz_j, with the rule's own w: a row with w outside
//       [wlo, whi] = [zlo - D', zhi + D'], D' = (radius + CL_EDGE*Z)(1 + CL_EDGE), has ew*ew > r2 and is not accepted -
//       the sweep's second test in front of the segment loop.  For the bounds: w = (double)pz - cz rounds once,
//       u*(Z + radius).
//   (c) in the plane.  For ux*ux + uy*uy = 1 + delta, |delta| <= CL_UNIT, (dx, dy) = R^T (m, t) / (1 + delta) with
//       R = [[ux, uy], [-uy, ux]]: the row lies at c + R^T (m, t) / (1 + delta), the point it is measured to at
//       c + R^T (x_j, 0) / (1 + delta), and their distance sqrt((m - x_j)^2 + t^2) / sqrt(1 + delta) is at most
//       sqrt(d2) (1 + 0.51 CL_UNIT) <= radius (1 + 0.52 CL_UNIT) by (a).  The bounds take the end points as
//       c + mlo*u and c + mhi*u, without the division: off by at most 1.01 CL_UNIT * A.  The roundings of m and t
//       (three each, relative to |dx ux| + |dy uy| <= 1.5 B), of dx and dy (u*B) and of the end points' products
//       (u*A) are below 1e-15 B - nothing beside CL_SLACK * B = 2e-6 B, which covers 1.01 CL_UNIT A + 0.52 CL_UNIT
//       radius with room.
// So the bounds are the box of the two end points in xy and [cz + zlo, cz + zhi] in z, widened by
// W = (radius + CL_SLACK * B)(1 + 1e-9) - the factor for the few roundings of W itself - and then moved outwards by
// 2^-50 of their own magnitude (eight units of roundoff: the two additions centre + offset -+ W round by one each, which
// is what counts beside a centre of 3e6 and a radius of 1e-3).  A direction further from unit than CL_UNIT, or bounds
// that overflow, give -inf / +inf (or NaN): a span whose bounds are not all finite is never culled.
constexpr double CL_UNIT  = 1e-6;
constexpr double CL_SLACK = 2e-6;
constexpr double CL_EDGE  = 0x1p-40;

__device__ __forceinline__ double cl_down(double v) { return v - fabs(v) * 0x1p-50; }
__device__ __forceinline__ double cl_up(double v) { return v + fabs(v) * 0x1p-50; }

__global__ __launch_bounds__(CL_THREADS) void cl_bounds_k(const double* __restrict__ curves5,
                                                          const double* __restrict__ segs, int nspans, int nseg,
                                                          double radius, ClSpan* __restrict__ out,
                                                          uint32_t* __restrict__ take) {
    const int k = blockIdx.x * CL_THREADS + threadIdx.x;
    if (k >= nspans) return;
    const double* c = curves5 + 5 * (size_t)k;
    const double* sg = segs + 5 * (size_t)k * nseg;
    bool finite = true;
    for (int a = 0; a < 5; ++a) finite = finite && isfinite(c[a]);
    double mlo = INFINITY, mhi = -INFINITY, zlo = INFINITY, zhi = -INFINITY;
    for (int j = 0; j < nseg; ++j) {
        const double m = sg[5 * j], z = sg[5 * j + 1], dm = sg[5 * j + 2], dz = sg[5 * j + 3], inv = sg[5 * j + 4];
        finite = finite && isfinite(m) && isfinite(z) && isfinite(dm) && isfinite(dz) && isfinite(inv);
        const double m2 = m + dm, z2 = z + dz;
        mlo = fmin(mlo, fmin(m, m2)); mhi = fmax(mhi, fmax(m, m2));
        zlo = fmin(zlo, fmin(z, z2)); zhi = fmax(zhi, fmax(z, z2));
    }
    take[k] = finite ? 1u : 0u;
    ClSpan s;
    const double A = fmax(fabs(mlo), fabs(mhi)), Z = fmax(fabs(zlo), fabs(zhi));
    const double D = (radius + CL_EDGE * A) * (1.0 + CL_EDGE);
    const double Dz = (radius + CL_EDGE * Z) * (1.0 + CL_EDGE);
    s.flo = mlo - D;
    s.fhi = mhi + D;
    s.wlo = zlo - Dz;
    s.whi = zhi + Dz;
    const double ux = c[3], uy = c[4];
    const double g = (ux * ux + uy * uy) - 1.0;
    const bool unit = finite && fabs(g) <= CL_UNIT;      // NaN fails the comparison
    if (!unit) {
        for (int a = 0; a < 3; ++a) { s.lo[a] = -INFINITY; s.hi[a] = INFINITY; }
    } else {
        const double W = (radius + CL_SLACK * (fmax(A, Z) + radius)) * (1.0 + 1e-9);
        const double ex0 = c[0] + mlo * ux, ex1 = c[0] + mhi * ux, ey0 = c[1] + mlo * uy, ey1 = c[1] + mhi * uy;
        s.lo[0] = cl_down(fmin(ex0, ex1) - W); s.hi[0] = cl_up(fmax(ex0, ex1) + W);
        s.lo[1] = cl_down(fmin(ey0, ey1) - W); s.hi[1] = cl_up(fmax(ey0, ey1) + W);
        s.lo[2] = cl_down((c[2] + zlo) - W);   s.hi[2] = cl_up((c[2] + zhi) + W);
    }
    out[k] = s;
}

int cl_bounds_run(const double* curves5, const double* segs, int nspans, int nseg, double radius, ClSpan* out,
                  uint32_t* take, hipStream_t s) {
    PCH_LAUNCH("clearance_bounds", cl_bounds_k, dim3((unsigned)ceil_div(nspans, CL_THREADS)), dim3(CL_THREADS), 0, s,
               curves5, segs, nspans, nseg, radius, out, take);
    return PCH_OK;
}

// tally / viol / maxinv: ClWs's tally / second / maxinv, zeroed by the caller.  loops (2 words): the (row, span) segment
// loops run and the (tile, span) pairs walked - what the probe reports.
__global__ __launch_bounds__(CL_THREADS) void cl_sweep_k(const float* __restrict__ xyz, const uint8_t* __restrict__ skip,
                                                         int64_t n, const double* __restrict__ curves5,
                                                         const double* __restrict__ segs, int nspans, int nseg,
                                                         const ClSpan* __restrict__ sp, const uint32_t* __restrict__ take,
                                                         double r2, double l2, double* __restrict__ out_dist2,
                                                         int32_t* __restrict__ out_span,
                                                         unsigned long long* __restrict__ tally,
                                                         unsigned long long* __restrict__ viol,
                                                         unsigned long long* __restrict__ maxinv,
                                                         unsigned long long* __restrict__ loops) {
    __shared__ uint64_t active[CL_WORDS];
    __shared__ uint32_t hist[CL_MAXSPAN];                // count in the low half, violations in the high half
    __shared__ double wlo[CL_WAVES][3], whi[CL_WAVES][3];
    const int w = wave_id(), l = lane_id();
    const int64_t base = (int64_t)blockIdx.x * CL_TILE + (int64_t)w * (64 * CL_ROUNDS);
    const ClRow* __restrict__ rows = reinterpret_cast<const ClRow*>(xyz);
    // every load of the tile is issued before anything is waited for, and none stands under a condition: a load behind
    // a branch is waited for on the spot, one after the other
    ClRow q[CL_ROUNDS];
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
    // the tile's bounding box over its finite rows that are not skipped (no other row can be accepted)
    bool ok[CL_ROUNDS];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        ok[r] = i < n && sk[r] == 0 && isfinite(q[r].x) && isfinite(q[r].y) && isfinite(q[r].z);
        if (ok[r]) {
            lo[0] = fmin(lo[0], (double)q[r].x); hi[0] = fmax(hi[0], (double)q[r].x);
            lo[1] = fmin(lo[1], (double)q[r].y); hi[1] = fmax(hi[1], (double)q[r].y);
            lo[2] = fmin(lo[2], (double)q[r].z); hi[2] = fmax(hi[2], (double)q[r].z);
        }
    }
    cl_tile_spans(active, nspans, sp, take, lo, hi, wlo, whi);

    double best[CL_ROUNDS];
    int who[CL_ROUNDS];
    uint32_t ran, walked;
    cl_walk_spans(active, nspans, curves5, segs, nseg, sp, q, ok, [&](int r) { return (double)q[r].z; },
                  [&](int) { return r2; }, best, who, ran, walked);

    // dist2 and span for every row of the tile; per span of a wave's round one LDS add and one fold of the smallest
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        if (i < n) { out_dist2[i] = best[r]; out_span[i] = who[r]; }
        cl_fold_owners(who[r], [&](int k, bool same, uint32_t owned) {
            const uint32_t nv = (uint32_t)__popcll(__ballot(same && best[r] <= l2));
            const double v = wave_reduce_min(same ? best[r] : (double)INFINITY);
            if (l == 0) {
                atomicAdd(&hist[k], owned + (nv << 16));
                atomicMax(&maxinv[k], cl_minkey(v));
            }
        });
    }
    if (loops && l == 0 && (ran || walked)) {
        if (ran) atomicAdd(&loops[0], (unsigned long long)ran);
        if (w == 0) atomicAdd(&loops[1], (unsigned long long)walked);
    }
    __syncthreads();
    cl_flush_hist(hist, nspans, tally, viol);
}

// the table, and the lowest row that attains a span's smallest distance (out_min_row arrives as all ones = -1)
__global__ __launch_bounds__(CL_THREADS) void cl_finish_k(const double* __restrict__ dist2,
                                                          const int32_t* __restrict__ span, int64_t n, int nspans,
                                                          const unsigned long long* __restrict__ tally,
                                                          const unsigned long long* __restrict__ viol,
                                                          const unsigned long long* __restrict__ maxinv,
                                                          const unsigned long long* __restrict__ loops,
                                                          int64_t* __restrict__ out_count,
                                                          int64_t* __restrict__ out_violations,
                                                          double* __restrict__ out_min_dist2,
                                                          unsigned long long* __restrict__ out_min_row,
                                                          int64_t* __restrict__ out_loops) {
    const int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
    if (i < nspans) {
        out_count[i] = (int64_t)tally[i];
        out_violations[i] = (int64_t)viol[i];
        out_min_dist2[i] = cl_minkey_value(maxinv[i]);
    }
    if (out_loops && i < 2) out_loops[i] = (int64_t)loops[i];
    if (i >= n) return;
    const int32_t k = span[i];
    if (k < 0 || k >= nspans) return;
    if (cl_minkey(dist2[i]) == maxinv[k]) atomicMin(&out_min_row[k], (unsigned long long)i);
}

int cl_finish_run(const double* dist2, const int32_t* span, int64_t n, int nspans, const unsigned long long* tally,
                  const unsigned long long* second, const unsigned long long* maxinv,
                  const unsigned long long* counters, int64_t* out_count, int64_t* out_second, double* out_min_dist2,
                  int64_t* out_min_row, int64_t* out_loops, hipStream_t s) {
    const int64_t most = n > nspans ? n : (int64_t)nspans;
    PCH_LAUNCH("clearance_finish", cl_finish_k, dim3((unsigned)ceil_div(most, CL_THREADS)), dim3(CL_THREADS), 0, s, dist2,
               span, n, nspans, tally, second, maxinv, counters, out_count, out_second, out_min_dist2,
               reinterpret_cast<unsigned long long*>(out_min_row), out_loops);
    return PCH_OK;
}

static void cl_plan(Arena& a, int32_t nspans, ClWs& w) {
    cl_plan_front(a, nspans, 2, w);
    cl_plan_back(a, nspans, w);
}
static bool cl_sizes_ok(int64_t n, int32_t nspans, int32_t nseg) {
    return n >= 0 && n < (int64_t(1) << 32) && cl_spans_ok(nspans, nseg);
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_clearance_ws_bytes(int64_t n, int32_t nspans, int32_t nsegments) {
    if (!cl_sizes_ok(n, nspans, nsegments)) return 0;
    Arena a;
    ClWs w;
    cl_plan(a, nspans, w);
    return a.off;
}

extern "C" int pch_clearance_f32(const float* xyz, const uint8_t* skip, int64_t n, const double* curves5,
                                 const double* segs, int32_t nspans, int32_t nsegments, double radius, double limit,
                                 double* out_dist2, int32_t* out_span, int64_t* out_count, int64_t* out_violations,
                                 double* out_min_dist2, int64_t* out_min_row, int64_t* out_loops, void* ws,
                                 size_t ws_bytes, void* stream) {
    PCH_REQUIRE(cl_sizes_ok(n, nspans, nsegments), "0 <= n < 2^32, 0 <= nspans <= 4096, 1 <= nsegments <= 128");
    PCH_REQUIRE(isfinite(radius) && isfinite(limit) && limit > 0.0 && limit <= radius,
                "radius and limit must be finite with 0 < limit <= radius");
    PCH_REQUIRE(n == 0 || (xyz && out_dist2 && out_span), "null row buffer");
    PCH_REQUIRE(nspans == 0 || (curves5 && segs && out_count && out_violations && out_min_dist2 && out_min_row),
                "null span buffer");
    PCH_REQUIRE(ws, "null workspace");
    PCH_DEVICE_GUARD(ws);
    hipStream_t s = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    ClWs w;
    cl_plan(a, nspans, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    if (n == 0 && nspans == 0) return PCH_OK;
    const double r2 = radius * radius, l2 = limit * limit;
    PCH_HIP_TRY(hipMemsetAsync(ws, 0, cl_front_bytes(ws, w), s));
    if (nspans == 0 && out_loops) PCH_HIP_TRY(hipMemsetAsync(out_loops, 0, 2 * sizeof(int64_t), s));
    if (nspans > 0) {
        PCH_HIP_TRY(hipMemsetAsync(out_min_row, 0xFF, sizeof(int64_t) * (size_t)nspans, s));
        PCH_TRY(cl_bounds_run(curves5, segs, (int)nspans, (int)nsegments, radius, w.sp, w.take, s));
    }
    if (n > 0)
        PCH_LAUNCH("clearance_sweep", cl_sweep_k, dim3((unsigned)ceil_div(n, CL_TILE)), dim3(CL_THREADS), 0, s, xyz, skip,
                   n, curves5, segs, (int)nspans, (int)nsegments, (const ClSpan*)w.sp, (const uint32_t*)w.take, r2, l2,
                   out_dist2, out_span, w.tally, w.second, w.maxinv, w.counters);
    if (nspans > 0)
        PCH_TRY(cl_finish_run(out_dist2, out_span, n, (int)nspans, w.tally, w.second, w.maxinv, w.counters, out_count,
                              out_violations, out_min_dist2, out_min_row, out_loops, s));
    return PCH_OK;
}
