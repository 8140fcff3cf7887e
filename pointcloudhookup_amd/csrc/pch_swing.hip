// Wind swing clearance: for every row of a cloud the squared distance to the nearest conductor as the
// wind can swing it - each span's polyline turned about its chord by the angle, within [-Theta, Theta], that points it
// at the row - within a radius, the span and the sine of that angle; per span the rows attributed to it, those inside a
// limit, the smallest distance and its row.  The rule is spelled out in include/pch_hip.h; every output is the rule's,
// bit for bit, whatever is culled here.
//   bounds  : one thread per span - the "takes part" flag, the cull bounds of the whole swung family, the along-track
//             and height intervals and the lateral bound outside which no row can lie within the radius
//   sweep   : tiles of 1024 rows.  Its own: the loads (issued as cl_sweep_k's), the lane's box over its finite rows that
//             are not skipped, the walk of the tile's spans with the 3-D segment loop of the rule - the head and segment
//             records through wave-uniform (scalar) loads -; dist2, span and sin for every row of the tile; per owning
//             span the count and the violations tallied in LDS and the smallest distance folded with a 64-bit integer
//             atomic on cl_minkey.  Shared (pch_spancull.h, pch_tilecull.h): the tile's box and the bitmap of the spans
//             whose bounds meet it (cl_tile_spans), the walk of that bitmap (cull_next_bit), the loop over a round's
//             owning spans (cl_fold_owners), the tallies added once per (tile, span) (cl_flush_hist)
//   finish  : cl_finish_k (pch_clearance.hip) through cl_finish_run - the lowest row of every minimum; the table
// No inline assembly, no floating-point atomic, nothing waits on another workgroup; the same bits on every run.
#include "pch_common.h"
#include "pch_spancull.h"

#include <math.h>

namespace pch {

struct SwRow { float x, y, z; };

constexpr int SW_HEAD = 11;                              // cx, cy, cz, ux, uy, mA, mB, zA, kap, sT, cT
constexpr int SW_SEG  = 6;                               // m_j, z_j, f_j, dm_j, dz_j, df_j

// what the sweep tests of a span's lateral offset before the segment loop, beside ClSpan's two intervals:
// |t| <= |s|*tf + td must hold for a row to be accepted at its own sine s
struct SwLat { double tf, td; };

// ---- the cull bounds.  The rule accepts row p for span k only if g <= r2, where g is the smallest of the
// d = (vm*vm + vt*vt) + vw*vw over the segments; d is at least each of its three squares (rounding is monotone and the
// squares are not negative).  For the (s, c) the rule picks write e = 1 - c and, for segment j and its q in [0,1], the
// point the rule measures to as (x, y, h) = (m_j + q*dm_j, (f_j + q*df_j)*s, (z_j + q*dz_j) + (f_j + q*df_j)*e): x lies
// between two vertices' m, y between two vertices' f*s and h between two vertices' z + f*e.  [mlo, mhi] and [zlo, zhi]
// are the ranges of the vertices' m and z, F = max |f| and Z = max |z| over the vertices, A = max(|mlo|, |mhi|),
// u = 2^-53.
//   The turn.  In the sector (|t|*cT <= bb*sT, bb > 0) squaring gives t*t*(sT*sT + cT*cT) <= (t*t + bb*bb)*sT*sT, so
//       s*s <= sT*sT / (1 - 1e-6) and c*c >= cT*cT / (1 + 1e-6) by the participation test, up to the five roundings of
//       rho, s and c; c = bb/rho <= 1, as rho >= sqrt(bb*bb) = bb.  Outside it (s, c) = (+-sT, cT).  Either way
//       |s| <= sB = sT*(1 + 2e-6) and 0 <= e <= eB = (1 - cT) + 2e-6.
//   (a) along the track.  vm = (m - m_j) - q*dm_j is the clearance rule's em, term for term: (a) of the derivation in
//       front of cl_bounds_k holds as it stands, and [flo, fhi] = [mlo - D, mhi + D] with D = (radius + SW_EDGE*A)
//       (1 + SW_EDGE), SW_EDGE = 2^-40, is the interval outside which vm*vm > r2.
//   (b) height.  h is linear in q and in e, so it lies in [hlo, hhi] = the range of z_v and z_v + f_v*eB over the
//       vertices v.  vw = (w - pw) - q*ez with pw = z_j + f_j*e and ez = dz_j + df_j*e: beside the three roundings of
//       (a) two each in pw and ez and one each in the vertex sums z_j + dz_j and f_j + df_j, all relative to terms no
//       larger than Z + F.  With Zf = (Z + F)(1 + 1e-5) in A's place the argument of (a) gives: a row with w outside
//       [wlo, whi] = [hlo - D', hhi + D'], D' = (radius + SW_EDGE*Zf)(1 + SW_EDGE), has vw*vw > r2 - 8192 u of room for
//       a dozen roundings.
//   (c) lateral.  |y| <= |s|*F(1 + 4u) (py = f_j*s rounds once, py + ey twice more).  vt = (t - py) - q*ey: by the
//       argument of (a) with |s|*F in A's place, a row with |t| > |s|*tf + td, tf = F(1 + SW_EDGE) and
//       td = (radius + SW_EDGE*F)(1 + SW_EDGE), has vt*vt > r2.  This is the sweep's third test, with the row's own s;
//       since |s| <= sB it implies |t| <= Y + td with Y = F*sT*(1 + 1e-5) for every row that can be accepted.
//   (d) in the plane.  As (c) of cl_bounds_k: for a direction within SW_UNIT of unit the row lies at
//       c + R^T (m, t) / (1 + delta) and the point at c + R^T (x, y) / (1 + delta), no further apart in xy than
//       sqrt(d) (1 + 0.51 SW_UNIT) <= radius (1 + 0.52 SW_UNIT); the point is the one of the rest polyline moved
//       sideways by |y| / sqrt(1 + delta) <= Y.  So the xy bounds are cl_bounds_k's box of the two end points widened by
//       W + Y, W = (radius + SW_SLACK * B)(1 + 1e-9) with B = max(A, Zf) + Y + radius, and the height bounds
//       [cz + hlo, cz + hhi] widened by W; both moved outwards by 2^-50 of their magnitude for their own roundings.
// A direction further from unit than SW_UNIT, or bounds that overflow, give -inf / +inf (or NaN): a span whose bounds
// are not all finite is never culled, and the sweep's three tests are written so that a NaN bound culls nothing.
// The constants are cl_bounds_k's.
constexpr double SW_UNIT  = 1e-6;
constexpr double SW_SLACK = 2e-6;
constexpr double SW_EDGE  = 0x1p-40;
constexpr double SW_TURN  = 1e-6;                        // |sT*sT + cT*cT - 1| of a span that takes part

__device__ __forceinline__ double sw_down(double v) { return v - fabs(v) * 0x1p-50; }
__device__ __forceinline__ double sw_up(double v) { return v + fabs(v) * 0x1p-50; }

__global__ __launch_bounds__(CL_THREADS) void sw_bounds_k(const double* __restrict__ heads,
                                                          const double* __restrict__ segs, int nspans, int nseg,
                                                          double radius, ClSpan* __restrict__ out,
                                                          SwLat* __restrict__ lat, uint32_t* __restrict__ take) {
    const int k = blockIdx.x * CL_THREADS + threadIdx.x;
    if (k >= nspans) return;
    const double* c = heads + SW_HEAD * (size_t)k;
    const double* sg = segs + SW_SEG * (size_t)k * nseg;
    bool finite = true;
    for (int a = 0; a < SW_HEAD; ++a) finite = finite && isfinite(c[a]);
    const double mA = c[5], mB = c[6], sT = c[9], cT = c[10];
    const double eB = (1.0 - cT) + 2e-6;
    double mlo = INFINITY, mhi = -INFINITY, hlo = INFINITY, hhi = -INFINITY, F = 0.0, Z = 0.0;
    for (int j = 0; j < nseg; ++j) {
        const double* v = sg + SW_SEG * j;
        for (int a = 0; a < SW_SEG; ++a) finite = finite && isfinite(v[a]);
        const double m = v[0], z = v[1], f = v[2], m2 = v[0] + v[3], z2 = v[1] + v[4], f2 = v[2] + v[5];
        mlo = fmin(mlo, fmin(m, m2)); mhi = fmax(mhi, fmax(m, m2));
        const double zs = z + f * eB, zs2 = z2 + f2 * eB;
        hlo = fmin(hlo, fmin(fmin(z, z2), fmin(zs, zs2)));
        hhi = fmax(hhi, fmax(fmax(z, z2), fmax(zs, zs2)));
        F = fmax(F, fmax(fabs(f), fabs(f2)));
        Z = fmax(Z, fmax(fabs(z), fabs(z2)));
    }
    const double turn = ((sT * sT) + (cT * cT)) - 1.0;
    const bool part = finite && mB > mA && 0.0 <= sT && sT <= 1.0 && 0.0 < cT && cT <= 1.0 && fabs(turn) <= SW_TURN;
    take[k] = part ? 1u : 0u;
    ClSpan s;
    SwLat t;
    const double A = fmax(fabs(mlo), fabs(mhi)), Zf = (Z + F) * (1.0 + 1e-5), Y = (F * sT) * (1.0 + 1e-5);
    const double D = (radius + SW_EDGE * A) * (1.0 + SW_EDGE);
    const double Dz = (radius + SW_EDGE * Zf) * (1.0 + SW_EDGE);
    s.flo = mlo - D;
    s.fhi = mhi + D;
    s.wlo = hlo - Dz;
    s.whi = hhi + Dz;
    t.tf = F * (1.0 + SW_EDGE);
    t.td = (radius + SW_EDGE * F) * (1.0 + SW_EDGE);
    const double ux = c[3], uy = c[4];
    const double g = (ux * ux + uy * uy) - 1.0;
    const bool unit = part && fabs(g) <= SW_UNIT;        // NaN fails the comparison
    if (!unit) {
        for (int a = 0; a < 3; ++a) { s.lo[a] = -INFINITY; s.hi[a] = INFINITY; }
    } else {
        const double W = (radius + SW_SLACK * ((fmax(A, Zf) + Y) + radius)) * (1.0 + 1e-9);
        const double Wy = W + Y;
        const double ex0 = c[0] + mlo * ux, ex1 = c[0] + mhi * ux, ey0 = c[1] + mlo * uy, ey1 = c[1] + mhi * uy;
        s.lo[0] = sw_down(fmin(ex0, ex1) - Wy); s.hi[0] = sw_up(fmax(ex0, ex1) + Wy);
        s.lo[1] = sw_down(fmin(ey0, ey1) - Wy); s.hi[1] = sw_up(fmax(ey0, ey1) + Wy);
        s.lo[2] = sw_down((c[2] + hlo) - W);    s.hi[2] = sw_up((c[2] + hhi) + W);
    }
    out[k] = s;
    lat[k] = t;
}

// The rule for a wave's CL_ROUNDS rows against the spans of the tile's bitmap, in ascending span order: best[r] = the
// smallest g <= r2 over the spans, who[r] = the lowest span that attains it and sn[r] = the sine of the turn at which it
// does (INFINITY, -1 and NaN where there is none).  ok[r] = the row can be accepted at all.  Every parenthesis is the
// rule's: with -ffp-contract=off the written order is what is computed; / and sqrt are IEEE's.  ran / walked: the
// (row, span) segment loops run and the spans walked by this wave.
//
// Three tests stand in front of the segment loop: (a), (b) and (c) of the derivation in front of sw_bounds_k.  They are
// written as "not outside", so that a bound that is NaN stops nothing.
__device__ __forceinline__ void sw_walk_spans(const uint64_t* active, int nspans, const double* __restrict__ heads,
                                              const double* __restrict__ segs, int nseg,
                                              const ClSpan* __restrict__ sp, const SwLat* __restrict__ lat,
                                              const SwRow (&q)[CL_ROUNDS], const bool (&ok)[CL_ROUNDS], double r2,
                                              double (&best)[CL_ROUNDS], int (&who)[CL_ROUNDS], double (&sn)[CL_ROUNDS],
                                              uint32_t& ran, uint32_t& walked) {
    const int nwords = (nspans + 63) >> 6;
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) {
        best[r] = INFINITY;
        who[r] = -1;
        sn[r] = __longlong_as_double(0x7ff8000000000000LL);
    }
    ran = 0;
    walked = 0;
    int word = -1;
    uint64_t bits = 0;
    for (int k = cull_next_bit(active, nwords, word, bits); k >= 0; k = cull_next_bit(active, nwords, word, bits)) {
        const double* __restrict__ c = heads + SW_HEAD * (size_t)k;
        const double cx = c[0], cy = c[1], cz = c[2], ux = c[3], uy = c[4], mA = c[5], mB = c[6], zA = c[7], kap = c[8],
                     sT = c[9], cT = c[10];
        const double flo = sp[k].flo, fhi = sp[k].fhi, hlo = sp[k].wlo, hhi = sp[k].whi;
        double m[CL_ROUNDS], t[CL_ROUNDS], h[CL_ROUNDS];
        bool go[CL_ROUNDS];
        bool some = false;
#pragma unroll
        for (int r = 0; r < CL_ROUNDS; ++r) {
            const double dx = (double)q[r].x - cx, dy = (double)q[r].y - cy;
            h[r] = (double)q[r].z - cz;
            m[r] = (dx * ux) + (dy * uy);
            t[r] = (dy * ux) - (dx * uy);
            go[r] = ok[r] && !(m[r] < flo) && !(m[r] > fhi) && !(h[r] < hlo) && !(h[r] > hhi);
            some = some || go[r];
        }
        ++walked;
        if (__ballot(some) == 0) continue;               // (wave-uniform)
        const double tf = lat[k].tf, td = lat[k].td;
        double s[CL_ROUNDS], e[CL_ROUNDS], g[CL_ROUNDS];
        some = false;
#pragma unroll
        for (int r = 0; r < CL_ROUNDS; ++r) {
            double mh = m[r];
            if (mh < mA) mh = mA;
            if (mh > mB) mh = mB;
            const double bb = (zA + ((mh - mA) * kap)) - h[r];
            double cc;
            if (bb > 0.0 && (fabs(t[r]) * cT) <= (bb * sT)) {
                const double rho = sqrt((t[r] * t[r]) + (bb * bb));
                s[r] = t[r] / rho;
                cc = bb / rho;
            } else {
                s[r] = t[r] >= 0.0 ? sT : -sT;
                cc = cT;
            }
            e[r] = 1.0 - cc;
            g[r] = INFINITY;
            go[r] = go[r] && !(fabs(t[r]) > (fabs(s[r]) * tf) + td);
            some = some || go[r];
        }
        if (__ballot(some) == 0) continue;               // (wave-uniform)
#pragma unroll
        for (int r = 0; r < CL_ROUNDS; ++r) ran += (uint32_t)__popcll(__ballot(go[r]));
        const double* __restrict__ sg = segs + SW_SEG * (size_t)k * nseg;
        for (int j = 0; j < nseg; ++j) {
            const double mj = sg[SW_SEG * j], zj = sg[SW_SEG * j + 1], fj = sg[SW_SEG * j + 2], dm = sg[SW_SEG * j + 3],
                         dz = sg[SW_SEG * j + 4], df = sg[SW_SEG * j + 5];
            const double dm2 = dm * dm;
#pragma unroll
            for (int r = 0; r < CL_ROUNDS; ++r) {
                const double py = fj * s[r], pw = zj + (fj * e[r]), ey = df * s[r], ez = dz + (df * e[r]);
                const double rm = m[r] - mj, rt = t[r] - py, rw = h[r] - pw;
                const double len2 = (dm2 + (ey * ey)) + (ez * ez);
                double qq = len2 > 0.0 ? (((rm * dm) + (rt * ey)) + (rw * ez)) / len2 : 0.0;
                if (qq < 0.0) qq = 0.0;
                if (qq > 1.0) qq = 1.0;
                const double vm = rm - (qq * dm), vt = rt - (qq * ey), vw = rw - (qq * ez);
                const double d = ((vm * vm) + (vt * vt)) + (vw * vw);
                if (d < g[r]) g[r] = d;
            }
        }
#pragma unroll
        for (int r = 0; r < CL_ROUNDS; ++r)
            if (go[r] && g[r] <= r2 && g[r] < best[r]) { best[r] = g[r]; who[r] = k; sn[r] = s[r]; }
    }
}

// tally / viol / maxinv: ClWs's tally / second / maxinv, zeroed by the caller.  loops (2 words): the (row, span) segment
// loops run and the (tile, span) pairs walked - what the probe reports.
__global__ __launch_bounds__(CL_THREADS) void sw_sweep_k(const float* __restrict__ xyz, const uint8_t* __restrict__ skip,
                                                         int64_t n, const double* __restrict__ heads,
                                                         const double* __restrict__ segs, int nspans, int nseg,
                                                         const ClSpan* __restrict__ sp, const SwLat* __restrict__ lat,
                                                         const uint32_t* __restrict__ take, double r2, double l2,
                                                         double* __restrict__ out_dist2, int32_t* __restrict__ out_span,
                                                         double* __restrict__ out_sin,
                                                         unsigned long long* __restrict__ tally,
                                                         unsigned long long* __restrict__ viol,
                                                         unsigned long long* __restrict__ maxinv,
                                                         unsigned long long* __restrict__ loops) {
    __shared__ uint64_t active[CL_WORDS];
    __shared__ uint32_t hist[CL_MAXSPAN];                // count in the low half, violations in the high half
    __shared__ double wlo[CL_WAVES][3], whi[CL_WAVES][3];
    const int w = wave_id(), l = lane_id();
    const int64_t base = (int64_t)blockIdx.x * CL_TILE + (int64_t)w * (64 * CL_ROUNDS);
    const SwRow* __restrict__ rows = reinterpret_cast<const SwRow*>(xyz);
    // every load of the tile is issued before anything is waited for, and none stands under a condition (cl_sweep_k)
    SwRow q[CL_ROUNDS];
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

    double best[CL_ROUNDS], sn[CL_ROUNDS];
    int who[CL_ROUNDS];
    uint32_t ran, walked;
    sw_walk_spans(active, nspans, heads, segs, nseg, sp, lat, q, ok, r2, best, who, sn, ran, walked);

    // dist2, span and sin for every row of the tile; per span of a wave's round one LDS add and one fold of the smallest
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        if (i < n) { out_dist2[i] = best[r]; out_span[i] = who[r]; out_sin[i] = sn[r]; }
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

struct SwWs : ClWs { SwLat* lat; };
static void sw_plan(Arena& a, int32_t nspans, SwWs& w) {
    cl_plan_front(a, nspans, 2, w);
    cl_plan_back(a, nspans, w);
    w.lat = a.take<SwLat>(cl_slots(nspans));
}
static bool sw_sizes_ok(int64_t n, int32_t nspans, int32_t nseg) {
    return n >= 0 && n < (int64_t(1) << 32) && cl_spans_ok(nspans, nseg);
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_swing_clearance_ws_bytes(int64_t n, int32_t nspans, int32_t nsegments) {
    if (!sw_sizes_ok(n, nspans, nsegments)) return 0;
    Arena a;
    SwWs w;
    sw_plan(a, nspans, w);
    return a.off;
}

extern "C" int pch_swing_clearance_f32(const float* xyz, const uint8_t* skip, int64_t n, const double* heads,
                                       const double* segs, int32_t nspans, int32_t nsegments, double radius,
                                       double limit, double* out_dist2, int32_t* out_span, double* out_sin,
                                       int64_t* out_count, int64_t* out_violations, double* out_min_dist2,
                                       int64_t* out_min_row, int64_t* out_loops, void* ws, size_t ws_bytes,
                                       void* stream) {
    PCH_REQUIRE(sw_sizes_ok(n, nspans, nsegments), "0 <= n < 2^32, 0 <= nspans <= 4096, 1 <= nsegments <= 128");
    PCH_REQUIRE(isfinite(radius) && isfinite(limit) && limit > 0.0 && limit <= radius,
                "radius and limit must be finite with 0 < limit <= radius");
    PCH_REQUIRE(n == 0 || (xyz && out_dist2 && out_span && out_sin), "null row buffer");
    PCH_REQUIRE(nspans == 0 || (heads && segs && out_count && out_violations && out_min_dist2 && out_min_row),
                "null span buffer");
    PCH_REQUIRE(ws, "null workspace");
    PCH_DEVICE_GUARD(ws);
    hipStream_t s = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    SwWs w;
    sw_plan(a, nspans, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    if (n == 0 && nspans == 0) return PCH_OK;
    const double r2 = radius * radius, l2 = limit * limit;
    PCH_HIP_TRY(hipMemsetAsync(ws, 0, cl_front_bytes(ws, w), s));
    if (nspans == 0 && out_loops) PCH_HIP_TRY(hipMemsetAsync(out_loops, 0, 2 * sizeof(int64_t), s));
    if (nspans > 0) {
        PCH_HIP_TRY(hipMemsetAsync(out_min_row, 0xFF, sizeof(int64_t) * (size_t)nspans, s));
        PCH_LAUNCH("swing_bounds", sw_bounds_k, dim3((unsigned)ceil_div(nspans, CL_THREADS)), dim3(CL_THREADS), 0, s,
                   heads, segs, (int)nspans, (int)nsegments, radius, w.sp, w.lat, w.take);
    }
    if (n > 0)
        PCH_LAUNCH("swing_sweep", sw_sweep_k, dim3((unsigned)ceil_div(n, CL_TILE)), dim3(CL_THREADS), 0, s, xyz, skip, n,
                   heads, segs, (int)nspans, (int)nsegments, (const ClSpan*)w.sp, (const SwLat*)w.lat,
                   (const uint32_t*)w.take, r2, l2, out_dist2, out_span, out_sin, w.tally, w.second, w.maxinv,
                   w.counters);
    if (nspans > 0)
        PCH_TRY(cl_finish_run(out_dist2, out_span, n, (int)nspans, w.tally, w.second, w.maxinv, w.counters, out_count,
                              out_violations, out_min_dist2, out_min_row, out_loops, s));
    return PCH_OK;
}
