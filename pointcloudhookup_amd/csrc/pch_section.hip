// Span sections: station by station along every fitted span curve, the rows that lie in the corridor under
// the wire - how many, how many within the vertical limit, the smallest vertical distance and its row - and for every row
// the span and station where the wire hangs lowest above it.  The rule is spelled out in include/pch_hip.h; every output
// is the rule's, bit for bit, whatever is culled here.
//   bounds  : one thread per span - the "takes part" flag (ten finite values, m1 > m0) and the cull record: a world box
//             around the corridor rectangle and the heights a row under the wire can have
//   sweep   : tiles of 1024 rows.  The loads and the lane's box as cl_sweep_k's; the tile's box, the bitmap of the spans
//             whose record meets it and the wave-uniform walk of that bitmap are pch_tilecull.h's, the span's ten values
//             come through scalar loads.  There is no segment loop: a (row, span) pair costs two products for t and m,
//             four comparisons, and for the rows inside the rectangle the parabola, a division and a cast.  The tile
//             combines its rows per station in LDS (128 slots of key and packed counts; the rows of a wave's round that
//             share a station are reduced across the lanes first) and flushes the slots that are not empty once per
//             (tile, span): a cell that thousands of rows fall into receives two global atomics per tile that touched
//             it - the key's minimum and the packed tally -, not two per row
//   decode  : the cells' keys (smallest distance, lowest row) to out_min_v / out_min_row, the packed tallies to
//             out_count / out_violations; the counters to out_stats
// No inline assembly, integer atomics only, nothing waits on another workgroup; the same bits on every run.
#include "pch_common.h"
#include "pch_spancull.h"

#include <math.h>

namespace pch {

struct ScRow { float x, y, z; };

constexpr int SC_MAXST = 128;                            // stations per span
constexpr int SC_STATLINES = 256;                        // copies of the three counters, one 128-byte line each
constexpr int SC_STATWORDS = 16;
constexpr unsigned long long SC_EMPTY = ~0ull;          // a key no row can have: its upper half is a NaN's bits

// the cull record of a span: no row outside this world box can take part in it
struct ScSpan { double lo[3], hi[3]; };

// ---- the cull record.  The rule takes row p for span k only if the computed m lies in [m0, m1], the computed t in
// [-half, half] and the computed v = zw - w in [0, depth].  Write A = max(|m0|, |m1|), Bm = A + half, u = 2^-53.
//   (a) in the plane.  For ux*ux + uy*uy = 1 + delta, |delta| <= SC_UNIT, (dx, dy) = R^T (m, t) / (1 + delta) with
//       R = [[ux, uy], [-uy, ux]] ((c) of the derivation in front of cl_bounds_k): the row lies at
//       c + R^T (m, t) / (1 + delta), inside the rectangle with the corners c + m_e*(ux, uy) +- half*(-uy, ux),
//       m_e in {m0, m1}, scaled about c by 1 / (1 + delta) - off the unscaled one by at most 1.01 SC_UNIT * Bm.  The
//       roundings of m and t (three each, relative to |dx ux| + |dy uy| <= 1.5 Bm) and of dx and dy (u * Bm) move a row
//       that passes the four comparisons at most 1e-15 Bm outside the exact rectangle.  So the xy bounds are the box of
//       the four corners widened by W = SC_SLACK * Bm (1 + 1e-9), SC_SLACK = 2e-6, which leaves half of itself for the
//       handful of roundings of the corners' own sums.
//   (b) height.  v >= 0 holds for the computed difference iff zw >= w, and v <= depth only if zw - w <= depth (1 + u):
//       w = (double)pz - cz (one rounding) lies in [zw - depth, zw] up to u (|zw| + depth).  The computed
//       zw = a + m (b + c m) is within 4u Zb of the parabola at the computed m, Zb = |a| + (|b| + |c| Bm) Bm, and that m
//       is within 1e-15 Bm of a station in [m0, m1], which moves the parabola by at most (|b| + 2|c|A) 1e-15 Bm
//       <= 2e-15 Zb.  Over [m0, m1] the parabola lies between zlo and zhi, the smallest and largest of its two end
//       values and, where mv = -b / (2c) falls strictly inside, its value there (computed with the same few roundings;
//       a c of zero gives an mv that is not finite and fails both comparisons).  So pz lies in
//       [cz + zlo - depth - E, cz + zhi + E] with E = SC_SLACK (Zb + depth)(1 + 1e-9): nine orders above what is needed.
// Both are moved outwards by 2^-50 of their own magnitude, as cl_bounds_k's, for the roundings of the last additions
// beside a centre of 3e6.  A direction further from unit than SC_UNIT, or bounds that overflow, give -inf / +inf (or
// NaN): cull_tile_bitmap never culls a span whose bounds are not all finite.
constexpr double SC_UNIT  = 1e-6;
constexpr double SC_SLACK = 2e-6;

__device__ __forceinline__ double sc_down(double v) { return v - fabs(v) * 0x1p-50; }
__device__ __forceinline__ double sc_up(double v) { return v + fabs(v) * 0x1p-50; }

__global__ __launch_bounds__(CL_THREADS) void sc_bounds_k(const double* __restrict__ curves10, int nspans, double half,
                                                          double depth, ScSpan* __restrict__ out,
                                                          uint32_t* __restrict__ take) {
    const int k = blockIdx.x * CL_THREADS + threadIdx.x;
    if (k >= nspans) return;
    const double* c = curves10 + 10 * (size_t)k;
    bool finite = true;
    for (int i = 0; i < 10; ++i) finite = finite && isfinite(c[i]);
    const double cx = c[0], cy = c[1], cz = c[2], ux = c[3], uy = c[4], a = c[5], b = c[6], cc = c[7], m0 = c[8],
                 m1 = c[9];
    const bool part = finite && m1 > m0;
    take[k] = part ? 1u : 0u;
    ScSpan s;
    const double g = (ux * ux + uy * uy) - 1.0;
    const bool unit = part && fabs(g) <= SC_UNIT;        // NaN fails the comparison
    if (!unit) {
        for (int i = 0; i < 3; ++i) { s.lo[i] = -INFINITY; s.hi[i] = INFINITY; }
    } else {
        const double A = fmax(fabs(m0), fabs(m1)), Bm = A + half;
        const double W = (SC_SLACK * Bm) * (1.0 + 1e-9);
        const double hx = half * fabs(uy), hy = half * fabs(ux);
        const double ex0 = cx + m0 * ux, ex1 = cx + m1 * ux, ey0 = cy + m0 * uy, ey1 = cy + m1 * uy;
        s.lo[0] = sc_down((fmin(ex0, ex1) - hx) - W); s.hi[0] = sc_up((fmax(ex0, ex1) + hx) + W);
        s.lo[1] = sc_down((fmin(ey0, ey1) - hy) - W); s.hi[1] = sc_up((fmax(ey0, ey1) + hy) + W);
        const double z0 = a + (m0 * (b + (cc * m0))), z1 = a + (m1 * (b + (cc * m1)));
        double zlo = fmin(z0, z1), zhi = fmax(z0, z1);
        const double mv = -b / (2.0 * cc);
        if (mv > m0 && mv < m1) {
            const double zv = a + (mv * (b + (cc * mv)));
            zlo = fmin(zlo, zv);
            zhi = fmax(zhi, zv);
        }
        const double Zb = fabs(a) + (fabs(b) + fabs(cc) * Bm) * Bm;
        const double E = (SC_SLACK * (Zb + depth)) * (1.0 + 1e-9);
        s.lo[2] = sc_down(((cz + zlo) - depth) - E);
        s.hi[2] = sc_up((cz + zhi) + E);
    }
    out[k] = s;
}

// gkey: the cells' keys (all ones on entry), in the caller's out_min_row; gtally: the cells' rows in the low and their
// violations in the high 32 bits (n < 2^32, so neither half carries), zeroed, in the caller's out_count.  stats
// (SC_STATLINES lines of three words, zeroed): the (row, span) pairs that took part, the (tile, span) pairs walked, the cell flushes.
__global__ __launch_bounds__(CL_THREADS) void sc_sweep_k(const float* __restrict__ xyz, const uint8_t* __restrict__ skip,
                                                         int64_t n, const double* __restrict__ curves10, int nspans,
                                                         int nst, const ScSpan* __restrict__ sp,
                                                         const uint32_t* __restrict__ take, double half, double depth,
                                                         double limit, float* __restrict__ out_v,
                                                         int32_t* __restrict__ out_span,
                                                         int32_t* __restrict__ out_station,
                                                         unsigned long long* __restrict__ gkey,
                                                         unsigned long long* __restrict__ gtally,
                                                         unsigned long long* __restrict__ stats) {
    __shared__ uint64_t active[CL_WORDS];
    __shared__ unsigned long long skey[SC_MAXST];                // per station: (bits(vf) << 32) | row
    __shared__ uint32_t scnt[SC_MAXST];                          // rows in the low half, violations in the high half
    __shared__ double wlo[CL_WAVES][3], whi[CL_WAVES][3];
    __shared__ uint32_t sstat[3];
    static_assert(CL_TILE < 65536, "scnt packs a tile's rows and violations into 16 bits each");
    const int w = wave_id(), l = lane_id();
    const int64_t base = (int64_t)blockIdx.x * CL_TILE + (int64_t)w * (64 * CL_ROUNDS);
    const ScRow* __restrict__ rows = reinterpret_cast<const ScRow*>(xyz);
    // every load of the tile is issued before anything is waited for, and none stands under a condition (cl_sweep_k)
    ScRow q[CL_ROUNDS];
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
    for (int j = threadIdx.x; j < nst; j += CL_THREADS) { skey[j] = SC_EMPTY; scnt[j] = 0u; }
    if (threadIdx.x < 3) sstat[threadIdx.x] = 0u;
    // the tile's bounding box over its finite rows that are not skipped (no other row can take part)
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
    cull_tile_box(lo, hi, wlo, whi);
    cull_tile_bitmap<CL_WAVES>(active, nspans, lo, hi, [&](int t, const double*& blo, const double*& bhi) {
        blo = sp[t].lo;
        bhi = sp[t].hi;
        return take[t] != 0;
    });

    float best[CL_ROUNDS];
    int who[CL_ROUNDS], at[CL_ROUNDS];
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) { best[r] = INFINITY; who[r] = -1; at[r] = -1; }
    uint32_t ran = 0, walked = 0, flushed = 0;
    const int nwords = (nspans + 63) >> 6, last = nst - 1;
    const double nstd = (double)nst, lastd = (double)last, nhalf = -half;
    int word = -1;
    uint64_t bits = 0;
    for (int k = cull_next_bit(active, nwords, word, bits); k >= 0; k = cull_next_bit(active, nwords, word, bits)) {
        const double* __restrict__ c = curves10 + 10 * (size_t)k;
        const double cx = c[0], cy = c[1], cz = c[2], ux = c[3], uy = c[4], a = c[5], b = c[6], cc = c[7], m0 = c[8],
                     m1 = c[9];
        const double step = (m1 - m0) / nstd;
        ++walked;
        bool any = false;                                // (wave-uniform)
#pragma unroll
        for (int r = 0; r < CL_ROUNDS; ++r) {
            // every parenthesis is the rule's: with -ffp-contract=off the written order is what is computed
            const double dx = (double)q[r].x - cx, dy = (double)q[r].y - cy;
            const double t = (dy * ux) - (dx * uy);
            const double m = (dx * ux) + (dy * uy);
            bool in = ok[r] && t >= nhalf && t <= half && m >= m0 && m <= m1;
            if (__ballot(in) == 0) continue;             // (wave-uniform)
            const double h = (double)q[r].z - cz;
            const double zw = a + (m * (b + (cc * m)));
            const double v = zw - h;
            in = in && v >= 0.0 && v <= depth;
            const uint64_t part = __ballot(in);
            if (part == 0) continue;                     // (wave-uniform)
            any = true;
            ran += (uint32_t)__popcll(part);
            const double jd = floor((m - m0) / step);
            int j = jd >= lastd ? last : (int)jd;
            if (!(jd >= 0.0)) j = 0;                     // (never under the rule's m >= m0; keeps the slot index in range)
            const float vf = fabsf((float)v);
            const uint32_t row = (uint32_t)(base + r * 64 + l);
            const unsigned long long key = ((unsigned long long)__float_as_uint(vf) << 32) | row;
            const bool vio = in && v <= limit;
            if (in && vf < best[r]) { best[r] = vf; who[r] = k; at[r] = j; }
            // the wave's rows of one span mostly share a station: then one lane adds the lot
            const int j0 = __builtin_amdgcn_readlane(j, (int)__builtin_ctzll(part));
            if (__ballot(in && j != j0) == 0) {
                const unsigned long long low = wave_reduce_min(in ? key : SC_EMPTY);
                const uint32_t nv = (uint32_t)__popcll(__ballot(vio));
                if (l == 0) {
                    atomicMin(&skey[j0], low);
                    atomicAdd(&scnt[j0], (uint32_t)__popcll(part) + (nv << 16));
                }
            } else if (in) {
                atomicMin(&skey[j], key);
                atomicAdd(&scnt[j], vio ? 0x10001u : 1u);
            }
        }
        // the tile's slots that are not empty go out, once per (tile, span), and are empty again.  Every wave walks
        // the same bitmap, so every wave stands at these barriers the same number of times
        if (__syncthreads_or(any ? 1 : 0)) {
            for (int j = threadIdx.x; j < nst; j += CL_THREADS) {
                const unsigned long long key = skey[j];
                if (key != SC_EMPTY) {
                    const uint32_t cv = scnt[j];
                    skey[j] = SC_EMPTY;
                    scnt[j] = 0u;
                    const size_t cell = (size_t)k * (size_t)nst + (size_t)j;
                    atomicMin(&gkey[cell], key);
                    atomicAdd(&gtally[cell], ((unsigned long long)(cv >> 16) << 32) | (unsigned long long)(cv & 0xFFFFu));
                    ++flushed;
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        if (i < n) { out_v[i] = best[r]; out_span[i] = who[r]; out_station[i] = at[r]; }
    }
    // the three counters: summed over the tile in LDS, then added to one of SC_STATLINES cache lines - every workgroup
    // adding to the same three words keeps the whole sweep waiting on one line
    flushed = wave_reduce_add(flushed);
    if (l == 0) {
        if (ran) atomicAdd(&sstat[0], ran);
        if (w == 0 && walked) atomicAdd(&sstat[1], walked);
        if (flushed) atomicAdd(&sstat[2], flushed);
    }
    __syncthreads();
    if (threadIdx.x < 3 && sstat[threadIdx.x])
        atomicAdd(&stats[(blockIdx.x % SC_STATLINES) * SC_STATWORDS + threadIdx.x], (unsigned long long)sstat[threadIdx.x]);
}

// keys (in out_min_row's place) to the smallest distance and its row - an empty cell keeps its -1 and gets +inf -, the
// packed tallies (in out_count's place) to the rows and the violations
__global__ __launch_bounds__(CL_THREADS) void sc_decode_k(int64_t cells, unsigned long long* __restrict__ keys,
                                                          unsigned long long* __restrict__ tally,
                                                          int64_t* __restrict__ out_violations,
                                                          float* __restrict__ out_min_v,
                                                          const unsigned long long* __restrict__ stats,
                                                          int64_t* __restrict__ out_stats) {
    const int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
    if (out_stats && i < 3) {
        unsigned long long sum = 0;
        for (int s = 0; s < SC_STATLINES; ++s) sum += stats[s * SC_STATWORDS + i];
        out_stats[i] = (int64_t)sum;
    }
    if (i >= cells) return;
    const unsigned long long tv = tally[i];
    tally[i] = tv & 0xFFFFFFFFull;
    out_violations[i] = (int64_t)(tv >> 32);
    const unsigned long long key = keys[i];
    if (key == SC_EMPTY) {
        out_min_v[i] = INFINITY;
    } else {
        out_min_v[i] = __uint_as_float((uint32_t)(key >> 32));
        keys[i] = key & 0xFFFFFFFFull;
    }
}

struct ScWs {
    unsigned long long* stats;
    ScSpan* sp;
    uint32_t* take;
};
static void sc_plan(Arena& a, int32_t nspans, ScWs& w) {
    w.stats = a.take<unsigned long long>((size_t)SC_STATLINES * SC_STATWORDS);
    w.sp = a.take<ScSpan>(cl_slots(nspans));
    w.take = a.take<uint32_t>(cl_slots(nspans));
}
static bool sc_sizes_ok(int64_t n, int32_t nspans, int32_t nst) {
    return n >= 0 && n < (int64_t(1) << 32) && nspans >= 0 && nspans <= CL_MAXSPAN && nst >= 1 && nst <= SC_MAXST;
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_span_section_ws_bytes(int64_t n, int32_t nspans, int32_t nstations) {
    if (!sc_sizes_ok(n, nspans, nstations)) return 0;
    Arena a;
    ScWs w;
    sc_plan(a, nspans, w);
    return a.off;
}

extern "C" int pch_span_section_f32(const float* xyz, const uint8_t* skip, int64_t n, const double* curves10,
                                    int32_t nspans, int32_t nstations, double half_width, double depth, double limit,
                                    float* out_v, int32_t* out_span, int32_t* out_station, int64_t* out_count,
                                    int64_t* out_violations, float* out_min_v, int64_t* out_min_row, int64_t* out_stats,
                                    void* ws, size_t ws_bytes, void* stream) {
    PCH_REQUIRE(sc_sizes_ok(n, nspans, nstations), "0 <= n < 2^32, 0 <= nspans <= 4096, 1 <= nstations <= 128");
    PCH_REQUIRE(isfinite(half_width) && isfinite(depth) && isfinite(limit) && half_width > 0.0 && limit > 0.0 &&
                    limit <= depth,
                "half_width, depth and limit must be finite with half_width > 0 and 0 < limit <= depth");
    PCH_REQUIRE(n == 0 || (xyz && out_v && out_span && out_station), "null row buffer");
    PCH_REQUIRE(nspans == 0 || (curves10 && out_count && out_violations && out_min_v && out_min_row),
                "null span buffer");
    PCH_REQUIRE(ws, "null workspace");
    PCH_DEVICE_GUARD(ws);
    hipStream_t s = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    ScWs w;
    sc_plan(a, nspans, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    if (nspans == 0 && out_stats) PCH_HIP_TRY(hipMemsetAsync(out_stats, 0, 3 * sizeof(int64_t), s));
    if (n == 0 && nspans == 0) return PCH_OK;
    const size_t cells = (size_t)nspans * (size_t)nstations;
    PCH_HIP_TRY(hipMemsetAsync(w.stats, 0, sizeof(unsigned long long) * SC_STATLINES * SC_STATWORDS, s));
    if (nspans > 0) {
        PCH_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(int64_t) * cells, s));
        PCH_HIP_TRY(hipMemsetAsync(out_min_row, 0xFF, sizeof(int64_t) * cells, s));
        PCH_LAUNCH("section_bounds", sc_bounds_k, dim3((unsigned)ceil_div(nspans, CL_THREADS)), dim3(CL_THREADS), 0, s,
                   curves10, (int)nspans, half_width, depth, w.sp, w.take);
    }
    if (n > 0)
        PCH_LAUNCH("section_sweep", sc_sweep_k, dim3((unsigned)ceil_div(n, CL_TILE)), dim3(CL_THREADS), 0, s, xyz, skip, n,
                   curves10, (int)nspans, (int)nstations, (const ScSpan*)w.sp, (const uint32_t*)w.take, half_width, depth,
                   limit, out_v, out_span, out_station, reinterpret_cast<unsigned long long*>(out_min_row),
                   reinterpret_cast<unsigned long long*>(out_count), w.stats);
    if (nspans > 0)
        PCH_LAUNCH("section_decode", sc_decode_k, dim3((unsigned)ceil_div((int64_t)cells, CL_THREADS)), dim3(CL_THREADS),
                   0, s, (int64_t)cells, reinterpret_cast<unsigned long long*>(out_min_row),
                   reinterpret_cast<unsigned long long*>(out_count), out_violations, out_min_v,
                   (const unsigned long long*)w.stats, out_stats);
    return PCH_OK;
}
