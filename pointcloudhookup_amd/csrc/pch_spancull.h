// What the sweeps of row tiles over span polylines share (pch_clearance.hip, pch_treefall.hip, pch_swing.hip) on top of
// pch_tilecull.h:
// the tile geometry, the per-span cull record that cl_bounds_k writes (its derivation stands in front of the kernel, in
// pch_clearance.hip), the walk of a tile's spans that carries the rule of include/pch_hip.h, the fold of a round's
// answers per owning span, the per-span tallies and the front of the workspace that holds them.
#pragma once
#include "pch_common.h"
#include "pch_tilecull.h"

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

// cl_finish_k on the stream: the table out of the zeroed front of a ClWs (tally, second, maxinv, counters) and, over
// dist2 and span of the n rows, the lowest row that attains a span's smallest distance (out_min_row arrives as all ones
// = -1; nspans > 0; out_loops may be null)
int cl_finish_run(const double* dist2, const int32_t* span, int64_t n, int nspans, const unsigned long long* tally,
                  const unsigned long long* second, const unsigned long long* maxinv,
                  const unsigned long long* counters, int64_t* out_count, int64_t* out_second, double* out_min_dist2,
                  int64_t* out_min_row, int64_t* out_loops, hipStream_t s);

static bool cl_spans_ok(int32_t nspans, int32_t nseg) {
    return nspans >= 0 && nspans <= CL_MAXSPAN && nseg >= 1 && nseg <= CL_MAXSEG;
}

// The workspace of a span sweep.  In front what one fill zeroes, [ws, sp): per span the rows attributed to it (tally),
// those of them its sweep singles out (second: violations, strikes) and the largest cl_minkey seen (maxinv), then the
// sweep's counters; cl_plan_front leaves the arena there, so a sweep with more to zero takes it before cl_plan_back.
// Behind it what cl_bounds_run writes.
struct ClWs {
    unsigned long long *tally, *second, *maxinv, *counters;
    ClSpan* sp;
    uint32_t* take;
};
static size_t cl_slots(int32_t nspans) { return nspans > 0 ? (size_t)nspans : 1; }
static void cl_plan_front(Arena& a, int32_t nspans, int ncounters, ClWs& w) {
    w.tally = a.take<unsigned long long>(cl_slots(nspans));
    w.second = a.take<unsigned long long>(cl_slots(nspans));
    w.maxinv = a.take<unsigned long long>(cl_slots(nspans));
    w.counters = a.take<unsigned long long>((size_t)ncounters);
}
static void cl_plan_back(Arena& a, int32_t nspans, ClWs& w) {
    w.sp = a.take<ClSpan>(cl_slots(nspans));
    w.take = a.take<uint32_t>(cl_slots(nspans));
}
static size_t cl_front_bytes(const void* ws, const ClWs& w) {
    return (size_t)(reinterpret_cast<const char*>(w.sp) - static_cast<const char*>(ws));
}

#ifdef __HIPCC__
// the smallest d2 of a span is kept as the LARGEST ~bits(d2), so that it folds with an integer atomicMax into a word that
// starts as zero = no row yet (non-negative doubles order as their bit patterns)
__device__ __forceinline__ unsigned long long cl_minkey(double d2) {
    return ~(unsigned long long)__double_as_longlong(d2);
}
__device__ __forceinline__ double cl_minkey_value(unsigned long long key) {
    return key ? __longlong_as_double((long long)~key) : (double)INFINITY;
}

// the spans a tile has to walk, out of every lane's box (lo, hi) around its rows that can be accepted: those that take
// part and that cull_tile_bitmap keeps.  Two barriers; wlo / whi as cull_tile_box takes them.
__device__ __forceinline__ void cl_tile_spans(uint64_t* active, int nspans, const ClSpan* __restrict__ sp,
                                              const uint32_t* __restrict__ take, double (&lo)[3], double (&hi)[3],
                                              double (&wlo)[CL_WAVES][3], double (&whi)[CL_WAVES][3]) {
    cull_tile_box(lo, hi, wlo, whi);
    cull_tile_bitmap<CL_WAVES>(active, nspans, lo, hi, [&](int t, const double*& blo, const double*& bhi) {
        blo = sp[t].lo;
        bhi = sp[t].hi;
        return take[t] != 0;
    });
}

// The rule for a wave's CL_ROUNDS rows against the spans of the tile's bitmap, in ascending span order: best[r] = the
// smallest d2 <= r2(r) over the spans and who[r] = the lowest span that attains it (INFINITY and -1 where there is
// none).  A row is measured from (q[r].x, q[r].y, height(r)); ok[r] = it can be accepted at all.  The span and segment
// records come through wave-uniform (scalar) loads.  Every parenthesis is the rule's: with -ffp-contract=off the written
// order is what is computed.  ran / walked: the (row, span) segment loops run and the spans walked by this wave.
//
// Four tests stand in front of the segment loop.  d2 = g + t*t >= t*t (g >= 0), so a row with t*t > r2 or t*t >= best
// cannot be taken; nor can one with m outside [flo, fhi] or w outside [wlo, whi]: (a) and (b) of the derivation in front
// of cl_bounds_k, which holds for every r2(r) up to the square of the radius the bounds were made for.  A NaN fails every
// comparison, as it does in the rule.
template <class Row, class Height, class Radius2>
__device__ __forceinline__ void cl_walk_spans(const uint64_t* active, int nspans, const double* __restrict__ curves5,
                                              const double* __restrict__ segs, int nseg,
                                              const ClSpan* __restrict__ sp, const Row (&q)[CL_ROUNDS],
                                              const bool (&ok)[CL_ROUNDS], Height height, Radius2 r2,
                                              double (&best)[CL_ROUNDS], int (&who)[CL_ROUNDS], uint32_t& ran,
                                              uint32_t& walked) {
    const int nwords = (nspans + 63) >> 6;
#pragma unroll
    for (int r = 0; r < CL_ROUNDS; ++r) { best[r] = INFINITY; who[r] = -1; }
    ran = 0;
    walked = 0;
    int word = -1;
    uint64_t bits = 0;
    for (int k = cull_next_bit(active, nwords, word, bits); k >= 0; k = cull_next_bit(active, nwords, word, bits)) {
        const double* __restrict__ c = curves5 + 5 * (size_t)k;
        const double cx = c[0], cy = c[1], cz = c[2], ux = c[3], uy = c[4];
        const double flo = sp[k].flo, fhi = sp[k].fhi, hlo = sp[k].wlo, hhi = sp[k].whi;
        double m[CL_ROUNDS], h[CL_ROUNDS], tt[CL_ROUNDS], g[CL_ROUNDS];
        bool go[CL_ROUNDS];
        bool some = false;
#pragma unroll
        for (int r = 0; r < CL_ROUNDS; ++r) {
            const double dx = (double)q[r].x - cx, dy = (double)q[r].y - cy;
            h[r] = height(r) - cz;
            m[r] = (dx * ux) + (dy * uy);
            const double t = (dy * ux) - (dx * uy);
            tt[r] = t * t;
            go[r] = ok[r] && tt[r] <= r2(r) && tt[r] < best[r] && m[r] >= flo && m[r] <= fhi && h[r] >= hlo &&
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
            if (go[r] && d2 <= r2(r) && d2 < best[r]) { best[r] = d2; who[r] = k; }
        }
    }
}

// one round's answers by owning span: fold(k, same, owned) once per distinct span k among the lanes' `who`, in the
// order of the lowest lane that holds it; same = this lane's row is k's, owned = how many lanes' are (wave-uniform)
template <class Fold>
__device__ __forceinline__ void cl_fold_owners(int who, Fold fold) {
    uint64_t pend = __ballot(who >= 0);
    while (pend) {
        const int k = __builtin_amdgcn_readlane(who, (int)__builtin_ctzll(pend));
        const bool same = who == k;
        const uint64_t mask = __ballot(same);
        fold(k, same, (uint32_t)__popcll(mask));
        pend &= ~mask;
    }
}

// a tile's per-span LDS tallies go out once per (tile, span): hist packs the rows attributed to the span in the low
// half and those singled out in the high half (a tile has 1024 rows).  Every wave's adds must be behind a barrier.
__device__ __forceinline__ void cl_flush_hist(const uint32_t* hist, int nspans, unsigned long long* __restrict__ tally,
                                              unsigned long long* __restrict__ second) {
    for (int j = threadIdx.x; j < nspans; j += CL_THREADS) {
        const uint32_t hv = hist[j];
        if (hv & 0xFFFFu) atomicAdd(&tally[j], (unsigned long long)(hv & 0xFFFFu));
        if (hv >> 16) atomicAdd(&second[j], (unsigned long long)(hv >> 16));
    }
}
#endif  // __HIPCC__

}  // namespace pch
