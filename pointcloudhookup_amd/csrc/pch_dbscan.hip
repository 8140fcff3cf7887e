// Stage C: exact DBSCAN for every file-order chunk at once (reference:
// utils/tower_extraction.py:96-117 -> sklearn.cluster.DBSCAN(...).fit(chunk)).
//
// Method (grid DBSCAN, exact): points are binned into cubic cells of side
//   s = eps/sqrt(3) * (1 - 2^-16)
// so any two points of one cell are closer than eps under sklearn's own float64 predicate
// (DESIGN.md "cell-side margin").  Consequences used below:
//   * a cell holding >= min_samples points consists of core points only (no distance tests);
//   * all core points of one cell belong to one cluster, so clusters are the connected
//     components of a graph over CELLS (edge: some core pair of the two cells within eps);
//   * every neighbour of a point lies in the 5x5x5 block of cells around its own cell.
// Cell key = [chunk | cz | cy | cx] (x in the low bits), so for a fixed (dy,dz) the five
// x-neighbour cells are one contiguous run of the sorted point array: 25 runs per cell.
// Cluster numbering reproduces sklearn's sweep: id = rank of the component's smallest core
// index; a border point takes the smallest id among its core neighbours.
//
// Where what lives: pch_dbscan_cells.hip turns the rows into the cell table, this file runs the fit on that table
// (core points, union, labels) and keeps the workspace plan and the retained fit, pch_dbscan_query.hip holds the
// calls that continue a retained fit; pch_dbscan.h is what they share.
#include "pch_dbscan.h"
#include "pch_unionfind.h"

namespace pch {

constexpr int DB_FEW_QUERIES = 24;
constexpr int DB_AHEAD = 3;              // db_core_k, long sweeps: 64-candidate groups whose loads are in flight together
constexpr long long DB_LONG_TOT = 8192;  // ... a cell counts as long from this many candidates in its neighbourhood
constexpr int DB_SEGS = 43;          // 9 inner + 9 + 9 end pieces of the near runs + 16 outer runs

// ---- one query per lane against a staged tile of candidates --------------------------------
// The tile holds candidates in pairs (x0 x1 | y0 y1 | z0 z1), so the float32 pre-filter of db_within2 runs on
// packed two-wide arithmetic (v_pk_add/mul/fma_f32: same operations, same roundings) and without a branch per
// candidate: the lane counts d <= eps2_lo and d < eps2_hi separately; only if the two counts differ - some
// candidate fell into the 2^-20 guard band - is the tile counted again with the exact predicate.  The LDS reads
// of four pairs are issued ahead of their arithmetic.  7 VALU instructions per test (before: 13 and a wait for
// LDS per candidate).
typedef float f32x2 __attribute__((ext_vector_type(2)));
struct __attribute__((aligned(16))) DbPair { f32x2 x, y, z, pad; };

__device__ __forceinline__ void db_tile_put(DbPair* __restrict__ tile, int l, const float4& p) {
    float* f = reinterpret_cast<float*>(&tile[l >> 1]);
    f[l & 1] = p.x; f[2 + (l & 1)] = p.y; f[4 + (l & 1)] = p.z;
}
__device__ __forceinline__ float4 db_tile_get(const DbPair* __restrict__ tile, int k) {
    const float* f = reinterpret_cast<const float*>(&tile[k >> 1]);
    float4 p;
    p.x = f[k & 1]; p.y = f[2 + (k & 1)]; p.z = f[4 + (k & 1)]; p.w = 0.0f;
    return p;
}
// nj candidates staged (padding beyond nj up to a multiple of 8 must be far away: +3e38); returns the number
// of them within eps of q
__device__ __forceinline__ int db_tile_count(const float4& q, const DbPair* __restrict__ tile, int nj,
                                             const DbGrid& g) {
    const f32x2 qx = {q.x, q.x}, qy = {q.y, q.y}, qz = {q.z, q.z};
    const float lo = g.eps2_lo, hi = g.eps2_hi;
    int c_lo = 0, c_hi = 0;
    const int np = ((nj + 7) & ~7) >> 1;
    for (int k = 0; k < np; k += 4) {
        f32x2 px[4], py[4], pz[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { px[u] = tile[k + u].x; py[u] = tile[k + u].y; pz[u] = tile[k + u].z; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const f32x2 dx = qx - px[u], dy = qy - py[u], dz = qz - pz[u];
            f32x2 d = dx * dx;
            d = __builtin_elementwise_fma(dy, dy, d);
            d = __builtin_elementwise_fma(dz, dz, d);
            c_lo += (d.x <= lo ? 1 : 0) + (d.y <= lo ? 1 : 0);
            c_hi += (d.x < hi ? 1 : 0) + (d.y < hi ? 1 : 0);
        }
    }
    if (c_lo != c_hi) {                                    // a candidate inside the guard band: exact recount
        c_lo = 0;
        for (int k = 0; k < nj; ++k) c_lo += db_within2(q, db_tile_get(tile, k), g) ? 1 : 0;
    }
    return c_lo;
}

// the same between two boxes (db_box_d2)
__device__ __forceinline__ double db_boxbox_d2(const float* __restrict__ a, const float* __restrict__ b) {
    const double gx = fmax(fmax((double)b[0] - (double)a[3], (double)a[0] - (double)b[3]), 0.0);
    const double gy = fmax(fmax((double)b[1] - (double)a[4], (double)a[1] - (double)b[4]), 0.0);
    const double gz = fmax(fmax((double)b[2] - (double)a[5], (double)a[2] - (double)b[5]), 0.0);
    double d = gx * gx;
    d += gy * gy;
    d += gz * gz;
    return d;
}

// ---- bounding box of the finite input points (only when the caller did not provide one) ------
__global__ __launch_bounds__(DB_THREADS) void db_aabb_in_k(const float* __restrict__ xyz, int64_t n,
                                                           uint32_t* __restrict__ mm) {
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * DB_THREADS) {
        const float x = xyz[3 * i + 0], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (!(fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY)) continue;
        const float v[3] = {x, y, z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t k = f32_ordered(v[a]);
            lo[a] = k < lo[a] ? k : lo[a];
            hi[a] = k > hi[a] ? k : hi[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = wave_reduce_min(lo[a]);
        hi[a] = wave_reduce_max(hi[a]);
        if (lane_id() == 0) {
            if (lo[a] != 0xFFFFFFFFu) atomicMin(&mm[a], lo[a]);
            if (hi[a] != 0u) atomicMax(&mm[3 + a], hi[a]);
        }
    }
}

__global__ __launch_bounds__(DB_THREADS) void db_add_offset_k(int32_t* __restrict__ labels, int64_t n, int32_t off) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i < n && labels[i] >= 0) labels[i] += off;
}

// neighbour-row table: [cell][25] cell-index ranges, shared by the core / union / border kernels
__global__ __launch_bounds__(DB_THREADS) void db_rowtab_k(DbGrid g, const uint64_t* __restrict__ cell_key,
                                                          int m, int2* __restrict__ rowtab) {
    const int c = (blockIdx.x * DB_WAVES + wave_id()) * 2 + (lane_id() >> 5);   // two cells per wave
    const int l = lane_id() & 31;
    if (c >= m || l >= DB_ROWS) return;
    rowtab[(int64_t)c * DB_ROWS + l] = db_row_run(g, cell_key, cell_key[c], l);
}

// ---- core points ---------------------------------------------------------------------
// A straggler of db_core_k's phase 2: one query against what is left of the candidate segments sa[r] .. sb[r],
// r < DB_SEGS, from row j0 of segment r on.  The lanes take 64 candidates each per group, AHEAD groups per trip, and
// the sweep leaves at min_samples, checked per trip.  Returns the count.  COUNT: the tallies of db_core_k<true>, 64
// lane slots per group that holds a candidate.
// AHEAD: a lone point beside a tower core that is NOT core passes every candidate of its neighbourhood (13 585 in the
// bench tile) - one dependent load per 64 candidates made such a wave the tail of the kernel.  Where the neighbourhood
// is that large (DB_LONG_TOT) the callers sweep DB_AHEAD groups per trip, their loads in flight together, else one:
// the same candidates in the same order, and a sweep leaves at min_samples either way.
template <bool COUNT, int AHEAD>
__device__ __forceinline__ int db_query_sweep(const DbGrid& g, const float4* __restrict__ pts, const float4 qp,
                                              int count, int r, uint32_t j0, const uint32_t* sa, const uint32_t* sb,
                                              unsigned long long& n_useful, unsigned long long& n_slots) {
    const int l = lane_id();
    while (r < DB_SEGS && count < g.min_samples) {
        const uint32_t pb = sb[r];
        if (j0 >= pb) { ++r; if (r < DB_SEGS) j0 = sa[r]; continue; }
        float4 P[AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const uint32_t j = j0 + 64u * u + l;
            P[u] = pts[j < pb ? j : pb - 1];               // past the end: the last row again, not counted below
        }
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const uint32_t jb = j0 + 64u * u;
            const bool hit = jb + l < pb && db_within2(qp, P[u], g);
            count += (int)__popcll(__ballot(hit));
            if (COUNT && jb < pb) { n_useful += (pb - jb) < 64u ? (pb - jb) : 64u; n_slots += 64; }
        }
        j0 += 64u * AHEAD;
    }
    return count;
}

// ---- a cell's summary, written by the wave of db_core_k that owns the cell (the staged route only; every other route
// sweeps the rows for it, db_cellstats_k): cell_box, a box that CONTAINS the cell's core points, and cell_min, their
// smallest original row.  Every reader of cell_box uses it to reject ("box distance > eps^2: skip", the strip's x
// range) and tests real points otherwise, so any containing box gives the same links and labels.
// no core point: the values db_cell_decode yields for an empty accumulator
__device__ __forceinline__ void db_summary_none(float* __restrict__ cell_box, int* __restrict__ cell_min, int c) {
    const int l = lane_id();
    if (l < 6) cell_box[6 * (int64_t)c + l] = l < 3 ? INFINITY : -INFINITY;
    if (l == 0) cell_min[c] = INT_BIG;
}
// Dense cell (all rows core): the cell's own bounds, origin + index * s per axis.  A row of cell i lies in
// [origin + (i - 2^-21) s, origin + (i + 1 + 2^-21) s] (the rounding of db_cell_coords' product, see DbGrid); the bounds
// are taken DB_BOX_MARGIN = 2^-16 cells further out, which also covers the roundings of this float64 expression (below
// 2^-21 cells, or below one float32 step of coordinates that large), and are rounded outward to float32.  cell_min
// stays what db_celltab_k staged: the smallest row of the cell.
constexpr double DB_BOX_MARGIN = 1.0 / 65536.0;
__device__ __forceinline__ void db_summary_dense(const DbGrid& g, uint64_t key, float* __restrict__ cell_box, int c) {
    const int l = lane_id();
    if (l >= 6) return;
    const int a = l % 3;
    const bool up = l >= 3;
    const uint64_t i = a == 0 ? key & ((1ull << g.bx) - 1)
                     : a == 1 ? (key >> g.bx) & ((1ull << g.by) - 1) : (key >> (g.bx + g.by)) & ((1ull << g.bz) - 1);
    const double o = a == 0 ? (double)g.ox : a == 1 ? (double)g.oy : (double)g.oz;
    const double edge = o + ((double)i + (up ? 1.0 + DB_BOX_MARGIN : -DB_BOX_MARGIN)) * g.cell;
    float f = (float)edge;
    if (up ? (double)f < edge : (double)f > edge) f = nextafterf(f, up ? INFINITY : -INFINITY);
    cell_box[6 * (int64_t)c + l] = f;
}
// Sparse cell: the exact values, folded over the rounds of 64 of its rows that the wave holds as queries anyway.
// Seven words of LDS per wave, so that nothing is carried in registers through the sweeps: the coordinates as ordered
// keys (f32_ordered), min xyz | max xyz | smallest row
__device__ __forceinline__ void db_summary_start(uint32_t* sm) {
    const int l = lane_id();
    if (l < 7) sm[l] = l < 3 ? 0xFFFFFFFFu : (l < 6 ? 0u : (uint32_t)INT_BIG);
    __builtin_amdgcn_wave_barrier();
}
// one row per lane: p.w is its original row.  LDS atomics of the core lanes, no wave reductions: seven of those side by
// side cost db_core_k<false> six to eight VGPRs and a wave of occupancy
__device__ __forceinline__ void db_summary_fold(uint32_t* sm, bool is_core, const float4& p) {
    if (!is_core) return;
    const float v[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t key = f32_ordered(v[k]);
        atomicMin(&sm[k], key);
        atomicMax(&sm[3 + k], key);
    }
    atomicMin(&sm[6], __float_as_uint(p.w));
}
// no core row: +inf / -inf and INT_BIG, as db_summary_none
__device__ __forceinline__ void db_summary_put(const uint32_t* sm, float* __restrict__ cell_box,
                                               int* __restrict__ cell_min, int c) {
    __builtin_amdgcn_wave_barrier();
    const int l = lane_id();
    if (l >= 7) return;
    const uint32_t v = sm[l];
    if (l == 6) cell_min[c] = (int)v;
    else cell_box[6 * (int64_t)c + l] = sm[6] == (uint32_t)INT_BIG ? (l < 3 ? INFINITY : -INFINITY) : f32_unordered(v);
}
// one wave per cell.  Dense cell: all core.  Sparse cell: n-body tile loop - every lane owns one
// query point of the cell, candidate tiles (64 points of the sorted neighbour runs) are staged
// once in LDS and broadcast to all queries; the wave leaves as soon as every query has reached
// min_samples (checked per tile).  Each candidate is loaded once per cell, not once per query.
// COUNT (measurement builds of the SAME control flow, pch_dbscan_set_pair_counting): the wave tallies the distance
// tests it makes - useful ones (a real query against a real candidate) and issued lane slots (64 per
// wave-instruction group, padding and idle lanes included) - and adds them to stats[0..3] once, at its end:
// [0] useful pair tests, [1] issued lane slots, [2] cells that reached the test path, [3] LDS tiles staged.
template <bool COUNT>
__global__ __launch_bounds__(DB_THREADS) void db_core_k(DbGrid g, const float4* __restrict__ pts,
                                                        const uint32_t* __restrict__ cell_start,
                                                        const uint64_t* __restrict__ cell_key, int m,
                                                        const int2* __restrict__ rowtab,
                                                        uint8_t* __restrict__ core_s,
                                                        uint32_t* __restrict__ cell_ncore,
                                                        float* __restrict__ cell_box, int* __restrict__ cell_min,
                                                        unsigned long long* __restrict__ stats) {
    const bool summary = cell_box != nullptr;              // the staged route: this wave writes the cell's summary
    unsigned long long n_useful = 0, n_slots = 0, n_tiles = 0;
    auto tally = [&]() {
        if (COUNT && lane_id() == 0) {
            atomicAdd(&stats[0], n_useful); atomicAdd(&stats[1], n_slots);
            atomicAdd(&stats[2], 1ull); atomicAdd(&stats[3], n_tiles);
        }
    };
    __shared__ RowSet rows[DB_WAVES];
    __shared__ DbPair tiles[DB_WAVES][32];
    __shared__ uint32_t seg_a[DB_WAVES][DB_SEGS], seg_b[DB_WAVES][DB_SEGS];
    __shared__ uint32_t sums[DB_WAVES][8];                 // db_summary_fold
    const int c = blockIdx.x * DB_WAVES + wave_id();
    if (c >= m) return;
    const int l = lane_id();
    const uint32_t s = cell_start[c], e = cell_start[c + 1];
    const int cnt = (int)(e - s);
    {
        const int sh = g.bx + g.by + g.bz;
        if (g.chunk_bad[sh < 64 ? (cell_key[c] >> sh) : 0]) {            // points of NaN/inf chunks
            for (uint32_t i = s + l; i < e; i += 64) core_s[i] = 0;
            if (l == 0) cell_ncore[c] = 0;
            if (summary) db_summary_none(cell_box, cell_min, c);
            return;
        }
    }
    if (cnt >= g.min_samples) {
        for (uint32_t i = s + l; i < e; i += 64) core_s[i] = 1;
        if (l == 0) cell_ncore[c] = (uint32_t)cnt;
        if (summary) db_summary_dense(g, cell_key[c], cell_box, c);
        return;
    }
    RowSet* rs = &rows[wave_id()];
    db_rows(g, cell_key, cell_key[c], rs, rowtab, c);
    // candidate total: if even all candidates together are too few, nobody is core
    long long tot = 0;
    if (l < DB_ROWS) tot = (long long)cell_start[rs->cb[l]] - (long long)cell_start[rs->ca[l]];
    tot = wave_reduce_add(tot);
    if (tot < (long long)g.min_samples) {
        for (uint32_t i = s + l; i < e; i += 64) core_s[i] = 0;
        if (l == 0) cell_ncore[c] = 0;
        if (summary) db_summary_none(cell_box, cell_min, c);
        return;
    }
    // candidate segments in nearest-first order: the 27-cell neighbourhood first (x-1..x+1 of the
    // nine nearest runs), then the x-2 / x+2 ends of those runs, then the sixteen outer runs
    uint32_t* sa = seg_a[wave_id()];
    uint32_t* sb = seg_b[wave_id()];
    {
        const uint64_t xmask = (1ull << g.bx) - 1;
        const int cx = (int)(cell_key[c] & xmask);
        if (l < DB_ROWS) {
            const int ca = rs->ca[l], cb = rs->cb[l];
            if (l < 9) {
                int ia = ca, ib = cb;
                if (ca < cb) {
                    if ((int)(cell_key[ca] & xmask) == cx - 2) ia = ca + 1;
                    if (ib > ia && (int)(cell_key[cb - 1] & xmask) == cx + 2) ib = cb - 1;
                }
                sa[l] = cell_start[ia];      sb[l] = cell_start[ib];          // inner part
                sa[9 + l] = cell_start[ca];  sb[9 + l] = cell_start[ia];      // x-2 end
                sa[18 + l] = cell_start[ib]; sb[18 + l] = cell_start[cb];     // x+2 end
            } else {
                sa[18 + l] = cell_start[ca]; sb[18 + l] = cell_start[cb];     // outer runs: slots 27..42
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    uint32_t ncore = 0;
    uint32_t* sum = sums[wave_id()];
    if (summary) db_summary_start(sum);
    const bool long_sweep = tot >= DB_LONG_TOT;            // wave-uniform
    if (cnt < DB_FEW_QUERIES) {
        unsigned long long cores = 0;                      // bit q - s: query q is core
        // a handful of queries (cluster fringe): lanes sweep the candidates of one query at a
        // time and leave at min_samples - usually within the first tile of a dense neighbour.  The two sweeps are
        // db_query_sweep's from (0, sa[0]), written out: through that function db_core took 0.126 ms on the bench tile
        // against 0.120 (measured in three forms of the function; registers and LDS the same).
        for (uint32_t q = s; q < e; ++q) {
            const float4 qp = pts[q];
            int count = 0;
            if (long_sweep) {
                // DB_AHEAD groups per trip, their loads in flight together (db_query_sweep has the reason)
                for (int r = 0; r < DB_SEGS && count < g.min_samples; ++r) {
                    const uint32_t pa = sa[r], pb = sb[r];
                    for (uint32_t j0 = pa; j0 < pb && count < g.min_samples; j0 += 64u * DB_AHEAD) {
                        float4 P[DB_AHEAD];
#pragma unroll
                        for (int u = 0; u < DB_AHEAD; ++u) {
                            const uint32_t j = j0 + 64u * u + l;
                            P[u] = pts[j < pb ? j : pb - 1];
                        }
#pragma unroll
                        for (int u = 0; u < DB_AHEAD; ++u) {
                            const uint32_t jb = j0 + 64u * u;
                            const bool hit = jb + l < pb && db_within2(qp, P[u], g);
                            count += (int)__popcll(__ballot(hit));
                            if (COUNT && jb < pb) { n_useful += (pb - jb) < 64u ? (pb - jb) : 64u; n_slots += 64; }
                        }
                    }
                }
            } else {
                for (int r = 0; r < DB_SEGS && count < g.min_samples; ++r) {
                    const uint32_t pa = sa[r], pb = sb[r];
                    for (uint32_t j0 = pa; j0 < pb && count < g.min_samples; j0 += 64) {
                        const uint32_t j = j0 + l;
                        bool hit = false;
                        if (j < pb) hit = db_within2(qp, pts[j], g);
                        count += (int)__popcll(__ballot(hit));
                        if (COUNT) { n_useful += (pb - j0) < 64u ? (pb - j0) : 64u; n_slots += 64; }
                    }
                }
            }
            const bool is_core = count >= g.min_samples;
            if (l == 0) core_s[q] = is_core ? 1 : 0;
            ncore += is_core;
            cores |= (unsigned long long)is_core << (q - s);
        }
        if (l == 0) cell_ncore[c] = ncore;
        if (summary) {                                     // the cell's rows once more, one per lane
            const bool is_core = (cores >> l) & 1ull;
            db_summary_fold(sum, is_core, pts[is_core ? s + l : s]);
            db_summary_put(sum, cell_box, cell_min, c);
        }
        tally();
        return;
    }
    DbPair* tile = tiles[wave_id()];
    for (uint32_t q0 = s; q0 < e; q0 += 64) {              // 64 query points per round
        const bool valid = q0 + l < e;
        float4 Q;
        Q.x = Q.y = Q.z = 3.0e37f; Q.w = 0.0f;             // idle lanes sit far away (finite)
        if (valid) Q = pts[q0 + l];
        int count = 0;
        unsigned long long active = __ballot(valid);        // queries still below min_samples
        int r = 0;
        uint32_t j0 = sa[0];
        // phase 1: all queries against one staged candidate tile at a time, while enough of
        // them are still counting to keep the lanes busy
        while (r < DB_SEGS && __popcll(active) >= DB_FEW_QUERIES / 2) {
            const uint32_t pb = sb[r];
            if (j0 >= pb) { ++r; if (r < DB_SEGS) j0 = sa[r]; continue; }
            const int nj = (int)((pb - j0) < 64u ? (pb - j0) : 64u);
            float4 P;
            P.x = P.y = P.z = 3.0e38f; P.w = 0.0f;         // padding: squared distance overflows to +inf
            if (l < nj) P = pts[j0 + l];
            __builtin_amdgcn_wave_barrier();
            db_tile_put(tile, l, P);
            __builtin_amdgcn_wave_barrier();
            count += db_tile_count(Q, tile, nj, g);
            if (COUNT) {
                n_useful += (unsigned long long)__popcll(__ballot(valid)) * (unsigned)nj;
                n_slots += 64ull * (unsigned)((nj + 7) & ~7);
                ++n_tiles;
            }
            j0 += 64;
            active = __ballot(valid && count < g.min_samples);
        }
        // phase 2: the few stragglers one by one, lanes over the remaining candidates
        while (active) {
            const int ql = (int)__builtin_ctzll(active);
            active &= active - 1;
            float4 qp;
            qp.x = __shfl(Q.x, ql, 64); qp.y = __shfl(Q.y, ql, 64); qp.z = __shfl(Q.z, ql, 64); qp.w = 0.0f;
            const int c0 = __shfl(count, ql, 64);
            const int cq = long_sweep
                ? db_query_sweep<COUNT, DB_AHEAD>(g, pts, qp, c0, r, j0, sa, sb, n_useful, n_slots)
                : db_query_sweep<COUNT, 1>(g, pts, qp, c0, r, j0, sa, sb, n_useful, n_slots);
            if (l == ql) count = cq;
        }
        const bool is_core = valid && count >= g.min_samples;
        if (valid) core_s[q0 + l] = is_core ? 1 : 0;
        ncore += (uint32_t)__popcll(__ballot(is_core));
        if (summary) {
            Q.w = pts[valid ? q0 + l : s].w;               // the original row, not kept through the sweeps
            db_summary_fold(sum, is_core, Q);
        }
    }
    if (l == 0) cell_ncore[c] = ncore;
    if (summary) db_summary_put(sum, cell_box, cell_min, c);
    tally();
}

// ---- per-cell box of the core points, union-find init ----------------------------------
// ---- per-cell statistics of the core points: bounding box and smallest original row ----------
// Points-parallel (a dense tower cell holds thousands of points - one wave per cell would leave a
// long tail): a wave walks 1024 consecutive sorted points, 64 per round.  Inside a round the
// values are combined by a segmented scan over the lanes (the points are sorted by cell, so a
// cell is a run of lanes); a run that ends inside the round is folded into the cell's accumulator
// with atomics, the run that reaches lane 63 is carried into the next round.  Accumulators hold
// ordered uint32 keys folded with atomicMax (minima as the complement), so 0 = nothing yet.
constexpr int DB_CS_ROUNDS = 16;

__device__ __forceinline__ void db_cellstats_flush(uint32_t* __restrict__ acc, uint32_t c, const uint32_t (&v)[7]) {
#pragma unroll
    for (int k = 0; k < 7; ++k)
        if (v[k]) atomicMax(&acc[8 * (int64_t)c + k], v[k]);
}

__global__ __launch_bounds__(DB_THREADS) void db_cellstats_k(const float4* __restrict__ pts,
                                                             const uint32_t* __restrict__ cid,
                                                             const uint8_t* __restrict__ core_s, int64_t n,
                                                             uint32_t* __restrict__ acc,
                                                             uint32_t* __restrict__ bits, int64_t nw) {
    {   // the row bitmap db_mark_k sets bits in starts empty: n/32 words, and this grid has n/16 threads
        const int64_t t = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
        if (t < nw) bits[t] = 0u;
    }
    const int64_t base = ((int64_t)blockIdx.x * DB_WAVES + wave_id()) * (64 * DB_CS_ROUNDS);
    if (base >= n) return;
    const int l = lane_id();
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    uint32_t carry_c = NONE;                                   // cell of the run that reached lane 63 ...
    uint32_t carry[7] = {0, 0, 0, 0, 0, 0, 0};                 // ... its values so far (wave-uniform) ...
    uint32_t mine[7] = {0, 0, 0, 0, 0, 0, 0};                  // ... plus whole rounds of it, still per lane
    auto fold_mine = [&]() {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const uint32_t t = wave_reduce_max(mine[k]);
            carry[k] = t > carry[k] ? t : carry[k];
            mine[k] = 0;
        }
    };
    for (int r0 = 0; r0 < DB_CS_ROUNDS; r0 += 4) {
    if (base + r0 * 64 >= n) break;
    uint32_t c4[4], core4[4];
    float4 p4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {                              // four rounds of loads in flight
        const int64_t i = base + (r0 + u) * 64 + l;
        const bool in = i < n;
        c4[u] = in ? cid[i] : NONE - 1u;                       // past the end: a run of its own
        core4[u] = in ? core_s[i] : 0u;
        p4[u] = pts[in ? i : base];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = base + (r0 + u) * 64 + l;
        const bool in = i < n;
        const uint32_t c = c4[u];
        uint32_t v[7] = {0, 0, 0, 0, 0, 0, 0};
        if (core4[u]) {
            const float4 p = p4[u];
            const uint32_t kx = f32_ordered(p.x), ky = f32_ordered(p.y), kz = f32_ordered(p.z);
            v[0] = ~kx; v[1] = ~ky; v[2] = ~kz; v[3] = kx; v[4] = ky; v[5] = kz;
            v[6] = ~__float_as_uint(p.w);                      // original row (< 2^31)
        }
        if (__ballot(c != carry_c) == 0) {                     // the whole round belongs to the carried cell
#pragma unroll
            for (int k = 0; k < 7; ++k) mine[k] = v[k] > mine[k] ? v[k] : mine[k];
            continue;
        }
        if (carry_c != NONE) fold_mine();
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                     // segmented inclusive max-scan
            const uint32_t cu = __shfl_up(c, o, 64);
            const bool same = l >= o && cu == c;
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const uint32_t t = __shfl_up(v[k], o, 64);
                if (same) v[k] = t > v[k] ? t : v[k];
            }
        }
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)c, 0);
        if (carry_c != NONE) {
            if (carry_c == c0) {                               // the carried run continues: its end lane needs the carry
                if (c == c0) {
#pragma unroll
                    for (int k = 0; k < 7; ++k) v[k] = carry[k] > v[k] ? carry[k] : v[k];
                }
            } else if (l == 0) {
                db_cellstats_flush(acc, carry_c, carry);
            }
        }
        const uint32_t cn = __shfl_down(c, 1, 64);
        const bool run_end = l == 63 || cn != c;
        if (run_end && l != 63 && in) db_cellstats_flush(acc, c, v);
        carry_c = (uint32_t)__builtin_amdgcn_readlane((int)c, 63);
        if (carry_c == NONE - 1u) carry_c = NONE;              // lane 63 is past the end: nothing to carry
#pragma unroll
        for (int k = 0; k < 7; ++k) carry[k] = (uint32_t)__builtin_amdgcn_readlane((int)v[k], 63);
    }
    }
    if (carry_c != NONE) {
        fold_mine();
        if (l == 0) db_cellstats_flush(acc, carry_c, carry);
    }
}

// a cell's accumulators -> bounding box floats of its core points (none: +inf / -inf); returns their smallest row
// (none: INT_BIG)
__device__ __forceinline__ int db_cell_decode(const uint32_t* __restrict__ acc, int64_t c, float (&box)[6]) {
    uint32_t a[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) a[k] = acc[8 * c + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        box[k] = INFINITY;
        box[3 + k] = -INFINITY;
        if (a[k] != 0u) box[k] = f32_unordered(~a[k]);
        if (a[3 + k] != 0u) box[3 + k] = f32_unordered(a[3 + k]);
    }
    return a[6] != 0u ? (int)(~a[6]) : INT_BIG;
}

// the decoded accumulators of every cell; also resets the union-find forest (db_chunkunion_k does both for its chunk)
__global__ __launch_bounds__(DB_THREADS) void db_cellfin_k(const uint32_t* __restrict__ acc, int m,
                                                           float* __restrict__ cell_box,
                                                           int* __restrict__ cell_min,
                                                           int* __restrict__ parent,
                                                           int* __restrict__ comp_min) {
    const int c = blockIdx.x * DB_THREADS + threadIdx.x;
    if (c >= m) return;
    float box[6];
    const int mn = db_cell_decode(acc, c, box);
#pragma unroll
    for (int k = 0; k < 6; ++k) cell_box[6 * (int64_t)c + k] = box[k];
    cell_min[c] = mn;
    parent[c] = c;
    comp_min[c] = INT_BIG;
}

// ---- wave-wide test: do cells A and B hold a pair of core points within eps? -------------------
// A plain double loop finds a hit at once when most pairs are hits, but between two large cells
// that touch only at a corner it can scan all of B for thousands of A points before it reaches one
// that has a partner.  So first a few steps of alternating nearest-point descent (the point of A
// nearest to B's box, its nearest point in B, that one's nearest point in A, ...) - every
// candidate pair is checked with the exact predicate, so a hit is a proof; only if the descent
// stalls above eps does the exhaustive search run, the A side filtered 64 points at a time.
__device__ __forceinline__ float db_box_d2f(const float4& q, const float* __restrict__ box) {
    const float gx = fmaxf(fmaxf(box[0] - q.x, q.x - box[3]), 0.0f);
    const float gy = fmaxf(fmaxf(box[1] - q.y, q.y - box[4]), 0.0f);
    const float gz = fmaxf(fmaxf(box[2] - q.z, q.z - box[5]), 0.0f);
    return __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, gx * gx));
}
// index of the core point of [s, e) that minimises f (lane-parallel, four loads in flight); -1: none
template <typename F>
__device__ __forceinline__ int db_argmin(const float4* __restrict__ pts, const uint8_t* __restrict__ core_s,
                                         uint32_t s, uint32_t e, bool dense, F f) {
    const int l = lane_id();
    unsigned long long best = ~0ull;
    for (uint32_t i0 = s; i0 < e; i0 += 256) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = i0 + 64 * u + l;
            if (i < e && (dense || core_s[i])) {
                const float d = f(pts[i]);
                const unsigned long long k = ((unsigned long long)__float_as_uint(d) << 32) | i;   // d >= 0: bits order
                best = k < best ? k : best;
            }
        }
    }
    best = wave_reduce_min(best);
    return best == ~0ull ? -1 : (int)(uint32_t)best;
}

__device__ __forceinline__ bool db_cells_connected(const DbGrid& g, const float4* __restrict__ pts,
                                                   const uint8_t* __restrict__ core_s, uint32_t as, uint32_t ae,
                                                   bool a_dense, uint32_t bs, uint32_t be, bool b_dense,
                                                   const float* __restrict__ boxB, uint32_t a_from) {
    const int l = lane_id();
    if (ae - as > 64 || be - bs > 64) {                    // descent only pays between larger cells
        int ia = db_argmin(pts, core_s, as, ae, a_dense, [&](const float4& p) { return db_box_d2f(p, boxB); });
        if (ia < 0) return false;
        float4 q = pts[ia];
        for (int it = 0; it < 3; ++it) {
            const int jb = db_argmin(pts, core_s, bs, be, b_dense, [&](const float4& p) { return db_d2f(q, p); });
            if (jb < 0) return false;
            const float4 pb = pts[jb];
            if (db_within2(q, pb, g)) return true;
            const int ia2 = db_argmin(pts, core_s, as, ae, a_dense, [&](const float4& p) { return db_d2f(p, pb); });
            const float4 pa = pts[ia2];
            if (db_within2(pa, pb, g)) return true;
            if (ia2 == ia) break;                          // a local minimum above eps: decide exhaustively
            ia = ia2;
            q = pa;
        }
    }
    for (uint32_t a0 = a_from; a0 < ae; a0 += 64) {
        const uint32_t ia = a0 + l;
        float4 pa;
        pa.x = pa.y = pa.z = pa.w = 0.0f;
        bool near = false;
        if (ia < ae && (a_dense || core_s[ia])) {
            pa = pts[ia];
            near = !(db_box_d2(pa, boxB) > g.eps2);
        }
        unsigned long long todo = __ballot(near);
        while (todo) {
            const int src = (int)__builtin_ctzll(todo);
            todo &= todo - 1;
            float4 q;
            q.x = __shfl(pa.x, src, 64); q.y = __shfl(pa.y, src, 64); q.z = __shfl(pa.z, src, 64); q.w = 0.0f;
            for (uint32_t j0 = bs; j0 < be; j0 += 64) {
                const uint32_t j = j0 + l;
                bool hit = false;
                if (j < be && (b_dense || core_s[j])) hit = db_within2(q, pts[j], g);
                if (__ballot(hit)) return true;
            }
        }
    }
    return false;
}

// ---- union-find over cells: uf_load / uf_find / uf_union of pch_unionfind.h (hook larger root under smaller; lock free)

// face neighbour dir (0: +x, 1: +y, 2: +z) of the cell `key`: the key it has if it exists and, for +y / +z, the row
// that holds it ((dy,dz) = (1,0) / (0,1): rows 1 and 3 of DB_ROW_DY/DZ); +x is the next cell in sorted order
struct DbFace { int row; uint64_t want; };
__device__ __forceinline__ DbFace db_face(const DbGrid& g, uint64_t key, int dir) {
    return {dir == 1 ? 1 : 3, key + (dir == 0 ? 1ull : (dir == 1 ? (1ull << g.bx) : (1ull << (g.bx + g.by))))};
}
// may core cells A and B still need a link: core boxes within eps, and plain (possibly stale) parents differ - equal
// parents were in one set at some time, and sets only ever merge
__device__ __forceinline__ bool db_link_open(const DbGrid& g, const float* __restrict__ cell_box,
                                             const float* __restrict__ boxB, const int* parent, int A, int B) {
    return parent[A] != parent[B] && !(db_boxbox_d2(cell_box + 6 * (int64_t)A, boxB) > g.eps2);
}

// The per-cell words the union rounds read and their forest.  Either the global arrays, indexed by cell (db_union_pairs_k,
// db_union_face_k, db_union_k), or one chunk's copies in LDS, indexed from the chunk's first cell (db_chunkunion_k).
// cell_start holds rows of pts either way, so the bodies below are the same code on both.
struct DbForest {
    const uint32_t* cell_start; const uint32_t* cell_ncore; const float* cell_box; int* parent;
};

// may core cell A still need a link to cell B: B core, db_link_open, and the roots differ now
__device__ __forceinline__ bool db_link_live(const DbGrid& g, const DbForest& f, int A, int B) {
    bool live = f.cell_ncore[B] != 0 && db_link_open(g, f.cell_box, f.cell_box + 6 * (int64_t)B, f.parent, A, B);
    if (live) live = uf_find(f.parent, A) != uf_find(f.parent, B);
    return live;
}

// The general round for one core cell A, wave-wide; rs: its neighbour rows.  Phase 1 (64 candidate cells at a time,
// one per lane): neighbour core cells B > A whose core boxes are within eps and whose root differs from A's survive.
// Phase 2 (wave-wide per survivor): look for one core pair within eps (lanes over B's points,
// scalar loop over A's points, leave at the first hit), then unite.
// The face round has looked at the (up to 3) face-adjacent cells with a larger index before: for
// dense data they connect at the first tile and leave almost nothing but root comparisons here.
__device__ __forceinline__ void db_union_cell(const DbGrid& g, const float4* __restrict__ pts,
                                              const uint8_t* __restrict__ core_s, const DbForest& f, int A,
                                              const RowSet* rs, int* cd) {
    const int l = lane_id();
    int total;
    {
        // flatten the <= 25 runs of <= 5 cells into one candidate list (prefix over the run lengths)
        int len = 0;
        if (l < DB_ROWS) { len = rs->cb[l] - rs->ca[l]; len = len < 0 ? 0 : len; }
        const int incl = wave_scan_incl(len);
        total = __shfl(incl, 63, 64);
        if (l < DB_ROWS)
            for (int k = 0; k < len; ++k) cd[incl - len + k] = rs->ca[l] + k;
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t as = f.cell_start[A], ae = f.cell_start[A + 1];
    const bool a_dense = f.cell_ncore[A] == (ae - as);
    for (int base = 0; base < total; base += 64) {
        int B = -1;
        if (base + l < total) B = cd[base + l];
        const bool live = B > A && db_link_live(g, f, A, B);          // every unordered pair once
        unsigned long long todo = __ballot(live);
        while (todo) {
            const int src = (int)__builtin_ctzll(todo);
            todo &= todo - 1;
            const int Bs = __builtin_amdgcn_readlane(B, src);
            {                                              // united meanwhile through another cell?
                int same = 0;
                if (l == 0) same = uf_find(f.parent, A) == uf_find(f.parent, Bs);
                if (__builtin_amdgcn_readfirstlane(same)) continue;
            }
            const uint32_t bs = f.cell_start[Bs], be = f.cell_start[Bs + 1];
            const bool b_dense = f.cell_ncore[Bs] == (be - bs);
            const float* boxB = f.cell_box + 6 * (int64_t)Bs;
            const bool connected = db_cells_connected(g, pts, core_s, as, ae, a_dense, bs, be, b_dense, boxB, as);
            if (connected && l == 0) uf_union(f.parent, A, Bs);
        }
    }
}

// one wave per core cell A
__global__ __launch_bounds__(DB_THREADS) void db_union_k(DbGrid g, const float4* __restrict__ pts,
                                                         const uint32_t* __restrict__ cell_start,
                                                         const uint64_t* __restrict__ cell_key, int m,
                                                         const int2* __restrict__ rowtab,
                                                         const uint8_t* __restrict__ core_s,
                                                         const uint32_t* __restrict__ cell_ncore,
                                                         const float* __restrict__ cell_box,
                                                         int* __restrict__ parent) {
    __shared__ RowSet rows[DB_WAVES];
    __shared__ int cand[DB_WAVES][128];
    const int A = blockIdx.x * DB_WAVES + wave_id();
    if (A >= m) return;
    if (cell_ncore[A] == 0) return;
    RowSet* rs = &rows[wave_id()];
    db_rows(g, cell_key, cell_key[A], rs, rowtab, A);
    db_union_cell(g, pts, core_s, DbForest{cell_start, cell_ncore, cell_box, parent}, A, rs, cand[wave_id()]);
}

// ROUND 0, first half: one LANE per (cell, face direction).  A wave per cell walks one chain of dependent loads
// (neighbour lookup -> counts and boxes -> roots -> first points) per cell; on sparse data (millions of cells of
// a few dozen points) that chain, not arithmetic, is the whole cost.  Here 64 such chains are in flight per wave:
// the lane finds its neighbour, compares boxes and parents and tries the first DB_PAIR_TRIES core points of either
// cell against each other - adjacent cells almost always connect there - and unites on a hit.  Pairs it cannot
// decide are flagged in face_todo[cell]; only those cells are looked at by the wave-wide face round.
constexpr int DB_PAIR_TRIES = 3;

// one lane: core cell A (ncoreA core points) against its face neighbour B (-1: none).  true: undecided
__device__ __forceinline__ bool db_pair_lane(const DbGrid& g, const float4* __restrict__ pts,
                                             const uint8_t* __restrict__ core_s, const DbForest& f, int A,
                                             uint32_t ncoreA, int B) {
    if (B <= A) return false;
    const uint32_t nB = f.cell_ncore[B];
    if (nB == 0) return false;
    float boxB[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) boxB[a] = f.cell_box[6 * (int64_t)B + a];
    if (!db_link_open(g, f.cell_box, boxB, f.parent, A, B)) return false;
    const int rootA = uf_find(f.parent, A), rootB = uf_find(f.parent, B);
    if (rootA == rootB) return false;
    const uint32_t as = f.cell_start[A], ae = f.cell_start[A + 1];
    const uint32_t bs = f.cell_start[B], be = f.cell_start[B + 1];
    const bool a_dense = ncoreA == (ae - as), b_dense = nB == (be - bs);
    float4 pb[DB_PAIR_TRIES];
    int nb = 0;
    for (uint32_t j = bs; j < be && nb < DB_PAIR_TRIES; ++j) {
        if (!b_dense && !core_s[j]) continue;
        const float4 p = pts[j];
#pragma unroll
        for (int u = 0; u < DB_PAIR_TRIES; ++u)            // pb stays in registers: no slot indexed by a variable
            if (u == nb) pb[u] = p;
        ++nb;
    }
    bool connected = false;
    int na = 0;
    for (uint32_t i = as; i < ae && na < DB_PAIR_TRIES && !connected; ++i) {
        if (!a_dense && !core_s[i]) continue;
        ++na;
        const float4 pa = pts[i];
        if (db_box_d2(pa, boxB) > g.eps2) continue;
#pragma unroll
        for (int j = 0; j < DB_PAIR_TRIES; ++j)
            if (j < nb && db_within2(pa, pb[j], g)) connected = true;
    }
    if (connected) uf_union(f.parent, rootA, rootB);
    return !connected;
}
// the three face bits of a cell from its four lanes' `undecided` (lanes 4 k .. 4 k + 3 hold cell k's +x, +y, +z, idle)
__device__ __forceinline__ uint32_t db_pair_bits(bool undecided) {
    return (uint32_t)((__ballot(undecided) >> (lane_id() & ~3)) & 7ull);
}

__global__ __launch_bounds__(DB_THREADS) void db_union_pairs_k(DbGrid g, const float4* __restrict__ pts,
                                                               const uint32_t* __restrict__ cell_start,
                                                               const uint64_t* __restrict__ cell_key, int m,
                                                               const int2* __restrict__ rowtab,
                                                               const uint8_t* __restrict__ core_s,
                                                               const uint32_t* __restrict__ cell_ncore,
                                                               const float* __restrict__ cell_box,
                                                               int* __restrict__ parent,
                                                               uint8_t* __restrict__ face_todo) {
    const int64_t t = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    const int A = (int)(t >> 2), dir = (int)(t & 3);       // four lanes per cell: +x, +y, +z, idle
    const bool lane_on = A < m && dir < 3;
    bool undecided = false;
    if (lane_on) {
        const uint32_t ncoreA = cell_ncore[A];
        if (ncoreA != 0) {
            const DbFace f = db_face(g, cell_key[A], dir);
            int B = -1;
            if (dir == 0) {
                if (A + 1 < m && cell_key[A + 1] == f.want) B = A + 1;
            } else {
                const int2 run = rowtab[(int64_t)A * DB_ROWS + f.row];
                for (int k = run.x; k < run.y; ++k)
                    if (cell_key[k] == f.want) { B = k; break; }
            }
            undecided = db_pair_lane(g, pts, core_s, DbForest{cell_start, cell_ncore, cell_box, parent}, A, ncoreA, B);
        }
    }
    const uint32_t bits = db_pair_bits(undecided);
    if (A < m && dir == 0) face_todo[A] = (uint8_t)bits;
}

// ROUND 0, wave-wide: the (up to) three face neighbours with a larger key are examined side
// by side, 21 lanes each, so that the chain of dependent loads (neighbour lookup, roots, first
// points) is walked once per cell instead of once per neighbour.  Adjacent dense cells connect at
// the first point pair; a pair that is still undecided after DB_FACE_TRIES points of A is handed
// to the full-wave search of the general round.
constexpr int DB_FACE_TRIES = 8;

// lanes 21 k .. 21 k + 20 are group k (0: +x, 1: +y, 2: +z); lane 63: group 3, idle
struct DbFaceLane { int grp, gl; unsigned long long gmask; };
__device__ __forceinline__ DbFaceLane db_face_lane() {
    const int l = lane_id(), grp = l / 21;
    return {grp, l - 21 * grp, grp < 3 ? (0x1FFFFFull << (21 * grp)) : 0ull};
}

// one wave: core cell A (ncoreA core points) against B, its group's face neighbour (-1: none)
__device__ __forceinline__ void db_face_cell(const DbGrid& g, const float4* __restrict__ pts,
                                             const uint8_t* __restrict__ core_s, const DbForest& f, int A,
                                             uint32_t ncoreA, int B) {
    const int l = lane_id();
    const DbFaceLane fl = db_face_lane();
    const int grp = fl.grp, gl = fl.gl;
    const unsigned long long gmask = fl.gmask;
    const uint32_t as = f.cell_start[A], ae = f.cell_start[A + 1];
    const bool a_dense = ncoreA == (ae - as);
    const float4 pa0 = pts[as];                            // in flight with the neighbour look-ups below
    uint32_t bs = 0, be = 0;
    bool b_dense = false, pend = false;
    float boxB[6] = {0, 0, 0, 0, 0, 0};
    if (B > A) {
        const uint32_t nB = f.cell_ncore[B];
        bs = f.cell_start[B];
        be = f.cell_start[B + 1];
        b_dense = nB == (be - bs);
#pragma unroll
        for (int a = 0; a < 6; ++a) boxB[a] = f.cell_box[6 * (int64_t)B + a];
        pend = nB != 0 && db_link_open(g, f.cell_box, boxB, f.parent, A, B);
    }
    if (gl != 0) pend = false;                             // one lane per group looks the roots up
    int rootA = A, rootB = B;
    if (pend) {
        rootA = uf_find(f.parent, A);
        rootB = uf_find(f.parent, B);
        pend = rootA != rootB;
    }
    pend = __shfl((int)pend, grp < 3 ? 21 * grp : 0, 64) != 0 && grp < 3;
    bool connected = false;
    uint32_t ia = as;
    for (int tries = 0; ia < ae && tries < DB_FACE_TRIES; ++ia) {
        if (__ballot(pend) == 0) break;
        if (!a_dense && !core_s[ia]) continue;
        ++tries;
        const float4 pa = ia == as ? pa0 : pts[ia];
        bool near = pend && !(db_box_d2(pa, boxB) > g.eps2);
        const uint32_t maxlen = wave_reduce_max(near ? be - bs : 0u);
        for (uint32_t j0 = 0; j0 < maxlen; j0 += 21) {
            const uint32_t j = bs + j0 + gl;
            bool hit = false;
            if (near && j < be && (b_dense || core_s[j])) hit = db_within2(pa, pts[j], g);
            if (__ballot(hit) & gmask) { connected = true; pend = false; near = false; }
            if (__ballot(near) == 0) break;
        }
    }
    if (connected && gl == 0) uf_union(f.parent, rootA, rootB);    // starts from the roots found above
    // undecided pairs (rare): the full-wave search, one pair after the other
    unsigned long long todo = __ballot(pend && gl == 0);
    while (todo) {
        const int src = (int)__builtin_ctzll(todo);
        todo &= todo - 1;
        const int Bs = __shfl(B, src, 64);
        const uint32_t bs2 = f.cell_start[Bs], be2 = f.cell_start[Bs + 1];
        const bool b_dense2 = f.cell_ncore[Bs] == (be2 - bs2);
        const float* boxB2 = f.cell_box + 6 * (int64_t)Bs;
        const bool conn = db_cells_connected(g, pts, core_s, as, ae, a_dense, bs2, be2, b_dense2, boxB2, ia);
        if (conn && l == 0) uf_union(f.parent, A, Bs);
    }
}

__global__ __launch_bounds__(DB_THREADS) void db_union_face_k(DbGrid g, const float4* __restrict__ pts,
                                                              const uint32_t* __restrict__ cell_start,
                                                              const uint64_t* __restrict__ cell_key, int m,
                                                              const int2* __restrict__ rowtab,
                                                              const uint8_t* __restrict__ core_s,
                                                              const uint32_t* __restrict__ cell_ncore,
                                                              const float* __restrict__ cell_box,
                                                              int* __restrict__ parent,
                                                              const uint8_t* __restrict__ face_todo) {
    __shared__ RowSet rows[DB_WAVES];
    const int A = blockIdx.x * DB_WAVES + wave_id();
    if (A >= m) return;
    if (face_todo && face_todo[A] == 0) return;            // db_union_pairs_k has settled this cell's faces
    const uint32_t ncoreA = cell_ncore[A];
    if (ncoreA == 0) return;
    const DbFaceLane fl = db_face_lane();
    const int grp = fl.grp, gl = fl.gl;
    RowSet* rs = &rows[wave_id()];
    const uint64_t keyA = cell_key[A];
    db_rows(g, cell_key, keyA, rs, rowtab, A);
    int B = -1;
    {
        bool found = false;
        int k = -1;
        if (grp < 3) {
            const DbFace f = db_face(g, keyA, grp);
            if (grp == 0) {
                k = A + 1;
                found = gl == 0 && k < m && cell_key[k] == f.want;
            } else {
                k = rs->ca[f.row] + gl;
                found = k < rs->cb[f.row] && cell_key[k] == f.want;
            }
        }
        const unsigned long long fm = __ballot(found) & fl.gmask;
        if (fm) B = __shfl(k, (int)__builtin_ctzll(fm), 64);
    }
    db_face_cell(g, pts, core_s, DbForest{cell_start, cell_ncore, cell_box, parent}, A, ncoreA, B);
}

// path compression between the union rounds: afterwards parent[c] is the root of c
__global__ __launch_bounds__(DB_THREADS) void db_flatten_k(int* __restrict__ parent, int m) {
    const int c = blockIdx.x * DB_THREADS + threadIdx.x;
    if (c >= m) return;
    const int r = uf_find(parent, c);
    if (r != c) parent[c] = r;
}

// root of every core cell + smallest original row among the component's core points
__global__ __launch_bounds__(DB_THREADS) void db_compmin_k(const int* __restrict__ cell_min,
                                                           const uint32_t* __restrict__ cell_ncore, int m,
                                                           int* __restrict__ parent,
                                                           int* __restrict__ root,
                                                           int* __restrict__ comp_min) {
    const int c = blockIdx.x * DB_THREADS + threadIdx.x;
    if (c >= m) return;
    if (cell_ncore[c] == 0) { root[c] = -1; return; }
    const int r = uf_find(parent, c);
    root[c] = r;
    atomicMin(&comp_min[r], cell_min[c]);
}

__global__ __launch_bounds__(DB_THREADS) void db_mark_k(const int* __restrict__ root,
                                                        const int* __restrict__ comp_min, int m,
                                                        uint32_t* __restrict__ flag) {
    const int c = blockIdx.x * DB_THREADS + threadIdx.x;
    if (c >= m) return;
    if (root[c] == c) {                                    // one bit per original row: the smallest core row of a cluster
        const uint32_t r = (uint32_t)comp_min[c];
        atomicOr(&flag[r >> 5], 1u << (r & 31u));
    }
}

// ---- the staged route: all of the above for one chunk, in LDS ------------------------------------
// Neighbours share the chunk, so a chunk's cells [chunk_cells[c], chunk_cells[c + 1]) are a union-find problem of
// their own, and where the cell table came from the staged lists a chunk holds at most CT_CELLS of them: one
// workgroup per chunk keeps the cell keys, first rows, core counts, core boxes, smallest core rows and the forest in
// LDS, indexed from the chunk's first cell, and runs db_cellfin_k, the face round (db_pair_lane, db_face_cell), the
// flattening, the general round (db_union_cell), db_compmin_k and db_mark_k on them.  A uf_find hop, a neighbour
// look-up (binary search over the chunk's keys: no row table) and the whole candidate filter then cost LDS
// latency; global loads are left for the point pairs that prove a link.  Workgroups never wait for one another,
// and inside one the forest stays lock free (CAS retry only); every barrier below is reached by all threads.
// The results are the words the seven kernels leave: whether two cells link does not depend on the order of the
// tests, and the larger root hooks under the smaller, so a component's root is its smallest cell.
constexpr int CU_THREADS = 1024;
constexpr int CU_WAVES   = CU_THREADS / 64;
static_assert(CU_THREADS == CT_CELLS, "a thread per cell of the chunk");

// local index of the cell with key `want` among the chunk's nc sorted keys; -1: no such cell
__device__ __forceinline__ int cu_cell(const uint32_t* key, int nc, uint32_t want) {
    const int k = db_lower(key, nc, want);
    return k < nc && key[k] == want ? k : -1;
}
// face neighbour dir of local cell A (db_face; the grid's edge has none)
__device__ __forceinline__ int cu_face(const DbGrid& g, const uint32_t* key, int nc, int A, int dir) {
    const uint32_t k = key[A];
    const DbFace f = db_face(g, k, dir);
    if (dir == 0) return A + 1 < nc && key[A + 1] == (uint32_t)f.want ? A + 1 : -1;
    const int at = dir == 1 ? (int)((k >> g.bx) & ((1u << g.by) - 1)) : (int)((k >> (g.bx + g.by)) & ((1u << g.bz) - 1));
    return at < (dir == 1 ? g.my : g.mz) ? cu_cell(key, nc, (uint32_t)f.want) : -1;
}
// db_row_run on the chunk's keys: local range of neighbour row `row` of the cell with key k
__device__ __forceinline__ int2 cu_row_run(const DbGrid& g, const uint32_t* key, int nc, uint32_t k, int row) {
    int2 v;
    v.x = 0; v.y = 0;
    DbRowAt at;
    if (db_row_at(g, k, row, at))
        v = db_run_in(key, nc, (uint32_t)db_pack(g, 0, (uint64_t)at.nz, (uint64_t)at.ny, (uint64_t)at.xlo),
                      (uint32_t)db_pack(g, 0, (uint64_t)at.nz, (uint64_t)at.ny, (uint64_t)at.xhi));
    return v;
}

__global__ __launch_bounds__(CU_THREADS) void db_chunkunion_k(DbGrid g, const float4* __restrict__ pts,
                                                              const uint32_t* __restrict__ cell_start,
                                                              const uint64_t* __restrict__ cell_key, int m,
                                                              const uint8_t* __restrict__ core_s,
                                                              const uint32_t* __restrict__ cell_ncore,
                                                              const float* __restrict__ cell_box,
                                                              const int* __restrict__ cell_min,
                                                              int* __restrict__ root,
                                                              int* __restrict__ comp_min,
                                                              uint32_t* __restrict__ flag, int64_t n) {
    __shared__ uint32_t key[CT_CELLS], start[CT_CELLS + 1], ncore[CT_CELLS];
    __shared__ uint32_t todo[CT_CELLS];                    // face bits of the face round, then row bits of the general one
    __shared__ float box[6 * CT_CELLS];
    __shared__ int cmin[CT_CELLS], parent[CT_CELLS];
    __shared__ RowSet rows[CU_WAVES];
    __shared__ int cand[CU_WAVES][128];
    const int tid = threadIdx.x, l = lane_id();
    // a chunk_cells that is not what db_chunkcells_k writes must neither leave LDS nor the table
    int first = (int)g.chunk_cells[blockIdx.x], nc = (int)g.chunk_cells[blockIdx.x + 1] - first;
    first = first < 0 ? 0 : (first > m ? m : first);
    nc = nc < 0 ? 0 : (nc > CT_CELLS ? CT_CELLS : nc);
    nc = nc > m - first ? m - first : nc;
    const DbForest f = {start, ncore, box, parent};

    // db_cellfin_k: the cell's words, its summary as db_celltab_k and db_core_k left it
    if (tid < nc) {
        const int64_t c = first + tid;
        const int sh = g.bx + g.by + g.bz;                 // <= 31 on this route
        key[tid] = (uint32_t)cell_key[c] & ((1u << sh) - 1u);
        start[tid] = cell_start[c];
        if (tid == nc - 1) start[nc] = cell_start[c + 1];
        ncore[tid] = cell_ncore[c];
        cmin[tid] = cell_min[c];
#pragma unroll
        for (int k = 0; k < 6; ++k) box[6 * tid + k] = cell_box[6 * c + k];
        parent[tid] = tid;
    }
    __syncthreads();

    // db_union_pairs_k: four lanes per cell
    for (int t0 = 0; t0 < 4 * nc; t0 += CU_THREADS) {
        const int A = (t0 + tid) >> 2, dir = tid & 3;
        bool undecided = false;
        if (A < nc && dir < 3) {
            const uint32_t ncoreA = ncore[A];
            if (ncoreA != 0) undecided = db_pair_lane(g, pts, core_s, f, A, ncoreA, cu_face(g, key, nc, A, dir));
        }
        const uint32_t bits = db_pair_bits(undecided);
        if (A < nc && dir == 0) todo[A] = bits;
    }
    __syncthreads();

    // db_union_face_k: a wave per cell that has a face left
    for (int A = wave_id(); A < nc; A += CU_WAVES) {
        const uint32_t ncoreA = ncore[A];
        if (todo[A] == 0 || ncoreA == 0) continue;
        const int grp = db_face_lane().grp;
        db_face_cell(g, pts, core_s, f, A, ncoreA, grp < 3 ? cu_face(g, key, nc, A, grp) : -1);
    }
    __syncthreads();

    // db_flatten_k
    if (tid < nc) {
        const int r = uf_find(parent, tid);
        if (r != tid) parent[tid] = r;
        todo[tid] = 0u;
    }
    __syncthreads();

    // db_union_k, its filter first: a lane per (cell, neighbour row) notes the rows that hold a live candidate.  Every
    // pair is taken from its smaller cell, and the cells are sorted by (z, y, x): only the row of the cell itself and
    // the 12 rows with dz > 0 or dz == 0 < dy - the odd ones of DB_ROW_DY/DZ - hold a larger cell
    for (int t0 = 0; t0 < 16 * nc; t0 += CU_THREADS) {
        const int A = (t0 + tid) >> 4, u = tid & 15, row = u == 0 ? 0 : 2 * u - 1;
        if (A < nc && u < 13 && ncore[A] != 0) {
            const int2 run = cu_row_run(g, key, nc, key[A], row);
            const int pA = parent[A];
            uint32_t open = 0u;                            // what the parents alone leave of the (up to) five, side by side
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int B = run.x + i;
                if (B < run.y && B > A && parent[B] != pA) open |= 1u << i;
            }
            bool live = false;
            while (open != 0u && !live) {
                const int i = __builtin_ctz(open);
                open &= open - 1u;
                live = db_link_live(g, f, A, run.x + i);
            }
            if (live) atomicOr(&todo[A], 1u << row);
        }
    }
    __syncthreads();
    // ... then a wave per cell with such rows, on those rows
    for (int A = wave_id(); A < nc; A += CU_WAVES) {
        const uint32_t live_rows = todo[A];
        if (live_rows == 0) continue;
        RowSet* rs = &rows[wave_id()];
        if (l < DB_ROWS) {
            int2 v;
            v.x = 0; v.y = 0;
            if ((live_rows >> l) & 1u) v = cu_row_run(g, key, nc, key[A], l);
            rs->ca[l] = v.x;
            rs->cb[l] = v.y;
        }
        __builtin_amdgcn_wave_barrier();
        db_union_cell(g, pts, core_s, f, A, rs, cand[wave_id()]);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();

    // db_compmin_k and db_mark_k: every core cell's root, the component's smallest core row on it, its bit
    int r = -1;
    if (tid < nc && ncore[tid] != 0) {
        r = uf_find(parent, tid);
        if (r != tid) atomicMin(&cmin[r], cmin[tid]);      // only roots are written, only other cells write
    }
    __syncthreads();
    if (tid < nc) {
        const int64_t c = first + tid;
        root[c] = r < 0 ? -1 : first + r;
        comp_min[c] = r == tid ? cmin[tid] : INT_BIG;
        if (r == tid) {
            const uint32_t row = (uint32_t)cmin[tid];  // a core cell's smallest core row: below n
            if ((int64_t)row < n) atomicOr(&flag[row >> 5], 1u << (row & 31u));
        }
    }
}

// Per-cluster bounding boxes, accumulated where the labels are made (the grouping stage then needs no pass of its
// own over the points): acc[8 k + a], a = 0..2: max of ~ordered(x|y|z) (the minimum), a = 3..5: max of ordered(.)
// - folded with atomicMax so that a zeroed table is the neutral start.
constexpr int DB_LAB_ROUNDS = 8;                       // 64-point rounds per wave in db_label_k
constexpr int DB_LAB_TILE   = DB_THREADS * DB_LAB_ROUNDS;

__device__ __forceinline__ void db_box_flush(uint32_t* __restrict__ acc, int cur, uint32_t (&m)[6]) {
    const int l = lane_id();
    uint32_t v = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const uint32_t t = wave_reduce_max(m[a]);
        if (l == a) v = t;
        m[a] = 0u;
    }
    if (cur >= 0 && l < 6 && v) atomicMax(&acc[8 * (int64_t)cur + l], v);
}
// one row per lane joins the box of its cluster `mine` (-1: none).  The wave carries the per-lane running box m[] of
// ONE cluster, `cur` (wave-uniform), and hands it over whenever a lane brings another
__device__ __forceinline__ void db_box_round(uint32_t* __restrict__ acc, int& cur, uint32_t (&m)[6], int mine, float x,
                                             float y, float z) {
    const uint32_t k[3] = {f32_ordered(x), f32_ordered(y), f32_ordered(z)};
    unsigned long long todo = __ballot(mine >= 0);
    while (todo) {
        const int L = __builtin_amdgcn_readlane(mine, (int)__builtin_ctzll(todo));
        const bool in = mine == L;
        todo &= ~__ballot(in);
        if (L != cur) {                                    // another cluster: hand the carried box over
            db_box_flush(acc, cur, m);
            cur = L;
        }
        if (in) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                m[a] = ~k[a] > m[a] ? ~k[a] : m[a];
                m[3 + a] = k[a] > m[3 + a] ? k[a] : m[3 + a];
            }
        }
    }
}

// labels of core points (original order), label of every cell, optional core mask.
// A wave walks DB_LAB_ROUNDS consecutive groups of 64 sorted points.  The points are sorted by cell, so a wave
// mostly sees ONE cluster: it keeps a per-lane running box while the label stays the same and pays the wave
// reduction + six atomics only when the label changes (one flush per 64 points cost more than the separate pass
// over the points it replaced: ~10^6 atomics on a few hundred lines).
// Block -> sorted range: with many chunks (bpc > 0) the blocks of one chunk share blockIdx % 8, i.e. one XCD and
// one L2 (MI355X deals blocks round-robin over its 8 XCDs; a speed assumption only): the 4-byte label stores of a
// chunk scatter over that chunk's own 200 KB window of `labels`, and lines written from several XCDs would leave
// every L2 as partial lines (measured: 94.6 -> 68.8 us).
__global__ __launch_bounds__(DB_THREADS) void db_label_k(const float4* __restrict__ pts,
                                                         const uint32_t* __restrict__ cid,
                                                         const uint8_t* __restrict__ core_s,
                                                         const int* __restrict__ root,
                                                         const int* __restrict__ comp_min,
                                                         const uint32_t* __restrict__ bits,
                                                         const uint32_t* __restrict__ rank, int64_t n,
                                                         const uint32_t* __restrict__ cell_start,
                                                         int* __restrict__ cell_label,
                                                         int32_t* __restrict__ labels,
                                                         uint8_t* __restrict__ core_out, int64_t chunk_size, int bpc,
                                                         int64_t nchunks, uint32_t* __restrict__ box_acc,
                                                         int32_t box_cap) {
    int64_t lo, hi;                                        // this wave's sorted range [lo, hi)
    {
        const int64_t woff = (int64_t)wave_id() * (64 * DB_LAB_ROUNDS);
        if (bpc > 0) {
            const int64_t slot = blockIdx.x >> 3;
            const int64_t c = (slot / bpc) * 8 + (blockIdx.x & 7);
            const int64_t within = (slot % bpc) * DB_LAB_TILE + woff;
            lo = c * chunk_size + within;
            hi = (c < nchunks && within < chunk_size) ? (c + 1) * chunk_size : lo;
        } else {
            lo = (int64_t)blockIdx.x * DB_LAB_TILE + woff;
            hi = n;
        }
        if (hi > n) hi = n;
        if (hi > lo + 64 * DB_LAB_ROUNDS) hi = lo + 64 * DB_LAB_ROUNDS;
    }
    if (lo >= hi) return;                                  // wave-uniform
    const int l = lane_id();
    // the gather chain cid -> root -> comp_min -> (rank, bits) is four dependent loads deep: all rounds of the wave
    // go through it level by level, eight loads in flight per lane and level
    constexpr int R = DB_LAB_ROUNDS;
    bool valid[R], is_core[R];
    uint32_t c[R], cs[R], row[R], rk[R], bw[R];
    int rt[R], lab[R];
    float4 p[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int64_t i = lo + u * 64 + l;
        valid[u] = i < hi;
        c[u] = valid[u] ? cid[i] : 0u;
        p[u] = pts[valid[u] ? i : lo];
        is_core[u] = valid[u] && core_s[i] != 0;
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
        rt[u] = valid[u] ? root[c[u]] : -1;
        cs[u] = valid[u] ? cell_start[c[u]] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < R; ++u) row[u] = rt[u] >= 0 ? (uint32_t)comp_min[rt[u]] : 0u;
#pragma unroll
    for (int u = 0; u < R; ++u) {
        rk[u] = rt[u] >= 0 ? rank[row[u] >> 5] : 0u;
        bw[u] = rt[u] >= 0 ? bits[row[u] >> 5] : 0u;
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int64_t i = lo + u * 64 + l;
        // clusters are numbered by their smallest core row
        lab[u] = rt[u] >= 0 ? (int)(rk[u] + (uint32_t)__popc(bw[u] & ((1u << (row[u] & 31u)) - 1u))) : INT_BIG;
        if (valid[u]) {
            const uint32_t o = __float_as_uint(p[u].w);
            labels[o] = is_core[u] ? lab[u] : -1;
            if (core_out) core_out[o] = is_core[u] ? 1 : 0;
            if (cs[u] == (uint32_t)i) cell_label[c[u]] = lab[u];
        }
    }
    if (!box_acc) return;
    int cur = -1;                                          // label of the box carried in m[] (wave-uniform)
    uint32_t m[6] = {0u, 0u, 0u, 0u, 0u, 0u};              // per-lane running box of `cur`
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int mine = (is_core[u] && lab[u] != INT_BIG && lab[u] >= 0 && lab[u] < box_cap) ? lab[u] : -1;
        db_box_round(box_acc, cur, m, mine, p[u].x, p[u].y, p[u].z);
    }
    db_box_flush(box_acc, cur, m);
}

// ---- the staged route's labels (DbCells::chunk_union): every row has ONE owner.  The rows of a dense cell (every row
// core, so every row carries the cell's label) belong to db_filelabel_k, which never looks at the sorted rows: a row's
// cell is a function of its coordinates, a chunk holds at most CT_CELLS cells, so a workgroup takes a tile of
// consecutive INPUT rows of one chunk, keeps that chunk's cell keys and the labels of its dense cells in LDS and
// finds every row's cell there - 12 bytes read and 4 (+1) written per row, both coalesced, no cid column, no
// scattered store.  The rows of every other cell - a few per cent - belong to db_border_k<true>, which visits those
// cells anyway.  The cells' labels, which db_label_k leaves as a side effect, are made per cell in front of both, in
// db_prelabel_k's launch.
__global__ void db_prelabel_cells_k(const uint32_t* __restrict__ total, int32_t* __restrict__ out_nclusters,
                                    uint32_t* __restrict__ box_acc, int64_t box_words,
                                    const int* __restrict__ root, const int* __restrict__ comp_min,
                                    const uint32_t* __restrict__ bits, const uint32_t* __restrict__ rank, int m,
                                    int* __restrict__ cell_label) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out_nclusters = (int32_t)*total;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (box_acc && i < box_words) box_acc[i] = 0u;
    if (i >= m) return;
    const int rt = root[i];
    int lab = INT_BIG;                                     // no core point: the cell attracts nothing
    if (rt >= 0) {                                         // db_label_k's chain: the cluster's smallest core row, ranked
        const uint32_t row = (uint32_t)comp_min[rt];
        lab = (int)(rank[row >> 5] + (uint32_t)__popc(bits[row >> 5] & ((1u << (row & 31u)) - 1u)));
    }
    cell_label[i] = lab;
}

constexpr int DB_FL_NONE = -0x7fffffff - 1;                // db_filelabel_k: not a dense cell, the row is db_border_k's
constexpr int FL_SLOTS = 2 * CT_CELLS;                     // ... its table of the chunk's cells, never more than half full
__device__ __forceinline__ uint32_t fl_hash(uint32_t k) { return (k * 0x9E3779B1u) >> 21; }
static_assert(FL_SLOTS == 1 << 11, "fl_hash yields 11 bits");

__global__ __launch_bounds__(DB_THREADS) void db_filelabel_k(const float* __restrict__ xyz, int64_t n, DbGrid g,
                                                             const uint32_t* __restrict__ cell_start,
                                                             const uint64_t* __restrict__ cell_key, int m,
                                                             const uint32_t* __restrict__ cell_ncore,
                                                             const int* __restrict__ cell_label,
                                                             int32_t* __restrict__ labels,
                                                             uint8_t* __restrict__ core_out, int bpc, int64_t nchunks,
                                                             uint32_t* __restrict__ box_acc, int32_t box_cap) {
    __shared__ uint2 tab[FL_SLOTS];                        // open addressing: (the cell's key in its chunk, a dense cell's
                                                           // label or DB_FL_NONE for any other cell)
    const int tid = threadIdx.x;
    // the blocks of one chunk share blockIdx % 8, as db_label_k's do
    const int64_t slot = blockIdx.x >> 3;
    const int64_t c = (slot / bpc) * 8 + (blockIdx.x & 7);
    const int64_t within = (slot % bpc) * DB_LAB_TILE;
    if (c >= nchunks || within >= g.chunk_size) return;    // workgroup-uniform, as every return in front of the barrier
    const int64_t t0 = c * g.chunk_size + within;
    int64_t t1 = (c + 1) * g.chunk_size < n ? (c + 1) * g.chunk_size : n;
    if (t1 > t0 + DB_LAB_TILE) t1 = t0 + DB_LAB_TILE;
    if (t0 >= t1) return;
    // the tile's rows are on their way while the chunk's table is put together
    constexpr int R = DB_LAB_ROUNDS;
    const Row3* __restrict__ rows = reinterpret_cast<const Row3*>(xyz);
    Row3 q[R];
    uint32_t k[R];
    int lab[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int64_t i = t0 + u * DB_THREADS + tid;
        q[u] = rows[i < t1 ? i : t0];
    }
    if (g.chunk_bad[c]) {                                  // a NaN/inf chunk is noise as a whole
        for (int64_t i = t0 + tid; i < t1; i += DB_THREADS) {
            labels[i] = -1;
            if (core_out) core_out[i] = 0;
        }
        return;
    }
    // a chunk_cells that is not what db_chunkcells_k writes must neither leave LDS nor the table (db_chunkunion_k)
    int first = (int)g.chunk_cells[c], nc = (int)g.chunk_cells[c + 1] - first;
    first = first < 0 ? 0 : (first > m ? m : first);
    nc = nc < 0 ? 0 : (nc > CT_CELLS ? CT_CELLS : nc);
    nc = nc > m - first ? m - first : nc;
    const int sh = g.bx + g.by + g.bz;                     // <= 31 on this route
    for (int j = tid; j < FL_SLOTS; j += DB_THREADS) tab[j].x = CT_EMPTY;
    __syncthreads();
    for (int j = tid; j < nc; j += DB_THREADS) {           // keys are distinct and nc <= FL_SLOTS / 2: a free slot is found
        const int64_t A = first + j;
        const uint32_t key = (uint32_t)cell_key[A] & ((1u << sh) - 1u);
        const int label = cell_ncore[A] == cell_start[A + 1] - cell_start[A] ? cell_label[A] : DB_FL_NONE;
        uint32_t h = fl_hash(key);
        for (int p = 0; p < FL_SLOTS; ++p, h = (h + 1u) & (FL_SLOTS - 1))
            if (atomicCAS(&tab[h].x, CT_EMPTY, key) == CT_EMPTY) { tab[h].y = (uint32_t)label; break; }
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
        bool ok;
        k[u] = cs_cell_key(g, q[u].x, q[u].y, q[u].z, ok);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int64_t i = t0 + u * DB_THREADS + tid;
        lab[u] = DB_FL_NONE;                               // (a key the table does not hold: nobody's row, not written)
        if (i < t1) {
            uint32_t h = fl_hash(k[u]);
            for (int p = 0; p < FL_SLOTS; ++p, h = (h + 1u) & (FL_SLOTS - 1)) {
                const uint2 e = tab[h];
                if (e.x == k[u]) { lab[u] = (int)e.y; break; }
                if (e.x == CT_EMPTY) break;
            }
        }
        if (lab[u] != DB_FL_NONE) {
            labels[i] = lab[u];
            if (core_out) core_out[i] = 1;
        }
    }
    if (!box_acc) return;
    // In file order the clusters of a chunk take turns from row to row, so a box carried from round to round
    // (db_box_round) would be handed over at every turn: all rounds' labels are known here, so the wave makes one pass
    // over its rounds per cluster its rows hold, and one hand-over each
    unsigned long long todo[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
        if (!(lab[u] != DB_FL_NONE && lab[u] != INT_BIG && lab[u] >= 0 && lab[u] < box_cap)) lab[u] = -1;
        todo[u] = __ballot(lab[u] >= 0);
    }
    for (;;) {
        int L = -1;                                        // wave-uniform: the next cluster
#pragma unroll
        for (int u = 0; u < R; ++u)
            if (L < 0 && todo[u]) L = __builtin_amdgcn_readlane(lab[u], (int)__builtin_ctzll(todo[u]));
        if (L < 0) break;
        uint32_t mm[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const bool in = lab[u] == L;
            todo[u] &= ~__ballot(in);
            if (in) {
                const uint32_t kk[3] = {f32_ordered(q[u].x), f32_ordered(q[u].y), f32_ordered(q[u].z)};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    mm[a] = ~kk[a] > mm[a] ? ~kk[a] : mm[a];
                    mm[3 + a] = kk[a] > mm[3 + a] ? kk[a] : mm[3 + a];
                }
            }
        }
        db_box_flush(box_acc, L, mm);
    }
}

// border points: smallest cluster id among the core points within eps.
// OWN (the staged route's labels, see db_filelabel_k): nobody has written the rows of a cell that is not dense, so the
// wave writes every one of them, once - a core row's label (the cell's) and the core flags in front of the early
// exits, a row that is not core either -1 where the cell has no core cell around or what the border rule says - and
// folds the cell's core box, which db_core_k left exact for such a cell, into its cluster's box.  A NaN/inf chunk's
// rows are db_filelabel_k's.
template <bool OWN>
__global__ __launch_bounds__(DB_THREADS) void db_border_k(DbGrid g, const float4* __restrict__ pts,
                                                          const uint32_t* __restrict__ cell_start,
                                                          const uint64_t* __restrict__ cell_key, int m,
                                                          const int2* __restrict__ rowtab,
                                                          const uint8_t* __restrict__ core_s,
                                                          const uint32_t* __restrict__ cell_ncore,
                                                          const float* __restrict__ cell_box,
                                                          const int* __restrict__ cell_label,
                                                          int32_t* __restrict__ labels,
                                                          uint32_t* __restrict__ box_acc, int32_t box_cap,
                                                          uint8_t* __restrict__ core_out) {
    __shared__ RowSet rows[DB_WAVES];
    const int A = blockIdx.x * DB_WAVES + wave_id();
    if (A >= m) return;
    const uint32_t as = cell_start[A], ae = cell_start[A + 1];
    const uint32_t ncoreA = cell_ncore[A];
    if (ncoreA == (ae - as)) return;                       // no border candidates here
    const int l = lane_id();
    if constexpr (OWN) {
        const int sh = g.bx + g.by + g.bz;
        if (g.chunk_bad[sh < 64 ? (cell_key[A] >> sh) : 0]) return;
        const int labA = cell_label[A];
        for (uint32_t q = as + l; q < ae; q += 64) {
            const bool is_core = core_s[q] != 0;
            const uint32_t o = __float_as_uint(pts[q].w);
            if (is_core) labels[o] = labA;
            if (core_out) core_out[o] = is_core ? 1 : 0;
        }
        if (box_acc && ncoreA != 0 && labA != INT_BIG && labA >= 0 && labA < box_cap && l < 6) {
            const uint32_t k = f32_ordered(cell_box[6 * (int64_t)A + l]);
            atomicMax(&box_acc[8 * (int64_t)labA + l], l < 3 ? ~k : k);
        }
    }
    RowSet* rs = &rows[wave_id()];
    db_rows(g, cell_key, cell_key[A], rs, rowtab, A);
    // quick reject: no core cell anywhere around
    if (!db_any_core(rs, cell_ncore)) {
        if constexpr (OWN)                                 // (ncoreA is 0 here: the cell is in its own neighbourhood)
            for (uint32_t q = as + l; q < ae; q += 64)
                if (!core_s[q]) labels[__float_as_uint(pts[q].w)] = -1;
        return;
    }
    DbCoreCells cc;
    db_gather_core_cells(cc, rs, true, cell_start, cell_ncore, cell_box, cell_label);
    for (uint32_t q = as; q < ae; ++q) {
        if (core_s[q]) continue;
        const float4 qp = pts[q];
        const int best = db_border_label(g, qp, cc, pts, cell_start, core_s);
        if (l == 0 && (OWN || best != INT_BIG)) labels[__float_as_uint(qp.w)] = best != INT_BIG ? best : -1;
        if (box_acc && best != INT_BIG && best >= 0 && best < box_cap && l < 6) {     // a border point joins its box
            const float v = l % 3 == 0 ? qp.x : (l % 3 == 1 ? qp.y : qp.z);
            const uint32_t k = f32_ordered(v);
            atomicMax(&box_acc[8 * (int64_t)best + l], l < 3 ? ~k : k);
        }
    }
}

// publishes the cluster count and zeroes the box accumulators (neutral start of db_box_fold)
__global__ void db_prelabel_k(const uint32_t* __restrict__ total, int32_t* __restrict__ out_nclusters,
                              uint32_t* __restrict__ box_acc, int64_t box_words) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out_nclusters = (int32_t)*total;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (box_acc && i < box_words) box_acc[i] = 0u;
}

void db_plan(Arena& a, int64_t n, DbWs& w) {
    const int64_t nn = n > 0 ? n : 1;
    w.meta = a.take<DbMeta>(1);                          // DbWs::clear_from runs across these three: nothing may be
    w.scan1_b = a.take<uint32_t>(scan1_ws_u32(nn / 32 + 1));   // carved between them
    w.chunk_cells = a.take<uint32_t>(nn + 8);
    assert(!w.chunk_cells || ((void*)(w.meta + 1) == w.scan1_b && (char*)w.chunk_cells - (char*)w.scan1_b ==
                              (ptrdiff_t)((scan1_ws_u32(nn / 32 + 1) * sizeof(uint32_t) + 255) & ~size_t(255))));
    w.core_stats = a.take<unsigned long long>(4);
    w.chunk_bad = a.take<uint32_t>(nn + 8);              // one word per chunk (chunk_size >= 1)
    w.chunk_ovf = a.take<uint32_t>(nn + 8);              // (written for every chunk by db_cellscatter_k)
    w.k0 = a.take<uint64_t>(nn);
    w.k1 = a.take<uint64_t>(nn);
    w.v0 = a.take<uint32_t>(nn);
    w.v1 = a.take<uint32_t>(nn);
    w.head = a.take<uint32_t>(nn + 8);
    w.cid = a.take<uint32_t>(nn);
    w.pts = a.take<float4>(nn);
    w.xbuf = a.take<float4>(nn);                        // spare rows array of the chunk-local sort
    w.core_s = a.take<uint8_t>(nn);
    w.cell_key = a.take<uint64_t>(nn);
    w.cell_start = a.take<uint32_t>(nn + 8);
    w.cell_ncore = a.take<uint32_t>(nn);
    w.cell_box = a.take<float>(6 * nn);
    w.cell_acc = a.take<uint32_t>(8 * nn);
    w.cell_min = a.take<int>(nn);
    w.parent = a.take<int>(nn);
    w.root = a.take<int>(nn);
    w.comp_min = a.take<int>(nn);
    w.cell_label = a.take<int>(nn);
    w.bits = a.take<uint32_t>(nn / 16 + 256);             // row bitmap (n/32 words) + its scanned word counts (wrank)
    w.radix_ws = a.take<uint32_t>(radix_ws_u32(nn));
    w.scan_ws = a.take<uint32_t>(scan_ws_u32(nn));
    // neighbour-row table (200 B per cell) for up to max(n/4, 64Ki) cells; beyond that the rows are
    // searched on the fly
    w.rowtab_cells = nn / 4 > 65536 ? nn / 4 : (nn < 65536 ? nn : 65536);
    w.rowtab = a.take<int2>((size_t)w.rowtab_cells * DB_ROWS);
    w.comp = a.take<uint32_t>(3 * nn);
    w.flag2 = a.take<uint32_t>(nn + 8);
    w.wrank = w.bits ? w.bits + ((ceil_div(nn, 32) + 63) & ~int64_t(63)) : nullptr;
    w.face_todo = reinterpret_cast<uint8_t*>(w.root);
    w.stage = {w.v1, w.k0, w.v0, w.head};
    w.cell_route = w.meta ? &w.meta->pad[0] : nullptr;
#ifdef PCH_CS_STAMPS
    w.cs_stamps = reinterpret_cast<unsigned long long*>(w.cell_box);
#endif
}

// Stage C's tuning switches, read here only, once per process.  PCH_DBSCAN_SORT=chunk|global: the cell sort (0
// automatic, 1 chunk-local, 2 global), which pch_dbscan_set_sort_mode() overrides for the whole process.
// Pair counting (pch_dbscan_set_pair_counting) is set per thread.
struct DbTuning { int sort_mode; bool count_pairs; };
static int g_sort_mode = -1;
static thread_local bool g_count_pairs = false;
static DbTuning db_tuning() {
    int m = __atomic_load_n(&g_sort_mode, __ATOMIC_RELAXED);
    if (m < 0) {
        const char* e = getenv("PCH_DBSCAN_SORT");
        m = (e && strcmp(e, "chunk") == 0) ? 1 : (e && strcmp(e, "global") == 0) ? 2 : 0;
        __atomic_store_n(&g_sort_mode, m, __ATOMIC_RELAXED);
    }
    return {m, g_count_pairs};
}

// the retained fit of this thread: one per thread, dropped by ws_touched
thread_local DbLastRun g_last = {nullptr, 0, 0, {}, 0, false, 0.0, 0};

void ws_touched(const void* base, size_t bytes) {
    if (!g_last.ws) return;
    const char* a0 = static_cast<const char*>(base);
    const char* b0 = static_cast<const char*>(g_last.ws);
    if (a0 < b0 + g_last.ws_bytes && b0 < a0 + bytes) g_last.ws = nullptr;
}

// The entry points that continue the grid the last pch_dbscan_f32 of this thread left in `ws` carve it up again
// here; `entry` names the caller in the error
int db_continue(const char* entry, int64_t n, void* ws, size_t ws_bytes, DbWs& w) {
    if (g_last.ws != ws || g_last.ws_bytes != ws_bytes || g_last.n != n || ws == nullptr) {
        set_error("%s must follow pch_dbscan_f32 of this thread on the same, untouched workspace", entry);
        return PCH_ERR_ARG;
    }
    Arena a(ws, ws_bytes, true);
    db_plan(a, g_last.plan_n, w);            // as the run carved it (the fused call: for nf_cap rows)
    return PCH_OK;
}

// host mirror of f32_unordered
static float host_unordered(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// ---- the steps of dbscan_run, in the order it runs them
int db_all_noise(const DbRun& r) {
    PCH_HIP_TRY(hipMemsetAsync(r.labels, 0xFF, sizeof(int32_t) * (size_t)r.n, r.s));
    if (r.core) PCH_HIP_TRY(hipMemsetAsync(r.core, 0, (size_t)r.n, r.s));
    PCH_HIP_TRY(hipMemsetAsync(r.out_nclusters, 0, sizeof(int32_t), r.s));
    return PCH_OK;
}

// bounding box: the caller's host copy, or measured over the finite rows.  done: not one finite row, the outputs
// are written
static int db_bounds(const DbRun& r, const float* aabb_host, float (&box)[6], bool& done) {
    if (aabb_host) {
        memcpy(box, aabb_host, sizeof(box));
    } else {
        uint32_t* key = r.w.meta->box_key;
        PCH_HIP_TRY(hipMemsetAsync(key, 0xFF, 3 * sizeof(uint32_t), r.s));
        PCH_HIP_TRY(hipMemsetAsync(key + 3, 0, 3 * sizeof(uint32_t), r.s));
        PCH_LAUNCH("db_aabb_in", db_aabb_in_k, dim3(db_stride_blocks(r.n)), dim3(DB_THREADS), 0, r.s, r.xyz, r.n, key);
        DbMeta back;
        PCH_HIP_TRY(hipMemcpyAsync(back.box_key, key, sizeof(back.box_key), hipMemcpyDeviceToHost, r.s));
        PCH_HIP_TRY(hipStreamSynchronize(r.s));
        if (back.box_key[0] == 0xFFFFFFFFu) {              // not a single finite point: every chunk fails
            done = true;
            return db_all_noise(r);
        }
        for (int k = 0; k < 6; ++k) box[k] = host_unordered(back.box_key[k]);
    }
    if (!db_box_finite(box)) {
        set_error("bounding box is not finite");
        return PCH_ERR_ARG;
    }
    return PCH_OK;
}

// largest cell coordinate per axis -> g.mx..mz and the key bits per axis; returns the bits of a cell
int db_cell_bits(DbGrid& g, int mx, int my, int mz) {
    g.mx = mx; g.my = my; g.mz = mz;
    g.bx = bits_for((uint64_t)mx + 1); g.by = bits_for((uint64_t)my + 1); g.bz = bits_for((uint64_t)mz + 1);
    return g.bx + g.by + g.bz;
}

// the part of the grid that eps, min_samples and the workspace give: everything but the origin, mx..mz and bx..bz
static DbGrid db_grid_proto(const DbWs& w, int64_t chunk_size, double eps, int32_t min_samples) {
    DbGrid g;
    memset(&g, 0, sizeof(g));
    g.cell = eps / 1.7320508075688772 * (1.0 - 1.0 / 65536.0);
    g.inv_cell = 1.0 / g.cell;
    const DbBand band = db_band(eps);
    g.eps2 = band.r2; g.eps2_lo = band.lo; g.eps2_hi = band.hi;
    g.chunk_size = chunk_size;
    g.chunk_bad = w.chunk_bad;
    g.chunk_cells = w.chunk_cells;
    g.min_samples = min_samples;
    return g;
}

// the grid of cells of side eps/sqrt(3) over the box, and the bits of its key: a cell (cellbits), then the chunk
// (nbits in all).  Returns true when that key does not fit 64 bits.
static bool db_grid(const DbRun& r, const float (&box)[6], double eps, int32_t min_samples, DbGrid& g, int& cellbits,
                    int& nbits) {
    g = db_grid_proto(r.w, r.chunk_size, eps, min_samples);
    return db_plan_grid(box, r.nchunks, g, cellbits, nbits);
}

// key beyond 64 bits, several chunks: every chunk on its own, with its own bounding box (the reference fits them one
// by one anyway)
static int db_run_chunks(const DbRun& r, double eps, int32_t min_samples, void* ws, size_t ws_bytes, int32_t* k_host) {
    int32_t offset = 0;
    for (int64_t c = 0; c < r.nchunks; ++c) {
        const int64_t lo = c * r.chunk_size, cn = (r.n - lo) < r.chunk_size ? (r.n - lo) : r.chunk_size;
        int32_t kc = 0;
        PCH_TRY(dbscan_run(r.xyz + 3 * lo, cn, eps, min_samples, 0, nullptr, r.labels + lo,
                           r.core ? r.core + lo : nullptr, r.out_nclusters, ws, ws_bytes, r.s, &kc, nullptr, nullptr));
        if (kc > 0 && offset > 0)
            PCH_LAUNCH("db_add_offset", db_add_offset_k, dim3((unsigned)ceil_div(cn, DB_THREADS)), dim3(DB_THREADS), 0,
                       r.s, r.labels + lo, cn, offset);
        offset += kc;                    // utils/tower_extraction.py:114-116
    }
    PCH_HIP_TRY(hipMemcpyAsync(r.out_nclusters, &offset, sizeof(int32_t), hipMemcpyHostToDevice, r.s));
    PCH_HIP_TRY(hipStreamSynchronize(r.s));
    if (k_host) *k_host = offset;
    g_last.ws = nullptr;                 // no single grid is left to relabel on
    return PCH_OK;
}

// the cells of the sorted keys (db_cell_table), their row table, the core flags and the per-cell statistics; c: the
// cell table
static int db_cells_core(const DbRun& r, const DbGrid& g, int cellbits, const uint64_t* ks, bool staged,
                         bool count_pairs, DbCells& c, const DbHead* head) {
    const DbWs& w = r.w; const hipStream_t s = r.s; const int64_t n = r.n;
    DbMeta back;                             // status, ncells ... the route word
    PCH_TRY(db_cell_table(r, g, cellbits, ks, staged, back, head));
    const int m = (int)back.ncells;
    const unsigned gc = (unsigned)ceil_div(m, DB_WAVES);
    c = {g, w.pts, w.cell_start, w.cell_key, m, m <= w.rowtab_cells ? w.rowtab : nullptr, w.core_s, w.cell_ncore,
         w.cell_box, staged && back.pad[0] == 0u};
    if (c.rowtab && !c.chunk_union)                      // (the staged route: db_celltab_k wrote the rows)
        PCH_LAUNCH("db_rowtab", db_rowtab_k, dim3((unsigned)ceil_div(m, 2 * DB_WAVES)), dim3(DB_THREADS), 0, s, g,
                   w.cell_key, m, w.rowtab);
    // the staged route: db_core_k writes every cell's summary (db_celltab_k staged cell_min and cleared w.bits); any
    // other route sweeps the rows for it
    float* const sum_box = c.chunk_union ? w.cell_box : nullptr;
    int* const sum_min = c.chunk_union ? w.cell_min : nullptr;
    if (count_pairs) {
        PCH_HIP_TRY(hipMemsetAsync(w.core_stats, 0, 4 * sizeof(unsigned long long), s));
        PCH_LAUNCH("db_core_counting", db_core_k<true>, dim3(gc), dim3(DB_THREADS), 0, s, DB_GRID_ARGS(c), w.core_s,
                   w.cell_ncore, sum_box, sum_min, w.core_stats);
    } else {
        PCH_LAUNCH("db_core", db_core_k<false>, dim3(gc), dim3(DB_THREADS), 0, s, DB_GRID_ARGS(c), w.core_s,
                   w.cell_ncore, sum_box, sum_min, nullptr);
    }
    if (!c.chunk_union) {
        PCH_LAUNCH("db_cellstats", db_cellstats_k, dim3((unsigned)ceil_div(n, (int64_t)DB_WAVES * 64 * DB_CS_ROUNDS)),
                   dim3(DB_THREADS), 0, s, w.pts, w.cid, w.core_s, n, w.cell_acc, w.bits, ceil_div(n, 32));
        PCH_LAUNCH("db_cellfin", db_cellfin_k, dim3((unsigned)ceil_div(m, DB_THREADS)), dim3(DB_THREADS), 0, s,
                   w.cell_acc, m, w.cell_box, w.cell_min, w.parent, w.comp_min);
    }
    return PCH_OK;
}

// clusters of the core cells: union-find over their links, each component's smallest core row
static int db_union(const DbRun& r, const DbCells& c) {
    const DbWs& w = r.w; const hipStream_t s = r.s; const int m = c.m;
    const unsigned gc = (unsigned)ceil_div(m, DB_WAVES);
    if (c.chunk_union) {                                 // every chunk on its own, in LDS; parent stays unused
        PCH_LAUNCH("db_chunkunion", db_chunkunion_k, dim3((unsigned)r.nchunks), dim3(CU_THREADS), 0, s, c.g, c.pts,
                   c.cell_start, c.cell_key, m, c.core_s, c.cell_ncore, c.cell_box, w.cell_min, w.root, w.comp_min,
                   w.bits, r.n);
        return PCH_OK;
    }
    // face neighbours: lane-per-pair first (needs the row table), the wave-wide search for what that left open
    if (c.rowtab)
        PCH_LAUNCH("db_union_pairs", db_union_pairs_k, dim3((unsigned)ceil_div(4 * (int64_t)m, DB_THREADS)),
                   dim3(DB_THREADS), 0, s, DB_CELL_ARGS(c), w.parent, w.face_todo);
    PCH_LAUNCH("db_union0", db_union_face_k, dim3(gc), dim3(DB_THREADS), 0, s, DB_CELL_ARGS(c), w.parent,
               c.rowtab ? (const uint8_t*)w.face_todo : nullptr);
    PCH_LAUNCH("db_flatten", db_flatten_k, dim3((unsigned)ceil_div(m, DB_THREADS)), dim3(DB_THREADS), 0, s,
               w.parent, m);
    PCH_LAUNCH("db_union1", db_union_k, dim3(gc), dim3(DB_THREADS), 0, s, DB_CELL_ARGS(c), w.parent);
    PCH_LAUNCH("db_compmin", db_compmin_k, dim3((unsigned)ceil_div(m, DB_THREADS)), dim3(DB_THREADS), 0, s,
               w.cell_min, w.cell_ncore, m, w.parent, w.root, w.comp_min);
    return PCH_OK;
}

// the labels of core and border rows (and, with `boxes`, the cluster boxes folded in); k_host: the cluster count
static int db_labels(const DbRun& r, const DbCells& c, int32_t* k_host, DbBoxOut* boxes) {
    const DbWs& w = r.w; const hipStream_t s = r.s; const int64_t n = r.n, nchunks = r.nchunks; const int m = c.m;
    // cluster id = rank of the cluster's smallest core row: a bitmap over the rows + a scan of its
    // word counts (n/32 elements instead of n)
    const int64_t nw = ceil_div(n, 32);
    static_assert(DB_CS_ROUNDS * 64 * DB_WAVES / DB_THREADS <= 32, "db_cellstats_k's grid has a thread per bitmap word");
    if (!c.chunk_union)
        PCH_LAUNCH("db_mark", db_mark_k, dim3((unsigned)ceil_div(m, DB_THREADS)), dim3(DB_THREADS), 0, s,
                   w.root, w.comp_min, m, w.bits);
    // word ranks: popcount on load
    if (scan1_pays(nw)) PCH_TRY(scan1_exclusive_popc_u32(w.bits, w.wrank, nw, w.scan1_b, &w.meta->nclusters, s));
    else PCH_TRY(scan_exclusive_popc_u32(w.bits, w.wrank, nw, w.scan_ws, &w.meta->nclusters, s));
    uint32_t* box_acc = (boxes && boxes->acc && boxes->cap > 0) ? boxes->acc : nullptr;
    const int32_t box_cap = box_acc ? boxes->cap : 0;
    const int64_t box_words = box_acc ? 8 * (int64_t)box_cap : 0;
    if (c.chunk_union) {                                 // ... and every cell's label, which both owners of the rows read
        PCH_LAUNCH("db_prelabel", db_prelabel_cells_k, dim3((unsigned)std::max<int64_t>(ceil_div(std::max<int64_t>(
                   box_words, m), 256), 1)), dim3(256), 0, s, &w.meta->nclusters, r.out_nclusters, box_acc, box_words,
                   w.root, w.comp_min, w.bits, w.wrank, m, w.cell_label);
    } else {
        PCH_LAUNCH("db_prelabel", db_prelabel_k, dim3((unsigned)std::max<int64_t>(ceil_div(box_words, 256), 1)),
                   dim3(256), 0, s, &w.meta->nclusters, r.out_nclusters, box_acc, box_words);
    }
    if (k_host) PCH_TRY(peek_enqueue(r.out_nclusters, sizeof(int32_t), s));    // read while the labels are written
    // many chunks: the blocks of one chunk share an XCD (see db_label_k); otherwise blocks in sorted order
    const int bpc = (nchunks >= 16 || c.chunk_union) ? (int)ceil_div(r.chunk_size, DB_LAB_TILE) : 0;
    const unsigned gl = bpc > 0 ? (unsigned)(8 * ceil_div(nchunks, 8) * bpc) : (unsigned)ceil_div(n, DB_LAB_TILE);
    if (c.chunk_union) {                                 // one owner per row: dense cells in file order, the rest per cell
        PCH_LAUNCH("db_label", db_filelabel_k, dim3(gl), dim3(DB_THREADS), 0, s, r.xyz, n, c.g, c.cell_start, c.cell_key,
                   m, c.cell_ncore, w.cell_label, r.labels, r.core, bpc, nchunks, box_acc, box_cap);
        PCH_LAUNCH("db_border", db_border_k<true>, dim3((unsigned)ceil_div(m, DB_WAVES)), dim3(DB_THREADS), 0, s,
                   DB_CELL_ARGS(c), w.cell_label, r.labels, box_acc, box_cap, r.core);
    } else {
        PCH_LAUNCH("db_label", db_label_k, dim3(gl), dim3(DB_THREADS), 0, s, w.pts, w.cid, w.core_s, w.root, w.comp_min,
                   w.bits, w.wrank, n, w.cell_start, w.cell_label, r.labels, r.core, r.chunk_size, bpc, nchunks, box_acc,
                   box_cap);
        PCH_LAUNCH("db_border", db_border_k<false>, dim3((unsigned)ceil_div(m, DB_WAVES)), dim3(DB_THREADS), 0, s,
                   DB_CELL_ARGS(c), w.cell_label, r.labels, box_acc, box_cap, nullptr);
    }
    if (box_acc) boxes->done = true;
    if (k_host) {
        PCH_TRY(peek_wait(k_host, sizeof(int32_t)));
        if (*k_host < 0) {                              // the rank scan's bounded wait gave up: the count reads -1
            set_error("stage C: a device-side look-back wait ran out of its budget; outputs are undefined");
            return PCH_ERR_TIMEOUT;
        }
    }
    return PCH_OK;
}

int db_border_again(const DbCells& c, const int* cell_label, int32_t* labels, hipStream_t s) {
    PCH_LAUNCH("db_border", db_border_k<false>, dim3((unsigned)ceil_div(c.m, DB_WAVES)), dim3(DB_THREADS), 0, s,
               DB_CELL_ARGS(c), cell_label, labels, nullptr, 0, nullptr);
    return PCH_OK;
}

}  // namespace pch

using namespace pch;

extern "C" int pch_first_nonfinite_row_f32(const float* xyz, int64_t n, int64_t* out_row, void* stream) {
    PCH_DEVICE_GUARD(out_row);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n >= 0 && out_row && (n == 0 || xyz), "bad argument");
    PCH_HIP_TRY(hipMemsetAsync(out_row, 0xFF, sizeof(int64_t), s));             // -1: every row finite
    if (n == 0) return PCH_OK;
    return db_first_bad(xyz, n, reinterpret_cast<unsigned long long*>(out_row), s);
}

extern "C" void pch_dbscan_set_sort_mode(int mode) {
    __atomic_store_n(&g_sort_mode, (mode == 1 || mode == 2) ? mode : 0, __ATOMIC_RELAXED);
}

extern "C" size_t pch_dbscan_ws_bytes(int64_t n) {
    if (n < 0) return 0;
    Arena a;
    DbWs w;
    db_plan(a, n, w);
    return a.off;
}

int pch::dbscan_run(const float* xyz, int64_t n, double eps, int32_t min_samples, int64_t chunk_size,
                    const float* aabb_host, int32_t* labels, uint8_t* core, int32_t* out_nclusters, void* ws,
                    size_t ws_bytes, hipStream_t s, int32_t* k_host, DbBoxOut* boxes, DbHeadRun* head) {
    if (k_host) *k_host = 0;
    if (head) head->route = 0;
    const int64_t plan_n = head ? head->plan_n : n;
    if (boxes) boxes->done = false;
    PCH_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "n out of range [0, 2^31)");
    PCH_REQUIRE(eps > 0.0, "eps must be > 0 (sklearn: InvalidParameterError)");
    PCH_REQUIRE(min_samples >= 1, "min_samples must be >= 1 (sklearn: InvalidParameterError)");
    PCH_REQUIRE(out_nclusters != nullptr, "out_nclusters is null");
    if (n == 0) {
        PCH_HIP_TRY(hipMemsetAsync(out_nclusters, 0, sizeof(int32_t), s));
        return PCH_OK;
    }
    PCH_REQUIRE(xyz && labels && ws, "null buffer");
    PCH_REQUIRE(plan_n >= n, "more rows than the workspace was planned for");
    Arena a(ws, ws_bytes);
    DbWs w;
    db_plan(a, plan_n, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    if (chunk_size <= 0 || chunk_size > n) chunk_size = n;
    const DbRun r = {xyz, n, chunk_size, ceil_div(n, chunk_size), plan_n, labels, core, out_nclusters, s, w};
    const DbTuning tune = db_tuning();

    float box[6];
    bool done = false;
    PCH_TRY(db_bounds(r, aabb_host, box, done));
    if (done) return PCH_OK;
    DbGrid g;
    int cellbits, nbits;
    const bool overflow = db_grid(r, box, eps, min_samples, g, cellbits, nbits);
    if (overflow) {
        // extent/eps beyond the 64-bit cell key (outliers, heavy tails).  Several chunks: every chunk on its own.
        // One chunk: compressed coordinates.
        if (r.nchunks > 1) return db_run_chunks(r, eps, min_samples, ws, ws_bytes, k_host);
        PCH_TRY(db_compress(r, g, cellbits, done));
        if (done) return PCH_OK;
        nbits = cellbits;
    }
    const uint64_t* ks;
    DbCells c;
    bool staged;
    // the fused call queued the head of this stage unread, up to db_celltab_k: go on behind it if the device planned
    // what was planned here - the same rows, chunks, origin (bit for bit), cell ranges and key bits.  Anything else:
    // from the top, with this plan (the head's launches wrote nothing that the run does not write again)
    const DbHead* const dh = head ? head->host : nullptr;
    const bool unread = dh && dh->go == 1u && !overflow && dh->n == n && dh->nchunks == r.nchunks &&
                        dh->g.chunk_size == r.chunk_size && memcmp(&dh->g.ox, &g.ox, 3 * sizeof(float)) == 0 &&
                        dh->g.mx == g.mx && dh->g.my == g.my && dh->g.mz == g.mz && dh->g.bx == g.bx &&
                        dh->g.by == g.by && dh->g.bz == g.bz && dh->cellbits == cellbits && dh->nbits == nbits;
    if (unread) {
        ks = w.k1;
        staged = true;
        head->route = 1;
    } else {
        PCH_TRY(db_sorted_keys(r, g, cellbits, nbits, overflow, tune.sort_mode, ks, staged));
    }
    PCH_TRY(db_cells_core(r, g, cellbits, ks, staged, tune.count_pairs, c, unread ? dh : nullptr));
    PCH_TRY(db_union(r, c));
    PCH_TRY(db_labels(r, c, k_host, boxes));
    g_last = {ws, ws_bytes, n, c, r.nchunks, overflow, eps, plan_n};
    return PCH_OK;
}

// The fused call, behind stage B's first results (a.scalars / count / aabb on the device): queue the head of the stage
// unread if the arguments allow the staged chunk route at all.  *queued says whether it was; dbscan_run then takes
// the host copy of *head in its DbHeadRun.  The workspace is carved as dbscan_run will carve it for a.plan_n rows.
int pch::dbscan_head(const float* xyz, DbHeadArgs a, double eps, int32_t min_samples, void* ws, size_t ws_bytes,
                     DbHead* head, const void* peek_dev, size_t peek_bytes, hipStream_t s, bool* queued) {
    *queued = false;
    a.sort_mode = db_tuning().sort_mode;
    const int64_t cap_chunks = (a.chunk_size <= 0 || a.chunk_size > a.plan_n) ? 1 : ceil_div(a.plan_n, a.chunk_size);
    if (!(eps > 0.0) || min_samples < 1 || !xyz || a.plan_n < 1 || a.plan_n >= (int64_t(1) << 31) ||
        a.sort_mode == 2 || cap_chunks > DB_TABLE_MAX_CHUNKS || (a.sort_mode != 1 && cap_chunks < CS_MIN_CHUNKS))
        return PCH_OK;                       // dbscan_run says what is wrong, or takes another route anyway
    Arena ar(ws, ws_bytes);
    DbWs w;
    db_plan(ar, a.plan_n, w);
    if (ar.overflow) return PCH_OK;
    a.clear_from = static_cast<uint32_t*>(w.clear_from());
    a.chunk_cells = w.chunk_cells;
    PCH_TRY(db_head_launch(xyz, a, db_grid_proto(w, a.chunk_size, eps, min_samples), w, head, peek_dev, peek_bytes, s));
    *queued = true;
    return PCH_OK;
}

extern "C" void pch_dbscan_set_pair_counting(int enable) { g_count_pairs = enable != 0; }

extern "C" int pch_dbscan_f32(const float* xyz, int64_t n, double eps, int32_t min_samples,
                              int64_t chunk_size, const float* aabb_host, int32_t* labels,
                              uint8_t* core, int32_t* out_nclusters, void* ws, size_t ws_bytes,
                              void* stream) {
    PCH_DEVICE_GUARD(xyz ? (const void*)xyz : (const void*)out_nclusters);
    return dbscan_run(xyz, n, eps, min_samples, chunk_size, aabb_host, labels, core, out_nclusters, ws, ws_bytes,
                      (hipStream_t)stream, nullptr);
}
