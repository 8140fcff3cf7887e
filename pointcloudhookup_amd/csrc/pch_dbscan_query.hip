// Stage C, continuations of a retained fit: the calls that carve the workspace of this thread's last pch_dbscan_f32
// up again (db_continue) and go on with its cell table - relabel, first core rows, pair statistics, strip pairs, and
// the four that hold new points against the fit: assign, k-th neighbour distances, neighbourhood moments and the k
// nearest rows.
#include "pch_dbscan.h"

namespace pch {

// ---- points that were NOT part of the fit, held against it (pch_dbscan_assign_f32): db_border_k's rule - smallest
// cluster id among the fit's core points within eps, else -1 - for query points the caller brings.  The queries are
// binned into the fit's own cells, sorted by cell and cut into pieces; one wave per piece walks the 5x5x5 block around
// the piece's cell with the functions db_border_k walks it with around a cell of the fit (db_gather_core_cells,
// db_border_label).
struct DbQuery {
    const float* xyz; int64_t nq;    // [nq][3] query rows
    float sx, sy, sz;                // q = fl32(row - s) per component (0: x - 0.0f is x, bit for bit, -0.0 and NaN too)
    const int32_t* chunk;            // [nq] chunk whose fit a query is held against; null: chunk 0
    int64_t nchunks;
};
constexpr uint32_t DQ_OUT   = 0x80000000u;   // in a query's value word (nq < 2^31): the answer is -1 whatever its cell holds
#ifndef PCH_DQ_PIECE
#define PCH_DQ_PIECE 64                      // tuning builds: make EXTRA=-DPCH_DQ_PIECE=256 (DESIGN.md section 5 has the figures)
#endif
constexpr int      DQ_PIECE = PCH_DQ_PIECE;  // queries a wave takes at most: one crowded cell does not serialise the launch

__device__ __forceinline__ float4 dq_point(const DbQuery& Q, int64_t i) {
    float4 q;
    q.x = Q.xyz[3 * i + 0] - Q.sx; q.y = Q.xyz[3 * i + 1] - Q.sy; q.z = Q.xyz[3 * i + 2] - Q.sz; q.w = 0.0f;
    return q;
}

// Query keys: [chunk | cz | cy | cx] in the fit's bit widths, the cell by db_cell_coords' expression.  Every point of
// the fit lies in a cell of [0, m] per axis, and a point within eps of the query lies at most two cells from the
// query's cell t (eps < 2 cell sides).  So a query with t < -2 or t > m + 2 on some axis has nobody in reach: -1 at
// once.  Any other t is clamped to c = min(max(t, 0), m), and that is exact: a valid cell v with |v - t| <= 2 has
// |v - c| <= 2 as well (c lies between t and v, or is t), so the block around c holds every cell the block around t
// would have offered, and the distance test decides as before.  The comparison and the clamp run in double: a
// coordinate of 1e30 has no integer cell.  NaN fails every comparison, inf the upper one.
__global__ __launch_bounds__(DB_THREADS) void dq_keys_k(DbQuery Q, DbGrid g, uint64_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= Q.nq) return;
    const float4 q = dq_point(Q, i);
    const int64_t c = Q.chunk ? (int64_t)Q.chunk[i] : 0;
    bool ok = c >= 0 && c < Q.nchunks;
    if (ok) ok = g.chunk_bad[c] == 0u;                     // a NaN/inf chunk has no fit
    const double fx = floor(((double)q.x - (double)g.ox) * g.inv_cell);
    const double fy = floor(((double)q.y - (double)g.oy) * g.inv_cell);
    const double fz = floor(((double)q.z - (double)g.oz) * g.inv_cell);
    const double mx = (double)g.mx, my = (double)g.my, mz = (double)g.mz;
    ok = ok && fx >= -2.0 && fx <= mx + 2.0 && fy >= -2.0 && fy <= my + 2.0 && fz >= -2.0 && fz <= mz + 2.0;
    uint64_t key = 0;
    if (ok)
        key = db_pack(g, (uint64_t)c, (uint64_t)fmin(fmax(fz, 0.0), mz), (uint64_t)fmin(fmax(fy, 0.0), my),
                      (uint64_t)fmin(fmax(fx, 0.0), mx));
    keys[i] = key;
    vals[i] = (uint32_t)i | (ok ? 0u : DQ_OUT);
}

// Pieces of the sorted queries: a piece starts where the key changes and at every multiple of PIECE, so it lies
// inside one cell and holds at most PIECE queries (dq_assign_k: DQ_PIECE = 64, one query per lane; measured against 256
// and 1024.  dq_kdist_k: DK_PIECE, dq_shape_k: DS_PIECE).  dq_heads_k writes the start flags (scanned in place),
// dq_pieces_k the first query of every piece and, behind the last one, nq.
template <int PIECE>
__device__ __forceinline__ bool dq_head(const uint64_t* __restrict__ keys, int64_t i) {
    return i % PIECE == 0 || keys[i] != keys[i - 1];
}
template <int PIECE>
__global__ __launch_bounds__(DB_THREADS) void dq_heads_k(const uint64_t* __restrict__ keys, int64_t nq,
                                                         uint32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i < nq) flag[i] = dq_head<PIECE>(keys, i) ? 1u : 0u;
}
template <int PIECE>
__global__ __launch_bounds__(DB_THREADS) void dq_pieces_k(const uint64_t* __restrict__ keys, int64_t nq,
                                                          const uint32_t* __restrict__ excl,
                                                          uint32_t* __restrict__ piece_start) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= nq) return;
    const bool h = dq_head<PIECE>(keys, i);
    if (h) piece_start[excl[i]] = (uint32_t)i;
    if (i == nq - 1) piece_start[excl[i] + (h ? 1u : 0u)] = (uint32_t)nq;
}

// One wave per piece (the grid is sized on the host from nq alone, so the waves stride over the piece count the
// device holds).  Rows of the piece's cell with db_row_run - not the row table: the query's cell need not exist in the
// fit -, the core cells of those rows one per lane (db_gather_core_cells), then query after query through
// db_border_label.  The queries are loaded 64 at a time, one per lane, and handed round; every lane stores the answer of
// its own query.
__global__ __launch_bounds__(DB_THREADS) void dq_assign_k(DbQuery Q, DbGrid g, const float4* __restrict__ pts,
                                                          const uint32_t* __restrict__ cell_start,
                                                          const uint64_t* __restrict__ cell_key,
                                                          const uint8_t* __restrict__ core_s,
                                                          const uint32_t* __restrict__ cell_ncore,
                                                          const float* __restrict__ cell_box,
                                                          const int* __restrict__ cell_label,
                                                          const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ vals,
                                                          const uint32_t* __restrict__ piece_start,
                                                          const uint32_t* __restrict__ npieces,
                                                          int32_t* __restrict__ out) {
    __shared__ RowSet rows[DB_WAVES];
    const int l = lane_id();
    RowSet* rs = &rows[wave_id()];
    const uint32_t np = *npieces;
    for (uint32_t p = blockIdx.x * DB_WAVES + wave_id(); p < np; p += gridDim.x * DB_WAVES) {   // wave-uniform
        const uint32_t ps = piece_start[p], pe = piece_start[p + 1];
        const uint64_t key = keys[ps];
        __builtin_amdgcn_wave_barrier();                   // the piece before this one has read its rows
        db_rows(g, cell_key, key, rs, nullptr, 0);
        const bool none = !db_any_core(rs, cell_ncore);    // no core cell in reach: the whole piece is -1
        DbCoreCells cc;
        db_gather_core_cells(cc, rs, !none, cell_start, cell_ncore, cell_box, cell_label);
        for (uint32_t q0 = ps; q0 < pe; q0 += 64) {
            const bool have = q0 + l < pe;
            const uint32_t v = have ? vals[q0 + l] : DQ_OUT;
            float4 mine;
            mine.x = mine.y = mine.z = mine.w = 0.0f;
            if (have && !none && !(v & DQ_OUT)) mine = dq_point(Q, (int64_t)v);
            int res = -1;
            const int cnt = (int)(pe - q0 < 64u ? pe - q0 : 64u);
            for (int j = 0; j < cnt && !none; ++j) {
                if ((uint32_t)__builtin_amdgcn_readlane((int)v, j) & DQ_OUT) continue;          // wave-uniform
                float4 qp;
                qp.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.x), j));
                qp.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.y), j));
                qp.z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.z), j));
                qp.w = 0.0f;
                const int best = db_border_label(g, qp, cc, pts, cell_start, core_s);
                if (l == j && best != INT_BIG) res = best;
            }
            if (have) out[v & ~DQ_OUT] = res;
        }
    }
}

// ---- the k-th neighbour distance of every query among the rows of the fit (pch_dbscan_kdist_f32): the k-distance
// plot that sets eps.  Queries are binned, sorted and cut into pieces as for dq_assign_k (of DK_PIECE queries), one
// wave per piece.  The 25 neighbour rows of the piece's cell are 25 runs of consecutive rows of the sorted copy,
// [cell_start[ca], cell_start[cb]); the wave numbers their rows 0 .. T-1 across the runs (seg_off: first number of a
// run, seg_a: its first row), so a sweep keeps 64 lanes busy whatever the runs' lengths.  Per query:
//   * one sweep forms d2 of every candidate in float64 (db_d2, db_within's sum); the float32 value of db_within2 only
//     skips candidates that are surely outside (d32 >= eps2_hi).  Those with d2 <= eps2 are counted, the first DK_CAP
//     bit patterns are kept in LDS, and the histogram of their top byte is taken;
//   * an exact MSB-first radix select on the 64-bit pattern of d2 (non-negative doubles order as unsigned integers; d2
//     is a sum of squares, never -0.0), a byte per pass: the wave scans the 256 bins, four per lane, picks the bin that
//     holds rank k, and tallies the next byte of the keys that share the prefix so far - from the LDS copy when all
//     in-range keys fitted, else by sweeping the candidates again (the neighbourhood of a tower core: thousands).
// Nothing here leaves the wave: no global atomics, no waiting on another workgroup.
constexpr int DK_CAP = 1024;                 // in-range keys a wave keeps in LDS (8 KiB of the workgroup's 37 KiB)
constexpr int DK_PIECE = 8;                  // queries per piece: a query costs up to eight sweeps of its neighbourhood, so
                                             // short pieces, many waves (DESIGN.md section 5a has the figures)
constexpr int DK_AHEAD = 4;                  // 64-candidate groups whose loads are in flight together (as DB_AHEAD)
struct DkRuns { uint32_t seg_off[DB_ROWS + 1], seg_a[DB_ROWS]; };     // 204 bytes: all the LDS dq_shape_k's wave has
struct DkWave {
    uint64_t buf[DK_CAP];
    uint32_t hist[256];
    DkRuns runs;
};
// LDS written by some lanes is read by others of the same wave: the wave's DS operations execute in order, the fence
// and the barrier keep the compiler from reordering them
__device__ __forceinline__ void dk_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// hist[d] += 1 for every lane of the ballot m; the lanes of a group mostly share the leading bytes, and 64 adds to one
// word would serialise
__device__ __forceinline__ void dk_tally(uint32_t* hist, bool on, uint32_t d, uint64_t m) {
    if (m == 0) return;                                    // wave-uniform
    const int first = __ffsll((unsigned long long)m) - 1;
    const uint32_t d0 = (uint32_t)__shfl((int)d, first, 64);
    if (__ballot(on && d != d0) == 0) {
        if (lane_id() == first) atomicAdd(&hist[d0], (uint32_t)__popcll(m));
    } else if (on) {
        atomicAdd(&hist[d], 1u);
    }
}
// The runs of the piece's cell `key` into W, numbered across: lanes 0..24 find one run each (db_row_run), a wave scan
// numbers their rows.  Returns T, the number of candidates.
__device__ __forceinline__ uint32_t dk_runs(const DbGrid& g, const uint32_t* __restrict__ cell_start,
                                            const uint64_t* __restrict__ cell_key, uint64_t key, DkRuns& W) {
    const int l = lane_id();
    uint32_t a = 0, len = 0;
    if (l < DB_ROWS) {
        const int2 v = db_row_run(g, cell_key, key, l);
        a = cell_start[v.x];
        len = cell_start[v.y] - a;
    }
    const uint32_t incl = wave_scan_incl(len);
    const uint32_t T = (uint32_t)__shfl((int)incl, 63, 64);
    dk_sync();                                             // the piece before this one has read its runs
    if (l < DB_ROWS) { W.seg_a[l] = a; W.seg_off[l + 1] = incl; }
    if (l == 0) W.seg_off[0] = 0u;
    dk_sync();
    return T;
}
// f(in, key, dx, dy, dz, row) for every group of 64 candidates, called by all lanes: in = the lane holds a candidate
// with d2 <= band.r2, key = the bit pattern of its d2, (dx, dy, dz) = candidate - query in float64 (exact: both are
// float32; zeros where the lane holds no candidate or the float32 value already says outside), row = the candidate's
// row in file order (the w of the sorted copy; 0 where the lane holds no candidate).  d2 is db_d2's number: the squares
// of p - q are those of q - p, and the sum runs in its order.
template <typename F>
__device__ __forceinline__ void dk_sweep(const DbBand& band, const float4* __restrict__ pts, const DkRuns& W,
                                         uint32_t T, const float4& q, F&& f) {
    const int l = lane_id();
    int r = 0;
    for (uint32_t t0 = 0; t0 < T; t0 += 64u * DK_AHEAD) {  // wave-uniform
        float4 P[DK_AHEAD];
#pragma unroll
        for (int u = 0; u < DK_AHEAD; ++u) {
            const uint32_t t = t0 + 64u * u + l;
            P[u].x = P[u].y = P[u].z = P[u].w = 0.0f;
            if (t < T) {
                while (t >= W.seg_off[r + 1]) ++r;         // t < T = seg_off[DB_ROWS]: r stays below DB_ROWS
                P[u] = pts[W.seg_a[r] + (t - W.seg_off[r])];
            }
        }
#pragma unroll
        for (int u = 0; u < DK_AHEAD; ++u) {
            if (t0 + 64u * u >= T) break;                  // wave-uniform
            bool in = false;
            uint64_t key = 0;
            double dx = 0.0, dy = 0.0, dz = 0.0;
            if (t0 + 64u * u + l < T) {
                const float4 p = P[u];
                if (!(db_d2f(q, p) >= band.hi)) {                     // (db_within2's band: d32 >= hi implies d64 > r2)
                    dx = (double)p.x - (double)q.x;
                    dy = (double)p.y - (double)q.y;
                    dz = (double)p.z - (double)q.z;
                    double d2 = dx * dx;
                    d2 += dy * dy;
                    d2 += dz * dz;
                    in = d2 <= band.r2;
                    key = (uint64_t)__double_as_longlong(d2);
                }
            }
            f(in, key, dx, dy, dz, __float_as_uint(P[u].w));
        }
    }
}
// The bin of W.hist that holds rank kk (1-based; the bins hold kk keys at least): its number, and kk becomes the rank
// inside it.  The wave scans the 256 bins, four per lane.
__device__ __forceinline__ uint32_t dk_pick(const DkWave& W, uint32_t& kk) {
    const int l = lane_id();
    dk_sync();
    uint32_t h[4], sum = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) { h[u] = W.hist[4 * l + u]; sum += h[u]; }
    const uint32_t incl = wave_scan_incl(sum);
    uint32_t e = incl - sum, digit = 0, knew = 0;
    const bool mine = e < kk && kk <= incl;                // one lane
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (mine && e < kk && kk <= e + h[u]) { digit = 4u * l + u; knew = kk - e; }
        e += h[u];
    }
    const int src = __ffsll((unsigned long long)__ballot(mine)) - 1;
    kk = (uint32_t)__shfl((int)knew, src, 64);
    return (uint32_t)__shfl((int)digit, src, 64);
}
// the k-th smallest d2 <= eps2 among the T candidates of the wave's piece, +inf if there are fewer; count: how many.
// Where count >= k, slots is the rank of the k-th among the candidates whose d2 equals the answer (1-based: k - slots
// candidates lie below it), and W.hist is left holding the last pass: bin (answer & 255) says how many they are.
__device__ __forceinline__ double dk_select_rank(const DbGrid& g, const float4* __restrict__ pts, DkWave& W, uint32_t T,
                                                 const float4& q, int32_t k, int& count_out, uint32_t& slots) {
    const int l = lane_id();
#pragma unroll
    for (int u = 0; u < 4; ++u) W.hist[l + 64 * u] = 0u;
    dk_sync();
    const DbBand band = {g.eps2, g.eps2_lo, g.eps2_hi};
    uint32_t count = 0;
    dk_sweep(band, pts, W.runs, T, q, [&](bool in, uint64_t key, double, double, double, uint32_t) {
        const uint64_t m = __ballot(in);
        if (in) {
            const uint32_t pos = count + (uint32_t)__popcll(m & lanemask_lt());
            if (pos < (uint32_t)DK_CAP) W.buf[pos] = key;
        }
        dk_tally(W.hist, in, (uint32_t)(key >> 56), m);
        count += (uint32_t)__popcll(m);
    });
    count_out = (int)count;
    if (count < (uint32_t)k) return __longlong_as_double(0x7FF0000000000000ll);
    const bool kept = count <= (uint32_t)DK_CAP;
    uint64_t prefix = 0;
    uint32_t kk = (uint32_t)k;                              // rank among the keys that share the prefix, 1-based
    for (int shift = 56;; shift -= 8) {
        const uint32_t digit = dk_pick(W, kk);
        prefix |= (uint64_t)digit << shift;
        if (shift == 0) break;
        dk_sync();                                         // every lane has read its bins
#pragma unroll
        for (int u = 0; u < 4; ++u) W.hist[l + 64 * u] = 0u;
        dk_sync();
        const int ns = shift - 8;
        auto tally = [&](bool in, uint64_t key, double = 0.0, double = 0.0, double = 0.0, uint32_t = 0u) {
            const bool on = in && (key >> shift) == (prefix >> shift);
            dk_tally(W.hist, on, (uint32_t)(key >> ns) & 255u, __ballot(on));
        };
        if (kept) {
            for (uint32_t i0 = 0; i0 < count; i0 += 64) {
                const bool in = i0 + l < count;
                tally(in, in ? W.buf[i0 + l] : 0ull);
            }
        } else {
            dk_sweep(band, pts, W.runs, T, q, tally);
        }
    }
    slots = kk;
    return __longlong_as_double((long long)prefix);
}
__device__ __forceinline__ double dk_select(const DbGrid& g, const float4* __restrict__ pts, DkWave& W, uint32_t T,
                                            const float4& q, int32_t k, int& count_out) {
    uint32_t slots;
    return dk_select_rank(g, pts, W, T, q, k, count_out, slots);
}

__global__ __launch_bounds__(DB_THREADS) void dq_kdist_k(DbQuery Q, DbGrid g, const float4* __restrict__ pts,
                                                         const uint32_t* __restrict__ cell_start,
                                                         const uint64_t* __restrict__ cell_key,
                                                         const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ vals,
                                                         const uint32_t* __restrict__ piece_start,
                                                         const uint32_t* __restrict__ npieces, int32_t k,
                                                         double* __restrict__ out_d2, int32_t* __restrict__ out_count) {
    __shared__ DkWave waves[DB_WAVES];
    const int l = lane_id();
    DkWave& W = waves[wave_id()];
    const uint32_t np = *npieces;
    for (uint32_t p = blockIdx.x * DB_WAVES + wave_id(); p < np; p += gridDim.x * DB_WAVES) {   // wave-uniform
        const uint32_t ps = piece_start[p], pe = piece_start[p + 1];
        const uint32_t T = dk_runs(g, cell_start, cell_key, keys[ps], W.runs);
        for (uint32_t q0 = ps; q0 < pe; q0 += 64) {
            const bool have = q0 + l < pe;
            const uint32_t v = have ? vals[q0 + l] : DQ_OUT;
            float4 mine;
            mine.x = mine.y = mine.z = mine.w = 0.0f;
            if (have && T != 0u && !(v & DQ_OUT)) mine = dq_point(Q, (int64_t)v);
            double res = __longlong_as_double(0x7FF0000000000000ll);
            int res_count = 0;
            const int cnt = (int)(pe - q0 < 64u ? pe - q0 : 64u);
            for (int j = 0; j < cnt && T != 0u; ++j) {
                if ((uint32_t)__builtin_amdgcn_readlane((int)v, j) & DQ_OUT) continue;          // wave-uniform
                float4 qp;
                qp.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.x), j));
                qp.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.y), j));
                qp.z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.z), j));
                qp.w = 0.0f;
                int c;
                const double d = dk_select(g, pts, W, T, qp, k, c);
                if (l == j) { res = d; res_count = c; }
            }
            if (have) {
                out_d2[v & ~DQ_OUT] = res;
                if (out_count) out_count[v & ~DQ_OUT] = res_count;
            }
        }
    }
}

// ---- the k nearest rows of every query among the rows of the fit (pch_dbscan_knn_f32): which rows the neighbours
// are, in (d2, row) order.  dq_kdist_k's skeleton and its LDS, per query:
//   * dk_select_rank gives tau, the k-th smallest d2, with count, and how the rows that tie at tau stand to the cut:
//     `slots` of them belong to the answer, and the last bin of the select says how many they are.  count <= k:
//     everything in reach is the answer;
//   * only where more rows tie than there are slots a second MSB-first radix select runs, over the 32-bit rows of
//     the candidates with d2 == tau, by sweeps (dk_select_row): rho, the largest row admitted.  Else rho is all ones;
//   * one emit sweep: a candidate belongs to the answer iff d2 < tau, or d2 == tau and row <= rho - min(k, count) of
//     them, compacted by ballot into (key, row) arrays.  The select is over by then, so the arrays lie in W.buf: the
//     kernel has dq_kdist_k's LDS and no more.  Keeping rows beside the kept keys to spare this sweep where count <=
//     DK_CAP would cost 4 KiB a wave and the fourth workgroup of a CU;
//   * a rank sort in the wave - the (key, row) pairs are distinct, so a lane counts for each of its (at most four)
//     entries how many entries are smaller and stores it there -, then the lanes store out_rows and out_d2 of the
//     query as contiguous runs, the empty slots (-1, +inf) behind the answer.  A query with nobody in reach (DQ_OUT,
//     or T == 0) stores k empty slots the same way.
// Nothing leaves the wave: no global atomics, no waiting on another workgroup.
constexpr int KNN_K = PCH_KNN_MAX_K;
static_assert(3 * KNN_K <= DK_CAP && KNN_K % 64 == 0, "the unsorted and the sorted answer lie in DkWave::buf");
// the slots-th smallest row (1-based) among the candidates whose d2 has the bit pattern tau
__device__ __forceinline__ uint32_t dk_select_row(const DbBand& band, const float4* __restrict__ pts, DkWave& W,
                                                  uint32_t T, const float4& q, uint64_t tau, uint32_t slots) {
    const int l = lane_id();
    uint32_t prefix = 0, kk = slots;
    for (int shift = 24;; shift -= 8) {
        dk_sync();                                         // every lane has read its bins
#pragma unroll
        for (int u = 0; u < 4; ++u) W.hist[l + 64 * u] = 0u;
        dk_sync();
        dk_sweep(band, pts, W.runs, T, q, [&](bool in, uint64_t key, double, double, double, uint32_t row) {
            const bool on = in && key == tau && (shift == 24 || (row >> (shift + 8)) == (prefix >> (shift + 8)));
            dk_tally(W.hist, on, (row >> shift) & 255u, __ballot(on));
        });
        prefix |= dk_pick(W, kk) << shift;
        if (shift == 0) break;
    }
    return prefix;
}

__global__ __launch_bounds__(DB_THREADS) void dq_knn_k(DbQuery Q, DbGrid g, const float4* __restrict__ pts,
                                                       const uint32_t* __restrict__ cell_start,
                                                       const uint64_t* __restrict__ cell_key,
                                                       const uint64_t* __restrict__ keys,
                                                       const uint32_t* __restrict__ vals,
                                                       const uint32_t* __restrict__ piece_start,
                                                       const uint32_t* __restrict__ npieces, int32_t k,
                                                       int32_t* __restrict__ out_rows, double* __restrict__ out_d2,
                                                       int32_t* __restrict__ out_count) {
    __shared__ DkWave waves[DB_WAVES];
    const int l = lane_id();
    DkWave& W = waves[wave_id()];
    uint64_t* akey = W.buf;                                              // the answer as the emit sweep meets it
    uint32_t* arow = reinterpret_cast<uint32_t*>(W.buf + KNN_K);
    uint64_t* skey = W.buf + KNN_K + KNN_K / 2;                          // and in (d2, row) order
    uint32_t* srow = reinterpret_cast<uint32_t*>(W.buf + 2 * KNN_K + KNN_K / 2);
    const DbBand band = {g.eps2, g.eps2_lo, g.eps2_hi};
    const uint32_t np = *npieces;
    for (uint32_t p = blockIdx.x * DB_WAVES + wave_id(); p < np; p += gridDim.x * DB_WAVES) {   // wave-uniform
        const uint32_t ps = piece_start[p], pe = piece_start[p + 1];
        const uint32_t T = dk_runs(g, cell_start, cell_key, keys[ps], W.runs);
        for (uint32_t q0 = ps; q0 < pe; q0 += 64) {
            const bool have = q0 + l < pe;
            const uint32_t v = have ? vals[q0 + l] : DQ_OUT;
            float4 mine;
            mine.x = mine.y = mine.z = mine.w = 0.0f;
            if (have && T != 0u && !(v & DQ_OUT)) mine = dq_point(Q, (int64_t)v);
            const int cnt = (int)(pe - q0 < 64u ? pe - q0 : 64u);
            for (int j = 0; j < cnt; ++j) {
                const uint32_t vj = (uint32_t)__builtin_amdgcn_readlane((int)v, j);
                uint32_t m = 0;                            // slots of the answer that hold a row
                int count = 0;
                if (T != 0u && !(vj & DQ_OUT)) {           // wave-uniform
                    float4 qp;
                    qp.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.x), j));
                    qp.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.y), j));
                    qp.z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.z), j));
                    qp.w = 0.0f;
                    uint32_t slots = 0;
                    const double d = dk_select_rank(g, pts, W, T, qp, k, count, slots);
                    uint64_t tau = ~0ull;                  // above every d2: all in reach
                    uint32_t rho = ~0u;
                    if (count > k) {
                        tau = (uint64_t)__double_as_longlong(d);
                        if (W.hist[tau & 255u] > slots) rho = dk_select_row(band, pts, W, T, qp, tau, slots);
                    }
                    dk_sync();                             // the selects have read buf and hist
                    dk_sweep(band, pts, W.runs, T, qp, [&](bool in, uint64_t key, double, double, double, uint32_t row) {
                        const bool take = in && (key < tau || (key == tau && row <= rho));
                        const uint64_t mk = __ballot(take);
                        const uint32_t pos = m + (uint32_t)__popcll(mk & lanemask_lt());
                        if (take && pos < (uint32_t)KNN_K) { akey[pos] = key; arow[pos] = row; }   // (pos < k: never outside)
                        m += (uint32_t)__popcll(mk);
                    });
                    m = m < (uint32_t)k ? m : (uint32_t)k;
                    dk_sync();
                    uint64_t ek[KNN_K / 64];
                    uint32_t er[KNN_K / 64], rank[KNN_K / 64];
#pragma unroll
                    for (int u = 0; u < KNN_K / 64; ++u) {
                        const uint32_t i = (uint32_t)l + 64u * u;
                        ek[u] = i < m ? akey[i] : 0ull;
                        er[u] = i < m ? arow[i] : 0u;
                        rank[u] = 0u;
                    }
                    for (uint32_t t = 0; t < m; ++t) {     // wave-uniform: every lane reads the same entry
                        const uint64_t kt = akey[t];
                        const uint32_t rt = arow[t];
#pragma unroll
                        for (int u = 0; u < KNN_K / 64; ++u)
                            rank[u] += (kt < ek[u] || (kt == ek[u] && rt < er[u])) ? 1u : 0u;
                    }
#pragma unroll
                    for (int u = 0; u < KNN_K / 64; ++u) {
                        if ((uint32_t)l + 64u * u < m && rank[u] < m) { skey[rank[u]] = ek[u]; srow[rank[u]] = er[u]; }
                    }
                    dk_sync();
                }
                const int64_t row = (int64_t)(vj & ~DQ_OUT);
                for (uint32_t i = (uint32_t)l; i < (uint32_t)k; i += 64u) {
                    const bool full = i < m;
                    out_rows[row * k + i] = full ? (int32_t)srow[i] : -1;
                    out_d2[row * k + i] = full ? __longlong_as_double((long long)skey[i])
                                               : __longlong_as_double(0x7FF0000000000000ll);
                }
                if (out_count && l == 0) out_count[row] = count;
                dk_sync();                                 // the next query's select writes buf
            }
        }
    }
}

// ---- what a neighbourhood looks like (pch_dbscan_shape_f32): count and the nine first and second moments of the
// rows of the fit within `band` of every query, taken about the query.  dq_kdist_k's skeleton - pieces of DS_PIECE
// queries of one cell, one wave per piece, the 25 runs numbered across (dk_runs), the queries handed round by readlane
// - and its sweep (dk_sweep), once per query: a lane adds the nine terms of its in-range candidates into nine float64
// registers, the count goes by ballot; nine wave butterflies, then lanes 0..8 store the sums side by side (72 bytes)
// and lane 0 the count.  A query that has nobody in reach (DQ_OUT, or T == 0) stores zeros the same way.  There is no
// dense-cell shortcut: a cell that is core as a whole has a count to give but no sums.  LDS: the run tables alone.
// Nothing leaves the wave.
#ifndef PCH_DS_PIECE
#define PCH_DS_PIECE 8                       // tuning builds: make EXTRA=-DPCH_DS_PIECE=16 (DESIGN.md section 5b has the figures)
#endif
constexpr int DS_PIECE = PCH_DS_PIECE;       // as DK_PIECE: a crowded cell's queries go to many waves
__global__ __launch_bounds__(DB_THREADS) void dq_shape_k(DbQuery Q, DbGrid g, DbBand band,
                                                         const float4* __restrict__ pts,
                                                         const uint32_t* __restrict__ cell_start,
                                                         const uint64_t* __restrict__ cell_key,
                                                         const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ vals,
                                                         const uint32_t* __restrict__ piece_start,
                                                         const uint32_t* __restrict__ npieces,
                                                         int32_t* __restrict__ out_count, double* __restrict__ out_m) {
    __shared__ DkRuns runs[DB_WAVES];
    const int l = lane_id();
    DkRuns& W = runs[wave_id()];
    const uint32_t np = *npieces;
    for (uint32_t p = blockIdx.x * DB_WAVES + wave_id(); p < np; p += gridDim.x * DB_WAVES) {   // wave-uniform
        const uint32_t ps = piece_start[p], pe = piece_start[p + 1];
        const uint32_t T = dk_runs(g, cell_start, cell_key, keys[ps], W);
        for (uint32_t q0 = ps; q0 < pe; q0 += 64) {
            const bool have = q0 + l < pe;
            const uint32_t v = have ? vals[q0 + l] : DQ_OUT;
            float4 mine;
            mine.x = mine.y = mine.z = mine.w = 0.0f;
            if (have && T != 0u && !(v & DQ_OUT)) mine = dq_point(Q, (int64_t)v);
            const int cnt = (int)(pe - q0 < 64u ? pe - q0 : 64u);
            for (int j = 0; j < cnt; ++j) {
                const uint32_t vj = (uint32_t)__builtin_amdgcn_readlane((int)v, j);
                double s[9];
#pragma unroll
                for (int a = 0; a < 9; ++a) s[a] = 0.0;
                uint32_t count = 0;
                if (T != 0u && !(vj & DQ_OUT)) {           // wave-uniform
                    float4 qp;
                    qp.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.x), j));
                    qp.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.y), j));
                    qp.z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.z), j));
                    qp.w = 0.0f;
                    dk_sweep(band, pts, W, T, qp, [&](bool in, uint64_t, double dx, double dy, double dz, uint32_t) {
                        count += (uint32_t)__popcll(__ballot(in));
                        if (in) {
                            s[0] += dx; s[1] += dy; s[2] += dz;
                            s[3] += dx * dx; s[4] += dy * dy; s[5] += dz * dz;
                            s[6] += dx * dy; s[7] += dx * dz; s[8] += dy * dz;
                        }
                    });
#pragma unroll
                    for (int a = 0; a < 9; ++a) s[a] = wave_reduce_add(s[a]);    // every lane holds every sum
                }
                double sl = s[0];
#pragma unroll
                for (int a = 1; a < 9; ++a) sl = l == a ? s[a] : sl;
                const int64_t row = (int64_t)(vj & ~DQ_OUT);
                if (l < 9) out_m[9 * row + l] = sl;
                if (l == 0) out_count[row] = (int32_t)count;
            }
        }
    }
}

// ---- eigenvalues of the neighbourhood's covariance from those moments (pch_shape_features_f64), one thread per
// query: n = max(count, 1), mu = M[0:3]/n, C = M2/n - mu mu^T (symmetric, not clamped), then cyclic Jacobi in float64 -
// SF_SWEEPS fixed sweeps over (0,1), (0,2), (1,2), every rotation branch-free.  A closed-form trigonometric solve loses
// the small eigenvalue of a line, Jacobi's rotations do not.  Of the eigenvectors only the z row is carried: what is
// asked for is |e1.z|.
constexpr int SF_SWEEPS = 6;
// one rotation that zeroes the (p, q) entry: app, aqq the diagonal, apq the entry, (arp, arq) the third row's entries
// in columns p and q, (vp, vq) the z components of eigenvector columns p and q.  apq == 0 (and a ratio beyond the
// range of float64, whose rotation would move nothing) gives the identity.
__device__ __forceinline__ void sf_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& vp,
                                          double& vq) {
    const bool zero = apq == 0.0;
    const double theta = (aqq - app) / (2.0 * (zero ? 1.0 : apq));
    double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    t = zero ? 0.0 : t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    const double wp = c * vp - s * vq, wq = s * vp + c * vq;
    vp = wp; vq = wq;
}
__global__ __launch_bounds__(DB_THREADS) void sf_features_k(const int32_t* __restrict__ count,
                                                            const double* __restrict__ M, int64_t nq,
                                                            double* __restrict__ out4) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= nq) return;
    const int32_t cn = count[i];
    const double n = (double)(cn > 1 ? cn : 1);
    const double* m = M + 9 * i;
    const double mx = m[0] / n, my = m[1] / n, mz = m[2] / n;
    double a00 = m[3] / n - mx * mx, a11 = m[4] / n - my * my, a22 = m[5] / n - mz * mz;
    double a01 = m[6] / n - mx * my, a02 = m[7] / n - mx * mz, a12 = m[8] / n - my * mz;
    double v0 = 0.0, v1 = 0.0, v2 = 1.0;                   // the z row of V = I
    for (int sweep = 0; sweep < SF_SWEEPS; ++sweep) {
        sf_rotate(a00, a11, a01, a02, a12, v0, v1);
        sf_rotate(a00, a22, a02, a01, a12, v0, v2);
        sf_rotate(a11, a22, a12, a01, a02, v1, v2);
    }
    // descending, ties to the lower index: the zero matrix gives e1 = (1, 0, 0), v = 0
    double l1 = a00, l2 = a11, l3 = a22, e1 = v0;
    if (l2 > l1) { const double t = l1; l1 = l2; l2 = t; e1 = v1; }
    if (l3 > l1) { const double t = l1; l1 = l3; l3 = t; e1 = v2; }
    if (l3 > l2) { const double t = l2; l2 = l3; l3 = t; }
    out4[4 * i + 0] = l1; out4[4 * i + 1] = l2; out4[4 * i + 2] = l3; out4[4 * i + 3] = fabs(e1);
}

// ---- relabelling with an external cluster map (cross-tile reconciliation, tiles.py): core points and
// cells take map[old id], every other point goes back to -1 and is assigned again by db_border_k, so
// that a border point takes the smallest NEW id among its core neighbours
__global__ __launch_bounds__(DB_THREADS) void db_remap_points_k(const float4* __restrict__ pts,
                                                                const uint8_t* __restrict__ core_s, int64_t n,
                                                                const int32_t* __restrict__ map, int32_t nmap,
                                                                int32_t* __restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = __float_as_uint(pts[i].w);
    int32_t lab = -1;
    if (core_s[i]) {
        const int32_t old = labels[o];
        lab = (old >= 0 && old < nmap) ? map[old] : -1;
    }
    labels[o] = lab;
}
__global__ __launch_bounds__(DB_THREADS) void db_remap_cells_k(int* __restrict__ cell_label,
                                                               const uint32_t* __restrict__ cell_ncore, int m,
                                                               const int32_t* __restrict__ map, int32_t nmap) {
    const int c = blockIdx.x * DB_THREADS + threadIdx.x;
    if (c >= m) return;
    if (cell_ncore[c] == 0) return;
    const int old = cell_label[c];
    const int neu = (old >= 0 && old < nmap) ? map[old] : -1;
    cell_label[c] = neu >= 0 ? neu : INT_BIG;              // a dropped cluster attracts no border points
}

// cluster id -> its smallest core row (the set bits of the row bitmap, in order)
__global__ __launch_bounds__(DB_THREADS) void db_first_rows_k(const uint32_t* __restrict__ bits,
                                                              const uint32_t* __restrict__ rank, int64_t nw,
                                                              int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= nw) return;
    uint32_t b = bits[i];
    uint32_t c = rank[i];
    while (b) {
        const int t = __builtin_ctz(b);
        b &= b - 1;
        out[c++] = (int32_t)(i * 32 + t);
    }
}

// Cross-tile links (config 4): one representative per cell of the core points with x in [x_lo, x_hi) - the strip
// around a tile edge.  All core points of a cell are mutually within eps (cell side eps/sqrt(3)), so they are one
// cluster in ANY tile that holds them with exact core flags: one (row, cluster) pair per cell tells the
// neighbouring tile everything the pairs of all its strip points would.  One wave per cell; cells whose core box
// misses the strip are rejected from the cell table alone.
__global__ __launch_bounds__(DB_THREADS) void db_strip_pairs_k(const float4* __restrict__ pts,
                                                               const uint32_t* __restrict__ cell_start,
                                                               const uint8_t* __restrict__ core_s,
                                                               const uint32_t* __restrict__ cell_ncore,
                                                               const float* __restrict__ cell_box,
                                                               const int* __restrict__ cell_label, int m, float x_lo,
                                                               float x_hi, int32_t cap, int32_t* __restrict__ out_pairs,
                                                               int32_t* __restrict__ out_count) {
    const int c = blockIdx.x * DB_WAVES + wave_id();
    if (c >= m) return;                                   // wave-uniform
    if (cell_ncore[c] == 0) return;
    if (!(cell_box[6 * (int64_t)c + 3] >= x_lo && cell_box[6 * (int64_t)c] < x_hi)) return;
    const int l = lane_id();
    const uint32_t a = cell_start[c], b = cell_start[c + 1];
    uint32_t best = 0xFFFFFFFFu;
    for (uint32_t i = a + l; i < b; i += 64) {
        if (!core_s[i]) continue;
        const float4 p = pts[i];
        if (p.x >= x_lo && p.x < x_hi) {
            const uint32_t row = __float_as_uint(p.w);
            best = row < best ? row : best;
        }
    }
    best = wave_reduce_min(best);
    if (l == 0 && best != 0xFFFFFFFFu) {
        const int32_t slot = atomicAdd(out_count, 1);     // the count keeps growing beyond cap: the caller sees it
        if (slot < cap) {
            out_pairs[2 * slot] = (int32_t)best;
            out_pairs[2 * slot + 1] = cell_label[c];
        }
    }
}

}  // namespace pch

using namespace pch;

extern "C" int pch_dbscan_first_core_rows_i32(int64_t n, int32_t* out_rows, void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(out_rows ? (const void*)out_rows : (const void*)ws);
    PCH_REQUIRE(n >= 0, "bad argument");
    if (n == 0) return PCH_OK;
    DbWs w;
    PCH_TRY(db_continue(__func__, n, ws, ws_bytes, w));
    PCH_REQUIRE(out_rows != nullptr, "null output");
    const int64_t nw = ceil_div(n, 32);
    PCH_LAUNCH("db_first_rows", db_first_rows_k, dim3((unsigned)ceil_div(nw, DB_THREADS)), dim3(DB_THREADS), 0,
               (hipStream_t)stream, w.bits, w.wrank, nw, out_rows);
    return PCH_OK;
}

extern "C" int pch_dbscan_pair_stats(int64_t n, uint64_t* out4_host, void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(ws);
    PCH_REQUIRE(n >= 0 && out4_host, "bad argument");
    memset(out4_host, 0, 4 * sizeof(uint64_t));
    if (n == 0) return PCH_OK;
    DbWs w;
    PCH_TRY(db_continue(__func__, n, ws, ws_bytes, w));
    PCH_HIP_TRY(hipMemcpyAsync(out4_host, w.core_stats, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    PCH_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return PCH_OK;
}

extern "C" int pch_dbscan_strip_pairs_i32(int64_t n, float x_lo, float x_hi, int32_t cap, int32_t* out_pairs,
                                          int32_t* out_count, void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(out_count);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n >= 0 && cap >= 0 && out_count && (cap == 0 || out_pairs), "bad argument");
    PCH_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(int32_t), s));
    if (n == 0 || !(x_lo < x_hi)) return PCH_OK;
    DbWs w;
    PCH_TRY(db_continue(__func__, n, ws, ws_bytes, w));
    const int m = g_last.c.m;
    PCH_LAUNCH("db_strip_pairs", db_strip_pairs_k, dim3((unsigned)ceil_div(m, DB_WAVES)), dim3(DB_THREADS), 0, s,
               w.pts, w.cell_start, w.core_s, w.cell_ncore, w.cell_box, w.cell_label, m, x_lo, x_hi, cap, out_pairs,
               out_count);
    return PCH_OK;
}

extern "C" int pch_dbscan_relabel_i32(const int32_t* map, int32_t nmap, int64_t n, int32_t* labels, void* ws,
                                      size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(labels);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n >= 0 && nmap >= 0 && (nmap == 0 || map) && (n == 0 || labels), "bad argument");
    if (n == 0) return PCH_OK;
    DbWs w;
    PCH_TRY(db_continue(__func__, n, ws, ws_bytes, w));
    const DbCells& c = g_last.c;
    PCH_LAUNCH("db_remap_points", db_remap_points_k, dim3((unsigned)ceil_div(n, DB_THREADS)), dim3(DB_THREADS), 0, s,
               w.pts, w.core_s, n, map, nmap, labels);
    PCH_LAUNCH("db_remap_cells", db_remap_cells_k, dim3((unsigned)ceil_div(c.m, DB_THREADS)), dim3(DB_THREADS), 0, s,
               w.cell_label, w.cell_ncore, c.m, map, nmap);
    return db_border_again(c, w.cell_label, labels, s);
}

// the query workspace of pch_dbscan_assign_f32
struct DqWs { uint64_t *k0, *k1; uint32_t *v0, *v1, *flag, *piece_start, *radix_ws, *scan_ws, *npieces; };
static void dq_plan(Arena& a, int64_t nq, DqWs& w) {
    const int64_t nn = nq > 0 ? nq : 1;
    w.npieces = a.take<uint32_t>(64);
    w.k0 = a.take<uint64_t>(nn);
    w.k1 = a.take<uint64_t>(nn);
    w.v0 = a.take<uint32_t>(nn);
    w.v1 = a.take<uint32_t>(nn);
    w.flag = a.take<uint32_t>(nn + 8);            // start flags of the pieces, scanned in place
    w.piece_start = a.take<uint32_t>(nn + 8);     // one more entry than pieces
    w.radix_ws = a.take<uint32_t>(radix_ws_u32(nn));
    w.scan_ws = a.take<uint32_t>(scan_ws_u32(nn));
}

extern "C" size_t pch_dbscan_assign_ws_bytes(int64_t nq) {
    if (nq < 0) return 0;
    Arena a;
    DqWs w;
    dq_plan(a, nq, w);
    return a.off;
}

// What pch_dbscan_assign_f32, pch_dbscan_kdist_f32, pch_dbscan_knn_f32 and pch_dbscan_shape_f32 share: the checks of a
// query call against the fit `entry` continues (nq != 0, `out` its output), then the queries binned into the fit's cells, sorted and cut into pieces.
struct DqPieces { DbQuery Q; const uint64_t* ks; const uint32_t* vs; const uint32_t *piece_start, *npieces; };
template <int PIECE>
static int dq_pieces(const char* entry, const float* query, int64_t nq, const float* sub3_host,
                     const int32_t* query_chunk, int64_t n, const void* out, void* qws, size_t qws_bytes, void* ws,
                     size_t ws_bytes, hipStream_t s, DbWs& w, DqPieces& P) {
    PCH_TRY(db_continue(entry, n, ws, ws_bytes, w));
    if (!(query && out && qws)) { set_error("%s: null buffer", entry); return PCH_ERR_ARG; }
    if (g_last.compressed) {
        set_error("%s: the fit took the compressed-coordinate path, which keeps no map from a coordinate to a cell",
                  entry);
        return PCH_ERR_RANGE;
    }
    if (!(query_chunk || g_last.nchunks == 1)) {
        set_error("%s: query_chunk is null but the fit has several chunks", entry);
        return PCH_ERR_ARG;
    }
    {
        const char* a0 = static_cast<const char*>(qws);
        const char* b0 = static_cast<const char*>(ws);
        if (a0 < b0 + ws_bytes && b0 < a0 + qws_bytes) {
            set_error("%s: the query workspace overlaps the fit's workspace", entry);
            return PCH_ERR_ARG;
        }
    }
    Arena qa(qws, qws_bytes);                     // (disjoint from the fit's workspace: the fit stays remembered)
    DqWs qw;
    dq_plan(qa, nq, qw);
    if (qa.overflow) { set_error("query workspace too small: need %zu bytes", qa.off); return PCH_ERR_WORKSPACE; }
    const DbCells& c = g_last.c;
    P.Q = {query, nq, sub3_host ? sub3_host[0] : 0.0f, sub3_host ? sub3_host[1] : 0.0f,
           sub3_host ? sub3_host[2] : 0.0f, query_chunk, g_last.nchunks};
    const unsigned gq = (unsigned)ceil_div(nq, DB_THREADS);
    const int nbits = c.g.bx + c.g.by + c.g.bz + bits_for((uint64_t)g_last.nchunks);     // <= 64: not compressed
    PCH_LAUNCH("dq_keys", dq_keys_k, dim3(gq), dim3(DB_THREADS), 0, s, P.Q, c.g, qw.k0, qw.v0);
    PCH_TRY(radix_sort_pairs(qw.k0, qw.v0, qw.k1, qw.v1, nq, nbits, qw.radix_ws, s));
    const bool in1 = radix_sort_result_buffer(nbits) == 1;
    P.ks = in1 ? qw.k1 : qw.k0;
    P.vs = in1 ? qw.v1 : qw.v0;
    PCH_LAUNCH("dq_heads", dq_heads_k<PIECE>, dim3(gq), dim3(DB_THREADS), 0, s, P.ks, nq, qw.flag);
    PCH_TRY(scan_exclusive_u32(qw.flag, qw.flag, nq, qw.scan_ws, qw.npieces, s));
    PCH_LAUNCH("dq_pieces", dq_pieces_k<PIECE>, dim3(gq), dim3(DB_THREADS), 0, s, P.ks, nq, qw.flag, qw.piece_start);
    P.piece_start = qw.piece_start;
    P.npieces = qw.npieces;
    return PCH_OK;
}
// pieces <= cells with queries + nq / PIECE; the host does not read the count: the waves stride over it
static unsigned dq_piece_blocks(int64_t nq) {
    return (unsigned)std::min(ceil_div(nq, (int64_t)DB_WAVES * 8), int64_t(16384));
}

extern "C" int pch_dbscan_assign_f32(const float* query, int64_t nq, const float* sub3_host, const int32_t* query_chunk,
                                     int64_t n, int32_t* out_labels, void* qws, size_t qws_bytes, void* ws,
                                     size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(out_labels ? (const void*)out_labels : (const void*)ws);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(nq >= 0 && nq < (int64_t(1) << 31), "nq out of range [0, 2^31)");
    PCH_REQUIRE(n >= 0, "bad argument");
    if (nq == 0) return PCH_OK;
    DbWs w;
    DqPieces P;
    PCH_TRY(dq_pieces<DQ_PIECE>(__func__, query, nq, sub3_host, query_chunk, n, out_labels, qws, qws_bytes, ws, ws_bytes, s,
                                w, P));
    const DbCells& c = g_last.c;
    PCH_LAUNCH("dq_assign", dq_assign_k, dim3(dq_piece_blocks(nq)), dim3(DB_THREADS), 0, s, P.Q, c.g, c.pts,
               c.cell_start, c.cell_key, c.core_s, c.cell_ncore, c.cell_box, (const int*)w.cell_label, P.ks, P.vs,
               P.piece_start, P.npieces, out_labels);
    return PCH_OK;
}

extern "C" size_t pch_dbscan_kdist_ws_bytes(int64_t nq) { return pch_dbscan_assign_ws_bytes(nq); }

extern "C" int pch_dbscan_kdist_f32(const float* query, int64_t nq, const float* sub3_host, const int32_t* query_chunk,
                                    int32_t k, int64_t n, double* out_d2, int32_t* out_count, void* qws,
                                    size_t qws_bytes, void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(out_d2 ? (const void*)out_d2 : (const void*)ws);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(k >= 1, "k must be >= 1");
    PCH_REQUIRE(nq >= 0 && nq < (int64_t(1) << 31), "nq out of range [0, 2^31)");
    PCH_REQUIRE(n >= 0, "bad argument");
    if (nq == 0) return PCH_OK;
    DbWs w;
    DqPieces P;
    PCH_TRY(dq_pieces<DK_PIECE>(__func__, query, nq, sub3_host, query_chunk, n, out_d2, qws, qws_bytes, ws, ws_bytes, s, w,
                                P));
    const DbCells& c = g_last.c;
    PCH_LAUNCH("dq_kdist", dq_kdist_k, dim3(dq_piece_blocks(nq)), dim3(DB_THREADS), 0, s, P.Q, c.g, c.pts,
               c.cell_start, c.cell_key, P.ks, P.vs, P.piece_start, P.npieces, k, out_d2, out_count);
    return PCH_OK;
}

extern "C" size_t pch_dbscan_knn_ws_bytes(int64_t nq) { return pch_dbscan_assign_ws_bytes(nq); }

extern "C" int pch_dbscan_knn_f32(const float* query, int64_t nq, const float* sub3_host, const int32_t* query_chunk,
                                  int32_t k, int64_t n, int32_t* out_rows, double* out_d2, int32_t* out_count,
                                  void* qws, size_t qws_bytes, void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(out_d2 ? (const void*)out_d2 : (const void*)ws);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(k >= 1 && k <= PCH_KNN_MAX_K, "k out of range [1, PCH_KNN_MAX_K]");
    PCH_REQUIRE(nq >= 0 && nq < (int64_t(1) << 31), "nq out of range [0, 2^31)");
    PCH_REQUIRE(n >= 0, "bad argument");
    if (nq == 0) return PCH_OK;
    PCH_REQUIRE(out_rows != nullptr, "null buffer");
    DbWs w;
    DqPieces P;
    PCH_TRY(dq_pieces<DK_PIECE>(__func__, query, nq, sub3_host, query_chunk, n, out_d2, qws, qws_bytes, ws, ws_bytes, s, w,
                                P));
    const DbCells& c = g_last.c;
    PCH_LAUNCH("dq_knn", dq_knn_k, dim3(dq_piece_blocks(nq)), dim3(DB_THREADS), 0, s, P.Q, c.g, c.pts, c.cell_start,
               c.cell_key, P.ks, P.vs, P.piece_start, P.npieces, k, out_rows, out_d2, out_count);
    return PCH_OK;
}

extern "C" size_t pch_dbscan_shape_ws_bytes(int64_t nq) { return pch_dbscan_assign_ws_bytes(nq); }

extern "C" int pch_dbscan_shape_f32(const float* query, int64_t nq, const float* sub3_host, const int32_t* query_chunk,
                                    double radius, int64_t n, int32_t* out_count, double* out_moments, void* qws,
                                    size_t qws_bytes, void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(out_moments ? (const void*)out_moments : (const void*)ws);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(radius > 0.0 && radius <= 1.7e308, "radius must be finite and > 0");     // (NaN fails the first)
    PCH_REQUIRE(nq >= 0 && nq < (int64_t(1) << 31), "nq out of range [0, 2^31)");
    PCH_REQUIRE(n >= 0, "bad argument");
    if (nq == 0) return PCH_OK;
    PCH_REQUIRE(out_count != nullptr, "null buffer");
    // the grid reaches two cells, which is the fit's eps: a larger radius would miss rows.  (Another workspace than
    // the remembered fit's is dq_pieces' error.)
    if (ws && g_last.ws == ws && !(radius <= g_last.eps)) {
        set_error("%s: radius %g exceeds the fit's eps %g", __func__, radius, g_last.eps);
        return PCH_ERR_ARG;
    }
    DbWs w;
    DqPieces P;
    PCH_TRY(dq_pieces<DS_PIECE>(__func__, query, nq, sub3_host, query_chunk, n, out_moments, qws, qws_bytes, ws, ws_bytes,
                                s, w, P));
    const DbCells& c = g_last.c;
    PCH_LAUNCH("dq_shape", dq_shape_k, dim3(dq_piece_blocks(nq)), dim3(DB_THREADS), 0, s, P.Q, c.g, db_band(radius),
               c.pts, c.cell_start, c.cell_key, P.ks, P.vs, P.piece_start, P.npieces, out_count, out_moments);
    return PCH_OK;
}

extern "C" int pch_shape_features_f64(const int32_t* count, const double* moments, int64_t nq, double* out4,
                                      void* stream) {
    PCH_DEVICE_GUARD(out4);
    PCH_REQUIRE(nq >= 0 && (nq == 0 || (count && moments && out4)), "bad argument");
    if (nq == 0) return PCH_OK;
    PCH_LAUNCH("sf_features", sf_features_k, dim3((unsigned)ceil_div(nq, DB_THREADS)), dim3(DB_THREADS), 0,
               (hipStream_t)stream, count, moments, nq, out4);
    return PCH_OK;
}
