// Stage C, rows to cell table: the rows of every chunk grouped by cell (w.pts) and the table of those cells -
// cell_start, cell_key, chunk_cells - that the fit (pch_dbscan.hip, which explains the method) works on.
#include "pch_dbscan.h"

namespace pch {

// ---- chunks that contain NaN/inf: sklearn raises for such a chunk (utils/tower_extraction.py:118-119);
// its rows keep their own chunk key and sit in ONE cell (0,0,0) of that chunk that is never core, so
// every chunk owns at least one cell and chunk_cells[] is complete (db_cells_k)
__device__ __forceinline__ bool db_row_bad(const float* __restrict__ xyz, int64_t i) {   // row i holds a NaN/inf
    const uint32_t a = __float_as_uint(xyz[3 * i + 0]) & 0x7FFFFFFFu;
    const uint32_t b = __float_as_uint(xyz[3 * i + 1]) & 0x7FFFFFFFu;
    const uint32_t c = __float_as_uint(xyz[3 * i + 2]) & 0x7FFFFFFFu;
    return a >= 0x7F800000u || b >= 0x7F800000u || c >= 0x7F800000u;
}
__global__ __launch_bounds__(DB_THREADS) void db_chunkbad_k(const float* __restrict__ xyz, int64_t n,
                                                            int64_t chunk_size, uint32_t* __restrict__ bad) {
    for (int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * DB_THREADS)
        if (db_row_bad(xyz, i)) atomicOr(&bad[i / chunk_size], 1u);
}

// ---- first row holding NaN/inf (what sklearn's check_array rejects before DBSCAN.fit starts) ----
__global__ __launch_bounds__(DB_THREADS) void db_first_bad_k(const float* __restrict__ xyz, int64_t n,
                                                             unsigned long long* __restrict__ first) {
    unsigned long long best = ~0ull;
    for (int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * DB_THREADS)
        if (db_row_bad(xyz, i) && (unsigned long long)i < best) best = (unsigned long long)i;
    best = wave_reduce_min(best);
    if (lane_id() == 0 && best != ~0ull) atomicMin(first, best);
}

// ---- cell keys -----------------------------------------------------------------------
__global__ __launch_bounds__(DB_THREADS) void db_keys_k(const float* __restrict__ xyz, int64_t n,
                                                        DbGrid g, const uint32_t* __restrict__ bad,
                                                        uint64_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals,
                                                        uint32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    vals[i] = (uint32_t)i;
    if (bad[i / g.chunk_size]) {                           // the whole chunk stays noise: one cell, never core
        keys[i] = db_pack(g, (uint64_t)(i / g.chunk_size), 0, 0, 0);
        return;
    }
    const float x = xyz[3 * i + 0], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    uint32_t cx, cy, cz;
    if (!db_cell_coords(g, x, y, z, cx, cy, cz)) atomicOr(status, 1u);
    keys[i] = db_pack(g, (uint64_t)(i / g.chunk_size), cz, cy, cx);
}

// ---- fallback for grids that do not fit the 64-bit key (extent/eps astronomically large: outliers, heavy
// tails): per-axis COMPRESSED cell coordinates.  The points are sorted along the axis; a gap of >= 3 cells
// between consecutive points starts a new segment (nothing on one side of such a gap is within eps of
// anything on the other side), cell indices are taken relative to the segment's first point (small, so the
// float64 product is as exact as on the main path) and segments are laid out 3 units apart.  Equal
// compressed index <=> same segment and same local cell; indices that differ by <= 2 are exactly as far
// apart as the true ones; everything else stays >= 3 apart: the 5x5x5 neighbourhood logic is unchanged,
// with at most 3n index values per axis.
__global__ __launch_bounds__(DB_THREADS) void dbc_axis_keys_k(const float* __restrict__ xyz, int64_t n, int axis,
                                                              uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    keys[i] = f32_ordered(xyz[3 * i + axis]);
    vals[i] = (uint32_t)i;
}
__global__ __launch_bounds__(DB_THREADS) void dbc_heads_k(const uint64_t* __restrict__ keys, int64_t n, double inv_cell,
                                                          uint32_t* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    bool h = i == 0;
    if (i > 0) {
        const double a = (double)f32_unordered((uint32_t)keys[i - 1]), b = (double)f32_unordered((uint32_t)keys[i]);
        h = (b - a) * inv_cell >= 3.0;
    }
    head[i] = h ? 1u : 0u;
}
__global__ __launch_bounds__(DB_THREADS) void dbc_local_k(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flag,
                                                          const uint32_t* __restrict__ excl, int64_t n, double inv_cell,
                                                          float* __restrict__ headx, int phase,
                                                          uint32_t* __restrict__ li, uint32_t* __restrict__ seglen,
                                                          uint32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t seg = excl[i] + flag[i] - 1u;                     // flags are kept beside their scan
    const float x = f32_unordered((uint32_t)keys[i]);
    if (phase == 0) {
        if (flag[i]) headx[seg] = x;
        return;
    }
    const double v = floor(((double)x - (double)headx[seg]) * inv_cell);
    uint32_t u = 0;
    if (v >= 0.0 && v < 2147483000.0) u = (uint32_t)v; else atomicOr(status, 2u);
    li[i] = u;
    const bool last = i + 1 == n || flag[i + 1] != 0u;
    if (last) seglen[seg] = u + 3u;                                  // next segment starts 3 units behind this one's last cell
}
__global__ __launch_bounds__(DB_THREADS) void dbc_comp_k(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ flag,
                                                         const uint32_t* __restrict__ excl, const uint32_t* __restrict__ li,
                                                         const uint32_t* __restrict__ segoff, int64_t n, int axis,
                                                         uint32_t* __restrict__ comp, uint32_t* __restrict__ cmax) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t seg = excl[i] + flag[i] - 1u;
    const uint32_t c = segoff[seg] + li[i];
    comp[3 * (int64_t)vals[i] + axis] = c;
    if (i == n - 1) cmax[axis] = c;                                  // sorted: the last one is the largest
}
__global__ __launch_bounds__(DB_THREADS) void db_keys_comp_k(const uint32_t* __restrict__ comp, int64_t n, DbGrid g,
                                                             uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    vals[i] = (uint32_t)i;
    keys[i] = db_pack(g, 0, comp[3 * i + 2], comp[3 * i + 1], comp[3 * i + 0]);
}

// sorted order: gather coordinates (+ original row in .w)
__global__ __launch_bounds__(DB_THREADS) void db_gather_k(const float* __restrict__ xyz,
                                                          const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ vals, int64_t n,
                                                          float4* __restrict__ pts) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = vals[i];
    float4 p;
    p.x = xyz[3 * (int64_t)o + 0];
    p.y = xyz[3 * (int64_t)o + 1];
    p.z = xyz[3 * (int64_t)o + 2];
    p.w = __uint_as_float(o);
    pts[i] = p;
}

// ---- chunk-local sort: keys + sort + gather for one chunk per workgroup --------------------
// Chunks are runs of consecutive input rows, so the chunk field of the key is already sorted;
// only the cell bits (<= 32) need sorting, and only inside a chunk.  One 1024-thread workgroup
// per chunk.  What moves through the LSD passes is the row itself, (x, y, z, original row) as one
// float4: the cell key is a cheap function of (x, y, z) and is recomputed wherever a digit is
// needed, so there is neither a key/index stream nor a random gather at the end (a 12-byte
// gather costs a whole cache line).  Sweep B finds the chunk's own box in cell coordinates: what is
// sorted is the key RELATIVE to it - same order, but as many bits as the chunk's extent needs (15-17 for a
// 50 000-row chunk) instead of the tile's (21+), i.e. two 8/9-bit passes instead of three.  Sweep H builds
// the digit histograms of every pass; pass 0 reads the input rows, the last pass writes the sorted rows and
// their full keys (the cell heads are read off those keys by db_heads_k / db_cells_k).  Replaces db_chunkbad, db_keys, every radix pass (histogram + 3 scan
// kernels + scatter) and db_gather of the global path.

// ---- what db_chunksort_k and db_cellscatter_k must agree on for the overflow hand-over.  One asymmetry stays:
// db_cellscatter_k stops sweeping once it has seen too many cells, so a NaN behind that point is found only by
// db_chunksort_k's sweep B - which is why the overflow kernel keeps the bad-chunk path of cs_rows_in_place.
constexpr int CS_HU = 8;                      // rows per thread in flight
// rows i0 + u * CS_THREADS + tid of the chunk, all loads issued before any is used; a row past the end repeats row 0
__device__ __forceinline__ void cs_load_rows(const Row3* __restrict__ rows, int i0, int cn, Row3 (&q)[CS_HU]) {
#pragma unroll
    for (int u = 0; u < CS_HU; ++u) {
        const int i = i0 + u * CS_THREADS + (int)threadIdx.x;
        q[u] = rows[i < cn ? i : 0];
    }
}
// row check: is q finite?  A row of the chunk (in) sets flags[0] if not, else flags[1] if outside the grid (!ok)
__device__ __forceinline__ bool cs_row_check(const Row3& q, bool in, bool ok, uint32_t* flags) {
    const bool fin = fabsf(q.x) < INFINITY && fabsf(q.y) < INFINITY && fabsf(q.z) < INFINITY;
    if (in && !fin) flags[0] = 1u;
    else if (in && !ok) flags[1] = 1u;
    return fin;
}
__device__ __forceinline__ uint64_t cs_chunk_field(const DbGrid& g, int64_t c) {    // of the keys of chunk c
    const int sh = g.bx + g.by + g.bz;
    return sh < 64 ? ((uint64_t)c << sh) : 0ull;
}
// a NaN/inf chunk (isbad: every key is cell 0) or a one-cell chunk: the rows stay where they are.  keys_out may be
// null (db_cellscatter_k on the table route: the chunk's single cell is staged instead)
__device__ __forceinline__ void cs_rows_in_place(const DbGrid& g, const Row3* __restrict__ rows, int cn, int64_t lo,
        uint64_t hi, bool isbad, float4* __restrict__ pts, uint64_t* __restrict__ keys_out) {
    for (int i = threadIdx.x; i < cn; i += CS_THREADS) {
        const Row3 q = rows[i];
        float4 o4;
        o4.x = q.x; o4.y = q.y; o4.z = q.z; o4.w = __uint_as_float((uint32_t)(lo + i));
        pts[lo + i] = o4;
        bool ok;
        if (keys_out) keys_out[lo + i] = isbad ? hi : (hi | cs_cell_key(g, q.x, q.y, q.z, ok));
    }
}

// gate: runs only the chunks whose word is set (those db_cellscatter_k handed over); the others return at once
__global__ __launch_bounds__(CS_THREADS) void db_chunksort_k(
    const float* __restrict__ xyz, int64_t n, DbGrid g, const uint32_t* __restrict__ gate, uint32_t* __restrict__ bad,
    float4* __restrict__ xbuf, float4* __restrict__ pts, uint64_t* __restrict__ keys_out,
    uint32_t* __restrict__ status, unsigned long long* __restrict__ stamps, const DbHead* __restrict__ head) {
    if (!db_head_take(head, n, g)) return;              // (the fused call's unread launch: n and g from *head)
    if (gate[blockIdx.x] == 0u) return;                 // workgroup-uniform
#ifdef PCH_CS_STAMPS                                    // phase timing of one workgroup (tuning builds only)
    int stamp_i = 0;
#define CS_STAMP() if (stamps && blockIdx.x == gridDim.x / 2 && threadIdx.x == 0) stamps[stamp_i++] = wall_clock64();
    unsigned long long tacc[3] = {0, 0, 0}, tlast = 0;       // inside the tile loop: rank | offsets | scatter
#define CS_TILE_STAMP(k) do { const unsigned long long _t = wall_clock64(); tacc[k] += _t - tlast; tlast = _t; } while (0)
#else
#define CS_STAMP()
#define CS_TILE_STAMP(k)
#endif
    CS_STAMP();
    __shared__ uint32_t hist[CS_PASSES][CS_HREP][CS_BINS];   // replicated: lanes of a wave that share a bin (most do: a
                                                             // chunk covers few cells) spread over CS_HREP addresses
    __shared__ uint32_t cnt[CS_WAVES][CS_BINS];
    __shared__ uint32_t off[CS_WAVES][CS_BINS];
    __shared__ uint32_t base[CS_BINS];
    __shared__ uint32_t wsum[CS_BINS / 64];
    __shared__ uint32_t flags[2];                       // [0] chunk holds NaN/inf, [1] point outside the box
    __shared__ uint32_t cbox[6];                        // the chunk's own box in cell coordinates: min xyz, max xyz
    const int tid = threadIdx.x, w = wave_id(), l = lane_id();
    const int64_t c = blockIdx.x;
    const int64_t lo = c * g.chunk_size;
    const int cn = (int)((n - lo) < g.chunk_size ? (n - lo) : g.chunk_size);
    const Row3* __restrict__ rows = reinterpret_cast<const Row3*>(xyz) + lo;
    for (int j = tid; j < CS_PASSES * CS_HREP * CS_BINS; j += CS_THREADS) (&hist[0][0][0])[j] = 0;
    for (int j = tid; j < CS_WAVES * CS_BINS; j += CS_THREADS) (&cnt[0][0])[j] = 0;
    if (tid < 2) flags[tid] = 0;
    if (tid < 6) cbox[tid] = tid < 3 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    // ---- sweep B: NaN/inf and range checks, the chunk's box in cell coordinates
    {
        uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
        for (int i0 = 0; i0 < cn; i0 += CS_HU * CS_THREADS) {
            Row3 q[CS_HU];
            cs_load_rows(rows, i0, cn, q);
#pragma unroll
            for (int u = 0; u < CS_HU; ++u) {
                const bool in = i0 + u * CS_THREADS + tid < cn;
                uint32_t cc[3];
                const bool ok = db_cell_coords(g, q[u].x, q[u].y, q[u].z, cc[0], cc[1], cc[2]);
                const bool fin = cs_row_check(q[u], in, ok, flags);
                if (in && fin && ok) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) { mn[a] = cc[a] < mn[a] ? cc[a] : mn[a]; mx[a] = cc[a] > mx[a] ? cc[a] : mx[a]; }
                }
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t lo_w = wave_reduce_min(mn[a]), hi_w = wave_reduce_max(mx[a]);
            if (l == 0) { atomicMin(&cbox[a], lo_w); atomicMax(&cbox[3 + a], hi_w); }
        }
    }
    __syncthreads();
    CS_STAMP();
    // widths of the relative key; rows outside the grid (the call fails for them) land on arbitrary digits
    const uint32_t ox = cbox[0], oy = cbox[1], oz = cbox[2];
    const bool any = cbox[3] >= ox && cbox[4] >= oy && cbox[5] >= oz;
    const int wx = any && cbox[3] > ox ? 32 - __clz(cbox[3] - ox) : 0;
    const int wy = any && cbox[4] > oy ? 32 - __clz(cbox[4] - oy) : 0;
    const int wz = any && cbox[5] > oz ? 32 - __clz(cbox[5] - oz) : 0;
    const int tb = wx + wy + wz;                         // <= bx + by + bz <= 32
    const int passes = (tb + 8) / 9;
    const int dbits = passes ? (tb + passes - 1) / passes : 1;
    const uint32_t mask = (1u << dbits) - 1u;
    const uint32_t gxm = (1u << g.bx) - 1u, gym = (1u << g.by) - 1u;
    auto relkey = [&](uint32_t k) -> uint32_t {
        const uint32_t cx = k & gxm, cy = (k >> g.bx) & gym, cz = k >> (g.bx + g.by);
        return (uint32_t)((((((uint64_t)(cz - oz)) << wy) | (uint64_t)(cy - oy)) << wx) | (uint64_t)(cx - ox));   // tb <= 32
    };
    // ---- sweep H: digit histograms of every pass
    for (int i0 = 0; i0 < cn; i0 += CS_HU * CS_THREADS) {  // workgroup-uniform trip count
        Row3 q[CS_HU];
        cs_load_rows(rows, i0, cn, q);
#pragma unroll
        for (int u = 0; u < CS_HU; ++u) {
            const bool in = i0 + u * CS_THREADS + tid < cn;
            bool ok;
            const uint32_t k = relkey(cs_cell_key(g, q[u].x, q[u].y, q[u].z, ok));
            if (in)
                for (int p = 0; p < passes; ++p) atomicAdd(&hist[p][l & (CS_HREP - 1)][(k >> (p * dbits)) & mask], 1u);
        }
    }
    __syncthreads();
    const bool isbad = flags[0] != 0;                   // the whole chunk stays noise: one cell, never core
    CS_STAMP();
    if (tid == 0) {
        bad[c] = isbad ? 1u : 0u;
        if (!isbad && flags[1]) atomicOr(status, 1u);
    }
    const uint64_t hi = cs_chunk_field(g, c);
    if (isbad || passes == 0) { cs_rows_in_place(g, rows, cn, lo, hi, isbad, pts, keys_out); return; }   // one cell
    // One pass, unswitched on what the compiler has to know statically: FIRST (the source rows are 12-byte input
    // rows), LAST (the full keys are written too) and, per tile, FULL (every lane holds a row).  In a full tile the
    // scattered stores are unconditional, so their number is a constant - and with it the wait for the NEXT tile's
    // rows, which are requested before them: the memory counter is one in-order queue of loads and stores, and a wait
    // that cannot count the stores behind a load drains them all (that drain, once per tile, was 40 % of the kernel).
    auto run_pass = [&](int p, auto FIRST_T, auto LAST_T) {
        constexpr bool FIRST = decltype(FIRST_T)::value, LAST = decltype(LAST_T)::value;
        const int shift = p * dbits;
        // pass p writes the sorted-rows array when an even number of passes follows, else the spare one
        const float4* __restrict__ src = ((passes - p) & 1) ? xbuf + lo : pts + lo;     // what pass p-1 wrote
        float4* __restrict__ dst = ((passes - 1 - p) & 1) ? xbuf + lo : pts + lo;
        // exclusive scan of this pass' histogram
        uint32_t hv = 0, incl = 0;
        if (tid < CS_BINS) {
            hv = 0;
#pragma unroll
            for (int r = 0; r < CS_HREP; ++r) hv += hist[p][r][tid];
            incl = wave_scan_incl(hv);
            if (l == 63) wsum[w] = incl;
        }
        __syncthreads();
        if (tid < CS_BINS) {
            uint32_t b = incl - hv;
            for (int w2 = 0; w2 < w; ++w2) b += wsum[w2];
            base[tid] = b;
        }
        __syncthreads();
        auto fetch = [&](int t0, float4 (&out)[CS_ROUNDS]) {
            const int seg = t0 + w * (64 * CS_ROUNDS);
#pragma unroll
            for (int r = 0; r < CS_ROUNDS; ++r) {
                const int i = seg + r * 64 + l;
                const int j = i < cn ? i : 0;
                if constexpr (FIRST) {
                    const Row3 q = rows[j];
                    out[r].x = q.x; out[r].y = q.y; out[r].z = q.z;
                    out[r].w = __uint_as_float((uint32_t)(lo + j));
                } else {
                    out[r] = src[j];
                }
            }
        };
        float4 nxt[CS_ROUNDS];
        auto tile = [&](int t0, auto FULL_T) {
            constexpr bool FULL = decltype(FULL_T)::value;
            float4 row[CS_ROUNDS];
            uint32_t key[CS_ROUNDS], rank[CS_ROUNDS];
            const int seg = t0 + w * (64 * CS_ROUNDS);
#pragma unroll
            for (int r = 0; r < CS_ROUNDS; ++r) row[r] = nxt[r];
            if (t0 + CS_TILE < cn) fetch(t0 + CS_TILE, nxt);        // in flight while this tile is ranked
#ifdef PCH_CS_STAMPS
            tlast = wall_clock64();
#endif
#pragma unroll
            for (int r = 0; r < CS_ROUNDS; ++r) {
                const bool valid = FULL || seg + r * 64 + l < cn;
                bool ok;
                key[r] = cs_cell_key(g, row[r].x, row[r].y, row[r].z, ok);
                const uint32_t d = (relkey(key[r]) >> shift) & mask;
                uint32_t np;
                const uint32_t rk = dbits <= 8 ? wave_match<8>(d, valid, np) : wave_match<9>(d, valid, np);
                const uint32_t prior = cnt[w][d];
                __builtin_amdgcn_wave_barrier();
                if (valid && rk == 0) cnt[w][d] = prior + np;
                __builtin_amdgcn_wave_barrier();
                rank[r] = prior + rk;
            }
            __syncthreads();
            CS_TILE_STAMP(0);
            if (tid < CS_BINS) {                        // digit tid: waves in order, counters cleared for the next tile
                uint32_t run = base[tid];
#pragma unroll
                for (int w2 = 0; w2 < CS_WAVES; ++w2) {
                    const uint32_t cc = cnt[w2][tid];
                    off[w2][tid] = run;
                    cnt[w2][tid] = 0;
                    run += cc;
                }
                base[tid] = run;
            }
            __syncthreads();
            CS_TILE_STAMP(1);
#pragma unroll
            for (int r = 0; r < CS_ROUNDS; ++r) {
                if (FULL || seg + r * 64 + l < cn) {
                    const uint32_t d = (relkey(key[r]) >> shift) & mask;
                    const uint32_t pos = off[w][d] + rank[r];
                    dst[pos] = row[r];
                    if constexpr (LAST) keys_out[lo + pos] = hi | key[r];
                }
            }
            // off[] is rewritten only behind the next tile's first barrier, which every wave reaches
            // after these reads
            CS_TILE_STAMP(2);
        };
        fetch(0, nxt);
        int t0 = 0;
        for (; t0 + CS_TILE <= cn; t0 += CS_TILE) tile(t0, std::true_type{});
        if (t0 < cn) tile(t0, std::false_type{});
        __syncthreads();                                // this pass' stores are visible to the whole workgroup
        CS_STAMP();
    };
    for (int p = 0; p < passes; ++p) {
        const bool first = p == 0, last = p == passes - 1;
        if (first && last) run_pass(p, std::true_type{}, std::true_type{});
        else if (first)    run_pass(p, std::true_type{}, std::false_type{});
        else if (last)     run_pass(p, std::false_type{}, std::true_type{});
        else               run_pass(p, std::false_type{}, std::false_type{});
    }
#ifdef PCH_CS_STAMPS
    __syncthreads();
    CS_STAMP();
    if (stamps && blockIdx.x == gridDim.x / 2 && threadIdx.x == 0) for (int k = 0; k < 3; ++k) stamps[8 + k] = tacc[k];
#endif
}

// ---- chunk-local counted scatter: the rows of one chunk grouped by cell, one workgroup per chunk ----------------
// A chunk holds few distinct cells (a 50 000-row corridor chunk 105-333, a uniform one up to ~2 800), so the rows are
// placed by a counting sort over the chunk's OWN cells instead of an LSD radix sort over 15-17-bit keys.  Sweep 1
// reads the rows, checks them (as db_chunksort_k's sweep B) and counts every cell in an open-addressing LDS table
// (CAS on the key word, per-lane atomics: 64 consecutive rows hold ~32 distinct cells, so wave aggregation does not
// pay).  Then the occupied slots are compacted, sorted by key (bitonic, sized by the cell count) and an exclusive
// scan of their counts in key order turns every count into the cell's first position.  Sweep 2 reads the rows again
// (the chunk was just read: L2 / MALL), looks the cell up and takes its position from the cell's cursor.  12 + 12
// bytes read, 16 + 8 written per row; the cell key is computed twice.  Rows of one cell are NOT in file order, and
// their order can change from run to run; no reader of the sorted rows depends on it.
// A chunk with more than CT_CELLS cells stops counting, sets ovf[c] and writes nothing else: db_chunksort_k, launched
// right behind with ovf as its gate, sorts it.  NaN/inf and one-cell chunks keep their rows in place, as db_chunksort_k does.
// TABLE (the run has at most DB_TABLE_MAX_CHUNKS chunks): the sorted cell list that the scan works on IS the chunk's
// part of the cell table, so it is staged - st.ncell[c], and at [lo, lo + ncell) the full keys in ascending order and
// every cell's first sorted position and smallest row (tmin: one more LDS atomic per row in sweep 1; it becomes cell_min,
// exact for a dense cell, corrected by db_core_k for a sparse one) - and no key is written per row: 16 bytes written per
// row instead of 24, one scattered store instead of two.  db_chunkcells_k and db_celltab_k (below) turn the staged lists
// into the table.
// Every chunk writes st.ncell[c] on every run (the workspace is not cleared): 0 for a chunk handed to db_chunksort_k.
// !TABLE: a full key per sorted row (keys_out), the table is read off those by db_heads_k / db_cells_k.
__device__ __forceinline__ uint32_t ct_hash(uint32_t k) { return (k * 0x9E3779B1u) >> (32 - CT_BITS); }

template <bool TABLE>
__global__ __launch_bounds__(CS_THREADS) void db_cellscatter_k(
    const float* __restrict__ xyz, int64_t n, DbGrid g, uint32_t* __restrict__ bad, uint32_t* __restrict__ ovf,
    float4* __restrict__ pts, uint64_t* __restrict__ keys_out, DbStage st, uint32_t* __restrict__ status,
    const DbHead* __restrict__ head) {
    if (!db_head_take(head, n, g)) return;              // (the fused call's unread launch: n and g from *head)
    __shared__ uint32_t tkey[CT_SLOTS];
    __shared__ uint32_t tcnt[CT_SLOTS];         // sweep 1: rows per cell; sweep 2: the cell's next position
    __shared__ uint32_t tmin[TABLE ? CT_SLOTS : 1];     // sweep 1: the cell's smallest row of the chunk
    __shared__ uint32_t skey[CT_CELLS];         // the chunk's cell keys, sorted
    __shared__ uint32_t wsum[CS_WAVES];
    __shared__ uint32_t flags[5];               // [0] NaN/inf, [1] point outside the grid, [2] cells, [3] too many
                                                // cells, [4] cells compacted so far
    const int tid = threadIdx.x, w = wave_id(), l = lane_id();
    const int64_t c = blockIdx.x;
    const int64_t lo = c * g.chunk_size;
    const int cn = (int)((n - lo) < g.chunk_size ? (n - lo) : g.chunk_size);
    const Row3* __restrict__ rows = reinterpret_cast<const Row3*>(xyz) + lo;
    for (int j = tid; j < CT_SLOTS; j += CS_THREADS) {
        tkey[j] = CT_EMPTY; tcnt[j] = 0u;
        if constexpr (TABLE) tmin[j] = 0xFFFFFFFFu;
    }
    if (tid < 5) flags[tid] = 0u;
    __syncthreads();
    // ---- sweep 1: checks, cell counts.  A row inserts only while flags[3] is clear, and at most one new key per
    // thread can be in flight when it is set, so the table holds at most CT_CELLS + CS_THREADS keys: a probe always
    // ends at its key or at an empty slot (the bound on the probe loop is never reached)
    for (int i0 = 0; i0 < cn; i0 += CS_HU * CS_THREADS) {
        if (__hip_atomic_load(&flags[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;   // too many cells
        Row3 q[CS_HU];
        cs_load_rows(rows, i0, cn, q);
#pragma unroll
        for (int u = 0; u < CS_HU; ++u) {
            const bool in = i0 + u * CS_THREADS + tid < cn;
            bool ok;
            const uint32_t k = cs_cell_key(g, q[u].x, q[u].y, q[u].z, ok);
            const bool fin = cs_row_check(q[u], in, ok, flags);
            if (in && fin && __hip_atomic_load(&flags[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u) {
                uint32_t h = ct_hash(k);
                for (int p = 0; p < CT_SLOTS; ++p, h = (h + 1u) & (CT_SLOTS - 1)) {
                    const uint32_t old = atomicCAS(&tkey[h], CT_EMPTY, k);
                    if (old == CT_EMPTY && atomicAdd(&flags[2], 1u) >= (uint32_t)CT_CELLS) flags[3] = 1u;
                    if (old == CT_EMPTY || old == k) {
                        atomicAdd(&tcnt[h], 1u);
                        if constexpr (TABLE) atomicMin(&tmin[h], (uint32_t)(i0 + u * CS_THREADS + tid));
                        break;
                    }
                }
            }
        }
    }
    __syncthreads();
    const bool isbad = flags[0] != 0u;                  // the whole chunk stays noise: one cell, never core
    const uint32_t ncell = flags[2];
    const bool over = !isbad && ncell > (uint32_t)CT_CELLS;
    if (tid == 0) {
        ovf[c] = over ? 1u : 0u;                        // written for every chunk: db_chunksort_k's gate
        if constexpr (TABLE) st.ncell[c] = over ? 0u : (isbad ? 1u : ncell);
        if (!over) {
            bad[c] = isbad ? 1u : 0u;
            if (!isbad && flags[1]) atomicOr(status, 1u);
        }
    }
    if (over) return;                                   // db_chunksort_k takes this chunk
    const uint64_t hi = cs_chunk_field(g, c);
    if (isbad || ncell == 1u) {                         // one cell
        if constexpr (TABLE) {
            // its key: cell 0 of a NaN/inf chunk, else the table's only key
            if (isbad) { if (tid == 0) st.key[lo] = hi; }
            else for (int j = tid; j < CT_SLOTS; j += CS_THREADS) if (tkey[j] != CT_EMPTY) st.key[lo] = hi | tkey[j];
            if (tid == 0) { st.start[lo] = (uint32_t)lo; st.minrow[lo] = (uint32_t)lo; }
        }
        cs_rows_in_place(g, rows, cn, lo, hi, isbad, pts, TABLE ? nullptr : keys_out);
        return;
    }
    // ---- the occupied slots, compacted (in any order) and padded to a power of two ...
    const int P = 1 << (32 - __clz((int)ncell - 1));    // 2 <= P <= CT_CELLS
    for (int j0 = 0; j0 < CT_SLOTS; j0 += CS_THREADS) {
        const uint32_t k = tkey[j0 + tid];
        const uint64_t m = __ballot(k != CT_EMPTY);
        uint32_t base = 0;
        if (l == 0 && m) base = atomicAdd(&flags[4], (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, 0, 64);
        if (k != CT_EMPTY) skey[base + (uint32_t)__popcll(m & lanemask_lt())] = k;
    }
    for (int j = (int)ncell + tid; j < P; j += CS_THREADS) skey[j] = CT_EMPTY;
    __syncthreads();
    // ... sorted by key (bitonic; keys are distinct) ...
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += CS_THREADS) {
                const int a = 2 * t - (t & (j - 1)), b = a + j;
                const uint32_t ka = skey[a], kb = skey[b];
                if ((ka > kb) == ((a & k) == 0)) { skey[a] = kb; skey[b] = ka; }
            }
            __syncthreads();
        }
    }
    // ... and their counts scanned in that order: tcnt[slot] becomes the cell's first position.  Thread t owns the
    // cells 4t .. 4t+3 of the sorted list (P <= 4 * CS_THREADS)
    {
        uint32_t slot[4], cnt[4], sum = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = 4 * tid + u;
            slot[u] = 0; cnt[u] = 0;
            if (j < (int)ncell) {
                const uint32_t k = skey[j];
                uint32_t h = ct_hash(k);
                for (int p = 0; p < CT_SLOTS && tkey[h] != k; ++p) h = (h + 1u) & (CT_SLOTS - 1);
                slot[u] = h;
                cnt[u] = tcnt[h];
            }
            sum += cnt[u];
        }
        const uint32_t incl = wave_scan_incl(sum);
        if (l == 63) wsum[w] = incl;
        __syncthreads();
        uint32_t run = incl - sum;
        for (int w2 = 0; w2 < w; ++w2) run += wsum[w2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (4 * tid + u < (int)ncell) {
                tcnt[slot[u]] = run;                    // only this thread touches these slots
                if constexpr (TABLE) {                  // ncell <= cn: the chunk's own part of the staging arrays
                    st.key[lo + 4 * tid + u] = hi | skey[4 * tid + u];
                    st.start[lo + 4 * tid + u] = (uint32_t)(lo + run);
                    st.minrow[lo + 4 * tid + u] = (uint32_t)lo + tmin[slot[u]];
                }
            }
            run += cnt[u];
        }
    }
    __syncthreads();
    // ---- sweep 2: every row to its cell's next position
    for (int i0 = 0; i0 < cn; i0 += CS_HU * CS_THREADS) {
        Row3 q[CS_HU];
        cs_load_rows(rows, i0, cn, q);
#pragma unroll
        for (int u = 0; u < CS_HU; ++u) {
            const int i = i0 + u * CS_THREADS + tid;
            if (i < cn) {
                bool ok;
                const uint32_t k = cs_cell_key(g, q[u].x, q[u].y, q[u].z, ok);
                uint32_t h = ct_hash(k);
                for (int p = 0; p < CT_SLOTS && tkey[h] != k; ++p) h = (h + 1u) & (CT_SLOTS - 1);
                const uint32_t pos = atomicAdd(&tcnt[h], 1u);
                if (pos >= (uint32_t)cn) continue;      // cannot happen (every row was counted): never write outside
                float4 o4;
                o4.x = q[u].x; o4.y = q[u].y; o4.z = q[u].z; o4.w = __uint_as_float((uint32_t)(lo + i));
                pts[lo + pos] = o4;
                if constexpr (!TABLE) keys_out[lo + pos] = hi | k;
            }
        }
    }
}

// ---- cells of the sorted rows.  A row is a cell head when its key differs from the key in front of it; nobody
// materialises those flags: db_heads_k counts them per SCAN_TILE rows, scan_tile_sums_u32 turns the counts into tile
// offsets (and the number of cells), and db_cells_k scans its tile again while it writes what depends on the cell
// index.  (Until round 3 the sort kernels wrote a flag per row, a three-launch scan rewrote it and db_cells_k read
// it back - and the chunk sort's own flag sweep ran on 196 workgroups.)
constexpr int DC_ITEMS = SCAN_TILE / DB_THREADS;          // 8 consecutive rows per thread
static_assert(DC_ITEMS == 8, "two 64-byte key loads per thread");

__device__ __forceinline__ void dc_load_keys(const uint64_t* __restrict__ keys, int64_t base, int64_t n,
                                             uint64_t (&k)[DC_ITEMS], uint64_t& prev) {
    if (base + DC_ITEMS <= n) {
        const ulonglong2* q = reinterpret_cast<const ulonglong2*>(keys + base);     // base is a multiple of 8
#pragma unroll
        for (int j = 0; j < DC_ITEMS / 2; ++j) { const ulonglong2 v = q[j]; k[2 * j] = v.x; k[2 * j + 1] = v.y; }
    } else {
#pragma unroll
        for (int j = 0; j < DC_ITEMS; ++j) k[j] = base + j < n ? keys[base + j] : 0ull;
    }
    prev = (base > 0 && base < n) ? keys[base - 1] : 0ull;
}

__global__ __launch_bounds__(DB_THREADS) void db_heads_k(const uint64_t* __restrict__ keys, int64_t n,
                                                         uint32_t* __restrict__ tile_sums) {
    __shared__ uint32_t wsum[DB_WAVES];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * DC_ITEMS;
    uint64_t k[DC_ITEMS], prev;
    dc_load_keys(keys, base, n, k, prev);
    uint32_t heads = 0;
#pragma unroll
    for (int j = 0; j < DC_ITEMS; ++j) {
        const int64_t i = base + j;
        heads += (i < n && (i == 0 || k[j] != (j ? k[j - 1] : prev))) ? 1u : 0u;
    }
    heads = wave_reduce_add(heads);
    if (lane_id() == 0) wsum[wave_id()] = heads;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < DB_WAVES; ++w) t += wsum[w];
        tile_sums[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(DB_THREADS) void db_cells_k(const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ tile_excl, int64_t n,
                                                         int sh, int64_t nchunks,
                                                         uint32_t* __restrict__ cid,
                                                         uint32_t* __restrict__ cell_start,
                                                         uint64_t* __restrict__ cell_key,
                                                         uint32_t* __restrict__ chunk_cells,
                                                         uint32_t* __restrict__ cell_acc) {
    __shared__ uint32_t wsum[DB_WAVES];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * DC_ITEMS;
    uint64_t k[DC_ITEMS], prev;
    dc_load_keys(keys, base, n, k, prev);
    bool hd[DC_ITEMS];
    uint32_t heads = 0;
#pragma unroll
    for (int j = 0; j < DC_ITEMS; ++j) {
        const int64_t i = base + j;
        hd[j] = i < n && (i == 0 || k[j] != (j ? k[j - 1] : prev));
        heads += hd[j] ? 1u : 0u;
    }
    const uint32_t incl = wave_scan_incl(heads);
    if (lane_id() == 63) wsum[wave_id()] = incl;
    __syncthreads();
    uint32_t c = tile_excl[blockIdx.x] + incl - heads;           // heads in front of this thread's first row
    for (int w = 0; w < wave_id(); ++w) c += wsum[w];
    uint32_t cc[DC_ITEMS];
#pragma unroll
    for (int j = 0; j < DC_ITEMS; ++j) {
        const int64_t i = base + j;
        c += hd[j] ? 1u : 0u;
        cc[j] = c - 1u;                                          // cell of row i (row 0 is a head, so c >= 1)
        if (hd[j]) {
            const uint64_t key = k[j], pk = j ? k[j - 1] : prev;
            cell_start[cc[j]] = (uint32_t)i;
            cell_key[cc[j]] = key;
            uint4* a4 = reinterpret_cast<uint4*>(cell_acc + 8 * (int64_t)cc[j]);   // neutral start of db_cellstats_k
            a4[0] = make_uint4(0u, 0u, 0u, 0u);
            a4[1] = make_uint4(0u, 0u, 0u, 0u);
            const uint64_t ch = sh < 64 ? key >> sh : 0, pch = sh < 64 ? pk >> sh : 0;
            if (i == 0 || ch != pch) chunk_cells[ch] = cc[j];    // every chunk holds rows, hence cells
        }
        if (i == n - 1) { cell_start[cc[j] + 1] = (uint32_t)n; chunk_cells[nchunks] = cc[j] + 1; }
    }
    if (base + DC_ITEMS <= n) {
        uint4* o = reinterpret_cast<uint4*>(cid + base);
        o[0] = make_uint4(cc[0], cc[1], cc[2], cc[3]);
        o[1] = make_uint4(cc[4], cc[5], cc[6], cc[7]);
    } else {
#pragma unroll
        for (int j = 0; j < DC_ITEMS; ++j)
            if (base + j < n) cid[base + j] = cc[j];
    }
}
// ---- the cell table from the lists that db_cellscatter_k<true> staged: no key per row is written or read ----------
// db_chunkcells_k (one workgroup) scans the chunks' cell counts into chunk_cells, which makes every staged cell's
// global index chunk_cells[c] + j, and says in *route whether a chunk overflowed.  db_celltab_k (behind the neighbour
// rows, which it also finds) then runs over the chunks' lists.  *route clear: it writes the table.  *route set (some
// chunk went through db_chunksort_k, which writes keys): it writes the keys of all OTHER chunks' rows instead, and
// the host, which reads the word in the wait it makes anyway, launches db_heads_k / db_cells_k on them.
constexpr int CC_THREADS = 1024;
constexpr int CC_ITEMS = (int)(DB_TABLE_MAX_CHUNKS / CC_THREADS);     // consecutive chunks per thread

// cells staged for chunk c of cn rows.  db_cellscatter_k<true> writes the word for every chunk on every run and a chunk
// has at most one cell per row, so the minimum never changes a value: it is purely a guard that keeps the reads of the
// staging arrays and the writes of the table inside them should a writer ever break that
__device__ __forceinline__ uint32_t ct_staged_cells(const uint32_t* __restrict__ ncell, int64_t c, int64_t cn) {
    const uint32_t v = ncell[c];
    return v < (uint32_t)cn ? v : (uint32_t)cn;
}

__global__ __launch_bounds__(CC_THREADS) void db_chunkcells_k(
    const uint32_t* __restrict__ ncell, const uint32_t* __restrict__ ovf, int nchunks, int64_t n, int64_t chunk_size,
    uint32_t* __restrict__ chunk_cells, uint32_t* __restrict__ cell_start, uint32_t* __restrict__ ncells,
    uint32_t* __restrict__ route, DbHead* __restrict__ head, const uint32_t* __restrict__ status) {
    if (head) {                                         // the fused call's unread launch
        if (head->go == 0u) return;
        nchunks = head->nchunks; n = head->n; chunk_size = head->g.chunk_size;
    }
    __shared__ uint32_t wsum[CC_THREADS / 64];
    const int tid = threadIdx.x, c0 = tid * CC_ITEMS;
    uint32_t v[CC_ITEMS], sum = 0;
    int over = 0;
#pragma unroll
    for (int u = 0; u < CC_ITEMS; ++u) {
        const int c = c0 + u;
        v[u] = 0u;
        if (c < nchunks) {
            const int64_t lo = (int64_t)c * chunk_size;
            v[u] = ct_staged_cells(ncell, c, (n - lo) < chunk_size ? (n - lo) : chunk_size);
            over |= ovf[c] != 0u;
        }
        sum += v[u];
    }
    over = __syncthreads_or(over);
    const uint32_t incl = wave_scan_incl(sum);
    if (lane_id() == 63) wsum[wave_id()] = incl;
    __syncthreads();
    uint32_t run = incl - sum, total = 0;
    for (int w = 0; w < CC_THREADS / 64; ++w) { if (w < wave_id()) run += wsum[w]; total += wsum[w]; }
#pragma unroll
    for (int u = 0; u < CC_ITEMS; ++u) {
        if (c0 + u < nchunks) chunk_cells[c0 + u] = run;
        run += v[u];
    }
    if (tid == 0) {
        *route = over ? 1u : 0u;
        if (!over) {                                    // else db_cells_k's to write
            chunk_cells[nchunks] = total;
            cell_start[total] = (uint32_t)n;            // total <= n
            *ncells = total;
        }
        // the words the host reads in front of db_celltab_k, beside the plan: one copy brings both
        if (head) { head->status = *status; head->ncells = over ? 0u : total; head->route = over ? 1u : 0u; }
    }
}

// ---- the chunk route's cell table per CELL: one workgroup per chunk (the host does not know the cell count yet) over
// the chunk's staged list [lo, lo + ncell).
// *route clear: cell_start, cell_key and cell_min of the chunk's cells, the chunk's words of the row bitmap cleared
// (two chunks may share a word: both store 0), and the cells' neighbour rows, db_rowtab_k's 25 searches per cell, over
// an LDS copy of the chunk's keys - no word per row: the staged route's labels need no cid (db_filelabel_k).
// *route set (fill mode): a chunk that did not overflow writes the keys of its own rows, a wave
// per cell; an overflowed one returns at once.
__global__ __launch_bounds__(CS_THREADS) void db_celltab_k(
    const uint32_t* __restrict__ route, DbStage st, const uint32_t* __restrict__ ovf, DbGrid g, int64_t n,
    uint32_t* __restrict__ cell_start, uint64_t* __restrict__ cell_key, int* __restrict__ cell_min,
    uint32_t* __restrict__ bits, int2* __restrict__ rowtab, int64_t rowtab_cells, uint64_t* __restrict__ keys_out,
    const DbHead* __restrict__ head) {
    if (!db_head_take(head, n, g)) return;              // (the fused call's unread launch: n and g from *head)
    __shared__ uint32_t key[CT_CELLS];
    const int tid = threadIdx.x, l = lane_id();
    const int64_t c = blockIdx.x, lo = c * g.chunk_size;
    const int64_t end = lo + g.chunk_size < n ? lo + g.chunk_size : n;
    const bool fill = *route != 0u;                        // uniform over the grid
    if (fill && ovf[c] != 0u) return;                      // db_chunksort_k wrote this chunk's keys
    int nc = (int)ct_staged_cells(st.ncell, c, end - lo);
    nc = nc > CT_CELLS ? CT_CELLS : nc;                    // what db_cellscatter_k stages never exceeds it
    if (fill) {
        for (int j = wave_id(); j < nc; j += CS_WAVES) {
            int64_t a = st.start[lo + j], b = j + 1 < nc ? (int64_t)st.start[lo + j + 1] : end;
            a = a < lo ? lo : a;
            b = b > end ? end : b;
            const uint64_t k = st.key[lo + j];
            for (int64_t i = a + l; i < b; i += 64) keys_out[i] = k;
        }
        return;
    }
    const int64_t cell0 = g.chunk_cells[c];
    if (cell0 + nc > n) return;                            // cannot happen (a cell per row at most): never write outside
    for (int64_t wd = (lo >> 5) + tid; wd <= ((end - 1) >> 5); wd += CS_THREADS) bits[wd] = 0u;
    if (tid < nc) {
        const uint64_t k = st.key[lo + tid];
        cell_start[cell0 + tid] = st.start[lo + tid];
        cell_key[cell0 + tid] = k;
        cell_min[cell0 + tid] = (int)st.minrow[lo + tid];  // of all its rows: db_core_k corrects it for a sparse cell
        const int sh = g.bx + g.by + g.bz;                 // <= 31 on this route
        key[tid] = (uint32_t)k & ((1u << sh) - 1u);
    }
    if (!rowtab) return;
    __syncthreads();
    for (int t = tid; t < 32 * nc; t += CS_THREADS) {      // db_row_run on the chunk's own keys
        const int j = t >> 5, row = t & 31;
        if (row >= DB_ROWS || cell0 + j >= rowtab_cells) continue;
        int2 v;
        v.x = 0; v.y = 0;
        DbRowAt at;
        if (db_row_at(g, key[j], row, at)) {
            v = db_run_in(key, nc, (uint32_t)db_pack(g, 0, (uint64_t)at.nz, (uint64_t)at.ny, (uint64_t)at.xlo),
                          (uint32_t)db_pack(g, 0, (uint64_t)at.nz, (uint64_t)at.ny, (uint64_t)at.xhi));
            v.x += (int)cell0;
            v.y += (int)cell0;
        }
        rowtab[(cell0 + j) * DB_ROWS + row] = v;
    }
}

// ---- the head of stage C planned on the device (DbHead, pch_dbscan.h): one workgroup behind stage B's first results.
// go is set when dbscan_run, reading the same words, would take the staged chunk route; the workgroup then zeroes what
// db_sorted_keys clears with a fill.  go clear: nothing but *head is written - the fallback sweep of stage B may still
// need its scratch, which shares the workspace.
constexpr int HP_THREADS = 256;
__global__ __launch_bounds__(HP_THREADS) void db_headplan_k(DbHeadArgs a, DbGrid g, DbHead* __restrict__ head) {
    __shared__ uint32_t sgo;
    __shared__ int snchunks;
    if (threadIdx.x == 0) {
        const int64_t n = *a.count;
        float box[6];
        for (int k = 0; k < 6; ++k) box[k] = a.aabb[k];
        bool go = a.scalars[5] == 0.0f && n > 0 && n <= a.plan_n;
        const int64_t cs = (a.chunk_size <= 0 || a.chunk_size > n) ? n : a.chunk_size;     // as dbscan_run
        const int64_t nchunks = go ? (n + cs - 1) / cs : 0;
        g.chunk_size = cs;
        int cellbits = 0, nbits = 0;
        go = go && db_box_finite(box);
        if (go) go = !db_plan_grid(box, nchunks, g, cellbits, nbits);
        go = go && cellbits <= 31 && cs <= CS_MAX_CHUNK && a.sort_mode != 2 &&
             (a.sort_mode == 1 || nchunks >= CS_MIN_CHUNKS) && nchunks <= DB_TABLE_MAX_CHUNKS;
        head->go = go ? 1u : 0u;
        head->nchunks = go ? (int32_t)nchunks : 0;
        head->n = n;
        head->cellbits = cellbits; head->nbits = nbits;
        head->status = 0u; head->ncells = 0u; head->route = 0u; head->pad = 0u;
        head->g = g;
        sgo = go ? 1u : 0u;
        snchunks = go ? (int)nchunks : 0;
    }
    __syncthreads();
    if (sgo == 0u) return;
    // DbWs::clear_bytes(nchunks): a.clear_from is 16-byte aligned and the arrays behind chunk_cells[nchunks] go on
    const size_t bytes = ((size_t)((char*)(a.chunk_cells + snchunks + 1) - (char*)a.clear_from) + 15) & ~size_t(15);
    uint4* const z = reinterpret_cast<uint4*>(a.clear_from);
    for (size_t i = threadIdx.x; i < bytes / 16; i += HP_THREADS) z[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- host side ----
int db_head_launch(const float* xyz, const DbHeadArgs& a, const DbGrid& proto, const DbWs& w, DbHead* head,
                   const void* peek_dev, size_t peek_bytes, hipStream_t s) {
    // grids for the most chunks a.plan_n rows make; the workgroups beyond the device's nchunks return at once
    const int64_t cap_chunks = (a.chunk_size <= 0 || a.chunk_size > a.plan_n) ? 1 : ceil_div(a.plan_n, a.chunk_size);
    const dim3 gh((unsigned)cap_chunks), blk(CS_THREADS);
    PCH_LAUNCH("db_headplan", db_headplan_k, dim3(1), dim3(HP_THREADS), 0, s, a, proto, head);
    // (n, the grid and the chunk counts passed by value are not read: *head overrides them)
    PCH_LAUNCH("db_cellscatter", db_cellscatter_k<true>, gh, blk, 0, s, xyz, a.plan_n, proto, w.chunk_bad, w.chunk_ovf,
               w.pts, w.k1, w.stage, &w.meta->status, (const DbHead*)head);
    PCH_LAUNCH("db_chunksort", db_chunksort_k, gh, blk, 0, s, xyz, a.plan_n, proto, w.chunk_ovf, w.chunk_bad, w.xbuf,
               w.pts, w.k1, &w.meta->status, w.cs_stamps, (const DbHead*)head);
    PCH_LAUNCH("db_chunkcells", db_chunkcells_k, dim3(1), dim3(CC_THREADS), 0, s, w.stage.ncell, w.chunk_ovf,
               (int)cap_chunks, a.plan_n, proto.chunk_size, w.chunk_cells, w.cell_start, &w.meta->ncells, w.cell_route,
               head, (const uint32_t*)&w.meta->status);
    PCH_TRY(peek_enqueue(peek_dev, peek_bytes, s));
    PCH_LAUNCH("db_celltab", db_celltab_k, gh, blk, 0, s, w.cell_route, w.stage, w.chunk_ovf, proto, a.plan_n,
               w.cell_start, w.cell_key, w.cell_min, w.bits, w.rowtab, w.rowtab_cells, w.k1, (const DbHead*)head);
    return PCH_OK;
}
int db_first_bad(const float* xyz, int64_t n, unsigned long long* first, hipStream_t s) {
    PCH_LAUNCH("db_first_bad", db_first_bad_k, dim3(db_stride_blocks(n)), dim3(DB_THREADS), 0, s, xyz, n, first);
    return PCH_OK;
}

// key beyond 64 bits, one chunk: compressed cell coordinates per axis (w.comp, see dbc_axis_keys_k) and the grid's
// mx..bz / cellbits over them.  done: the outputs are written
int db_compress(const DbRun& r, DbGrid& g, int& cellbits, bool& done) {
    const DbWs& w = r.w; const hipStream_t s = r.s; const int64_t n = r.n;
    const unsigned gn = (unsigned)ceil_div(n, DB_THREADS);
    PCH_HIP_TRY(hipMemsetAsync(&w.meta->first_bad, 0xFF, sizeof(int64_t), s));
    PCH_TRY(db_first_bad(r.xyz, n, reinterpret_cast<unsigned long long*>(&w.meta->first_bad), s));
    PCH_HIP_TRY(hipMemsetAsync(&w.meta->status, 0, offsetof(DbMeta, first_bad) - offsetof(DbMeta, status), s));
    for (int axis = 0; axis < 3; ++axis) {
        PCH_LAUNCH("dbc_axis_keys", dbc_axis_keys_k, dim3(gn), dim3(DB_THREADS), 0, s, r.xyz, n, axis, w.k0, w.v0);
        PCH_TRY(radix_sort_pairs(w.k0, w.v0, w.k1, w.v1, n, 32, w.radix_ws, s));
        const bool in1 = radix_sort_result_buffer(32) == 1;
        const uint64_t* ksa = in1 ? w.k1 : w.k0;
        const uint32_t* vsa = in1 ? w.v1 : w.v0;
        PCH_LAUNCH("dbc_heads", dbc_heads_k, dim3(gn), dim3(DB_THREADS), 0, s, ksa, n, g.inv_cell, w.flag2);
        PCH_TRY(scan_exclusive_u32(w.flag2, w.head, n, w.scan_ws, nullptr, s));
        PCH_HIP_TRY(hipMemsetAsync(w.cell_start, 0, sizeof(uint32_t) * (size_t)(n + 8), s));
        for (int phase = 0; phase < 2; ++phase)
            PCH_LAUNCH("dbc_local", dbc_local_k, dim3(gn), dim3(DB_THREADS), 0, s, ksa, w.flag2, w.head, n, g.inv_cell,
                       w.cell_box, phase, w.cid, w.cell_start, &w.meta->status);
        PCH_TRY(scan_exclusive_u32(w.cell_start, w.cell_start, n, w.scan_ws, nullptr, s));
        PCH_LAUNCH("dbc_comp", dbc_comp_k, dim3(gn), dim3(DB_THREADS), 0, s, vsa, w.flag2, w.head, w.cid, w.cell_start,
                   n, axis, w.comp, w.meta->comp_max);
    }
    DbMeta back;                             // status .. first_bad
    PCH_HIP_TRY(hipMemcpyAsync(&back.status, &w.meta->status, offsetof(DbMeta, pad) - offsetof(DbMeta, status),
                               hipMemcpyDeviceToHost, s));
    PCH_HIP_TRY(hipStreamSynchronize(s));
    if (back.first_bad >= 0) {               // NaN / inf in a single fit: sklearn rejects it, everything stays noise
        PCH_TRY(db_all_noise(r));
        g_last.ws = nullptr;
        done = true;
        return PCH_OK;
    }
    if (back.status != 0) { set_error("compressed cell coordinates out of range"); return PCH_ERR_RANGE; }
    cellbits = db_cell_bits(g, (int)back.comp_max[0], (int)back.comp_max[1], (int)back.comp_max[2]);
    if (cellbits > 64) {
        set_error("cell key needs %d bits even with compressed coordinates (%lld isolated points?)", cellbits, (long long)n);
        return PCH_ERR_RANGE;
    }
    return PCH_OK;
}

// the cell keys in sorted order (ks) and the points in that order (w.pts)
int db_sorted_keys(const DbRun& r, const DbGrid& g, int cellbits, int nbits, bool compressed, int sort_mode,
                   const uint64_t*& ks, bool& staged) {
    const DbWs& w = r.w; const hipStream_t s = r.s; const int64_t n = r.n, nchunks = r.nchunks;
    const unsigned gn = (unsigned)ceil_div(n, DB_THREADS);
    PCH_HIP_TRY(hipMemsetAsync(w.clear_from(), 0, w.clear_bytes(nchunks), s));
    staged = false;
    // One workgroup per chunk only pays with enough chunks to fill the GPU (measured break-even near
    // 100 chunks of 50 000 rows); PCH_DBSCAN_SORT=chunk / global forces a path (tests compare them)
    if (!compressed && cellbits <= 31 && r.chunk_size <= CS_MAX_CHUNK && sort_mode != 2 &&
        (sort_mode == 1 || nchunks >= CS_MIN_CHUNKS)) {
        // chunk-local path: one workgroup per chunk builds keys, groups the rows by cell and writes them; a chunk with
        // more cells than db_cellscatter_k's table takes goes through db_chunksort_k (gated by chunk_ovf: no host read).
        // staged: the chunks leave their cell lists instead of a key per row (db_chunkcells_k's single workgroup
        // bounds the number of chunks); db_cell_table takes the table from them unless a chunk overflowed
        staged = nchunks <= DB_TABLE_MAX_CHUNKS;
        const auto cellscatter = staged ? db_cellscatter_k<true> : db_cellscatter_k<false>;
        PCH_LAUNCH("db_cellscatter", cellscatter, dim3((unsigned)nchunks), dim3(CS_THREADS), 0, s, r.xyz, n, g,
                   w.chunk_bad, w.chunk_ovf, w.pts, w.k1, w.stage, &w.meta->status, (const DbHead*)nullptr);
        PCH_LAUNCH("db_chunksort", db_chunksort_k, dim3((unsigned)nchunks), dim3(CS_THREADS), 0, s, r.xyz, n, g,
                   w.chunk_ovf, w.chunk_bad, w.xbuf, w.pts, w.k1, &w.meta->status, w.cs_stamps, (const DbHead*)nullptr);
        if (staged)
            PCH_LAUNCH("db_chunkcells", db_chunkcells_k, dim3(1), dim3(CC_THREADS), 0, s, w.stage.ncell, w.chunk_ovf,
                       (int)nchunks, n, r.chunk_size, w.chunk_cells, w.cell_start, &w.meta->ncells, w.cell_route,
                       (DbHead*)nullptr, (const uint32_t*)nullptr);
#ifdef PCH_CS_STAMPS
        {
            unsigned long long t[11];                    // start | sweep B | sweep H | one per pass | heads
            PCH_HIP_TRY(hipStreamSynchronize(s));
            PCH_HIP_TRY(hipMemcpy(t, w.cs_stamps, sizeof(t), hipMemcpyDeviceToHost));
            for (int q = 1; q <= 6; ++q)
                fprintf(stderr, "chunksort phase %d: %.2f us\n", q, (double)(long long)(t[q] - t[q - 1]) / 100.0);
            fprintf(stderr, "chunksort tiles: rank %.2f us, offsets %.2f us, scatter %.2f us\n", (double)t[8] / 100.0,
                    (double)t[9] / 100.0, (double)t[10] / 100.0);
        }
#endif
        ks = w.k1;
        return PCH_OK;
    }
    // compressed or global: keys, one radix sort of all rows, gather
    PCH_HIP_TRY(hipMemsetAsync(w.chunk_bad, 0, sizeof(uint32_t) * (size_t)(nchunks + 1), s));
    if (compressed) {
        PCH_LAUNCH("db_keys_comp", db_keys_comp_k, dim3(gn), dim3(DB_THREADS), 0, s, w.comp, n, g, w.k0, w.v0);
    } else {
        PCH_LAUNCH("db_chunkbad", db_chunkbad_k, dim3(db_stride_blocks(n)), dim3(DB_THREADS), 0, s, r.xyz, n,
                   r.chunk_size, w.chunk_bad);
        PCH_LAUNCH("db_keys", db_keys_k, dim3(gn), dim3(DB_THREADS), 0, s, r.xyz, n, g, w.chunk_bad, w.k0, w.v0,
                   &w.meta->status);
    }
    PCH_TRY(radix_sort_pairs(w.k0, w.v0, w.k1, w.v1, n, nbits, w.radix_ws, s));
    const bool in1 = radix_sort_result_buffer(nbits) == 1;
    ks = in1 ? w.k1 : w.k0;
    PCH_LAUNCH("db_gather", db_gather_k, dim3(gn), dim3(DB_THREADS), 0, s, r.xyz, ks, in1 ? w.v1 : w.v0, n, w.pts);
    return PCH_OK;
}

// the cells of the sorted keys: the cell table (on the staged route the row table, cell_min and the cleared row bitmap
// too).  back: the host's copy of status, ncells and the route word (set: the table was read off the keys)
int db_cell_table(const DbRun& r, const DbGrid& g, int cellbits, const uint64_t* ks, bool staged, DbMeta& back,
                  const DbHead* head) {
    const DbWs& w = r.w; const hipStream_t s = r.s; const int64_t n = r.n;
    const int64_t ntile = ceil_div(n, (int64_t)SCAN_TILE);
    // the cell count sizes the next grids: fetch it while the kernel that writes the table (sized by n) runs
    constexpr size_t peek_bytes = offsetof(DbMeta, pad) + sizeof(uint32_t) - offsetof(DbMeta, status);
    back.pad[0] = 1u;
    if (head) {                              // db_head_launch queued db_celltab_k; the words came with the plan
        back.status = head->status; back.ncells = head->ncells; back.pad[0] = head->route;
    } else if (staged) {
        // db_chunkcells_k left ncells and the route word; db_celltab_k reads the word itself and writes either the
        // table (and the row table) or the keys that db_chunksort_k did not (then the table is read off the keys
        // below, as ever)
        PCH_TRY(peek_enqueue(&w.meta->status, peek_bytes, s));
        PCH_LAUNCH("db_celltab", db_celltab_k, dim3((unsigned)r.nchunks), dim3(CS_THREADS), 0, s, w.cell_route, w.stage,
                   w.chunk_ovf, g, n, w.cell_start, w.cell_key, w.cell_min, w.bits, w.rowtab, w.rowtab_cells, w.k1,
                   (const DbHead*)nullptr);
        PCH_TRY(peek_wait(&back.status, peek_bytes));
    }
    if (back.pad[0] != 0u) {
        PCH_LAUNCH("db_heads", db_heads_k, dim3((unsigned)ntile), dim3(DB_THREADS), 0, s, ks, n, w.scan_ws);
        PCH_TRY(scan_tile_sums_u32(w.scan_ws, ntile, &w.meta->ncells, s));
        PCH_TRY(peek_enqueue(&w.meta->status, 2 * sizeof(uint32_t), s));
        PCH_LAUNCH("db_cells", db_cells_k, dim3((unsigned)ntile), dim3(DB_THREADS), 0, s, ks, w.scan_ws, n, cellbits,
                   r.nchunks, w.cid, w.cell_start, w.cell_key, w.chunk_cells, w.cell_acc);
        PCH_TRY(peek_wait(&back.status, 2 * sizeof(uint32_t)));
    }
    if (back.status != 0) {
        set_error("finite coordinates outside the supplied bounding box");
        return PCH_ERR_ARG;
    }
    return PCH_OK;
}

}  // namespace pch
