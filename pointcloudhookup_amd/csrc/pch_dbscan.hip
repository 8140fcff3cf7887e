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
#include <assert.h>
#include "pch_prims.h"
#include "pch_unionfind.h"

namespace pch {

constexpr int DB_THREADS = 256;
constexpr int DB_WAVES   = DB_THREADS / 64;
constexpr int DB_ROWS    = 25;
constexpr int INT_BIG    = 0x7fffffff;
constexpr int DB_FEW_QUERIES = 24;
constexpr int DB_AHEAD = 3;              // db_core_k, long sweeps: 64-candidate groups whose loads are in flight together
constexpr long long DB_LONG_TOT = 8192;  // ... a cell counts as long from this many candidates in its neighbourhood
constexpr int DB_SEGS = 43;          // 9 inner + 9 + 9 end pieces of the near runs + 16 outer runs

struct DbGrid {
    float   ox, oy, oz;          // grid origin (lower corner of the bounding box)
    double  cell;                // cell side s
    double  inv_cell;            // 1/s: cell index = floor((x - origin) * inv_cell); the 2^-16 slack in s
                                 // covers the rounding of this product (< 2^-21 cells for indices < 2^31)
    double  eps2;                // eps*eps (sklearn _dist_to_rdist)
    float   eps2_lo, eps2_hi;    // float32 pre-filter: d32 <= lo is surely inside, d32 >= hi surely outside
    int     bx, by, bz;          // key bits per axis
    int     mx, my, mz;          // largest valid cell coordinate per axis
    int64_t chunk_size;
    const uint32_t* chunk_bad;   // != 0: the chunk holds NaN/inf and stays noise as a whole
    const uint32_t* chunk_cells; // [chunks + 1] first cell of every chunk (cells are sorted by chunk first)
    int     min_samples;
};

// (dy,dz) rows ordered by distance so that early exits trigger as soon as possible
__constant__ int8_t DB_ROW_DY[DB_ROWS] = {0, 1, -1, 0, 0, 1, 1, -1, -1, 2, -2, 0, 0,
                                          2, 2, -2, -2, 1, 1, -1, -1, 2, 2, -2, -2};
__constant__ int8_t DB_ROW_DZ[DB_ROWS] = {0, 0, 0, 1, -1, 1, -1, 1, -1, 0, 0, 2, -2,
                                          1, -1, 1, -1, 2, -2, 2, -2, 2, -2, 2, -2};

__device__ __forceinline__ uint64_t db_pack(const DbGrid& g, uint64_t chunk, uint64_t cz,
                                            uint64_t cy, uint64_t cx) {
    return ((((chunk << g.bz) | cz) << g.by | cy) << g.bx) | cx;
}

__device__ __forceinline__ double db_d2(const float4& q, const float4& p) {
    // euclidean_rdist: tmp = x1[j] - x2[j]; d += tmp * tmp   (float64, j = 0,1,2)
    const double dx = (double)q.x - (double)p.x;
    const double dy = (double)q.y - (double)p.y;
    const double dz = (double)q.z - (double)p.z;
    double d = dx * dx;
    d += dy * dy;
    d += dz * dz;
    return d;
}
__device__ __forceinline__ bool db_within(const float4& q, const float4& p, double eps2) {
    return db_d2(q, p) <= eps2;
}

// Same predicate, cheaper: the float32 value d32 of the squared distance carries a relative error
// below 5*2^-24 (one rounding per difference, product and accumulation, all terms non-negative),
// so with a 2^-20 guard band d32 <= eps2*(1-2^-20) implies d64 <= eps2 and d32 >= eps2*(1+2^-20)
// implies d64 > eps2; only pairs inside the band are evaluated exactly.
__device__ __forceinline__ bool db_within2(const float4& q, const float4& p, const DbGrid& g) {
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    float d = dx * dx;
    d = __builtin_fmaf(dy, dy, d);
    d = __builtin_fmaf(dz, dz, d);
    if (d <= g.eps2_lo) return true;
    if (d >= g.eps2_hi) return false;
    return db_within(q, p, g.eps2);
}

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

// squared distance from a point to an axis-aligned box, same operation order as db_within;
// never larger than the computed distance to any point inside the box (monotone rounding)
__device__ __forceinline__ double db_box_d2(const float4& q, const float* __restrict__ box) {
    const double gx = fmax(fmax((double)box[0] - (double)q.x, (double)q.x - (double)box[3]), 0.0);
    const double gy = fmax(fmax((double)box[1] - (double)q.y, (double)q.y - (double)box[4]), 0.0);
    const double gz = fmax(fmax((double)box[2] - (double)q.z, (double)q.z - (double)box[5]), 0.0);
    double d = gx * gx;
    d += gy * gy;
    d += gz * gz;
    return d;
}
__device__ __forceinline__ double db_boxbox_d2(const float* __restrict__ a, const float* __restrict__ b) {
    const double gx = fmax(fmax((double)b[0] - (double)a[3], (double)a[0] - (double)b[3]), 0.0);
    const double gy = fmax(fmax((double)b[1] - (double)a[4], (double)a[1] - (double)b[4]), 0.0);
    const double gz = fmax(fmax((double)b[2] - (double)a[5], (double)a[2] - (double)b[5]), 0.0);
    double d = gx * gx;
    d += gy * gy;
    d += gz * gz;
    return d;
}

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

// Cell coordinates of a point: floor((x - origin) / s) per axis, as a product with 1/s in float64
// (error < 2^-21 cells for indices < 2^31, covered by the 2^-16 slack in s).  false: outside the
// grid (or NaN), coordinates 0.
__device__ __forceinline__ bool db_cell_coords(const DbGrid& g, float x, float y, float z,
                                               uint32_t& cx, uint32_t& cy, uint32_t& cz) {
    const double fx = floor(((double)x - (double)g.ox) * g.inv_cell);
    const double fy = floor(((double)y - (double)g.oy) * g.inv_cell);
    const double fz = floor(((double)z - (double)g.oz) * g.inv_cell);
    const bool ok = fx >= 0.0 && fx <= (double)g.mx && fy >= 0.0 && fy <= (double)g.my &&
                    fz >= 0.0 && fz <= (double)g.mz;
    cx = ok ? (uint32_t)fx : 0u; cy = ok ? (uint32_t)fy : 0u; cz = ok ? (uint32_t)fz : 0u;
    return ok;
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
__global__ __launch_bounds__(DB_THREADS) void db_add_offset_k(int32_t* __restrict__ labels, int64_t n, int32_t off) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i < n && labels[i] >= 0) labels[i] += off;
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
struct Row3 { float x, y, z; };               // 4-byte aligned: loads as one global_load_dwordx3
constexpr int CS_THREADS = 1024;
constexpr int CS_WAVES   = CS_THREADS / 64;
constexpr int CS_ROUNDS  = 4;
constexpr int CS_TILE    = CS_THREADS * CS_ROUNDS;
constexpr int CS_PASSES  = 4;
constexpr int CS_HREP    = 4;         // copies of every digit histogram (power of two)
constexpr int CS_BINS    = 512;       // digits of up to 9 bits
constexpr int64_t CS_MAX_CHUNK = 1 << 17;     // larger chunks use the global sort
constexpr int64_t CS_MIN_CHUNKS = 96;         // fewer chunks: the global sort keeps more of the GPU busy

// cell key of a row inside its chunk (0 when the row is outside the grid); ok = inside
__device__ __forceinline__ uint32_t cs_cell_key(const DbGrid& g, float x, float y, float z, bool& ok) {
    uint32_t cx, cy, cz;
    ok = db_cell_coords(g, x, y, z, cx, cy, cz);
    return (((cz << g.by) | cy) << g.bx) | cx;
}

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
    uint32_t* __restrict__ status, unsigned long long* __restrict__ stamps) {
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
struct DbStage {
    uint32_t* ncell;        // [nchunks] cells of chunk c; 0: the chunk overflowed, its keys come from db_chunksort_k
    uint64_t* key;          // [n] at lo + j: key of the chunk's j-th cell, ascending
    uint32_t* start;        // [n] at lo + j: first sorted row of that cell (an index into pts)
    uint32_t* minrow;       // [n] at lo + j: smallest original row of that cell (db_celltab_k: cell_min)
};
constexpr int CT_SLOTS = 4096;                  // table slots (key + count: 32 KiB)
constexpr int CT_BITS  = 12;                    // log2(CT_SLOTS)
constexpr int CT_CELLS = 1024;                  // cells a chunk may hold here (measured: a uniform-cloud chunk of ~1 600
                                                // cells took longer here than in db_chunksort_k)
constexpr uint32_t CT_EMPTY = 0xFFFFFFFFu;      // no cell key has 32 bits (this path takes cellbits <= 31)
static_assert(CT_SLOTS == 1 << CT_BITS && CT_CELLS + CS_THREADS < CT_SLOTS, "the table never fills (see sweep 1)");

__device__ __forceinline__ uint32_t ct_hash(uint32_t k) { return (k * 0x9E3779B1u) >> (32 - CT_BITS); }

template <bool TABLE>
__global__ __launch_bounds__(CS_THREADS) void db_cellscatter_k(
    const float* __restrict__ xyz, int64_t n, DbGrid g, uint32_t* __restrict__ bad, uint32_t* __restrict__ ovf,
    float4* __restrict__ pts, uint64_t* __restrict__ keys_out, DbStage st, uint32_t* __restrict__ status) {
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
constexpr int64_t DB_TABLE_MAX_CHUNKS = 16384;  // beyond: db_cellscatter_k<false>, the table is read off the keys
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
    uint32_t* __restrict__ route) {
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
    }
}

// ---- neighbour rows of one cell: lanes 0..24 each find one (dy,dz) row ------------------
struct RowSet {
    int ca[DB_ROWS], cb[DB_ROWS];      // cell index range of every row
};

template <typename K>
__device__ __forceinline__ int db_lower(const K* __restrict__ a, int m, K k) {
    int lo = 0, hi = m;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < k) lo = mid + 1; else hi = mid; }
    return lo;
}
// neighbour row `row` (cells x-2 .. x+2 at (dy, dz) = DB_ROW_DY/DZ[row]) of the cell `key`: its y and z and the x range
// it covers inside the grid; false: the row lies outside
struct DbRowAt { int xlo, xhi, ny, nz; };
__device__ __forceinline__ bool db_row_at(const DbGrid& g, uint64_t key, int row, DbRowAt& at) {
    const uint64_t cx = key & ((1ull << g.bx) - 1);
    const uint64_t cy = (key >> g.bx) & ((1ull << g.by) - 1);
    const uint64_t cz = (key >> (g.bx + g.by)) & ((1ull << g.bz) - 1);
    at.ny = (int)cy + DB_ROW_DY[row];
    at.nz = (int)cz + DB_ROW_DZ[row];
    at.xlo = (int)cx - 2 < 0 ? 0 : (int)cx - 2;
    at.xhi = (int)cx + 2 > g.mx ? g.mx : (int)cx + 2;
    return at.ny >= 0 && at.ny <= g.my && at.nz >= 0 && at.nz <= g.mz;
}
// index range [x, y) of the keys klo .. khi among the sorted, unique a[0 .. n): the five cells of a neighbour row at most
template <typename K>
__device__ __forceinline__ int2 db_run_in(const K* __restrict__ a, int n, K klo, K khi) {
    int2 v;
    v.x = db_lower(a, n, klo);
    // the end of the run: cell keys are unique, so at most five cells (x - 2 .. x + 2) follow v.x, their keys
    // ascending - five loads side by side instead of a second binary search (fourteen dependent loads in a chunk
    // of 11 000 cells)
    K kk[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) kk[i] = v.x + i < n ? a[v.x + i] : ~K(0);
    int cntx = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) cntx += kk[i] <= khi ? 1 : 0;
    v.y = v.x + cntx;
    return v;
}
// cell-index range [x, y) of neighbour row `row` of the cell `key`
__device__ __forceinline__ int2 db_row_run(const DbGrid& g, const uint64_t* __restrict__ cell_key, uint64_t key,
                                           int row) {
    const int sh = g.bx + g.by + g.bz;
    const uint64_t chunk = sh < 64 ? (key >> sh) : 0;
    int2 v;
    v.x = 0; v.y = 0;
    DbRowAt at;
    if (db_row_at(g, key, row, at)) {
        const int c0 = (int)g.chunk_cells[chunk], c1 = (int)g.chunk_cells[chunk + 1];   // neighbours share the chunk
        v = db_run_in(cell_key + c0, c1 - c0, db_pack(g, chunk, (uint64_t)at.nz, (uint64_t)at.ny, (uint64_t)at.xlo),
                      db_pack(g, chunk, (uint64_t)at.nz, (uint64_t)at.ny, (uint64_t)at.xhi));
        v.x += c0;
        v.y += c0;
    }
    return v;
}

// the rows of `cell` (key `key`) into rs: from db_rowtab_k's table, or found here where the table is not built
__device__ __forceinline__ void db_rows(const DbGrid& g, const uint64_t* __restrict__ cell_key, uint64_t key,
                                        RowSet* __restrict__ rs, const int2* __restrict__ rowtab, int cell) {
    const int l = lane_id();
    if (rowtab) {
        if (l < DB_ROWS) {
            const int2 v = rowtab[(int64_t)cell * DB_ROWS + l];
            rs->ca[l] = v.x;
            rs->cb[l] = v.y;
        }
        __builtin_amdgcn_wave_barrier();
        return;
    }
    if (l < DB_ROWS) {
        const int2 v = db_row_run(g, cell_key, key, l);
        rs->ca[l] = v.x;
        rs->cb[l] = v.y;
    }
    __builtin_amdgcn_wave_barrier();
}

// neighbour-row table: [cell][25] cell-index ranges, shared by the core / union / border kernels
__global__ __launch_bounds__(DB_THREADS) void db_rowtab_k(DbGrid g, const uint64_t* __restrict__ cell_key,
                                                          int m, int2* __restrict__ rowtab) {
    const int c = (blockIdx.x * DB_WAVES + wave_id()) * 2 + (lane_id() >> 5);   // two cells per wave
    const int l = lane_id() & 31;
    if (c >= m || l >= DB_ROWS) return;
    rowtab[(int64_t)c * DB_ROWS + l] = db_row_run(g, cell_key, cell_key[c], l);
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
    uint32_t* __restrict__ bits, int2* __restrict__ rowtab, int64_t rowtab_cells, uint64_t* __restrict__ keys_out) {
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
__device__ __forceinline__ float db_d2f(const float4& a, const float4& b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}
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

// ---- the border rule: smallest cluster id among the core points within eps, else none (db_border_k, dq_assign_k) ----
// The neighbour cells with core points, ONE PER LANE (three rounds of twelve rows x five cells - a row holds the
// cells x-2 .. x+2 of one (y, z)): count, label and core box are read once per cell of the fit, side by side.  One cell
// after the other - count, label, six box words, each a dependent load, for up to 125 cells and every query again - was
// db_border_k: a lone noise point beside a tower tested ~100 boxes at ~0.4 us each, 51 us for 2.6 MB of traffic.
// A row never holds more than five cells: the keys of x-2 .. x+2 in one (chunk, y, z) are unique (db_row_run).
constexpr int DB_BR = 3, DB_BROWS = 12;
struct DbCoreCells {
    int cell[DB_BR], label[DB_BR];     // -1 / INT_BIG: this lane holds no core cell in that round
    bool dense[DB_BR];                 // every row of the cell is core: core_s need not be read
    float box[DB_BR][6];               // box of the cell's core points
};

// the core cells among the rows of rs, one per lane; `on` is wave-uniform, false: nothing is read and no lane holds a cell
__device__ __forceinline__ void db_gather_core_cells(DbCoreCells& cc, const RowSet* __restrict__ rs, bool on,
                                                     const uint32_t* __restrict__ cell_start,
                                                     const uint32_t* __restrict__ cell_ncore,
                                                     const float* __restrict__ cell_box,
                                                     const int* __restrict__ cell_label) {
    const int l = lane_id();
#pragma unroll
    for (int rd = 0; rd < DB_BR; ++rd) {
        const int row = rd * DB_BROWS + l / 5, k = l % 5;
        cc.cell[rd] = -1; cc.label[rd] = INT_BIG; cc.dense[rd] = false;
#pragma unroll
        for (int a = 0; a < 6; ++a) cc.box[rd][a] = 0.0f;
        if (on && l < 5 * DB_BROWS && row < DB_ROWS) {
            const int B = rs->ca[row] + k;
            if (B < rs->cb[row]) {
                const uint32_t nb = cell_ncore[B];
                if (nb != 0) {
                    cc.cell[rd] = B;
                    cc.label[rd] = cell_label[B];
                    cc.dense[rd] = nb == cell_start[B + 1] - cell_start[B];
#pragma unroll
                    for (int a = 0; a < 6; ++a) cc.box[rd][a] = cell_box[6 * (int64_t)B + a];
                }
            }
        }
    }
}

// The smallest label among the gathered cells that hold a core point within eps of qp, INT_BIG if there is none.
// Cells whose core box reaches the query, then: smallest label first - the first cell that really holds a core point
// within eps decides (what is asked for is the smallest label among such cells; the order of the cells with larger
// labels does not matter).  A cell whose cluster was dropped (label INT_BIG) attracts nothing.
__device__ __forceinline__ int db_border_label(const DbGrid& g, const float4 qp, const DbCoreCells& cc,
                                               const float4* __restrict__ pts,
                                               const uint32_t* __restrict__ cell_start,
                                               const uint8_t* __restrict__ core_s) {
    const int l = lane_id();
    bool cand[DB_BR];
#pragma unroll
    for (int rd = 0; rd < DB_BR; ++rd) cand[rd] = cc.cell[rd] >= 0 && !(db_box_d2(qp, cc.box[rd]) > g.eps2);
    for (;;) {                                             // every turn ends the loop or strikes one candidate cell
        int mine = INT_BIG, sel = -1;
#pragma unroll
        for (int rd = 0; rd < DB_BR; ++rd)
            if (cand[rd] && cc.label[rd] < mine) { mine = cc.label[rd]; sel = rd; }
        const int lo = wave_reduce_min(mine);
        if (lo == INT_BIG) return INT_BIG;
        const int owner = (int)__builtin_ctzll(__ballot(mine == lo));
        int Bsel = -1;
        bool dsel = false;
#pragma unroll
        for (int rd = 0; rd < DB_BR; ++rd)
            if (sel == rd) { Bsel = cc.cell[rd]; dsel = cc.dense[rd]; }
        const int B = __builtin_amdgcn_readlane(Bsel, owner);
        const bool b_dense = __builtin_amdgcn_readlane((int)dsel, owner) != 0;
        const uint32_t bs = cell_start[B], be = cell_start[B + 1];
        for (uint32_t j0 = bs; j0 < be; j0 += 64) {
            const uint32_t j = j0 + l;
            bool hit = false;
            if (j < be && (b_dense || core_s[j])) hit = db_within2(qp, pts[j], g);
            if (__ballot(hit)) return lo;
        }
        if (l == owner) {
#pragma unroll
            for (int rd = 0; rd < DB_BR; ++rd)
                if (sel == rd) cand[rd] = false;
        }
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
    int any = 0;
    if (l < DB_ROWS)
        for (int B = rs->ca[l]; B < rs->cb[l]; ++B) any |= (cell_ncore[B] != 0);
    if (!__ballot(any != 0)) {
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
// and 1024.  dq_kdist_k: DK_PIECE).  dq_heads_k writes the start flags (scanned in place),
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
        if (l < DB_ROWS) {
            const int2 v = db_row_run(g, cell_key, key, l);
            rs->ca[l] = v.x;
            rs->cb[l] = v.y;
        }
        __builtin_amdgcn_wave_barrier();
        int any = 0;
        if (l < DB_ROWS)
            for (int B = rs->ca[l]; B < rs->cb[l]; ++B) any |= (cell_ncore[B] != 0);
        const bool none = !__ballot(any != 0);             // no core cell in reach: the whole piece is -1
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
struct DkWave {
    uint64_t buf[DK_CAP];
    uint32_t hist[256];
    uint32_t seg_off[DB_ROWS + 1], seg_a[DB_ROWS];
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
// f(in, key) for every group of 64 candidates, called by all lanes: in = the lane holds a candidate with d2 <= eps2,
// key = the bit pattern of its d2
template <typename F>
__device__ __forceinline__ void dk_sweep(const DbGrid& g, const float4* __restrict__ pts, const DkWave& W, uint32_t T,
                                         const float4& q, F&& f) {
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
            if (t0 + 64u * u + l < T) {
                const float4 p = P[u];
                const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
                float d = dx * dx;
                d = __builtin_fmaf(dy, dy, d);
                d = __builtin_fmaf(dz, dz, d);
                if (!(d >= g.eps2_hi)) {                   // (db_within2's band: d32 >= eps2_hi implies d64 > eps2)
                    const double d2 = db_d2(q, p);
                    in = d2 <= g.eps2;
                    key = (uint64_t)__double_as_longlong(d2);
                }
            }
            f(in, key);
        }
    }
}
// the k-th smallest d2 <= eps2 among the T candidates of the wave's piece, +inf if there are fewer; count: how many
__device__ __forceinline__ double dk_select(const DbGrid& g, const float4* __restrict__ pts, DkWave& W, uint32_t T,
                                            const float4& q, int32_t k, int& count_out) {
    const int l = lane_id();
#pragma unroll
    for (int u = 0; u < 4; ++u) W.hist[l + 64 * u] = 0u;
    dk_sync();
    uint32_t count = 0;
    dk_sweep(g, pts, W, T, q, [&](bool in, uint64_t key) {
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
        dk_sync();
        uint32_t h[4], sum = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) { h[u] = W.hist[4 * l + u]; sum += h[u]; }
        const uint32_t incl = wave_scan_incl(sum);
        uint32_t e = incl - sum, digit = 0, knew = 0;
        const bool mine = e < kk && kk <= incl;            // one lane: the bins hold kk keys at least
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (mine && e < kk && kk <= e + h[u]) { digit = 4u * l + u; knew = kk - e; }
            e += h[u];
        }
        const int src = __ffsll((unsigned long long)__ballot(mine)) - 1;
        digit = (uint32_t)__shfl((int)digit, src, 64);
        kk = (uint32_t)__shfl((int)knew, src, 64);
        prefix |= (uint64_t)digit << shift;
        if (shift == 0) break;
        dk_sync();                                         // every lane has read its bins
#pragma unroll
        for (int u = 0; u < 4; ++u) W.hist[l + 64 * u] = 0u;
        dk_sync();
        const int ns = shift - 8;
        auto tally = [&](bool in, uint64_t key) {
            const bool on = in && (key >> shift) == (prefix >> shift);
            dk_tally(W.hist, on, (uint32_t)(key >> ns) & 255u, __ballot(on));
        };
        if (kept) {
            for (uint32_t i0 = 0; i0 < count; i0 += 64) {
                const bool in = i0 + l < count;
                tally(in, in ? W.buf[i0 + l] : 0ull);
            }
        } else {
            dk_sweep(g, pts, W, T, q, tally);
        }
    }
    return __longlong_as_double((long long)prefix);
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
        const uint64_t key = keys[ps];
        uint32_t a = 0, len = 0;
        if (l < DB_ROWS) {
            const int2 v = db_row_run(g, cell_key, key, l);
            a = cell_start[v.x];
            len = cell_start[v.y] - a;
        }
        const uint32_t incl = wave_scan_incl(len);
        const uint32_t T = (uint32_t)__shfl((int)incl, 63, 64);
        dk_sync();                                         // the piece before this one has read its runs
        if (l < DB_ROWS) { W.seg_a[l] = a; W.seg_off[l + 1] = incl; }
        if (l == 0) W.seg_off[0] = 0u;
        dk_sync();
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

// publishes the cluster count and zeroes the box accumulators (neutral start of db_box_fold)
__global__ void db_prelabel_k(const uint32_t* __restrict__ total, int32_t* __restrict__ out_nclusters,
                              uint32_t* __restrict__ box_acc, int64_t box_words) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out_nclusters = (int32_t)*total;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (box_acc && i < box_words) box_acc[i] = 0u;
}

// The 256-byte head of the workspace.  Kernels take pointers to single fields; the host reads fields of a copy.
struct DbMeta {
    uint32_t box_key[6];    // db_aabb_in_k: ordered keys of the finite rows' box, min xyz | max xyz; db_bounds reads
                            // them.  DbWs::clear_from starts at [4] for its 16-byte alignment: nobody reads [4..5] then
    uint32_t status;        // bit 0: a finite row outside the grid, bit 1: compressed coordinate out of range
    uint32_t ncells, nclusters;
    uint32_t comp_max[3];   // dbc_comp_k: largest compressed index per axis
    int64_t  first_bad;     // db_compress: first NaN/inf row, -1 if none
    uint32_t pad[50];       // [0]: DbWs::cell_route
};
static_assert(sizeof(DbMeta) == 256 && offsetof(DbMeta, box_key) == 0 && offsetof(DbMeta, status) == 24 &&
              offsetof(DbMeta, ncells) == 28 && offsetof(DbMeta, nclusters) == 32 && offsetof(DbMeta, comp_max) == 36 &&
              offsetof(DbMeta, first_bad) == 48 && offsetof(DbMeta, pad) == 56, "the layout every build so far had");

struct DbWs {
    DbMeta*   meta;
    uint64_t *k0, *k1, *cell_key;
    uint32_t *v0, *v1, *head, *cid, *cell_start, *cell_ncore, *radix_ws, *scan_ws;
    float4   *pts, *xbuf;
    uint8_t*  core_s;
    float*    cell_box;
    uint32_t* cell_acc;     // [cells][8] ordered-key accumulators of db_cellstats_k
    int*      cell_min;     // smallest original row among a cell's core points
    int      *parent, *root, *comp_min, *cell_label;
    int2*     rowtab;
    int64_t   rowtab_cells;
    uint32_t *chunk_bad, *chunk_cells;
    uint32_t* chunk_ovf;     // one word per chunk: db_cellscatter_k handed the chunk to db_chunksort_k
    uint32_t* comp;          // [n][3] compressed cell coordinates (fallback for grids beyond the 64-bit key)
    uint32_t* flag2;         // [n + 8] head flags kept beside their scan
    unsigned long long* core_stats;   // [4] tallies of db_core_k<true> (pch_dbscan_set_pair_counting)
    uint32_t* scan1_b;                // zeroed words of the single-pass scan of the cluster ranks
    uint32_t* bits;         // bitmap over the rows: db_cellstats_k clears it, db_mark_k sets the clusters' first core rows
                            // (the staged route: db_celltab_k and db_chunkunion_k)
    // Views that db_plan carves into the arrays above:
    uint32_t* wrank;        // bits' array from the next multiple of 64 words on: db_labels' scan of the bitmap's word
                            // counts.  Both are kept for pch_dbscan_first_core_rows_i32; the array has no other use
    uint8_t*  face_todo;    // root as bytes: db_union_pairs_k writes the face pairs it leaves to db_union_face_k.  root
                            // itself is first written by db_compmin_k, behind both
    DbStage   stage;        // the chunk route's staged cell lists (db_cellscatter_k<true>) in arrays that only the global
                            // sort uses: ncell = v1, key = k0, start = v0; and minrow = head, the compressed route's
    uint32_t* cell_route;   // meta->pad[0]: db_chunkcells_k says that a chunk overflowed, so the table comes from keys.
                            // One copy from meta->status up to here brings the host status, ncells and this word
    unsigned long long* cs_stamps = nullptr;     // cell_box (first written by db_core_k), PCH_CS_STAMPS builds only
    // One 16-byte aligned fill zeroes status / ncells / nclusters, scan1_b and the first-cell word of every chunk
    // (db_cells_k writes it at a chunk's first cell; the zeros make a chunk without a cell an empty range)
    void*  clear_from() const { return &meta->box_key[4]; }
    size_t clear_bytes(int64_t nchunks) const {
        return ((size_t)((char*)(chunk_cells + nchunks + 1) - (char*)clear_from()) + 15) & ~size_t(15);
    }
};

static void db_plan(Arena& a, int64_t n, DbWs& w) {
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

// The cell table in the parameter order of the neighbour kernels: db_core_k takes DB_GRID_ARGS (and writes core_s /
// cell_ncore), db_union*_k and db_border_k take DB_CELL_ARGS
struct DbCells {
    DbGrid g; const float4* pts; const uint32_t* cell_start; const uint64_t* cell_key; int m;
    const int2* rowtab;          // null: more cells than the row table holds, rows are searched on the fly
    const uint8_t* core_s; const uint32_t* cell_ncore; const float* cell_box;
    bool chunk_union;            // the table came from the staged lists (no chunk beyond CT_CELLS cells): db_union runs
                                 // db_chunkunion_k, which also does db_cellfin_k's and db_mark_k's work
};
#define DB_GRID_ARGS(c) (c).g, (c).pts, (c).cell_start, (c).cell_key, (c).m, (c).rowtab
#define DB_CELL_ARGS(c) DB_GRID_ARGS(c), (c).core_s, (c).cell_ncore, (c).cell_box

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

// the run whose workspace the entries below continue, and its cell table
// (nchunks and compressed: what pch_dbscan_assign_f32 needs to know about the grid beyond the cell table)
struct DbLastRun { void* ws; size_t ws_bytes; int64_t n; DbCells c; int64_t nchunks; bool compressed; };
static thread_local DbLastRun g_last = {nullptr, 0, 0, {}, 0, false};

void ws_touched(const void* base, size_t bytes) {
    if (!g_last.ws) return;
    const char* a0 = static_cast<const char*>(base);
    const char* b0 = static_cast<const char*>(g_last.ws);
    if (a0 < b0 + g_last.ws_bytes && b0 < a0 + bytes) g_last.ws = nullptr;
}

// The entry points that continue the grid the last pch_dbscan_f32 of this thread left in `ws` carve it up again
// here; `entry` names the caller in the error
static int db_continue(const char* entry, int64_t n, void* ws, size_t ws_bytes, DbWs& w) {
    if (g_last.ws != ws || g_last.ws_bytes != ws_bytes || g_last.n != n || ws == nullptr) {
        set_error("%s must follow pch_dbscan_f32 of this thread on the same, untouched workspace", entry);
        return PCH_ERR_ARG;
    }
    Arena a(ws, ws_bytes, true);
    db_plan(a, n, w);
    return PCH_OK;
}

// host mirror of f32_unordered
static float host_unordered(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// blocks of the grid-stride sweeps over the input rows (db_aabb_in_k, db_first_bad_k, db_chunkbad_k)
static unsigned db_stride_blocks(int64_t n) { return (unsigned)std::min(ceil_div(n, DB_THREADS * 8), int64_t(2048)); }

// ---- the steps of dbscan_run, in the order it runs them
// what they share: the run's rows, outputs, stream and carved workspace
struct DbRun {
    const float* xyz; int64_t n, chunk_size, nchunks;
    int32_t* labels; uint8_t* core; int32_t* out_nclusters;
    hipStream_t s; DbWs w;
};

static int db_all_noise(const DbRun& r) {
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
    for (int k = 0; k < 6; ++k) {
        if (!(box[k] == box[k]) || box[k] > 3.0e38f || box[k] < -3.0e38f) {
            set_error("bounding box is not finite");
            return PCH_ERR_ARG;
        }
    }
    return PCH_OK;
}

// largest cell coordinate per axis -> g.mx..mz and the key bits per axis; returns the bits of a cell
static int db_cell_bits(DbGrid& g, int mx, int my, int mz) {
    g.mx = mx; g.my = my; g.mz = mz;
    g.bx = bits_for((uint64_t)mx + 1); g.by = bits_for((uint64_t)my + 1); g.bz = bits_for((uint64_t)mz + 1);
    return g.bx + g.by + g.bz;
}

// the grid of cells of side eps/sqrt(3) over the box, and the bits of its key: a cell (cellbits), then the chunk
// (nbits in all).  Returns true when that key does not fit 64 bits.
static bool db_grid(const DbRun& r, const float (&box)[6], double eps, int32_t min_samples, DbGrid& g, int& cellbits,
                    int& nbits) {
    g.ox = box[0]; g.oy = box[1]; g.oz = box[2];
    g.cell = eps / 1.7320508075688772 * (1.0 - 1.0 / 65536.0);
    g.inv_cell = 1.0 / g.cell;
    g.eps2 = eps * eps;
    g.eps2_lo = nextafterf((float)(g.eps2 * (1.0 - 1.0 / 1048576.0)), -INFINITY);
    g.eps2_hi = nextafterf((float)(g.eps2 * (1.0 + 1.0 / 1048576.0)), INFINITY);
    if (!(g.eps2_hi < 3.0e38f)) { g.eps2_lo = -1.0f; g.eps2_hi = NAN; }    // absurd eps: exact path only
    g.chunk_size = r.chunk_size;
    g.chunk_bad = r.w.chunk_bad;
    g.chunk_cells = r.w.chunk_cells;
    g.min_samples = min_samples;
    int mc[3] = {0, 0, 0};
    bool overflow = false;
    for (int k = 0; k < 3; ++k) {
        const double ext = ((double)box[3 + k] - (double)box[k]) * g.inv_cell;
        if (!(ext < 2.0e9)) overflow = true;
        else mc[k] = (int)ext + 1;            // +1: slack for the rounding of the division
    }
    cellbits = db_cell_bits(g, mc[0], mc[1], mc[2]);
    nbits = cellbits + bits_for((uint64_t)r.nchunks);
    return overflow || nbits > 64;
}

// key beyond 64 bits, several chunks: every chunk on its own, with its own bounding box (the reference fits them one
// by one anyway)
static int db_run_chunks(const DbRun& r, double eps, int32_t min_samples, void* ws, size_t ws_bytes, int32_t* k_host) {
    int32_t offset = 0;
    for (int64_t c = 0; c < r.nchunks; ++c) {
        const int64_t lo = c * r.chunk_size, cn = (r.n - lo) < r.chunk_size ? (r.n - lo) : r.chunk_size;
        int32_t kc = 0;
        PCH_TRY(dbscan_run(r.xyz + 3 * lo, cn, eps, min_samples, 0, nullptr, r.labels + lo,
                           r.core ? r.core + lo : nullptr, r.out_nclusters, ws, ws_bytes, r.s, &kc));
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

// key beyond 64 bits, one chunk: compressed cell coordinates per axis (w.comp, see dbc_axis_keys_k) and the grid's
// mx..bz / cellbits over them.  done: the outputs are written
static int db_compress(const DbRun& r, DbGrid& g, int& cellbits, bool& done) {
    const DbWs& w = r.w; const hipStream_t s = r.s; const int64_t n = r.n;
    const unsigned gn = (unsigned)ceil_div(n, DB_THREADS);
    PCH_HIP_TRY(hipMemsetAsync(&w.meta->first_bad, 0xFF, sizeof(int64_t), s));
    PCH_LAUNCH("db_first_bad", db_first_bad_k, dim3(db_stride_blocks(n)), dim3(DB_THREADS), 0, s, r.xyz, n,
               reinterpret_cast<unsigned long long*>(&w.meta->first_bad));
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
static int db_sorted_keys(const DbRun& r, const DbGrid& g, int cellbits, int nbits, bool compressed, int sort_mode,
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
        // bounds the number of chunks); db_cells_core takes the table from them unless a chunk overflowed
        staged = nchunks <= DB_TABLE_MAX_CHUNKS;
        const auto cellscatter = staged ? db_cellscatter_k<true> : db_cellscatter_k<false>;
        PCH_LAUNCH("db_cellscatter", cellscatter, dim3((unsigned)nchunks), dim3(CS_THREADS), 0, s, r.xyz, n, g,
                   w.chunk_bad, w.chunk_ovf, w.pts, w.k1, w.stage, &w.meta->status);
        PCH_LAUNCH("db_chunksort", db_chunksort_k, dim3((unsigned)nchunks), dim3(CS_THREADS), 0, s, r.xyz, n, g,
                   w.chunk_ovf, w.chunk_bad, w.xbuf, w.pts, w.k1, &w.meta->status, w.cs_stamps);
        if (staged)
            PCH_LAUNCH("db_chunkcells", db_chunkcells_k, dim3(1), dim3(CC_THREADS), 0, s, w.stage.ncell, w.chunk_ovf,
                       (int)nchunks, n, r.chunk_size, w.chunk_cells, w.cell_start, &w.meta->ncells, w.cell_route);
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

// the cells of the sorted keys, their row table, the core flags and the per-cell statistics; c: the cell table
static int db_cells_core(const DbRun& r, const DbGrid& g, int cellbits, const uint64_t* ks, bool staged,
                         bool count_pairs, DbCells& c) {
    const DbWs& w = r.w; const hipStream_t s = r.s; const int64_t n = r.n;
    const int64_t ntile = ceil_div(n, (int64_t)SCAN_TILE);
    // the cell count sizes the next grids: fetch it while the kernel that writes the table (sized by n) runs
    DbMeta back;                             // status, ncells ... the route word
    constexpr size_t peek_bytes = offsetof(DbMeta, pad) + sizeof(uint32_t) - offsetof(DbMeta, status);
    back.pad[0] = 1u;
    if (staged) {
        // db_chunkcells_k left ncells and the route word; db_celltab_k reads the word itself and writes either the
        // table (and the row table) or the keys that db_chunksort_k did not (then the table is read off the keys
        // below, as ever)
        PCH_TRY(peek_enqueue(&w.meta->status, peek_bytes, s));
        PCH_LAUNCH("db_celltab", db_celltab_k, dim3((unsigned)r.nchunks), dim3(CS_THREADS), 0, s, w.cell_route, w.stage,
                   w.chunk_ovf, g, n, w.cell_start, w.cell_key, w.cell_min, w.bits, w.rowtab, w.rowtab_cells, w.k1);
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
    if (c.chunk_union)                                   // ... and every cell's label, which both owners of the rows read
        PCH_LAUNCH("db_prelabel", db_prelabel_cells_k, dim3((unsigned)std::max<int64_t>(ceil_div(std::max<int64_t>(
                   box_words, m), 256), 1)), dim3(256), 0, s, &w.meta->nclusters, r.out_nclusters, box_acc, box_words,
                   w.root, w.comp_min, w.bits, w.wrank, m, w.cell_label);
    else
        PCH_LAUNCH("db_prelabel", db_prelabel_k, dim3((unsigned)std::max<int64_t>(ceil_div(box_words, 256), 1)),
                   dim3(256), 0, s, &w.meta->nclusters, r.out_nclusters, box_acc, box_words);
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

}  // namespace pch

using namespace pch;

extern "C" int pch_first_nonfinite_row_f32(const float* xyz, int64_t n, int64_t* out_row, void* stream) {
    PCH_DEVICE_GUARD(out_row);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n >= 0 && out_row && (n == 0 || xyz), "bad argument");
    PCH_HIP_TRY(hipMemsetAsync(out_row, 0xFF, sizeof(int64_t), s));             // -1: every row finite
    if (n == 0) return PCH_OK;
    PCH_LAUNCH("db_first_bad", db_first_bad_k, dim3(db_stride_blocks(n)), dim3(DB_THREADS), 0, s, xyz, n,
               reinterpret_cast<unsigned long long*>(out_row));
    return PCH_OK;
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
                    size_t ws_bytes, hipStream_t s, int32_t* k_host, DbBoxOut* boxes) {
    if (k_host) *k_host = 0;
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
    Arena a(ws, ws_bytes);
    DbWs w;
    db_plan(a, n, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    if (chunk_size <= 0 || chunk_size > n) chunk_size = n;
    const DbRun r = {xyz, n, chunk_size, ceil_div(n, chunk_size), labels, core, out_nclusters, s, w};
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
    PCH_TRY(db_sorted_keys(r, g, cellbits, nbits, overflow, tune.sort_mode, ks, staged));
    PCH_TRY(db_cells_core(r, g, cellbits, ks, staged, tune.count_pairs, c));
    PCH_TRY(db_union(r, c));
    PCH_TRY(db_labels(r, c, k_host, boxes));
    g_last = {ws, ws_bytes, n, c, r.nchunks, overflow};
    return PCH_OK;
}

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

extern "C" void pch_dbscan_set_pair_counting(int enable) { g_count_pairs = enable != 0; }

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
    PCH_LAUNCH("db_border", db_border_k<false>, dim3((unsigned)ceil_div(c.m, DB_WAVES)), dim3(DB_THREADS), 0, s,
               DB_CELL_ARGS(c), w.cell_label, labels, nullptr, 0, nullptr);
    return PCH_OK;
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

// What pch_dbscan_assign_f32 and pch_dbscan_kdist_f32 share: the checks of a query call against the fit `entry`
// continues (nq != 0, `out` its output), then the queries binned into the fit's cells, sorted and cut into pieces.
struct DqPieces { DbQuery Q; const uint64_t* ks; const uint32_t* vs; const uint32_t *piece_start, *npieces; };
static int dq_pieces(const char* entry, const float* query, int64_t nq, const float* sub3_host,
                     const int32_t* query_chunk, int64_t n, const void* out, void* qws, size_t qws_bytes, void* ws,
                     size_t ws_bytes, hipStream_t s, bool kdist, DbWs& w, DqPieces& P) {
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
    if (kdist) PCH_LAUNCH("dq_heads", dq_heads_k<DK_PIECE>, dim3(gq), dim3(DB_THREADS), 0, s, P.ks, nq, qw.flag);
    else PCH_LAUNCH("dq_heads", dq_heads_k<DQ_PIECE>, dim3(gq), dim3(DB_THREADS), 0, s, P.ks, nq, qw.flag);
    PCH_TRY(scan_exclusive_u32(qw.flag, qw.flag, nq, qw.scan_ws, qw.npieces, s));
    if (kdist)
        PCH_LAUNCH("dq_pieces", dq_pieces_k<DK_PIECE>, dim3(gq), dim3(DB_THREADS), 0, s, P.ks, nq, qw.flag, qw.piece_start);
    else
        PCH_LAUNCH("dq_pieces", dq_pieces_k<DQ_PIECE>, dim3(gq), dim3(DB_THREADS), 0, s, P.ks, nq, qw.flag, qw.piece_start);
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
    PCH_TRY(dq_pieces(__func__, query, nq, sub3_host, query_chunk, n, out_labels, qws, qws_bytes, ws, ws_bytes, s, false, w,
                      P));
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
    PCH_TRY(dq_pieces(__func__, query, nq, sub3_host, query_chunk, n, out_d2, qws, qws_bytes, ws, ws_bytes, s, true, w, P));
    const DbCells& c = g_last.c;
    PCH_LAUNCH("dq_kdist", dq_kdist_k, dim3(dq_piece_blocks(nq)), dim3(DB_THREADS), 0, s, P.Q, c.g, c.pts,
               c.cell_start, c.cell_key, P.ks, P.vs, P.piece_start, P.npieces, k, out_d2, out_count);
    return PCH_OK;
}

extern "C" int pch_dbscan_f32(const float* xyz, int64_t n, double eps, int32_t min_samples,
                              int64_t chunk_size, const float* aabb_host, int32_t* labels,
                              uint8_t* core, int32_t* out_nclusters, void* ws, size_t ws_bytes,
                              void* stream) {
    PCH_DEVICE_GUARD(xyz ? (const void*)xyz : (const void*)out_nclusters);
    return dbscan_run(xyz, n, eps, min_samples, chunk_size, aabb_host, labels, core, out_nclusters, ws, ws_bytes,
                      (hipStream_t)stream, nullptr);
}
