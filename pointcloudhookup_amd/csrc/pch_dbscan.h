// Stage C (DBSCAN): what more than one of its three translation units uses - pch_dbscan_cells.hip (rows to cell
// table), pch_dbscan.hip (the fit on that table; the method is explained there) and pch_dbscan_query.hip
// (continuations of a retained fit).
#pragma once
#include <assert.h>
#include "pch_prims.h"

namespace pch {

constexpr int DB_THREADS = 256;
constexpr int DB_WAVES   = DB_THREADS / 64;
constexpr int DB_ROWS    = 25;
constexpr int INT_BIG    = 0x7fffffff;

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

// The band of one radius r: r*r and the float32 pre-filter of db_within2 around it (2^-20 guard band, one float32
// step further out).  The one place that forms it: DbGrid::eps2* from eps (db_grid), a query's radius (dq_shape_k).
struct DbBand { double r2; float lo, hi; };
inline DbBand db_band(double r) {
    DbBand b;
    b.r2 = r * r;
    b.lo = nextafterf((float)(b.r2 * (1.0 - 1.0 / 1048576.0)), -INFINITY);
    b.hi = nextafterf((float)(b.r2 * (1.0 + 1.0 / 1048576.0)), INFINITY);
    if (!(b.hi < 3.0e38f)) { b.lo = -1.0f; b.hi = NAN; }    // absurd radius: exact path only
    return b;
}

// ---- the part of the grid that depends on the rows' box: one function for the host (db_grid) and for db_headplan_k ----
__host__ __device__ inline int db_bits_for(uint64_t count) {    // bits_for (pch_common.h), for both sides
    int b = 0;
    while (b < 64 && (uint64_t(1) << b) < count) ++b;
    return b;
}
// g.inv_cell is set (it depends on eps alone).  Sets the origin, mx..mz and bx..bz of g and the bits of a cell
// (cellbits) and of a key (nbits, with the chunk).  Returns true when that key does not fit 64 bits.  A difference, a
// product, a compare and a truncation per axis: nothing a compiler could contract into a fused multiply-add.
__host__ __device__ inline bool db_plan_grid(const float* box, int64_t nchunks, DbGrid& g, int& cellbits, int& nbits) {
    g.ox = box[0]; g.oy = box[1]; g.oz = box[2];
    int mc[3] = {0, 0, 0};
    bool overflow = false;
    for (int k = 0; k < 3; ++k) {
        const double ext = ((double)box[3 + k] - (double)box[k]) * g.inv_cell;
        if (!(ext < 2.0e9)) overflow = true;
        else mc[k] = (int)ext + 1;            // +1: slack for the rounding of the division
    }
    g.mx = mc[0]; g.my = mc[1]; g.mz = mc[2];
    g.bx = db_bits_for((uint64_t)mc[0] + 1); g.by = db_bits_for((uint64_t)mc[1] + 1);
    g.bz = db_bits_for((uint64_t)mc[2] + 1);
    cellbits = g.bx + g.by + g.bz;
    nbits = cellbits + db_bits_for((uint64_t)nchunks);
    return overflow || nbits > 64;
}
__host__ __device__ inline bool db_box_finite(const float* box) {
    for (int k = 0; k < 6; ++k)
        if (!(box[k] == box[k]) || box[k] > 3.0e38f || box[k] < -3.0e38f) return false;
    return true;
}

constexpr int64_t CS_MAX_CHUNK = 1 << 17;     // larger chunks use the global sort
constexpr int64_t CS_MIN_CHUNKS = 96;         // fewer chunks: the global sort keeps more of the GPU busy
constexpr int64_t DB_TABLE_MAX_CHUNKS = 16384;  // beyond: db_cellscatter_k<false>, the table is read off the keys

// The head of stage C planned on the device (the fused call, pch_pipeline.hip): db_headplan_k, one workgroup behind
// stage B's results, plans the grid from the kept rows' box and count as dbscan_run would; db_cellscatter_k<true>,
// db_chunksort_k, db_chunkcells_k and db_celltab_k, launched for the largest count the caller allows for, take n,
// nchunks and the grid from here and return at once when go is clear.  The host reads the block in the wait it makes
// in front of db_celltab_k, plans again on the same box and goes on behind db_celltab_k if both plans agree.
struct DbHead {
    uint32_t go;                 // 1: the staged chunk route runs with the values below
    int32_t  nchunks;
    int64_t  n;                  // rows (stage B's kept count)
    int32_t  cellbits, nbits;
    uint32_t status, ncells, route;     // db_chunkcells_k: DbMeta::status, ncells and the route word, for the host
    uint32_t pad;
    DbGrid   g;
};
// what the host knows when it queues db_headplan_k
struct DbHeadArgs {
    const float*   scalars;      // stage B: [5] != 0 says the fallback threshold applies (the values are not final)
    const int64_t* count;        // stage B: rows kept (< 0: a look-back gave up)
    const float*   aabb;         // stage B: box of the kept rows
    int64_t  plan_n;             // most rows the launches and the workspace are sized for
    int64_t  chunk_size;         // as the caller gave it
    int      sort_mode;          // db_tuning().sort_mode
    uint32_t* clear_from;        // DbWs::clear_from() ..
    uint32_t* chunk_cells;       // .. up to chunk_cells[nchunks + 1], rounded to 16 bytes: zeroed when go is set
};
// a head kernel's first lines: false - return
__device__ __forceinline__ bool db_head_take(const DbHead* __restrict__ head, int64_t& n, DbGrid& g) {
    if (!head) return true;
    if (head->go == 0u || (int64_t)blockIdx.x >= (int64_t)head->nchunks) return false;
    n = head->n;
    g = head->g;
    return true;
}

// (dy,dz) rows ordered by distance so that early exits trigger as soon as possible (static: a copy per
// translation unit)
static __constant__ int8_t DB_ROW_DY[DB_ROWS] = {0, 1, -1, 0, 0, 1, 1, -1, -1, 2, -2, 0, 0,
                                                 2, 2, -2, -2, 1, 1, -1, -1, 2, 2, -2, -2};
static __constant__ int8_t DB_ROW_DZ[DB_ROWS] = {0, 0, 0, 1, -1, 1, -1, 1, -1, 0, 0, 2, -2,
                                                 1, -1, 1, -1, 2, -2, 2, -2, 2, -2, 2, -2};

__device__ __forceinline__ uint64_t db_pack(const DbGrid& g, uint64_t chunk, uint64_t cz,
                                            uint64_t cy, uint64_t cx) {
    return ((((chunk << g.bz) | cz) << g.by | cy) << g.bx) | cx;
}

// the squared distance in float32: one rounding per difference, product and accumulation (db_within2 has the bound)
__device__ __forceinline__ float db_d2f(const float4& a, const float4& b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
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
    const float d = db_d2f(q, p);
    if (d <= g.eps2_lo) return true;
    if (d >= g.eps2_hi) return false;
    return db_within(q, p, g.eps2);
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

// ---- rows and cells of one chunk (db_chunksort_k, db_cellscatter_k; the staged route's readers) ----
struct Row3 { float x, y, z; };               // 4-byte aligned: loads as one global_load_dwordx3
constexpr int CS_THREADS = 1024;
constexpr int CS_WAVES   = CS_THREADS / 64;
constexpr int CS_ROUNDS  = 4;
constexpr int CS_TILE    = CS_THREADS * CS_ROUNDS;
constexpr int CS_PASSES  = 4;
constexpr int CS_HREP    = 4;         // copies of every digit histogram (power of two)
constexpr int CS_BINS    = 512;       // digits of up to 9 bits

// cell key of a row inside its chunk (0 when the row is outside the grid); ok = inside
__device__ __forceinline__ uint32_t cs_cell_key(const DbGrid& g, float x, float y, float z, bool& ok) {
    uint32_t cx, cy, cz;
    ok = db_cell_coords(g, x, y, z, cx, cy, cz);
    return (((cz << g.by) | cy) << g.bx) | cx;
}

// the chunk route's staged cell lists (db_cellscatter_k<true> writes them, db_chunkcells_k and db_celltab_k read)
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

// quick reject in front of db_gather_core_cells: does any cell of the rows of rs hold a core point?  (wave-wide)
__device__ __forceinline__ bool db_any_core(const RowSet* __restrict__ rs, const uint32_t* __restrict__ cell_ncore) {
    const int l = lane_id();
    int any = 0;
    if (l < DB_ROWS)
        for (int B = rs->ca[l]; B < rs->cb[l]; ++B) any |= (cell_ncore[B] != 0);
    return __ballot(any != 0) != 0;
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

void db_plan(Arena& a, int64_t n, DbWs& w);

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

// the run whose workspace the entries of pch_dbscan_query.hip continue, and its cell table
// (nchunks and compressed: what pch_dbscan_assign_f32 needs to know about the grid beyond the cell table; eps: the
// largest radius pch_dbscan_shape_f32 may ask for; plan_n: the rows the workspace was carved for, n or the fused call's
// nf_cap)
struct DbLastRun { void* ws; size_t ws_bytes; int64_t n; DbCells c; int64_t nchunks; bool compressed; double eps;
                   int64_t plan_n; };
extern thread_local DbLastRun g_last;

// The entry points that continue the grid the last pch_dbscan_f32 of this thread left in `ws` carve it up again
// here; `entry` names the caller in the error
int db_continue(const char* entry, int64_t n, void* ws, size_t ws_bytes, DbWs& w);

// blocks of the grid-stride sweeps over the input rows (db_aabb_in_k, db_first_bad_k, db_chunkbad_k)
static unsigned db_stride_blocks(int64_t n) { return (unsigned)std::min(ceil_div(n, DB_THREADS * 8), int64_t(2048)); }

// what the steps of dbscan_run share: the run's rows, outputs, stream and carved workspace
struct DbRun {
    const float* xyz; int64_t n, chunk_size, nchunks;
    int64_t plan_n;              // >= n: what the workspace is carved for (db_plan)
    int32_t* labels; uint8_t* core; int32_t* out_nclusters;
    hipStream_t s; DbWs w;
};

// pch_dbscan.hip
int db_all_noise(const DbRun& r);
int db_cell_bits(DbGrid& g, int mx, int my, int mz);
// db_border_k<false> once more on the retained table c, with the cells' labels as they are now (pch_dbscan_relabel_i32)
int db_border_again(const DbCells& c, const int* cell_label, int32_t* labels, hipStream_t s);
// pch_dbscan_cells.hip
// *first (a device word that holds ~0) becomes the first row of xyz that holds a NaN/inf
int db_first_bad(const float* xyz, int64_t n, unsigned long long* first, hipStream_t s);
int db_compress(const DbRun& r, DbGrid& g, int& cellbits, bool& done);
int db_sorted_keys(const DbRun& r, const DbGrid& g, int cellbits, int nbits, bool compressed, int sort_mode,
                   const uint64_t*& ks, bool& staged);
// head (the fused call's host copy of DbHead): db_celltab_k is queued and status / ncells / route were read
int db_cell_table(const DbRun& r, const DbGrid& g, int cellbits, const uint64_t* ks, bool staged, DbMeta& back,
                  const DbHead* head);
// the fused call: db_headplan_k and the four head kernels on the workspace carved for a.plan_n rows, the peek of
// `peek_bytes` at `peek_dev` (they cover *head) queued in front of db_celltab_k
int db_head_launch(const float* xyz, const DbHeadArgs& a, const DbGrid& proto, const DbWs& w, DbHead* head,
                   const void* peek_dev, size_t peek_bytes, hipStream_t s);
// pch_dbscan.hip, for pch_pipeline.hip
int dbscan_head(const float* xyz, DbHeadArgs a, double eps, int32_t min_samples, void* ws, size_t ws_bytes,
                DbHead* head, const void* peek_dev, size_t peek_bytes, hipStream_t s, bool* queued);

}  // namespace pch
