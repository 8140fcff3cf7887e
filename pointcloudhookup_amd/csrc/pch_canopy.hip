// Canopy grid and tree crowns: the tallest return above the ground per cell of a fine xy grid, the cells
// that are tree tops, the crown of every top, one table record per tree and the tree of every row.  The rule is spelled
// out in include/pch_hip.h; every output is the rule's, bit for bit.
//   top     : tiles of 1024 rows (tl_low_k's skeleton, every row and skip load issued before anything is waited for);
//             the ground under a row through tl_ground_at; the rows of a tile that take part are combined in an
//             open-addressed LDS table of 2048 slots (cell id, largest key (key(H) << 32) | ~row, count; key 0 is
//             "empty"), then every occupied slot issues one 64-bit atomicMax on the key grid and one atomicAdd on count
//   decode  : one thread per cell - the key back to (top, top_row), (NaN, -1) where the count is 0; out_stats
//   smooth  : one thread per cell - the clipped square window of (2S+1)^2 cells, summed in the rule's order
//   parent  : one thread per cell - its window and its eight neighbours; the "is a top" flag and the parent
//   root    : pointer doubling, out[c] = in[in[c]], bits_for(cells) rounds between two buffers
//   count / scan / number : the tops numbered in ascending cell index - per block of 256 cells the number of flags, one
//             workgroup scans the block counts (and writes ntrees), every block then ranks its flags by ballot
//   crown   : one thread per cell - tree[c]; cells, rows and the (max_height, max_row) key by integer atomics per tree
//   table   : one thread per table entry - the key back to (max_height, max_row)
//   rows    : tiles of 1024 rows, tl_height_k's load structure, the ground gathers and one gather of the tree grid
// No inline assembly, no floating-point atomic, nothing waits on another workgroup; the same bits on every run.
#include "pch_common.h"
#include "pch_terrain.h"

#include <math.h>

namespace pch {

constexpr int CN_THREADS = 256;
constexpr int CN_ROUNDS  = 4;
constexpr int CN_TILE    = CN_THREADS * CN_ROUNDS;          // 1024 rows per workgroup
constexpr int CN_SLOTS   = 2048;                            // twice the rows of a tile: the table cannot fill
constexpr int CN_SLOT_BITS = 11;

struct CnRule { TlSub sub; TlGrid terrain, canopy; double h_min, h_max; };
struct CnRow { bool part; int32_t cell; double Hd; };

// (key(H) << 32) | ~row: the largest is the tallest and, among equals, the lowest row; never 0
__device__ __forceinline__ unsigned long long cn_key(float h, int32_t row) {
    return ((unsigned long long)f32_ordered(h) << 32) | (unsigned long long)(~(uint32_t)row);
}
__device__ __forceinline__ float cn_key_value(unsigned long long k) { return f32_unordered((uint32_t)(k >> 32)); }
__device__ __forceinline__ int32_t cn_key_row(unsigned long long k) { return (int32_t)(~(uint32_t)k); }

// The one statement of "takes part" (steps 1 and 9).  p: the row in the row frame; alive: the row exists and is not
// skipped.  Hd is Z - g for a finite row whose ground was looked up (always with want_height), NaN otherwise.
__device__ __forceinline__ CnRow cn_row(const TlRow& p, bool alive, const CnRule& R, const float* __restrict__ ground,
                                        bool want_height) {
    CnRow o;
    o.Hd = (double)tl_nan();
    int fx = 0, fy = 0;
    const bool fin = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    const bool cand = alive && fin && tl_cell(R.canopy, (double)p.x, (double)p.y, fx, fy);
    if (fin && (cand || want_height)) o.Hd = (double)p.z - tl_ground_at(R.terrain, ground, (double)p.x, (double)p.y);
    o.part = cand && R.h_min <= o.Hd && o.Hd <= R.h_max;    // a NaN fails both
    o.cell = fy * R.canopy.nx + fx;
    return o;
}

// stats (2 words, may be null): the rows that took part and the (tile, cell) flushes
__global__ __launch_bounds__(CN_THREADS) void cn_top_k(const float* __restrict__ xyz, const uint8_t* __restrict__ skip,
                                                       int64_t n, CnRule R, const float* __restrict__ ground,
                                                       unsigned long long* __restrict__ gkey,
                                                       int32_t* __restrict__ gcount, float* __restrict__ out_height,
                                                       unsigned long long* __restrict__ stats) {
    __shared__ int32_t ids[CN_SLOTS];
    __shared__ unsigned long long keys[CN_SLOTS];
    __shared__ uint32_t cnt[CN_SLOTS];
    const int w = wave_id(), l = lane_id();
    const int64_t base = (int64_t)blockIdx.x * CN_TILE + (int64_t)w * (64 * CN_ROUNDS);
    const TlRow* __restrict__ rows = reinterpret_cast<const TlRow*>(xyz);
    // every load of the tile is issued before anything is waited for; none stands under a condition
    TlRow q[CN_ROUNDS];
    uint8_t sk[CN_ROUNDS];
#pragma unroll
    for (int r = 0; r < CN_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        q[r] = rows[i < n ? i : 0];
    }
#pragma unroll
    for (int r = 0; r < CN_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        sk[r] = skip ? skip[i < n ? i : 0] : (uint8_t)0;
    }
    for (int j = threadIdx.x; j < CN_SLOTS; j += CN_THREADS) { ids[j] = -1; keys[j] = 0ull; cnt[j] = 0u; }
    __syncthreads();
    uint32_t mine = 0;
#pragma unroll
    for (int r = 0; r < CN_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        const CnRow o = cn_row(tl_frame(q[r], R.sub), i < n && sk[r] == 0, R, ground, out_height != nullptr);
        if (out_height && i < n) out_height[i] = o.Hd != o.Hd ? tl_nan() : (float)o.Hd;
        if (o.part) {
            uint32_t h = ((uint32_t)o.cell * 2654435761u) >> (32 - CN_SLOT_BITS);
            for (;;) {
                const int32_t prev = atomicCAS(&ids[h], -1, o.cell);
                if (prev == -1 || prev == o.cell) break;
                h = (h + 1) & (CN_SLOTS - 1);
            }
            atomicMax(&keys[h], cn_key((float)o.Hd, (int32_t)i));
            atomicAdd(&cnt[h], 1u);
            ++mine;
        }
    }
    __syncthreads();
    uint32_t flushed = 0;
    for (int j = threadIdx.x; j < CN_SLOTS; j += CN_THREADS) {
        const int32_t c = ids[j];
        if (c >= 0) {
            atomicMax(&gkey[c], keys[j]);
            atomicAdd(&gcount[c], (int32_t)cnt[j]);
            ++flushed;
        }
    }
    if (stats) {
        mine = wave_reduce_add(mine);
        flushed = wave_reduce_add(flushed);
        if (l == 0 && mine) atomicAdd(&stats[0], (unsigned long long)mine);
        if (l == 0 && flushed) atomicAdd(&stats[1], (unsigned long long)flushed);
    }
}

__global__ __launch_bounds__(CN_THREADS) void cn_decode_k(const unsigned long long* __restrict__ gkey,
                                                          const int32_t* __restrict__ gcount, int ncells,
                                                          float* __restrict__ out_top, int32_t* __restrict__ out_top_row,
                                                          const unsigned long long* __restrict__ stats,
                                                          int64_t* __restrict__ out_stats) {
    const int c = blockIdx.x * CN_THREADS + threadIdx.x;
    if (out_stats && c < 2) out_stats[c] = (int64_t)stats[c];
    if (c >= ncells) return;
    const bool has = gcount[c] > 0;
    out_top[c] = has ? cn_key_value(gkey[c]) : tl_nan();
    out_top_row[c] = has ? cn_key_row(gkey[c]) : -1;
}

__global__ __launch_bounds__(CN_THREADS) void cn_rows_k(const float* __restrict__ xyz, const uint8_t* __restrict__ skip,
                                                        int64_t n, CnRule R, const float* __restrict__ ground,
                                                        const int32_t* __restrict__ tree, int32_t* __restrict__ out_tree) {
    const int w = wave_id(), l = lane_id();
    const int64_t base = (int64_t)blockIdx.x * CN_TILE + (int64_t)w * (64 * CN_ROUNDS);
    const TlRow* __restrict__ rows = reinterpret_cast<const TlRow*>(xyz);
    TlRow q[CN_ROUNDS];
    uint8_t sk[CN_ROUNDS];
#pragma unroll
    for (int r = 0; r < CN_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        q[r] = rows[i < n ? i : 0];
    }
#pragma unroll
    for (int r = 0; r < CN_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        sk[r] = skip ? skip[i < n ? i : 0] : (uint8_t)0;
    }
    int32_t t[CN_ROUNDS];
#pragma unroll
    for (int r = 0; r < CN_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        const CnRow o = cn_row(tl_frame(q[r], R.sub), i < n && sk[r] == 0, R, ground, false);
        t[r] = o.part ? tree[o.cell] : -1;
    }
#pragma unroll
    for (int r = 0; r < CN_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        if (i < n) out_tree[i] = t[r];
    }
}

// ------------------------------------------------------------------ grid-sized kernels (steps 2 - 8)
__device__ __forceinline__ bool cn_beats(float a, int ca, float b, int cb) { return a > b || (a == b && ca < cb); }

__global__ __launch_bounds__(CN_THREADS) void cn_smooth_k(const float* __restrict__ top, int nx, int ny, int S,
                                                          float* __restrict__ sm) {
    const int c = blockIdx.x * CN_THREADS + threadIdx.x;
    if (c >= nx * ny) return;
    const float own = top[c];
    if (own != own) { sm[c] = tl_nan(); return; }
    const int fy = c / nx, fx = c - fy * nx;
    const int y0 = fy - S > 0 ? fy - S : 0, y1 = fy + S < ny - 1 ? fy + S : ny - 1;
    const int x0 = fx - S > 0 ? fx - S : 0, x1 = fx + S < nx - 1 ? fx + S : nx - 1;
    double sum = 0.0;
    int cnt = 0;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
            const float v = top[(size_t)y * nx + x];
            if (v != v) continue;
            sum = sum + (double)v;
            cnt = cnt + 1;
        }
    sm[c] = (float)(sum / (double)cnt);
}

// flag[c]: c is a top; parent[c]: the rule's, c itself for a cell without a value
__global__ __launch_bounds__(CN_THREADS) void cn_parent_k(const float* __restrict__ sm, int nx, int ny, double cell,
                                                          double r0, double r1, double top_min,
                                                          int32_t* __restrict__ parent, uint8_t* __restrict__ flag) {
    const int c = blockIdx.x * CN_THREADS + threadIdx.x;
    if (c >= nx * ny) return;
    const float s = sm[c];
    if (s != s) { parent[c] = c; flag[c] = 0; return; }
    const int fy = c / nx, fx = c - fy * nx;
    const double q = floor((r0 + (r1 * (double)s)) / cell);
    int W = 1;
    if (q >= 1.0) W = q > (double)PCH_CANOPY_MAX_WINDOW ? PCH_CANOPY_MAX_WINDOW : (int)q;
    // the greatest cell of the window
    int wc = -1;
    float wv = 0.0f;
    const int y0 = fy - W > 0 ? fy - W : 0, y1 = fy + W < ny - 1 ? fy + W : ny - 1;
    const int x0 = fx - W > 0 ? fx - W : 0, x1 = fx + W < nx - 1 ? fx + W : nx - 1;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
            const int dx = x - fx, dy = y - fy;
            if ((dx == 0 && dy == 0) || dx * dx + dy * dy > W * W) continue;
            const int k = y * nx + x;
            const float v = sm[k];
            if (v != v) continue;
            if (wc < 0 || cn_beats(v, k, wv, wc)) { wc = k; wv = v; }
        }
    const bool beaten = wc >= 0 && cn_beats(wv, wc, s, c);
    flag[c] = ((double)s >= top_min && !beaten) ? 1 : 0;
    // the greatest of the eight neighbours
    int bc = -1;
    float bv = 0.0f;
    for (int y = (fy > 0 ? fy - 1 : 0); y <= (fy < ny - 1 ? fy + 1 : ny - 1); ++y)
        for (int x = (fx > 0 ? fx - 1 : 0); x <= (fx < nx - 1 ? fx + 1 : nx - 1); ++x) {
            const int k = y * nx + x;
            if (k == c) continue;
            const float v = sm[k];
            if (v != v) continue;
            if (bc < 0 || cn_beats(v, k, bv, bc)) { bc = k; bv = v; }
        }
    parent[c] = (bc >= 0 && cn_beats(bv, bc, s, c)) ? bc : (beaten ? wc : c);
}

__global__ __launch_bounds__(CN_THREADS) void cn_root_k(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                        int ncells) {
    const int c = blockIdx.x * CN_THREADS + threadIdx.x;
    if (c < ncells) out[c] = in[in[c]];
}

// the number of flags in every block of CN_THREADS cells
__global__ __launch_bounds__(CN_THREADS) void cn_count_k(const uint8_t* __restrict__ flag, int ncells,
                                                         int32_t* __restrict__ bcount) {
    __shared__ int32_t wsum[CN_THREADS / 64];
    const int c = blockIdx.x * CN_THREADS + threadIdx.x;
    const unsigned long long m = __ballot(c < ncells && flag[c < ncells ? c : 0] != 0);
    if (lane_id() == 0) wsum[wave_id()] = (int32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) bcount[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
static_assert(CN_THREADS == 256, "cn_count_k and cn_number_k sum four wave totals");

// ONE workgroup: bcount[nb] becomes its exclusive prefix sum in place, *ntrees the total
__global__ __launch_bounds__(CN_THREADS) void cn_scan_k(int32_t* __restrict__ bcount, int nb,
                                                        int32_t* __restrict__ ntrees) {
    __shared__ int32_t part[CN_THREADS];
    const int per = (nb + CN_THREADS - 1) / CN_THREADS;
    const int lo = threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    int32_t sum = 0;
    for (int b = lo; b < hi; ++b) sum += bcount[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t run = 0;
        for (int t = 0; t < CN_THREADS; ++t) { const int32_t v = part[t]; part[t] = run; run += v; }
        *ntrees = run;
    }
    __syncthreads();
    int32_t run = part[threadIdx.x];
    for (int b = lo; b < hi; ++b) { const int32_t v = bcount[b]; bcount[b] = run; run += v; }
}

// id_of[c]: the number of top c, -1 for a cell that is no top; the table's top_cell for the tops below the cap
__global__ __launch_bounds__(CN_THREADS) void cn_number_k(const uint8_t* __restrict__ flag, int ncells,
                                                          const int32_t* __restrict__ boff, int32_t cap,
                                                          int32_t* __restrict__ id_of, int32_t* __restrict__ out_top_cell) {
    __shared__ int32_t wsum[CN_THREADS / 64];
    const int c = blockIdx.x * CN_THREADS + threadIdx.x;
    const bool is = c < ncells && flag[c < ncells ? c : 0] != 0;
    const unsigned long long m = __ballot(is);
    if (lane_id() == 0) wsum[wave_id()] = (int32_t)__popcll(m);
    __syncthreads();
    if (c >= ncells) return;
    int32_t t = boff[blockIdx.x] + (int32_t)__popcll(m & lanemask_lt());
    for (int w2 = 0; w2 < wave_id(); ++w2) t += wsum[w2];
    id_of[c] = is ? t : -1;
    if (is && t < cap) out_top_cell[t] = c;
}

__global__ __launch_bounds__(CN_THREADS) void cn_crown_k(const float* __restrict__ sm, const float* __restrict__ top,
                                                         const int32_t* __restrict__ top_row,
                                                         const int32_t* __restrict__ count,
                                                         const int32_t* __restrict__ root,
                                                         const int32_t* __restrict__ id_of, int nx, int ny,
                                                         double crown_frac, int Rc, int32_t cap,
                                                         int32_t* __restrict__ tree, int32_t* __restrict__ tcells,
                                                         unsigned long long* __restrict__ trows,
                                                         unsigned long long* __restrict__ tkey) {
    const int c = blockIdx.x * CN_THREADS + threadIdx.x;
    if (c >= nx * ny) return;
    const float s = sm[c];
    int32_t t = -1;
    if (s == s) {
        const int32_t r = root[c];
        const int32_t tr = id_of[r];
        if (tr >= 0) {
            const int64_t dx = (int64_t)(c % nx) - (int64_t)(r % nx), dy = (int64_t)(c / nx) - (int64_t)(r / nx);
            if ((double)s >= (crown_frac * (double)sm[r]) && dx * dx + dy * dy <= (int64_t)Rc * Rc) t = tr;
        }
    }
    tree[c] = t;
    if (t >= 0 && t < cap) {
        atomicAdd(&tcells[t], 1);
        atomicAdd(&trows[t], (unsigned long long)(long long)count[c]);
        atomicMax(&tkey[t], cn_key(top[c], top_row[c]));
    }
}

__global__ __launch_bounds__(CN_THREADS) void cn_table_k(const unsigned long long* __restrict__ tkey,
                                                         const int32_t* __restrict__ ntrees, int32_t cap,
                                                         float* __restrict__ out_max_height,
                                                         int32_t* __restrict__ out_max_row) {
    const int t = blockIdx.x * CN_THREADS + threadIdx.x;
    if (t >= cap) return;
    const unsigned long long k = tkey[t];
    const bool has = t < *ntrees && k != 0ull;
    out_max_height[t] = has ? cn_key_value(k) : tl_nan();
    out_max_row[t] = has ? cn_key_row(k) : -1;
}

struct CnTopWs { unsigned long long *key, *stats; };
static void cn_top_plan(Arena& a, int32_t ncells, CnTopWs& w) {
    w.key = a.take<unsigned long long>((size_t)ncells);
    w.stats = a.take<unsigned long long>(2);
}
struct CnTreesWs { float* sm; int32_t *pa, *pb, *pc, *id_of, *bcount; uint8_t* flag; unsigned long long* tkey; };
static void cn_trees_plan(Arena& a, int32_t ncells, int32_t cap, CnTreesWs& w) {
    w.sm = a.take<float>((size_t)ncells);
    w.pa = a.take<int32_t>((size_t)ncells);
    w.pb = a.take<int32_t>((size_t)ncells);
    w.pc = a.take<int32_t>((size_t)ncells);
    w.id_of = a.take<int32_t>((size_t)ncells);
    w.bcount = a.take<int32_t>((size_t)ceil_div(ncells, CN_THREADS));
    w.flag = a.take<uint8_t>((size_t)ncells);
    w.tkey = a.take<unsigned long long>((size_t)cap);
}
static bool cn_cap_ok(int32_t cap) { return cap >= 1 && cap <= PCH_TERRAIN_MAX_CELLS; }
// the rule of steps 1 and 9 as the kernels take it; false for arguments outside its limits
static bool cn_rule_of(const float* sub3_host, const PchTerrainGrid* terrain_host, const PchTerrainGrid* canopy_host,
                       double h_min, double h_max, CnRule& R) {
    if (!tl_grid_of(terrain_host, R.terrain) || !tl_grid_of(canopy_host, R.canopy)) return false;
    if (!(isfinite(h_min) && isfinite(h_max) && 0.0 <= h_min && h_min <= h_max)) return false;
    R.sub = tl_sub_of(sub3_host);
    R.h_min = h_min;
    R.h_max = h_max;
    return true;
}
#define CN_RULE_TEXT "both grids need cell > 0 and finite, nx, ny >= 1 and nx * ny <= 2^24; 0 <= h_min <= h_max, finite"

}  // namespace pch

using namespace pch;

extern "C" size_t pch_canopy_top_ws_bytes(int64_t n, int32_t ncells) {
    if (!tl_rows_ok(n) || !tl_cells_ok(ncells)) return 0;
    Arena a;
    CnTopWs w;
    cn_top_plan(a, ncells, w);
    return a.off;
}

extern "C" int pch_canopy_top_f32(const float* xyz, const uint8_t* skip, int64_t n, const float* sub3_host,
                                  const PchTerrainGrid* terrain_host, const float* ground,
                                  const PchTerrainGrid* canopy_host, double h_min, double h_max, float* out_top,
                                  int32_t* out_top_row, int32_t* out_count, float* out_height, int64_t* out_stats,
                                  void* ws, size_t ws_bytes, void* stream) {
    PCH_REQUIRE(tl_rows_ok(n), "0 <= n < 2^31");
    CnRule R;
    PCH_REQUIRE(cn_rule_of(sub3_host, terrain_host, canopy_host, h_min, h_max, R), CN_RULE_TEXT);
    PCH_REQUIRE(ground, "null ground grid");
    PCH_REQUIRE(n == 0 || xyz, "null row buffer");
    PCH_REQUIRE(out_top && out_top_row && out_count, "null grid buffer");
    PCH_REQUIRE(ws, "null workspace");
    PCH_DEVICE_GUARD(ws);
    {
        DeviceGuard in(ground);
        if (in.rc != PCH_OK) return in.rc;
    }
    hipStream_t s = (hipStream_t)stream;
    const int32_t ncells = R.canopy.nx * R.canopy.ny;
    Arena a(ws, ws_bytes);
    CnTopWs w;
    cn_top_plan(a, ncells, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    PCH_HIP_TRY(hipMemsetAsync(w.key, 0, sizeof(unsigned long long) * (size_t)ncells, s));
    PCH_HIP_TRY(hipMemsetAsync(w.stats, 0, 2 * sizeof(unsigned long long), s));
    PCH_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(int32_t) * (size_t)ncells, s));
    if (n > 0)
        PCH_LAUNCH("canopy_top", cn_top_k, dim3((unsigned)ceil_div(n, CN_TILE)), dim3(CN_THREADS), 0, s, xyz, skip, n, R,
                   ground, w.key, out_count, out_height, out_stats ? w.stats : (unsigned long long*)nullptr);
    PCH_LAUNCH("canopy_decode", cn_decode_k, dim3((unsigned)ceil_div(ncells, CN_THREADS)), dim3(CN_THREADS), 0, s,
               (const unsigned long long*)w.key, (const int32_t*)out_count, (int)ncells, out_top, out_top_row,
               (const unsigned long long*)w.stats, out_stats);
    return PCH_OK;
}

extern "C" size_t pch_canopy_trees_ws_bytes(int32_t ncells, int32_t tree_cap) {
    if (!tl_cells_ok(ncells) || !cn_cap_ok(tree_cap)) return 0;
    Arena a;
    CnTreesWs w;
    cn_trees_plan(a, ncells, tree_cap, w);
    return a.off;
}

extern "C" int pch_canopy_trees_f32(const float* top, const int32_t* top_row, const int32_t* count,
                                    const PchTerrainGrid* canopy_host, int32_t smooth, double r0, double r1,
                                    double top_min, double crown_frac, int32_t crown_cells, int32_t tree_cap,
                                    float* out_smooth, int32_t* out_tree, int32_t* out_ntrees, int32_t* out_top_cell,
                                    int32_t* out_cells, int64_t* out_rows, float* out_max_height, int32_t* out_max_row,
                                    void* ws, size_t ws_bytes, void* stream) {
    TlGrid g;
    PCH_REQUIRE(tl_grid_of(canopy_host, g), "the grid needs cell > 0 and finite, nx, ny >= 1 and nx * ny <= 2^24");
    PCH_REQUIRE(smooth >= 0 && smooth <= PCH_CANOPY_MAX_SMOOTH, "0 <= smooth <= 8");
    PCH_REQUIRE(isfinite(r0) && isfinite(r1) && r0 >= 0.0 && r1 >= 0.0, "r0 and r1 must be finite and >= 0");
    PCH_REQUIRE(isfinite(top_min) && top_min >= 0.0, "top_min must be finite and >= 0");
    PCH_REQUIRE(crown_frac >= 0.0 && crown_frac <= 1.0, "0 <= crown_frac <= 1");
    PCH_REQUIRE(crown_cells >= 1 && crown_cells <= PCH_CANOPY_MAX_CROWN, "1 <= crown_cells <= 256");
    PCH_REQUIRE(cn_cap_ok(tree_cap), "1 <= tree_cap <= 2^24");
    PCH_REQUIRE(top && top_row && count && out_tree && out_ntrees, "null grid buffer");
    PCH_REQUIRE(out_top_cell && out_cells && out_rows && out_max_height && out_max_row, "null table buffer");
    PCH_REQUIRE(ws, "null workspace");
    PCH_DEVICE_GUARD(ws);
    {
        DeviceGuard in(top);
        if (in.rc != PCH_OK) return in.rc;
    }
    hipStream_t s = (hipStream_t)stream;
    const int32_t ncells = g.nx * g.ny;
    Arena a(ws, ws_bytes);
    CnTreesWs w;
    cn_trees_plan(a, ncells, tree_cap, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    float* sm = out_smooth ? out_smooth : w.sm;
    const int nb = (int)ceil_div(ncells, CN_THREADS);
    const dim3 grid((unsigned)nb), block(CN_THREADS), tgrid((unsigned)ceil_div(tree_cap, CN_THREADS));
    PCH_HIP_TRY(hipMemsetAsync(out_top_cell, 0xFF, sizeof(int32_t) * (size_t)tree_cap, s));
    PCH_HIP_TRY(hipMemsetAsync(out_cells, 0, sizeof(int32_t) * (size_t)tree_cap, s));
    PCH_HIP_TRY(hipMemsetAsync(out_rows, 0, sizeof(int64_t) * (size_t)tree_cap, s));
    PCH_HIP_TRY(hipMemsetAsync(w.tkey, 0, sizeof(unsigned long long) * (size_t)tree_cap, s));
    PCH_LAUNCH("canopy_smooth", cn_smooth_k, grid, block, 0, s, top, g.nx, g.ny, (int)smooth, sm);
    PCH_LAUNCH("canopy_parent", cn_parent_k, grid, block, 0, s, (const float*)sm, g.nx, g.ny, g.cell, r0, r1, top_min,
               w.pa, w.flag);
    // roots: after k rounds a cell points 2^k steps up its chain, and no chain has ncells steps
    const int32_t* root = w.pa;
    int32_t* next = w.pb;
    for (int k = 0; k < bits_for((uint64_t)ncells); ++k) {
        PCH_LAUNCH("canopy_root", cn_root_k, grid, block, 0, s, root, next, (int)ncells);
        root = next;
        next = next == w.pb ? w.pc : w.pb;
    }
    PCH_LAUNCH("canopy_count", cn_count_k, grid, block, 0, s, (const uint8_t*)w.flag, (int)ncells, w.bcount);
    PCH_LAUNCH("canopy_scan", cn_scan_k, dim3(1), block, 0, s, w.bcount, nb, out_ntrees);
    PCH_LAUNCH("canopy_number", cn_number_k, grid, block, 0, s, (const uint8_t*)w.flag, (int)ncells,
               (const int32_t*)w.bcount, tree_cap, w.id_of, out_top_cell);
    PCH_LAUNCH("canopy_crown", cn_crown_k, grid, block, 0, s, (const float*)sm, top, top_row, count, root,
               (const int32_t*)w.id_of, g.nx, g.ny, crown_frac, (int)crown_cells, tree_cap, out_tree, out_cells,
               reinterpret_cast<unsigned long long*>(out_rows), w.tkey);
    PCH_LAUNCH("canopy_table", cn_table_k, tgrid, block, 0, s, (const unsigned long long*)w.tkey,
               (const int32_t*)out_ntrees, tree_cap, out_max_height, out_max_row);
    return PCH_OK;
}

extern "C" int pch_canopy_rows_f32(const float* xyz, const uint8_t* skip, int64_t n, const float* sub3_host,
                                   const PchTerrainGrid* terrain_host, const float* ground,
                                   const PchTerrainGrid* canopy_host, double h_min, double h_max, const int32_t* tree,
                                   int32_t* out_tree, void* stream) {
    PCH_REQUIRE(tl_rows_ok(n), "0 <= n < 2^31");
    CnRule R;
    PCH_REQUIRE(cn_rule_of(sub3_host, terrain_host, canopy_host, h_min, h_max, R), CN_RULE_TEXT);
    PCH_REQUIRE(ground && tree, "null grid buffer");
    PCH_REQUIRE(n == 0 || (xyz && out_tree), "null row buffer");
    PCH_DEVICE_GUARD(ground);
    {
        DeviceGuard in(tree);
        if (in.rc != PCH_OK) return in.rc;
    }
    if (n == 0) return PCH_OK;
    {
        DeviceGuard in(xyz);
        if (in.rc != PCH_OK) return in.rc;
    }
    hipStream_t s = (hipStream_t)stream;
    PCH_LAUNCH("canopy_rows", cn_rows_k, dim3((unsigned)ceil_div(n, CN_TILE)), dim3(CN_THREADS), 0, s, xyz, skip, n, R,
               ground, tree, out_tree);
    return PCH_OK;
}
