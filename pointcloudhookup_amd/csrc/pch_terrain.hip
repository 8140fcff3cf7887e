// Terrain grid: the lowest return per cell of an xy grid, the ground cells by a morphological opening
// and the fill of the rest, the height of every row above that ground and the ground under a position.  The rule is
// spelled out in include/pch_hip.h; every output is the rule's, bit for bit.
//   low     : tiles of 1024 rows (cl_sweep_k's structure, every load issued before anything is waited for); the rows
//             of a tile are combined in an open-addressed LDS table of 2048 slots (cell id, smallest key, count), then
//             every occupied slot issues one global atomicMin on the key grid and one atomicAdd on the counts
//   decode  : one thread per cell - the key back to a float, NaN where the count is 0; the two figures of out_stats
//   open    : one thread per cell and pass - the clipped window of 2R+1 cells along one axis, minimum or maximum
//   accept  : one thread per cell - the "is ground" flag
//   fill    : one thread per cell - ground and state; the walk of at most 4 G cells for a cell that is not ground
//   height  : tiles of 1024 rows, four gathers of the ground grid per row; sample: the same on float64 positions
// No inline assembly, no floating-point atomic, nothing waits on another workgroup; the same bits on every run.
#include "pch_common.h"
#include "pch_terrain.h"

#include <math.h>

namespace pch {

constexpr int TL_THREADS = 256;
constexpr int TL_ROUNDS  = 4;
constexpr int TL_TILE    = TL_THREADS * TL_ROUNDS;          // 1024 rows per workgroup
constexpr int TL_SLOTS   = 2048;                            // twice the rows of a tile: the table cannot fill
constexpr int TL_SLOT_BITS = 11;

// stats (2 words, may be null): the rows that took part and the (tile, cell) flushes
__global__ __launch_bounds__(TL_THREADS) void tl_low_k(const float* __restrict__ xyz, const uint8_t* __restrict__ skip,
                                                       int64_t n, TlSub sub, TlGrid g, uint32_t* __restrict__ gkey,
                                                       int32_t* __restrict__ gcount,
                                                       unsigned long long* __restrict__ stats) {
    __shared__ int32_t ids[TL_SLOTS];
    __shared__ uint32_t keys[TL_SLOTS];
    __shared__ uint32_t cnt[TL_SLOTS];
    const int w = wave_id(), l = lane_id();
    const int64_t base = (int64_t)blockIdx.x * TL_TILE + (int64_t)w * (64 * TL_ROUNDS);
    const TlRow* __restrict__ rows = reinterpret_cast<const TlRow*>(xyz);
    // every load of the tile is issued before anything is waited for; none stands under a condition
    TlRow q[TL_ROUNDS];
    uint8_t sk[TL_ROUNDS];
#pragma unroll
    for (int r = 0; r < TL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        q[r] = rows[i < n ? i : 0];
    }
#pragma unroll
    for (int r = 0; r < TL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        sk[r] = skip ? skip[i < n ? i : 0] : (uint8_t)0;
    }
    for (int j = threadIdx.x; j < TL_SLOTS; j += TL_THREADS) { ids[j] = -1; keys[j] = 0xFFFFFFFFu; cnt[j] = 0u; }
    __syncthreads();
    uint32_t mine = 0;
#pragma unroll
    for (int r = 0; r < TL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        const TlRow p = tl_frame(q[r], sub);
        int fx = 0, fy = 0;
        const bool in = tl_cell(g, (double)p.x, (double)p.y, fx, fy);
        if (i < n && sk[r] == 0 && in && isfinite(p.z)) {
            const int32_t c = fy * g.nx + fx;
            uint32_t h = ((uint32_t)c * 2654435761u) >> (32 - TL_SLOT_BITS);
            for (;;) {
                const int32_t prev = atomicCAS(&ids[h], -1, c);
                if (prev == -1 || prev == c) break;
                h = (h + 1) & (TL_SLOTS - 1);
            }
            atomicMin(&keys[h], f32_ordered(p.z));
            atomicAdd(&cnt[h], 1u);
            ++mine;
        }
    }
    __syncthreads();
    uint32_t flushed = 0;
    for (int j = threadIdx.x; j < TL_SLOTS; j += TL_THREADS) {
        const int32_t c = ids[j];
        if (c >= 0) {
            atomicMin(&gkey[c], keys[j]);
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

__global__ __launch_bounds__(TL_THREADS) void tl_decode_k(const uint32_t* __restrict__ gkey,
                                                          const int32_t* __restrict__ gcount, int ncells,
                                                          float* __restrict__ out_low,
                                                          const unsigned long long* __restrict__ stats,
                                                          int64_t* __restrict__ out_stats) {
    const int c = blockIdx.x * TL_THREADS + threadIdx.x;
    if (out_stats && c < 2) out_stats[c] = (int64_t)stats[c];
    if (c >= ncells) return;
    out_low[c] = gcount[c] > 0 ? f32_unordered(gkey[c]) : tl_nan();
}

// one pass of the opening: the clipped window of 2R+1 cells along x (axis 0) or y (axis 1), the minimum or the maximum
// of its non-NaN cells in ascending index, the first met of equal values kept
__global__ __launch_bounds__(TL_THREADS) void tl_open_k(const float* __restrict__ in, float* __restrict__ out, int nx,
                                                        int ny, int R, int axis, int domax) {
    const int c = blockIdx.x * TL_THREADS + threadIdx.x;
    if (c >= nx * ny) return;
    const int fy = c / nx, fx = c - fy * nx;
    const int at = axis ? fy : fx, len = axis ? ny : nx, stride = axis ? nx : 1;
    const int lo = at - R > 0 ? at - R : 0, hi = at + R < len - 1 ? at + R : len - 1;
    const float* __restrict__ line = in + (axis ? fx : fy * nx);
    float acc = tl_nan();
    for (int k = lo; k <= hi; ++k) {
        const float v = line[(size_t)k * stride];
        if (v != v) continue;
        if (acc != acc) acc = v;
        else if (domax ? v > acc : v < acc) acc = v;
    }
    out[c] = acc;
}

__global__ __launch_bounds__(TL_THREADS) void tl_accept_k(const float* __restrict__ low, const float* __restrict__ open,
                                                          int ncells, double dh, uint8_t* __restrict__ isg) {
    const int c = blockIdx.x * TL_THREADS + threadIdx.x;
    if (c >= ncells) return;
    const float lw = low[c];
    isg[c] = (lw == lw && ((double)lw - (double)open[c]) <= dh) ? 1 : 0;
}

__global__ __launch_bounds__(TL_THREADS) void tl_fill_k(const float* __restrict__ low, const uint8_t* __restrict__ isg,
                                                        int nx, int ny, int G, float* __restrict__ out_ground,
                                                        uint8_t* __restrict__ out_state) {
    const int c = blockIdx.x * TL_THREADS + threadIdx.x;
    if (c >= nx * ny) return;
    const float lw = low[c];
    const uint8_t rows = lw == lw ? 4 : 0;
    if (isg[c]) { out_ground[c] = lw; out_state[c] = 1 | rows; return; }
    const int fy = c / nx, fx = c - fy * nx;
    double num = 0.0, den = 0.0;
    bool found = false;
    const int dxs[4] = {-1, 1, 0, 0}, dys[4] = {0, 0, -1, 1};
#pragma unroll
    for (int dir = 0; dir < 4; ++dir) {
        for (int d = 1; d <= G; ++d) {
            const int x = fx + d * dxs[dir], y = fy + d * dys[dir];
            if (x < 0 || x >= nx || y < 0 || y >= ny) break;
            const int k = y * nx + x;
            if (isg[k]) {
                num = num + ((double)low[k] / (double)d);
                den = den + (1.0 / (double)d);
                found = true;
                break;
            }
        }
    }
    out_ground[c] = found ? (float)(num / den) : tl_nan();
    out_state[c] = (found ? 2 : 0) | rows;
}

__global__ __launch_bounds__(TL_THREADS) void tl_height_k(const float* __restrict__ xyz, int64_t n, TlSub sub, TlGrid g,
                                                          const float* __restrict__ ground,
                                                          float* __restrict__ out_height,
                                                          float* __restrict__ out_ground) {
    const int w = wave_id(), l = lane_id();
    const int64_t base = (int64_t)blockIdx.x * TL_TILE + (int64_t)w * (64 * TL_ROUNDS);
    const TlRow* __restrict__ rows = reinterpret_cast<const TlRow*>(xyz);
    TlRow q[TL_ROUNDS];
#pragma unroll
    for (int r = 0; r < TL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        q[r] = rows[i < n ? i : 0];
    }
    double gv[TL_ROUNDS];
#pragma unroll
    for (int r = 0; r < TL_ROUNDS; ++r) {
        q[r] = tl_frame(q[r], sub);
        const bool fin = isfinite(q[r].x) && isfinite(q[r].y) && isfinite(q[r].z);
        gv[r] = fin ? tl_ground_at(g, ground, (double)q[r].x, (double)q[r].y) : (double)tl_nan();
    }
#pragma unroll
    for (int r = 0; r < TL_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + l;
        if (i >= n) continue;
        const bool none = gv[r] != gv[r];
        out_height[i] = none ? tl_nan() : (float)((double)q[r].z - gv[r]);
        if (out_ground) out_ground[i] = none ? tl_nan() : (float)gv[r];
    }
}

__global__ __launch_bounds__(TL_THREADS) void tl_sample_k(const double* __restrict__ xy, int64_t m, TlGrid g,
                                                          const float* __restrict__ ground, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * TL_THREADS + threadIdx.x;
    if (i >= m) return;
    const double X = xy[2 * i], Y = xy[2 * i + 1];
    const double v = tl_ground_at(g, ground, X, Y);
    out[i] = v != v ? (double)tl_nan() : v;
}

struct TlLowWs { uint32_t* key; unsigned long long* stats; };
static void tl_low_plan(Arena& a, int32_t ncells, TlLowWs& w) {
    w.key = a.take<uint32_t>((size_t)ncells);
    w.stats = a.take<unsigned long long>(2);
}
struct TlGroundWs { float *a, *b, *open; uint8_t* isg; };
static void tl_ground_plan(Arena& a, int32_t ncells, TlGroundWs& w) {
    w.a = a.take<float>((size_t)ncells);
    w.b = a.take<float>((size_t)ncells);
    w.open = a.take<float>((size_t)ncells);
    w.isg = a.take<uint8_t>((size_t)ncells);
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_terrain_low_ws_bytes(int64_t n, int32_t ncells) {
    if (!tl_rows_ok(n) || !tl_cells_ok(ncells)) return 0;
    Arena a;
    TlLowWs w;
    tl_low_plan(a, ncells, w);
    return a.off;
}

extern "C" int pch_terrain_low_f32(const float* xyz, const uint8_t* skip, int64_t n, const float* sub3_host,
                                   const PchTerrainGrid* grid_host, float* out_low, int32_t* out_count,
                                   int64_t* out_stats, void* ws, size_t ws_bytes, void* stream) {
    PCH_REQUIRE(tl_rows_ok(n), "0 <= n < 2^31");
    TlGrid g;
    PCH_REQUIRE(tl_grid_of(grid_host, g), "the grid needs cell > 0 and finite, nx, ny >= 1 and nx * ny <= 2^24");
    PCH_REQUIRE(n == 0 || xyz, "null row buffer");
    PCH_REQUIRE(out_low && out_count, "null grid buffer");
    PCH_REQUIRE(ws, "null workspace");
    PCH_DEVICE_GUARD(ws);
    hipStream_t s = (hipStream_t)stream;
    const int32_t ncells = g.nx * g.ny;
    Arena a(ws, ws_bytes);
    TlLowWs w;
    tl_low_plan(a, ncells, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    PCH_HIP_TRY(hipMemsetAsync(w.key, 0xFF, sizeof(uint32_t) * (size_t)ncells, s));
    PCH_HIP_TRY(hipMemsetAsync(w.stats, 0, 2 * sizeof(unsigned long long), s));
    PCH_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(int32_t) * (size_t)ncells, s));
    if (n > 0)
        PCH_LAUNCH("terrain_low", tl_low_k, dim3((unsigned)ceil_div(n, TL_TILE)), dim3(TL_THREADS), 0, s, xyz, skip, n,
                   tl_sub_of(sub3_host), g, w.key, out_count, out_stats ? w.stats : (unsigned long long*)nullptr);
    PCH_LAUNCH("terrain_decode", tl_decode_k, dim3((unsigned)ceil_div(ncells, TL_THREADS)), dim3(TL_THREADS), 0, s,
               (const uint32_t*)w.key, (const int32_t*)out_count, (int)ncells, out_low,
               (const unsigned long long*)w.stats, out_stats);
    return PCH_OK;
}

extern "C" size_t pch_terrain_ground_ws_bytes(int32_t ncells) {
    if (!tl_cells_ok(ncells)) return 0;
    Arena a;
    TlGroundWs w;
    tl_ground_plan(a, ncells, w);
    return a.off;
}

extern "C" int pch_terrain_ground_f32(const float* low, const PchTerrainGrid* grid_host, int32_t window_cells, double dh,
                                      int32_t max_gap, float* out_open, float* out_ground, uint8_t* out_state, void* ws,
                                      size_t ws_bytes, void* stream) {
    TlGrid g;
    PCH_REQUIRE(tl_grid_of(grid_host, g), "the grid needs cell > 0 and finite, nx, ny >= 1 and nx * ny <= 2^24");
    PCH_REQUIRE(window_cells >= 0 && window_cells <= PCH_TERRAIN_MAX_WINDOW, "0 <= window_cells <= 64");
    PCH_REQUIRE(isfinite(dh) && dh >= 0.0, "dh must be finite and >= 0");
    PCH_REQUIRE(max_gap >= 0 && max_gap <= PCH_TERRAIN_MAX_GAP, "0 <= max_gap <= 256");
    PCH_REQUIRE(low && out_ground && out_state, "null grid buffer");
    PCH_REQUIRE(ws, "null workspace");
    PCH_DEVICE_GUARD(ws);
    {
        DeviceGuard in(low);
        if (in.rc != PCH_OK) return in.rc;
    }
    hipStream_t s = (hipStream_t)stream;
    const int32_t ncells = g.nx * g.ny;
    Arena a(ws, ws_bytes);
    TlGroundWs w;
    tl_ground_plan(a, ncells, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    float* open = out_open ? out_open : w.open;
    const dim3 grid((unsigned)ceil_div(ncells, TL_THREADS)), block(TL_THREADS);
    const int R = (int)window_cells;
    PCH_LAUNCH("terrain_open", tl_open_k, grid, block, 0, s, low, w.a, g.nx, g.ny, R, 0, 0);
    PCH_LAUNCH("terrain_open", tl_open_k, grid, block, 0, s, (const float*)w.a, w.b, g.nx, g.ny, R, 1, 0);
    PCH_LAUNCH("terrain_open", tl_open_k, grid, block, 0, s, (const float*)w.b, w.a, g.nx, g.ny, R, 0, 1);
    PCH_LAUNCH("terrain_open", tl_open_k, grid, block, 0, s, (const float*)w.a, open, g.nx, g.ny, R, 1, 1);
    PCH_LAUNCH("terrain_accept", tl_accept_k, grid, block, 0, s, low, (const float*)open, (int)ncells, dh, w.isg);
    PCH_LAUNCH("terrain_fill", tl_fill_k, grid, block, 0, s, low, (const uint8_t*)w.isg, g.nx, g.ny, (int)max_gap,
               out_ground, out_state);
    return PCH_OK;
}

extern "C" int pch_terrain_height_f32(const float* xyz, int64_t n, const float* sub3_host,
                                      const PchTerrainGrid* grid_host, const float* ground, float* out_height,
                                      float* out_ground, void* stream) {
    PCH_REQUIRE(tl_rows_ok(n), "0 <= n < 2^31");
    TlGrid g;
    PCH_REQUIRE(tl_grid_of(grid_host, g), "the grid needs cell > 0 and finite, nx, ny >= 1 and nx * ny <= 2^24");
    PCH_REQUIRE(ground, "null ground grid");
    PCH_REQUIRE(n == 0 || (xyz && out_height), "null row buffer");
    PCH_DEVICE_GUARD(ground);
    if (n == 0) return PCH_OK;
    {
        DeviceGuard in(xyz);
        if (in.rc != PCH_OK) return in.rc;
    }
    hipStream_t s = (hipStream_t)stream;
    PCH_LAUNCH("terrain_height", tl_height_k, dim3((unsigned)ceil_div(n, TL_TILE)), dim3(TL_THREADS), 0, s, xyz, n,
               tl_sub_of(sub3_host), g, ground, out_height, out_ground);
    return PCH_OK;
}

extern "C" int pch_terrain_sample_f64(const double* xy, int64_t m, const PchTerrainGrid* grid_host, const float* ground,
                                      double* out, void* stream) {
    PCH_REQUIRE(tl_rows_ok(m), "0 <= m < 2^31");
    TlGrid g;
    PCH_REQUIRE(tl_grid_of(grid_host, g), "the grid needs cell > 0 and finite, nx, ny >= 1 and nx * ny <= 2^24");
    PCH_REQUIRE(ground, "null ground grid");
    PCH_REQUIRE(m == 0 || (xy && out), "null position buffer");
    PCH_DEVICE_GUARD(ground);
    if (m == 0) return PCH_OK;
    {
        DeviceGuard in(xy);
        if (in.rc != PCH_OK) return in.rc;
    }
    hipStream_t s = (hipStream_t)stream;
    PCH_LAUNCH("terrain_sample", tl_sample_k, dim3((unsigned)ceil_div(m, TL_THREADS)), dim3(TL_THREADS), 0, s, xy, m, g,
               ground, out);
    return PCH_OK;
}
