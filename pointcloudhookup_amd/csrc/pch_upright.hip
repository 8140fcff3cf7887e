// Stage D1, opt-in upright mode: per cluster the box with z as one axis and the smallest rectangle around the footprint
// among 4096 table angles of [0, 90 deg) as the other two, found in two levels (128 coarse angles, then the 63 table
// angles around the coarse winner).  The rule is spelled out in include/pch_hip.h; everything is minima and maxima of
// float64 products, so the result does not depend on the order the rows are visited in and equals numpy's bit for bit.
//   up_sweep_k     grid (cluster, part): part p walks the row tiles p, p + P, ... of its cluster.  A tile's rows are
//                  gathered through perm into LDS as double x, y; every thread owns one angle and walks the tile with
//                  broadcast reads (all lanes read one address), so the loop holds no cross-lane step.  The partial
//                  bounds of a (cluster, part, angle) go to the workspace: no atomics, nothing waits on another group.
//   up_combine_k   one workgroup per cluster: bounds of the whole cluster per angle, areas, argmin (ties: smallest table
//                  index).  After level 0 it writes status, n, j0 and the z bounds, after level 1 j and the rectangle.
// Kept over atomicMin / atomicMax on ordered 64-bit keys: 4 x 128 atomics per tile-walk and workgroup would all land on
// the same 4 KiB of a big cluster, and the table would need a clearing launch; the workspace needs neither.
#include "pch_common.h"

#include <math.h>

namespace pch {

constexpr int UP_THREADS = 256;
constexpr int UP_TILE    = 256;                       // rows per tile: one gathered row per thread, 4 KiB of LDS
constexpr int UP_ROUND   = 4;                         // rows a thread walks between two loop tests
constexpr int UP_T       = 4096;                      // table angles in [0, 90 deg)
constexpr int UP_FAN     = PCH_UPRIGHT_FINE - 1;      // level 1 looks at j0 - 31 .. j0 + 31
constexpr int UP_SLOTS   = PCH_UPRIGHT_COARSE;        // angle slots per (cluster, part) in the workspace
constexpr int UP_PARTS_MAX = 1024;
constexpr int64_t UP_SLOT_BUDGET = 16384;             // (cluster, part) pairs the workspace holds when it can choose
static_assert(UP_T == PCH_UPRIGHT_COARSE * PCH_UPRIGHT_FINE, "the coarse stride is the fine count");
static_assert(2 * UP_FAN + 1 <= 64, "level 1 fits one wave");
static_assert(UP_TILE == UP_THREADS, "one gathered row per thread");

struct UpRow { float x, y, z; };
struct UpSpan { int64_t begin, cnt, ntiles; };

// rows of cluster k, clamped to the perm entries there are (offsets of a grouping whose wait timed out read -1)
__device__ __forceinline__ UpSpan up_span(const int64_t* __restrict__ offsets, int k, int64_t n_rows_cap) {
    const int64_t b = offsets[k];
    int64_t e = offsets[k + 1];
    if (e > n_rows_cap) e = n_rows_cap;
    UpSpan s;
    s.begin = b;
    s.cnt = (b >= 0 && e > b) ? e - b : 0;
    s.ntiles = (s.cnt + UP_TILE - 1) / UP_TILE;
    return s;
}

__device__ __forceinline__ bool up_finite(float v) { return fabsf(v) < INFINITY; }      // false for NaN

// The walk's minima and maxima as the bare instruction: fmin / fmax put a quieting v_max_f64 x, x in front of every
// accumulator that comes round the loop (4 of 14 float64 operations per row and angle).  On finite operands - the only
// ones whose result is kept, a cluster with any other has status 1 - both give the same value.
__device__ __forceinline__ double up_min(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double up_max(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// LANES angles per row phase: 128 for level 0 (two phases: each half of the threads takes alternate rows), 64 for level 1
// (63 angles, four phases).  Level 1 reads status and j0 of its cluster from the record level 0 wrote.
template <int LANES>
__global__ __launch_bounds__(UP_THREADS) void up_sweep_k(const float* __restrict__ xyz, const int32_t* __restrict__ perm,
                                                         const int64_t* __restrict__ offsets, int64_t n_rows_cap,
                                                         const double* __restrict__ cs,
                                                         const PchUprightBox* __restrict__ boxes, int nparts,
                                                         double* __restrict__ bounds, float* __restrict__ aux) {
    constexpr bool LEVEL0 = LANES == UP_SLOTS;
    constexpr int PHASES = UP_THREADS / LANES;
    constexpr int STEP = UP_ROUND * PHASES;               // rows of a tile per round of the walk
    static_assert(UP_TILE % STEP == 0, "a tile is whole rounds");
    __shared__ double2 tile[UP_TILE];
    __shared__ double red[(PHASES - 1) * LANES * 4];
    __shared__ float zred[3][UP_THREADS / 64];
    const int k = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const UpSpan sp = up_span(offsets, k, n_rows_cap);
    if (p >= sp.ntiles) return;
    int first = 0, stride = PCH_UPRIGHT_FINE, count = PCH_UPRIGHT_COARSE;
    if (!LEVEL0) {
        if (boxes[k].status != 0) return;
        first = boxes[k].j0 - UP_FAN; stride = 1; count = 2 * UP_FAN + 1;
    }
    const int a = tid % LANES, ph = tid / LANES;
    const int ja = a < count ? (first + a * stride + UP_T) & (UP_T - 1) : 0;
    const double c = cs[2 * ja], s = cs[2 * ja + 1];
    double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
    float zlo = INFINITY, zhi = -INFINITY;
    bool bad = false;

    // The rows of a tile are gathered one tile ahead of their use and their perm entries two tiles ahead, under no
    // condition: a thread past the end of the cluster reads its last row again (a row twice changes no minimum), so no
    // load waits at the join of a branch, no row address waits for its perm entry in front of the walk, and the walk
    // runs in whole rounds of UP_ROUND rows per phase.
    const int32_t* __restrict__ rows = perm + sp.begin;
    const int64_t last = sp.cnt - 1;
    const auto row_of = [&](int64_t tile_no) {
        const int64_t i = tile_no * UP_TILE + tid;
        return rows[i < last ? i : last];
    };
    UpRow r = reinterpret_cast<const UpRow*>(xyz)[row_of(p)];
    int32_t ahead = row_of((int64_t)p + nparts);
    for (int64_t t = p; t < sp.ntiles; t += nparts) {
        const int64_t left = sp.cnt - t * UP_TILE;
        const int m = (int)(left < UP_TILE ? left : UP_TILE);
        const int mpad = (m + STEP - 1) & ~(STEP - 1);     // <= UP_TILE: every cell of the tile holds a row
        __syncthreads();                                   // the walkers of the tile before are done
        tile[tid] = make_double2((double)r.x, (double)r.y);
        if (LEVEL0) {
            bad |= !(up_finite(r.x) && up_finite(r.y) && up_finite(r.z));
            zlo = fminf(zlo, r.z);
            zhi = fmaxf(zhi, r.z);
        }
        __syncthreads();
        // behind the barrier, which waits for every load in flight: the walk below covers both gathers
        r = reinterpret_cast<const UpRow*>(xyz)[ahead];
        ahead = row_of(t + 2 * (int64_t)nparts);
        for (int q0 = ph; q0 < mpad; q0 += STEP) {
#pragma unroll
            for (int i = 0; i < UP_ROUND; ++i) {
                const double2 xy = tile[q0 + i * PHASES];
                const double u = xy.x * c + xy.y * s;      // no FMA: the library is built with -ffp-contract=off
                const double v = xy.y * c - xy.x * s;
                umin = up_min(umin, u); umax = up_max(umax, u);
                vmin = up_min(vmin, v); vmax = up_max(vmax, v);
            }
        }
    }
    // the phases of an angle meet in LDS, phase 0 writes the part's bounds
    if (ph > 0) {
        double* d = red + ((ph - 1) * LANES + a) * 4;
        d[0] = umin; d[1] = umax; d[2] = vmin; d[3] = vmax;
    }
    if (LEVEL0) {
        zlo = wave_reduce_min(zlo);
        zhi = wave_reduce_max(zhi);
        const int anybad = __any(bad);
        if (lane_id() == 0) { zred[0][wave_id()] = zlo; zred[1][wave_id()] = zhi; zred[2][wave_id()] = anybad ? 1.f : 0.f; }
    }
    __syncthreads();
    const size_t slot = (size_t)k * nparts + p;
    if (ph == 0 && a < count) {
#pragma unroll
        for (int h = 0; h < PHASES - 1; ++h) {
            const double* d = red + (h * LANES + a) * 4;
            umin = fmin(umin, d[0]); umax = fmax(umax, d[1]);
            vmin = fmin(vmin, d[2]); vmax = fmax(vmax, d[3]);
        }
        double* out = bounds + (slot * UP_SLOTS + a) * 4;
        out[0] = umin; out[1] = umax; out[2] = vmin; out[3] = vmax;
    }
    if (LEVEL0 && tid == 0) {
        float lo = zred[0][0], hi = zred[1][0], b = zred[2][0];
#pragma unroll
        for (int w = 1; w < UP_THREADS / 64; ++w) {
            lo = fminf(lo, zred[0][w]); hi = fmaxf(hi, zred[1][w]); b = fmaxf(b, zred[2][w]);
        }
        float* o = aux + slot * 4;
        o[0] = lo; o[1] = hi; o[2] = b; o[3] = 0.f;
    }
}

constexpr int UC_THREADS = UP_SLOTS;                   // one thread per angle slot

__global__ __launch_bounds__(UC_THREADS) void up_combine_k(const int64_t* __restrict__ offsets, int64_t n_rows_cap,
                                                           int level, int nparts, const double* __restrict__ bounds,
                                                           const float* __restrict__ aux,
                                                           PchUprightBox* __restrict__ boxes) {
    __shared__ double s_area[UC_THREADS];
    __shared__ int s_j[UC_THREADS];
    __shared__ float s_z[3][UC_THREADS];
    const int k = blockIdx.x, a = threadIdx.x;
    const UpSpan sp = up_span(offsets, k, n_rows_cap);
    const int np = (int)(sp.ntiles < nparts ? sp.ntiles : nparts);
    const size_t slot0 = (size_t)k * nparts;
    PchUprightBox* box = boxes + k;
    int first = 0, stride = PCH_UPRIGHT_FINE, count = PCH_UPRIGHT_COARSE;
    if (level == 0) {
        float lo = INFINITY, hi = -INFINITY, b = 0.f;
        for (int p = a; p < np; p += UC_THREADS) {
            const float* o = aux + (slot0 + p) * 4;
            lo = fminf(lo, o[0]); hi = fmaxf(hi, o[1]); b = fmaxf(b, o[2]);
        }
        s_z[0][a] = lo; s_z[1][a] = hi; s_z[2][a] = b;
        __syncthreads();
        for (int w = UC_THREADS / 2; w > 0; w >>= 1) {
            if (a < w) {
                s_z[0][a] = fminf(s_z[0][a], s_z[0][a + w]);
                s_z[1][a] = fmaxf(s_z[1][a], s_z[1][a + w]);
                s_z[2][a] = fmaxf(s_z[2][a], s_z[2][a + w]);
            }
            __syncthreads();
        }
        if (sp.cnt == 0 || s_z[2][0] != 0.f) {             // no box: no row, or a coordinate that is not finite
            if (a == 0) {
                const double nan = (double)NAN;
                box->status = 1; box->j = -1; box->j0 = -1; box->reserved = 0; box->n = sp.cnt;
                box->umin = nan; box->umax = nan; box->vmin = nan; box->vmax = nan; box->zmin = nan; box->zmax = nan;
            }
            return;
        }
    } else {
        if (box->status != 0) return;
        first = box->j0 - UP_FAN; stride = 1; count = 2 * UP_FAN + 1;
    }
    double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
    const int ja = a < count ? (first + a * stride + UP_T) & (UP_T - 1) : 0x7fffffff;
    if (a < count) {
#pragma unroll 4                                           // (four parts' loads in flight: the fold is latency-bound)
        for (int p = 0; p < np; ++p) {
            const double* d = bounds + ((slot0 + p) * UP_SLOTS + a) * 4;
            umin = fmin(umin, d[0]); umax = fmax(umax, d[1]);
            vmin = fmin(vmin, d[2]); vmax = fmax(vmax, d[3]);
        }
    }
    // area from the bounds of the whole cluster; a status-0 cluster has finite bounds, so no area is NaN
    const double area = a < count ? (umax - umin) * (vmax - vmin) : (double)INFINITY;
    s_area[a] = area; s_j[a] = ja;
    __syncthreads();
    for (int w = UC_THREADS / 2; w > 0; w >>= 1) {
        if (a < w) {
            const double o = s_area[a + w];
            const int oj = s_j[a + w];
            if (o < s_area[a] || (o == s_area[a] && oj < s_j[a])) { s_area[a] = o; s_j[a] = oj; }
        }
        __syncthreads();
    }
    if (ja != s_j[0]) return;                              // the table indices of a level are distinct: one writer
    if (level == 0) {
        box->status = 0; box->j0 = ja; box->reserved = 0; box->n = sp.cnt;
        box->zmin = (double)s_z[0][0]; box->zmax = (double)s_z[1][0];
    }
    box->j = ja;
    box->umin = umin; box->umax = umax; box->vmin = vmin; box->vmax = vmax;
}

struct UpWs { double* bounds; float* aux; int nparts; };
// (cluster, part) pairs: every cluster may have as many parts as the cloud has tiles (at most UP_PARTS_MAX) while that
// stays within the budget, else the budget is shared evenly - and never less than one part per cluster.  The pair count
// is monotone in both arguments, so is the size.
static void up_plan(Arena& a, int32_t nclusters, int64_t n_rows_cap, UpWs& w) {
    const int64_t kk = nclusters > 0 ? nclusters : 0;
    int64_t tiles = ceil_div(n_rows_cap > 0 ? n_rows_cap : 0, UP_TILE);
    if (tiles < 1) tiles = 1;
    if (tiles > UP_PARTS_MAX) tiles = UP_PARTS_MAX;
    const int64_t budget = kk > UP_SLOT_BUDGET ? kk : UP_SLOT_BUDGET;
    const int64_t slots = kk * tiles < budget ? kk * tiles : budget;
    w.nparts = kk ? (int)(slots / kk) : 0;
    w.bounds = a.take<double>((size_t)slots * UP_SLOTS * 4);
    w.aux = a.take<float>((size_t)slots * 4);
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_upright_boxes_ws_bytes(int32_t nclusters, int64_t n_rows_cap) {
    if (nclusters < 0 || n_rows_cap < 0) return 0;
    Arena a;
    UpWs w;
    up_plan(a, nclusters, n_rows_cap, w);
    return a.off;
}

extern "C" int pch_upright_boxes_f32(const float* xyz, const int32_t* perm, const int64_t* offsets, int32_t nclusters,
                                     int64_t n_rows_cap, const double* cs_table_dev, PchUprightBox* out_boxes, void* ws,
                                     size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(cs_table_dev);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(nclusters >= 0 && n_rows_cap >= 0 && n_rows_cap < (int64_t(1) << 31), "bad size");
    PCH_REQUIRE(cs_table_dev, "null angle table");
    if (nclusters == 0) return PCH_OK;
    PCH_REQUIRE(offsets && out_boxes && ws, "null buffer");
    PCH_REQUIRE(n_rows_cap == 0 || (xyz && perm), "null buffer");
    Arena a(ws, ws_bytes);
    UpWs w;
    up_plan(a, nclusters, n_rows_cap, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    const dim3 grid((unsigned)nclusters, (unsigned)w.nparts);
    PCH_LAUNCH("upright_sweep0", (up_sweep_k<UP_SLOTS>), grid, dim3(UP_THREADS), 0, s, xyz, perm, offsets, n_rows_cap,
               cs_table_dev, (const PchUprightBox*)out_boxes, w.nparts, w.bounds, w.aux);
    PCH_LAUNCH("upright_combine0", up_combine_k, dim3((unsigned)nclusters), dim3(UC_THREADS), 0, s, offsets, n_rows_cap,
               0, w.nparts, (const double*)w.bounds, (const float*)w.aux, out_boxes);
    PCH_LAUNCH("upright_sweep1", (up_sweep_k<64>), grid, dim3(UP_THREADS), 0, s, xyz, perm, offsets, n_rows_cap,
               cs_table_dev, (const PchUprightBox*)out_boxes, w.nparts, w.bounds, w.aux);
    PCH_LAUNCH("upright_combine1", up_combine_k, dim3((unsigned)nclusters), dim3(UC_THREADS), 0, s, offsets, n_rows_cap,
               1, w.nparts, (const double*)w.bounds, (const float*)w.aux, out_boxes);
    return PCH_OK;
}
