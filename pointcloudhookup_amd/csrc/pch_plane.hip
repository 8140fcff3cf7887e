// Opt-in second ground rule of stage B: one global RANSAC plane z ~ (x, y) instead of one global percentile.
// Reference: test/main_ground.py:8-32 (remove_ground_ransac: RANSACRegressor on z ~ (x, y), residual_threshold 0.1,
// the rows off the plane are "non-ground").  The rule, in the frame of stage B (P = fl32(raw - centroid), then
// float64 in exactly the written association, no FMA: the library is built with -ffp-contract=off):
//   plane of the triple (p0, p1, p2):  u = p1 - p0, v = p2 - p0, n = u x v, nn = (nx nx + ny ny) + nz nz
//       valid iff nn finite, nz != 0, nz nz >= cos2 nn (slope gate), and a, b, c below finite
//       a = -nx / nz, b = -ny / nz, c = p0.z - (a p0.x + b p0.y)
//   residual of a row:  r = z - ((a x + b y) + c);  inlier iff |r| <= residual_threshold (NaN: never)
//   best: the valid hypothesis with the most inliers, the smallest index on a tie; none valid: -1
//   filter: keep r > offset ("above"), or keep !(|r| <= residual_threshold) ("off_plane", ~inlier_mask_)
// No refit on the inliers (sklearn's inlier_mask_ is the best trial's mask too).
// The opt-in third rule, the same plane once per xy tile (test/main_ground.py:77-115), follows in the second half.
#include "pch_compact.h"
#include "pch_prims.h"

namespace pch {

constexpr int PL_THREADS = 256;
constexpr int PL_ROWS    = 4;                           // rows a lane keeps as centred doubles
constexpr int PL_TILE    = PL_THREADS * PL_ROWS;        // 1024 rows per workgroup pass of pl_count_k
constexpr int PL_MAX_HYP = 4096;
constexpr int PL_GRID    = 2048;                        // workgroups of pl_count_k at most (grid-stride beyond)

struct PlPlane { double a, b, c, valid; };              // out_planes row; an invalid hypothesis is four zeros
struct PlRow3 { float x, y, z; };
typedef double PlVec4 __attribute__((ext_vector_type(4)));   // a PlPlane read as ONE 32-byte load

// ---- step 2: one thread per hypothesis.  The plane of one triple of raw rows (shared with the per-tile rule below)
__device__ __forceinline__ PlPlane pl_plane_of(const PlRow3 q0, const PlRow3 q1, const PlRow3 q2, const float* cen,
                                               double cos2) {
    PlPlane out = {0.0, 0.0, 0.0, 0.0};
    const double p0x = (double)(q0.x - cen[0]), p0y = (double)(q0.y - cen[1]), p0z = (double)(q0.z - cen[2]);
    const double ux = (double)(q1.x - cen[0]) - p0x, uy = (double)(q1.y - cen[1]) - p0y,
                 uz = (double)(q1.z - cen[2]) - p0z;
    const double vx = (double)(q2.x - cen[0]) - p0x, vy = (double)(q2.y - cen[1]) - p0y,
                 vz = (double)(q2.z - cen[2]) - p0z;
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double nn = (nx * nx + ny * ny) + nz * nz;
    if (fabs(nn) < INFINITY && nz != 0.0 && nz * nz >= cos2 * nn) {
        const double a = -nx / nz, b = -ny / nz;
        const double c = p0z - (a * p0x + b * p0y);
        if (fabs(a) < INFINITY && fabs(b) < INFINITY && fabs(c) < INFINITY) out = {a, b, c, 1.0};
    }
    return out;
}

__global__ void pl_planes_k(const float* __restrict__ raw, int64_t n, const float* __restrict__ centroid,
                            const int64_t* __restrict__ rows, int nhyp, double cos2, PlPlane* __restrict__ planes) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= nhyp) return;
    PlPlane out = {0.0, 0.0, 0.0, 0.0};
    const int64_t i0 = rows[3 * h], i1 = rows[3 * h + 1], i2 = rows[3 * h + 2];
    if (i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n) {      // a row outside the cloud: invalid
        const float cen[3] = {centroid[0], centroid[1], centroid[2]};
        const PlRow3* __restrict__ r3 = reinterpret_cast<const PlRow3*>(raw);
        out = pl_plane_of(r3[i0], r3[i1], r3[i2], cen, cos2);
    }
    planes[h] = out;
}

// the residual tests of one wave's PL_ROWS x 64 rows against nhyp planes (shared with the per-tile rule below)
__device__ __forceinline__ void pl_tally(const double (&x)[PL_ROWS], const double (&y)[PL_ROWS],
                                         const double (&z)[PL_ROWS], const PlPlane* __restrict__ planes, int nhyp,
                                         double thr, uint32_t* cnt_sh) {
    const int l = lane_id();
    for (int hb = 0; hb < nhyp; hb += 64) {
        uint32_t acc = 0u;
        const int he = nhyp - hb < 64 ? nhyp - hb : 64;
        for (int j = 0; j < he; ++j) {
            const PlVec4 p = reinterpret_cast<const PlVec4*>(planes)[hb + j];      // a, b, c, valid
            if (p.w != 0.0) {
                uint32_t c = 0u;
#pragma unroll
                for (int r = 0; r < PL_ROWS; ++r) {
                    const double res = z[r] - ((p.x * x[r] + p.y * y[r]) + p.z);
                    c += (uint32_t)__popcll(__ballot(fabs(res) <= thr));
                }
                acc = l == j ? c : acc;
            }
        }
        if (acc) atomicAdd(&cnt_sh[hb + l], acc);
    }
}

// ---- step 3, the hot kernel: nhyp x n residual tests in float64.  A lane keeps PL_ROWS rows as centred doubles; the
// loop over the hypotheses reads the plane wave-uniformly (scalar loads) and skips an invalid one with a uniform
// branch; a ballot per row round gives a wave-uniform count, which lands in lane (h & 63) of one accumulator register
// and goes to the workgroup's LDS counters once per 64 hypotheses, to the global counters once per workgroup.
// Nothing waits on another workgroup.  Rows beyond n are NaN: never inliers.
__global__ __launch_bounds__(PL_THREADS) void pl_count_k(const float* __restrict__ raw, int64_t n,
                                                         const float* __restrict__ centroid,
                                                         const PlPlane* __restrict__ planes, int nhyp, double thr,
                                                         unsigned long long* __restrict__ counts) {
    __shared__ uint32_t cnt_sh[PL_MAX_HYP];             // < 2^31 rows in all: 32 bits hold a workgroup's share
    for (int h = threadIdx.x; h < nhyp; h += PL_THREADS) cnt_sh[h] = 0u;
    __syncthreads();
    const float cen[3] = {centroid[0], centroid[1], centroid[2]};
    const PlRow3* __restrict__ r3 = reinterpret_cast<const PlRow3*>(raw);
    const int l = lane_id();
    const int64_t ntiles = (n + PL_TILE - 1) / PL_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t seg = tile * PL_TILE + (int64_t)wave_id() * (64 * PL_ROWS);
        if (seg >= n) continue;                         // wave-uniform: nothing of this wave's share exists
        double x[PL_ROWS], y[PL_ROWS], z[PL_ROWS];
#pragma unroll
        for (int r = 0; r < PL_ROWS; ++r) {
            const int64_t i = seg + r * 64 + l;
            const PlRow3 q = r3[i < n ? i : n - 1];
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            x[r] = i < n ? (double)(q.x - cen[0]) : nan;
            y[r] = i < n ? (double)(q.y - cen[1]) : nan;
            z[r] = i < n ? (double)(q.z - cen[2]) : nan;
        }
        pl_tally(x, y, z, planes, nhyp, thr, cnt_sh);
    }
    __syncthreads();
    for (int h = threadIdx.x; h < nhyp; h += PL_THREADS) {
        const uint32_t c = cnt_sh[h];
        if (c) atomicAdd(&counts[h], (unsigned long long)c);
    }
}

// ---- step 4: one workgroup; the key orders by count first and by the LOWER index second, 0 = no valid hypothesis
__device__ __forceinline__ unsigned long long pl_best_key(int64_t count, int h) {
    return ((unsigned long long)(count + 1) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)h);
}
__device__ __forceinline__ PchPlaneBest pl_best_record(const PlPlane* __restrict__ planes,
                                                       const int64_t* __restrict__ counts, unsigned long long key,
                                                       uint32_t nv) {
    PchPlaneBest out = {0.0, 0.0, 0.0, 0, -1, (int32_t)nv};
    if (key) {
        const int h = (int)(0xFFFFFFFFu - (uint32_t)key);
        out.a = planes[h].a;
        out.b = planes[h].b;
        out.c = planes[h].c;
        out.count = counts[h];
        out.best = h;
    }
    return out;
}

__global__ __launch_bounds__(PL_THREADS) void pl_best_k(const PlPlane* __restrict__ planes,
                                                        const int64_t* __restrict__ counts, int nhyp,
                                                        PchPlaneBest* __restrict__ best) {
    __shared__ unsigned long long key_sh[PL_THREADS / 64];
    __shared__ uint32_t nv_sh[PL_THREADS / 64];
    unsigned long long key = 0ull;
    uint32_t nv = 0u;
    for (int h = threadIdx.x; h < nhyp; h += PL_THREADS) {
        if (planes[h].valid == 0.0) continue;
        ++nv;
        const unsigned long long k = pl_best_key(counts[h], h);
        key = k > key ? k : key;
    }
    key = wave_reduce_max(key);
    nv = wave_reduce_add(nv);
    if (lane_id() == 0) { key_sh[wave_id()] = key; nv_sh[wave_id()] = nv; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < PL_THREADS / 64; ++w) {
        key = key_sh[w] > key ? key_sh[w] : key;
        nv += nv_sh[w];
    }
    *best = pl_best_record(planes, counts, key, nv);
}

// ---- step 5: the register-resident ordered compaction of pch_compact.h on float32 rows, with the box of the finite
// kept rows; what this file adds is the centring, where a row's plane comes from (Src) and the residual predicate
constexpr int PF_ROUNDS = 8;
constexpr int PF_TILE   = PL_THREADS * PF_ROUNDS;       // 2048 rows per workgroup

struct PfState {
    uint32_t ticket, pad[3];
    uint32_t slots[OC_SLOTS][6];                        // ~ordered(min xyz) / ordered(max xyz), folded with atomicMax
};
typedef OcWs<PfState, PF_TILE> PfWs;

// the tile of a centred row, the one arithmetic of the per-tile rule (grouping and filter): -1 outside the grid;
// NaN and inf fail the comparisons
__device__ __forceinline__ int plt_tile_of(double x, double y, const PchPlaneGrid& g) {
    const double fx = floor((x - g.x0) / g.tile), fy = floor((y - g.y0) / g.tile);
    if (!(fx >= 0.0 && fx < (double)g.nx && fy >= 0.0 && fy < (double)g.ny)) return -1;
    return (int)fy * g.nx + (int)fx;
}

// where a row's plane comes from: the one record of the global rule, or the record of the row's tile with a fallback
struct PfOnePlane {
    const PchPlaneBest* best;
    __device__ __forceinline__ bool none() const { return best->best < 0; }
    __device__ __forceinline__ bool plane(double, double, double& a, double& b, double& c) const {
        a = best->a; b = best->b; c = best->c;
        return true;
    }
};
struct PfTilePlanes {
    const PchPlaneBest* best;                           // [nx * ny]
    const PchPlaneBest* fallback;                       // may be null
    PchPlaneGrid g;
    __device__ __forceinline__ bool none() const { return false; }
    __device__ __forceinline__ bool plane(double x, double y, double& a, double& b, double& c) const {
        const int t = plt_tile_of(x, y, g);
        const PchPlaneBest* r = t >= 0 && best[t].best >= 0 ? best + t : fallback;
        if (!r || r->best < 0) return false;            // no plane at all: the row is not kept
        a = r->a; b = r->b; c = r->c;
        return true;
    }
};

template <class Src>
__global__ __launch_bounds__(PL_THREADS) void pl_filter_k(const float* __restrict__ raw, int64_t n,
                                                          const float* __restrict__ centroid,
                                                          const Src src, int keep_mode,
                                                          double val, PfState* __restrict__ st,
                                                          uint64_t* __restrict__ status, float* __restrict__ out_points,
                                                          int32_t* __restrict__ out_index,
                                                          int64_t* __restrict__ out_count) {
    __shared__ uint32_t box[OC_WAVES][6];
    if (src.none()) return;                             // no plane: nothing is kept, the count word stays 0
    const int64_t tile = oc_take_tile(&st->ticket);
    const float cen[3] = {centroid[0], centroid[1], centroid[2]};
    const int l = lane_id();
    const int64_t seg = tile * PF_TILE + (int64_t)wave_id() * (64 * PF_ROUNDS);
    const PlRow3* __restrict__ r3 = reinterpret_cast<const PlRow3*>(raw);
    PlRow3 q[PF_ROUNDS];
    unsigned long long m[PF_ROUNDS];
#pragma unroll
    for (int r = 0; r < PF_ROUNDS; ++r) {
        const int64_t i = seg + r * 64 + l;
        q[r] = r3[i < n ? i : 0];
    }
#pragma unroll
    for (int r = 0; r < PF_ROUNDS; ++r) {
        const int64_t i = seg + r * 64 + l;
        // points = raw_points - centroid (float32), as oc_emit stores them
        const double x = (double)(q[r].x - cen[0]), y = (double)(q[r].y - cen[1]), z = (double)(q[r].z - cen[2]);
        double pa = 0.0, pb = 0.0, pc = 0.0;
        const bool has = src.plane(x, y, pa, pb, pc);
        const double res = z - ((pa * x + pb * y) + pc);
        const bool keep = i < n && has && (keep_mode == 0 ? res > val : !(fabs(res) <= val));
        m[r] = __ballot(keep);
    }
    const uint32_t woff = oc_place(m, status, tile, out_count);
    if (woff == OC_NONE) return;
    uint32_t lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};
    oc_visit(m, woff, [&](int r, int64_t o) {
        oc_emit(q[r].x, q[r].y, q[r].z, cen, o, seg + r * 64 + l, out_points, out_index, lo, hi);
    });
    oc_fold_box(st->slots, tile, lo, hi, box);
}

// the bounding box of the finite kept rows; zeros when there are none (as gf_finalize_k reports it)
__global__ void pl_box_k(const PfState* __restrict__ st, float* __restrict__ out_aabb) {
    if (threadIdx.x < 6) out_aabb[threadIdx.x] = oc_box_word(st->slots, threadIdx.x);
}

// ==================================================================================================================
// Opt-in third ground rule: the same RANSAC plane per xy tile (test/main_ground.py:77-115, remove_ground_tiled_ransac),
// stated in include/pch_hip.h.  Grouping: a key per row (its tile, or ntiles for a row without one), the stable LSD
// radix sort of pch_prims on the bits in use with the row number as the value, and the tile offsets read off the
// sorted keys.  A counted scatter would need a [workgroup][key] table to stay stable across workgroups, which at
// 65 537 keys is larger than the cloud; the sort's per-pass table has 256 digits.  The count kernel reads its rows
// THROUGH the permutation (4 bytes of it and one 12-byte gather per row): a grouped copy of the centred rows would
// pay the same gather once to build the copy and then write and re-read 12 bytes per row on top.
constexpr int PLT_MAX_TILES    = 65536;
constexpr int PLT_MAX_TABLE    = 1 << 22;               // tiles x hypotheses
constexpr int PLT_SCAN_THREADS = 1024;

__global__ __launch_bounds__(PL_THREADS) void plt_key_k(const float* __restrict__ raw, int64_t n,
                                                        const float* __restrict__ centroid, const PchPlaneGrid g,
                                                        uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (i >= n) return;
    const PlRow3 q = reinterpret_cast<const PlRow3*>(raw)[i];
    const int t = plt_tile_of((double)(q.x - centroid[0]), (double)(q.y - centroid[1]), g);
    keys[i] = (uint64_t)(t < 0 ? g.nx * g.ny : t);      // rows without a tile sort behind the last tile
    vals[i] = (uint32_t)i;
}

// start[t] = the first grouped position of key t, for t in [0, ntiles + 1]: the exclusive scan of the per-key counts,
// read off the sorted keys (thread i writes the keys that begin between positions i - 1 and i; ntiles + 2 stores in all)
__global__ __launch_bounds__(PL_THREADS) void plt_starts_k(const uint64_t* __restrict__ keys, int64_t n, int ntiles,
                                                           uint32_t* __restrict__ start) {
    const int64_t i = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (i > n) return;
    const int64_t kp = i > 0 ? (int64_t)keys[i - 1] : -1, kc = i < n ? (int64_t)keys[i] : (int64_t)ntiles + 1;
    for (int64_t t = kp + 1; t <= kc && t <= (int64_t)ntiles + 1; ++t) start[t] = (uint32_t)i;
}

// one workgroup: the passes of every tile (0 for a tile under min_rows: it has no valid hypothesis, so nothing to
// count), their exclusive scan pstart[0 .. ntiles], and the per-tile row counts for the caller
__global__ __launch_bounds__(PLT_SCAN_THREADS) void plt_passes_k(const uint32_t* __restrict__ start, int ntiles,
                                                                 int min_rows, uint32_t* __restrict__ pstart,
                                                                 int64_t* __restrict__ out_tile_rows) {
    __shared__ uint32_t wsum[PLT_SCAN_THREADS / 64];
    const int per = (ntiles + PLT_SCAN_THREADS - 1) / PLT_SCAN_THREADS;
    const int t0 = threadIdx.x * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    uint32_t mine = 0u;
    for (int t = t0; t < t1; ++t) {
        const uint32_t nt = start[t + 1] - start[t];
        if (out_tile_rows) out_tile_rows[t] = (int64_t)nt;
        mine += nt >= (uint32_t)min_rows ? (nt + PL_TILE - 1) / PL_TILE : 0u;
    }
    const uint32_t incl = wave_scan_incl(mine);
    if (lane_id() == 63) wsum[wave_id()] = incl;
    __syncthreads();
    uint32_t run = incl - mine;
    for (int w = 0; w < wave_id(); ++w) run += wsum[w];
    for (int t = t0; t < t1; ++t) {
        const uint32_t nt = start[t + 1] - start[t];
        pstart[t] = run;
        run += nt >= (uint32_t)min_rows ? (nt + PL_TILE - 1) / PL_TILE : 0u;
    }
    if (threadIdx.x == PLT_SCAN_THREADS - 1) pstart[ntiles] = run;
}

// one thread per (tile, hypothesis): the triple is list_t[draws[h][k] mod n_t]
__global__ __launch_bounds__(PL_THREADS) void plt_planes_k(const float* __restrict__ raw,
                                                           const float* __restrict__ centroid,
                                                           const uint32_t* __restrict__ perm,
                                                           const uint32_t* __restrict__ start,
                                                           const int64_t* __restrict__ draws, int ntiles, int nhyp,
                                                           int min_rows, double cos2, PlPlane* __restrict__ planes) {
    const int idx = blockIdx.x * PL_THREADS + threadIdx.x;
    if (idx >= ntiles * nhyp) return;
    const int t = idx / nhyp, h = idx - t * nhyp;
    PlPlane out = {0.0, 0.0, 0.0, 0.0};
    const uint32_t s0 = start[t], nt = start[t + 1] - s0;
    const int64_t d0 = draws[3 * h], d1 = draws[3 * h + 1], d2 = draws[3 * h + 2];
    if (nt >= (uint32_t)min_rows && d0 >= 0 && d1 >= 0 && d2 >= 0) {
        const float cen[3] = {centroid[0], centroid[1], centroid[2]};
        const PlRow3* __restrict__ r3 = reinterpret_cast<const PlRow3*>(raw);
        const uint32_t i0 = perm[s0 + (uint32_t)(d0 % (int64_t)nt)], i1 = perm[s0 + (uint32_t)(d1 % (int64_t)nt)],
                       i2 = perm[s0 + (uint32_t)(d2 % (int64_t)nt)];
        out = pl_plane_of(r3[i0], r3[i1], r3[i2], cen, cos2);
    }
    planes[idx] = out;
}

// the hot kernel: pl_count_k's work on the grouped rows.  A pass is at most PL_TILE consecutive grouped rows of ONE
// tile; pass p belongs to the last tile t with pstart[t] <= p.  A workgroup takes a contiguous run of passes and keeps
// its counters in LDS; they go to counts[t][*] with vector atomics when the run's tile changes and at its end.
__global__ __launch_bounds__(PL_THREADS) void plt_count_k(const float* __restrict__ raw,
                                                          const float* __restrict__ centroid,
                                                          const uint32_t* __restrict__ perm,
                                                          const uint32_t* __restrict__ start,
                                                          const uint32_t* __restrict__ pstart, int ntiles,
                                                          const PlPlane* __restrict__ planes, int nhyp, double thr,
                                                          unsigned long long* __restrict__ counts) {
    __shared__ uint32_t cnt_sh[PL_MAX_HYP];
    const uint32_t P = pstart[ntiles];
    const uint32_t per = (P + gridDim.x - 1) / gridDim.x;
    const uint32_t p0 = blockIdx.x * per, p1 = P - p0 < per ? P : p0 + per;
    if (p0 >= P) return;                                // surplus workgroup of the host's upper bound
    for (int h = threadIdx.x; h < nhyp; h += PL_THREADS) cnt_sh[h] = 0u;
    __syncthreads();
    const float cen[3] = {centroid[0], centroid[1], centroid[2]};
    const PlRow3* __restrict__ r3 = reinterpret_cast<const PlRow3*>(raw);
    const int l = lane_id();
    int cur = -1;
    uint32_t cur_p0 = 0u, cur_p1 = 0u;                  // the passes of tile cur
    for (uint32_t p = p0; p < p1; ++p) {
        if (p >= cur_p1) {                              // workgroup-uniform: the run enters another tile
            int lo = 0, hi = ntiles;                    // pstart[lo] <= p < pstart[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (pstart[mid] <= p) lo = mid; else hi = mid;
            }
            if (cur >= 0) {
                __syncthreads();
                for (int h = threadIdx.x; h < nhyp; h += PL_THREADS) {
                    const uint32_t c = cnt_sh[h];
                    if (c) atomicAdd(&counts[(size_t)cur * nhyp + h], (unsigned long long)c);
                    cnt_sh[h] = 0u;
                }
                __syncthreads();
            }
            cur = __builtin_amdgcn_readfirstlane(lo);
            cur_p0 = pstart[cur];
            cur_p1 = pstart[cur + 1];
        }
        const uint32_t gend = start[cur + 1];
        const uint32_t seg = start[cur] + (p - cur_p0) * PL_TILE + (uint32_t)wave_id() * (64 * PL_ROWS);
        if (seg >= gend) continue;                      // wave-uniform: nothing of this wave's share exists
        double x[PL_ROWS], y[PL_ROWS], z[PL_ROWS];
#pragma unroll
        for (int r = 0; r < PL_ROWS; ++r) {
            const uint32_t gpos = seg + r * 64 + l;
            const bool in = gpos < gend;
            const PlRow3 q = r3[perm[in ? gpos : gend - 1]];
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            x[r] = in ? (double)(q.x - cen[0]) : nan;
            y[r] = in ? (double)(q.y - cen[1]) : nan;
            z[r] = in ? (double)(q.z - cen[2]) : nan;
        }
        pl_tally(x, y, z, planes + (size_t)cur * nhyp, nhyp, thr, cnt_sh);
    }
    __syncthreads();
    for (int h = threadIdx.x; h < nhyp; h += PL_THREADS) {
        const uint32_t c = cnt_sh[h];
        if (c) atomicAdd(&counts[(size_t)cur * nhyp + h], (unsigned long long)c);
    }
}

// one wave per tile, the key of pl_best_k
__global__ __launch_bounds__(PL_THREADS) void plt_best_k(const PlPlane* __restrict__ planes,
                                                         const int64_t* __restrict__ counts, int ntiles, int nhyp,
                                                         PchPlaneBest* __restrict__ best) {
    const int t = blockIdx.x * (PL_THREADS / 64) + wave_id();
    if (t >= ntiles) return;
    const PlPlane* __restrict__ pt = planes + (size_t)t * nhyp;
    const int64_t* __restrict__ ct = counts + (size_t)t * nhyp;
    unsigned long long key = 0ull;
    uint32_t nv = 0u;
    for (int h = lane_id(); h < nhyp; h += 64) {
        if (pt[h].valid == 0.0) continue;
        ++nv;
        const unsigned long long k = pl_best_key(ct[h], h);
        key = k > key ? k : key;
    }
    key = wave_reduce_max(key);
    nv = wave_reduce_add(nv);
    if (lane_id() == 0) best[t] = pl_best_record(pt, ct, key, nv);
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_plane_fit_ws_bytes(int64_t n, int32_t nhyp) {
    (void)n;
    (void)nhyp;
    return 0;                                           // the counters live in LDS and in out_counts
}

extern "C" int pch_plane_fit_f32(const float* raw, int64_t n, const float* centroid3_dev, const int64_t* rows_dev,
                                 int32_t nhyp, double residual_threshold, double cos2_max_slope, double* out_planes,
                                 int64_t* out_counts, PchPlaneBest* out_best_dev, void* ws, size_t ws_bytes,
                                 void* stream) {
    (void)ws;
    (void)ws_bytes;
    PCH_DEVICE_GUARD(out_best_dev);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && nhyp >= 1 && nhyp <= PL_MAX_HYP, "bad argument");
    PCH_REQUIRE(out_planes && out_counts && out_best_dev, "null output");
    static_assert(sizeof(PlPlane) == 4 * sizeof(double), "out_planes is [nhyp,4] float64");
    PlPlane* planes = reinterpret_cast<PlPlane*>(out_planes);
    PCH_HIP_TRY(hipMemsetAsync(out_counts, 0, (size_t)nhyp * sizeof(int64_t), s));
    if (n == 0) {                                       // no row to draw from: every hypothesis is invalid
        PCH_HIP_TRY(hipMemsetAsync(out_planes, 0, (size_t)nhyp * sizeof(PlPlane), s));
    } else {
        PCH_REQUIRE(raw && centroid3_dev && rows_dev, "null input");
        PCH_LAUNCH("pl_planes", pl_planes_k, dim3((unsigned)ceil_div(nhyp, 64)), dim3(64), 0, s, raw, n, centroid3_dev,
                   rows_dev, (int)nhyp, cos2_max_slope, planes);
        const int64_t nt = ceil_div(n, PL_TILE);
        PCH_LAUNCH("pl_count", pl_count_k, dim3((unsigned)(nt < PL_GRID ? nt : PL_GRID)), dim3(PL_THREADS), 0, s, raw,
                   n, centroid3_dev, (const PlPlane*)planes, (int)nhyp, residual_threshold,
                   reinterpret_cast<unsigned long long*>(out_counts));
    }
    PCH_LAUNCH("pl_best", pl_best_k, dim3(1), dim3(PL_THREADS), 0, s, (const PlPlane*)planes,
               (const int64_t*)out_counts, (int)nhyp, out_best_dev);
    return PCH_OK;
}

extern "C" size_t pch_filter_plane_ws_bytes(int64_t n) {
    return n < 0 ? 0 : PfWs::bytes(n);
}

// both filters behind their own argument checks; fn: the entry point, for the error text
template <class Src>
static int pl_filter_run(const char* fn, const char* launch, const float* raw, int64_t n, const float* centroid3_dev,
                         const Src& src, int32_t keep_mode, double offset_or_threshold, float* out_points,
                         int32_t* out_index, int64_t* out_count, float* out_aabb, void* ws, size_t ws_bytes,
                         hipStream_t s) {
    PCH_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(int64_t), s));
    if (out_aabb) PCH_HIP_TRY(hipMemsetAsync(out_aabb, 0, 6 * sizeof(float), s));
    if (n == 0) return PCH_OK;
    if (!(raw && centroid3_dev && src.best && out_points && ws)) { set_error("%s: null buffer", fn); return PCH_ERR_ARG; }
    Arena a(ws, ws_bytes);
    const PfWs w(a, n);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    PCH_HIP_TRY(hipMemsetAsync(ws, 0, a.off, s));
    PCH_LAUNCH(launch, pl_filter_k<Src>, dim3((unsigned)w.nt), dim3(PL_THREADS), 0, s, raw, n, centroid3_dev, src,
               (int)keep_mode, offset_or_threshold, w.st, w.status, out_points, out_index, out_count);
    if (out_aabb) PCH_LAUNCH("pl_box", pl_box_k, dim3(1), dim3(64), 0, s, (const PfState*)w.st, out_aabb);
    return PCH_OK;
}

extern "C" int pch_filter_plane_f32(const float* raw, int64_t n, const float* centroid3_dev,
                                    const PchPlaneBest* best_dev, int32_t keep_mode, double offset_or_threshold,
                                    float* out_points, int32_t* out_index, int64_t* out_count, float* out_aabb,
                                    void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(out_count);
    PCH_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && out_count && (keep_mode == 0 || keep_mode == 1), "bad argument");
    return pl_filter_run(__func__, "pl_filter", raw, n, centroid3_dev, PfOnePlane{best_dev}, keep_mode,
                         offset_or_threshold, out_points, out_index, out_count, out_aabb, ws, ws_bytes,
                         (hipStream_t)stream);
}

// ------------------------------------------------------------------ the per-tile rule
static bool plt_grid_ok(const PchPlaneGrid* g) {
    return g && g->tile > 0.0 && g->tile < INFINITY && g->x0 - g->x0 == 0.0 && g->y0 - g->y0 == 0.0 && g->nx >= 1 &&
           g->ny >= 1 && (int64_t)g->nx * g->ny <= PLT_MAX_TILES;
}

// the one carve-up of the fit's workspace (size query and call)
struct PltFitWs {
    uint64_t *k0, *k1;
    uint32_t *v0, *v1, *radix, *start, *pstart;
    PlPlane* planes;
    int64_t* counts;
    PltFitWs(Arena& a, int64_t n, int64_t ntiles, int64_t nhyp) {
        const int64_t m = n > 0 ? n : 1;
        k0 = a.take<uint64_t>(m);
        k1 = a.take<uint64_t>(m);
        v0 = a.take<uint32_t>(m);
        v1 = a.take<uint32_t>(m);
        radix = a.take<uint32_t>(radix_ws_u32(m));
        start = a.take<uint32_t>(ntiles + 2);
        pstart = a.take<uint32_t>(ntiles + 1);
        planes = a.take<PlPlane>(ntiles * nhyp);
        counts = a.take<int64_t>(ntiles * nhyp);
    }
};

extern "C" size_t pch_plane_tiles_fit_ws_bytes(int64_t n, int32_t ntiles, int32_t nhyp) {
    if (n < 0 || n >= (int64_t(1) << 31) || ntiles < 1 || ntiles > PLT_MAX_TILES || nhyp < 1 || nhyp > PL_MAX_HYP ||
        (int64_t)ntiles * nhyp > PLT_MAX_TABLE)
        return 0;
    Arena a;
    PltFitWs w(a, n, ntiles, nhyp);
    (void)w;
    return a.off;
}

extern "C" int pch_plane_tiles_fit_f32(const float* raw, int64_t n, const float* centroid3_dev,
                                       const PchPlaneGrid* grid_host, const int64_t* draws_dev, int32_t nhyp,
                                       int32_t min_tile_rows, double residual_threshold, double cos2_max_slope,
                                       PchPlaneBest* out_best_dev, int64_t* out_tile_rows, double* out_planes,
                                       int64_t* out_counts, void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(out_best_dev);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && nhyp >= 1 && nhyp <= PL_MAX_HYP && min_tile_rows >= 1,
                "bad argument");
    PCH_REQUIRE(plt_grid_ok(grid_host), "bad grid: tile > 0 and finite, nx, ny >= 1, nx * ny <= 65536");
    const PchPlaneGrid g = *grid_host;
    const int64_t ntiles = (int64_t)g.nx * g.ny, table = ntiles * nhyp;
    PCH_REQUIRE(table <= PLT_MAX_TABLE, "nx * ny * nhyp exceeds 2^22");
    PCH_REQUIRE(out_best_dev && ws, "null output or workspace");
    Arena a(ws, ws_bytes);
    PltFitWs w(a, n, ntiles, nhyp);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    PlPlane* planes = out_planes ? reinterpret_cast<PlPlane*>(out_planes) : w.planes;
    int64_t* counts = out_counts ? out_counts : w.counts;
    PCH_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)table * sizeof(int64_t), s));
    if (n == 0) {                                       // no row: every hypothesis of every tile is invalid
        PCH_HIP_TRY(hipMemsetAsync(planes, 0, (size_t)table * sizeof(PlPlane), s));
        if (out_tile_rows) PCH_HIP_TRY(hipMemsetAsync(out_tile_rows, 0, (size_t)ntiles * sizeof(int64_t), s));
    } else {
        PCH_REQUIRE(raw && centroid3_dev && draws_dev, "null input");
        // grouping: a key per row, the stable LSD sort of pch_prims on the bits in use, tile offsets from the sorted keys
        PCH_LAUNCH("plt_key", plt_key_k, dim3((unsigned)ceil_div(n, PL_THREADS)), dim3(PL_THREADS), 0, s, raw, n,
                   centroid3_dev, g, w.k0, w.v0);
        const int nbits = bits_for((uint64_t)ntiles + 1);
        PCH_TRY(radix_sort_pairs(w.k0, w.v0, w.k1, w.v1, n, nbits, w.radix, s));
        const bool second = radix_sort_result_buffer(nbits) == 1;
        const uint64_t* keys = second ? w.k1 : w.k0;
        const uint32_t* perm = second ? w.v1 : w.v0;
        PCH_LAUNCH("plt_starts", plt_starts_k, dim3((unsigned)ceil_div(n + 1, PL_THREADS)), dim3(PL_THREADS), 0, s, keys,
                   n, (int)ntiles, w.start);
        PCH_LAUNCH("plt_passes", plt_passes_k, dim3(1), dim3(PLT_SCAN_THREADS), 0, s, (const uint32_t*)w.start,
                   (int)ntiles, (int)min_tile_rows, w.pstart, out_tile_rows);
        PCH_LAUNCH("plt_planes", plt_planes_k, dim3((unsigned)ceil_div(table, PL_THREADS)), dim3(PL_THREADS), 0, s, raw,
                   centroid3_dev, perm, (const uint32_t*)w.start, draws_dev, (int)ntiles, (int)nhyp, (int)min_tile_rows,
                   cos2_max_slope, planes);
        // the host knows n and ntiles alone: at most n / 1024 + ntiles passes exist, surplus workgroups return
        const int64_t pmax = n / PL_TILE + ntiles;
        PCH_LAUNCH("plt_count", plt_count_k, dim3((unsigned)(pmax < PL_GRID ? pmax : PL_GRID)), dim3(PL_THREADS), 0, s,
                   raw, centroid3_dev, perm, (const uint32_t*)w.start, (const uint32_t*)w.pstart, (int)ntiles,
                   (const PlPlane*)planes, (int)nhyp, residual_threshold, reinterpret_cast<unsigned long long*>(counts));
    }
    PCH_LAUNCH("plt_best", plt_best_k, dim3((unsigned)ceil_div(ntiles, PL_THREADS / 64)), dim3(PL_THREADS), 0, s,
               (const PlPlane*)planes, (const int64_t*)counts, (int)ntiles, (int)nhyp, out_best_dev);
    return PCH_OK;
}

extern "C" size_t pch_filter_plane_tiles_ws_bytes(int64_t n, int32_t ntiles) {
    if (ntiles < 1 || ntiles > PLT_MAX_TILES) return 0;
    return pch_filter_plane_ws_bytes(n);                // the per-tile records are the caller's: no state per tile
}

extern "C" int pch_filter_plane_tiles_f32(const float* raw, int64_t n, const float* centroid3_dev,
                                          const PchPlaneGrid* grid_host, const PchPlaneBest* best_dev,
                                          const PchPlaneBest* fallback_dev, int32_t keep_mode,
                                          double offset_or_threshold, float* out_points, int32_t* out_index,
                                          int64_t* out_count, float* out_aabb, void* ws, size_t ws_bytes,
                                          void* stream) {
    PCH_DEVICE_GUARD(out_count);
    PCH_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && out_count && (keep_mode == 0 || keep_mode == 1), "bad argument");
    PCH_REQUIRE(plt_grid_ok(grid_host), "bad grid: tile > 0 and finite, nx, ny >= 1, nx * ny <= 65536");
    return pl_filter_run(__func__, "plt_filter", raw, n, centroid3_dev, PfTilePlanes{best_dev, fallback_dev, *grid_host},
                         keep_mode, offset_or_threshold, out_points, out_index, out_count, out_aabb, ws, ws_bytes,
                         (hipStream_t)stream);
}
