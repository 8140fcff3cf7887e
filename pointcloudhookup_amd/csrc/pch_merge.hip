// Between stages C and D0, opt-in: merge of the cluster pieces that the file-order chunks of stage C cut apart.
// The reference fits DBSCAN once per 50 000-row chunk (utils/tower_extraction.py:96-117), so a tower whose kept rows
// straddle a chunk boundary comes out as several clusters; its authors' own remedy is the post-processing step of
// test/tttt.py:93-175: the float32 mean of every cluster, KDTree.query_radius over the means, union-find over the hits,
// relabel.  The rule is spelled out in include/pch_hip.h; two kernel families implement it:
//   cc_centers_k   one wave per cluster: the sequential float32 sum of numpy's np.mean(axis=0), rows gathered ahead
//   cm_*           all pairs of centres in 64 x 64 tiles, lock-free union-find (pch_unionfind.h), roots ranked by a scan
#include "pch_prims.h"
#include "pch_unionfind.h"

#include <math.h>

namespace pch {

// ---- centres ------------------------------------------------------------------------------------------------------
// A workgroup is ONE wave and owns one cluster.  All 64 lanes gather the next tiles of rows (perm -> 12-byte row) into
// registers while lanes 0..2, one per column, add the tile in front of them from LDS in row order: only the float32
// adds sit on the dependent chain.  LDS operations of one wave execute in program order, so one tile buffer is enough.
constexpr int CC_ROUNDS = 4;                         // rows per lane and tile
constexpr int CC_TILE   = 64 * CC_ROUNDS;            // 256 rows = 3 KiB of LDS
constexpr int CC_AHEAD  = 16;                        // values an adding lane reads ahead of its adds
static_assert(CC_TILE % CC_AHEAD == 0, "full tiles are added in groups of CC_AHEAD");

struct CcRow { float x, y, z; };

// The gather of tile t runs in two steps, each a whole tile of adds ahead of its use: the perm entries of rows t0 + 64 q
// + l, q = 0..3 (cc_rows_of), and one tile later the 12-byte rows they name (cc_rows).  No load stands under a
// condition - a row past the end reads the cluster's last row again, and nobody adds it: a load inside a branch is
// waited for where the branch ends (the register moves of the join), which would put every one on the critical path.
__device__ __forceinline__ void cc_rows_of(const int32_t* __restrict__ perm, int64_t cnt, int64_t t0, int l,
                                           int32_t (&p)[CC_ROUNDS]) {
#pragma unroll
    for (int q = 0; q < CC_ROUNDS; ++q) {
        const int64_t j = t0 + (int64_t)q * 64 + l;
        p[q] = perm[j < cnt ? j : cnt - 1];
    }
}
__device__ __forceinline__ void cc_rows(const float* __restrict__ xyz, const int32_t (&p)[CC_ROUNDS],
                                        CcRow (&r)[CC_ROUNDS]) {
#pragma unroll
    for (int q = 0; q < CC_ROUNDS; ++q) r[q] = reinterpret_cast<const CcRow*>(xyz)[p[q]];
}

__global__ __launch_bounds__(64) void cc_centers_k(const float* __restrict__ xyz, const int32_t* __restrict__ perm,
                                                   const int64_t* __restrict__ offsets, int32_t nclusters,
                                                   float* __restrict__ out_centers, int64_t* __restrict__ out_sizes) {
    __shared__ float tile[3 * (CC_TILE + CC_AHEAD)];     // the spare rows are read ahead and never added
    const int k = blockIdx.x, l = threadIdx.x;
    if (k >= nclusters) return;
    const int64_t b = offsets[k], e = offsets[k + 1];
    const int64_t cnt = (b >= 0 && e > b) ? e - b : 0;   // (offsets of a grouping whose wait timed out read -1)
    CcRow r[CC_ROUNDS];
    int32_t p[CC_ROUNDS];
    float s = 0.0f;
    if (cnt > 0) {
        cc_rows_of(perm + b, cnt, 0, l, p);
        cc_rows(xyz, p, r);
        cc_rows_of(perm + b, cnt, CC_TILE, l, p);
    }
    for (int64_t t0 = 0; t0 < cnt; t0 += CC_TILE) {
#pragma unroll
        for (int q = 0; q < CC_ROUNDS; ++q) {
            float* dst = tile + 3 * (q * 64 + l);
            dst[0] = r[q].x; dst[1] = r[q].y; dst[2] = r[q].z;
        }
        // in flight during the adds below: the rows of the next tile, the perm entries of the one behind it
        cc_rows(xyz, p, r);
        cc_rows_of(perm + b, cnt, t0 + 2 * CC_TILE, l, p);
        // no workgroup barrier: it would wait for the loads just issued.  The workgroup is one wave, whose LDS
        // operations execute in program order; the wave barriers only keep the compiler from moving them
        __builtin_amdgcn_wave_barrier();
        if (l < 3) {
            const int m = (int)((cnt - t0) < CC_TILE ? (cnt - t0) : CC_TILE);
            const float* col = tile + l;
            int i = 0;
            if (m == CC_TILE) {
                // a full tile: the next CC_AHEAD values are read while these are added - under no condition (the buffer
                // ends in CC_AHEAD spare rows), so that no wait for them stands between the reads and the adds
                float a[CC_AHEAD];
#pragma unroll
                for (int u = 0; u < CC_AHEAD; ++u) a[u] = col[3 * u];
#pragma unroll 2
                for (; i < CC_TILE; i += CC_AHEAD) {
                    float nx[CC_AHEAD];
#pragma unroll
                    for (int u = 0; u < CC_AHEAD; ++u) nx[u] = col[3 * (i + CC_AHEAD + u)];
                    __builtin_amdgcn_sched_barrier(0);     // (the scheduler would sink the reads behind the adds)
#pragma unroll
                    for (int u = 0; u < CC_AHEAD; ++u) s = s + a[u];
#pragma unroll
                    for (int u = 0; u < CC_AHEAD; ++u) a[u] = nx[u];
                }
            }
            for (; i + 8 <= m; i += 8) {                   // the last tile of a cluster
                const float a0 = col[3 * (i + 0)], a1 = col[3 * (i + 1)], a2 = col[3 * (i + 2)],
                            a3 = col[3 * (i + 3)], a4 = col[3 * (i + 4)], a5 = col[3 * (i + 5)],
                            a6 = col[3 * (i + 6)], a7 = col[3 * (i + 7)];
                s = s + a0; s = s + a1; s = s + a2; s = s + a3;
                s = s + a4; s = s + a5; s = s + a6; s = s + a7;
            }
            for (; i < m; ++i) s = s + col[3 * i];
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (l < 3) out_centers[3 * (int64_t)k + l] = s / (float)cnt;      // no row: 0 / 0 = NaN
    if (l == 0 && out_sizes) out_sizes[k] = cnt;
}

// ---- merge --------------------------------------------------------------------------------------------------------
constexpr int CM_THREADS = 256;
constexpr int CM_TILE    = 64;                       // centres per side of a pair tile
constexpr int32_t CM_MAX_CLUSTERS = 65536;           // all pairs is the whole design

__global__ __launch_bounds__(CM_THREADS) void cm_init_k(int* __restrict__ parent, int32_t nclusters) {
    const int k = blockIdx.x * CM_THREADS + threadIdx.x;
    if (k < nclusters) parent[k] = k;
}

// tile pair (blockIdx.x, blockIdx.y), x <= y: thread (li, q) holds centre li of the first tile against 16 centres of the
// second.  The predicate is sklearn's KDTree.query_radius one: the reduced distance in float64, accumulated x, y, z
// (no FMA: the library is built with -ffp-contract=off), against r * r.  NaN compares false: linked to nothing.
__global__ __launch_bounds__(CM_THREADS) void cm_pairs_k(const float* __restrict__ centers, int32_t nclusters,
                                                         double r2, int* __restrict__ parent) {
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (ti > tj) return;
    __shared__ double c[2][3 * CM_TILE];
    for (int e = threadIdx.x; e < 2 * 3 * CM_TILE; e += CM_THREADS) {
        const int side = e / (3 * CM_TILE), w = e % (3 * CM_TILE);
        const int64_t g = (int64_t)(side ? tj : ti) * (3 * CM_TILE) + w;
        c[side][w] = g < 3 * (int64_t)nclusters ? (double)centers[g] : (double)NAN;
    }
    __syncthreads();
    const int li = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int i = ti * CM_TILE + li;
    const double ax = c[0][3 * li], ay = c[0][3 * li + 1], az = c[0][3 * li + 2];
    for (int jj = q * 16; jj < q * 16 + 16; ++jj) {
        const int j = tj * CM_TILE + jj;
        if (j >= nclusters || i >= j) continue;
        const double dx = ax - c[1][3 * jj], dy = ay - c[1][3 * jj + 1], dz = az - c[1][3 * jj + 2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d <= r2) uf_union(parent, i, j);
    }
}

// the root of every centre (unions are over: roots no longer move) into a table of its own - uf_find's path
// compression may still store a nearer ancestor into any parent word - and the roots flagged for the ranking scan
__global__ __launch_bounds__(CM_THREADS) void cm_flatten_k(int* __restrict__ parent, int32_t nclusters,
                                                           int* __restrict__ root, uint32_t* __restrict__ is_root) {
    const int k = blockIdx.x * CM_THREADS + threadIdx.x;
    if (k >= nclusters) return;
    const int r = uf_find(parent, k);
    root[k] = r;
    is_root[k] = r == k ? 1u : 0u;
}

// a component's root is its smallest member, so the rank of the root among the roots is the component's new id
__global__ __launch_bounds__(CM_THREADS) void cm_map_k(const int* __restrict__ root,
                                                       const uint32_t* __restrict__ rank, int32_t nclusters,
                                                       int32_t* __restrict__ out_map) {
    const int k = blockIdx.x * CM_THREADS + threadIdx.x;
    if (k < nclusters) out_map[k] = (int32_t)rank[root[k]];
}

__global__ __launch_bounds__(CM_THREADS) void cm_relabel_k(int32_t* __restrict__ labels, int64_t n,
                                                           const int32_t* __restrict__ map, int32_t nclusters) {
    const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t l = labels[i];
    labels[i] = (l >= 0 && l < nclusters) ? map[l] : -1;
}

struct CmWs { int *parent, *root; uint32_t *rank, *scan_ws; };
static void cm_plan(Arena& a, int32_t nclusters, CmWs& w) {
    const size_t kk = nclusters > 0 ? (size_t)nclusters : 1;
    w.parent = a.take<int>(kk);
    w.root = a.take<int>(kk);
    w.rank = a.take<uint32_t>(kk);
    w.scan_ws = a.take<uint32_t>(scan_ws_u32((int64_t)kk));
}

}  // namespace pch

using namespace pch;

extern "C" int pch_cluster_centers_f32(const float* xyz, const int32_t* perm, const int64_t* offsets,
                                       int32_t nclusters, float* out_centers, int64_t* out_sizes, void* stream) {
    PCH_DEVICE_GUARD(offsets);
    PCH_REQUIRE(nclusters >= 0, "negative cluster count");
    if (nclusters == 0) return PCH_OK;
    PCH_REQUIRE(offsets && out_centers, "null buffer");
    // (a grouping of no rows has no xyz / perm to point at: every cluster is then empty and neither is read)
    PCH_LAUNCH("merge_centers", cc_centers_k, dim3((unsigned)nclusters), dim3(64), 0, (hipStream_t)stream, xyz, perm,
               offsets, nclusters, out_centers, out_sizes);
    return PCH_OK;
}

extern "C" size_t pch_cluster_merge_ws_bytes(int32_t nclusters) {
    if (nclusters < 0) return 0;
    Arena a;
    CmWs w;
    cm_plan(a, nclusters, w);
    return a.off;
}

extern "C" int pch_cluster_merge_f32(const float* centers, int32_t nclusters, double merge_threshold, int32_t* labels,
                                     int64_t n, int32_t* out_map, int32_t* out_nmerged, void* ws, size_t ws_bytes,
                                     void* stream) {
    PCH_DEVICE_GUARD(out_nmerged);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(isfinite(merge_threshold) && merge_threshold >= 0.0, "merge_threshold must be finite and >= 0");
    PCH_REQUIRE(nclusters >= 0 && n >= 0 && n < (int64_t(1) << 31), "bad size");
    if (nclusters > CM_MAX_CLUSTERS) {
        set_error("pch_cluster_merge_f32: %d clusters, all pairs are tested for at most %d", nclusters, CM_MAX_CLUSTERS);
        return PCH_ERR_RANGE;
    }
    const unsigned gl = (unsigned)ceil_div(n, CM_THREADS);
    if (nclusters == 0) {
        PCH_HIP_TRY(hipMemsetAsync(out_nmerged, 0, sizeof(int32_t), s));
        if (labels && n > 0)                            // no cluster: every label is outside [0, K)
            PCH_LAUNCH("merge_relabel", cm_relabel_k, dim3(gl), dim3(CM_THREADS), 0, s, labels, n,
                       (const int32_t*)nullptr, 0);
        return PCH_OK;
    }
    PCH_REQUIRE(centers && out_map && ws, "null buffer");
    Arena a(ws, ws_bytes);
    CmWs w;
    cm_plan(a, nclusters, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    const unsigned gk = (unsigned)ceil_div(nclusters, CM_THREADS);
    const unsigned nt = (unsigned)ceil_div(nclusters, CM_TILE);
    PCH_LAUNCH("merge_init", cm_init_k, dim3(gk), dim3(CM_THREADS), 0, s, w.parent, nclusters);
    PCH_LAUNCH("merge_pairs", cm_pairs_k, dim3(nt, nt), dim3(CM_THREADS), 0, s, centers, nclusters,
               merge_threshold * merge_threshold, w.parent);
    PCH_LAUNCH("merge_flatten", cm_flatten_k, dim3(gk), dim3(CM_THREADS), 0, s, w.parent, nclusters, w.root,
               w.rank);
    PCH_TRY(scan_exclusive_u32(w.rank, w.rank, nclusters, w.scan_ws, reinterpret_cast<uint32_t*>(out_nmerged), s));
    PCH_LAUNCH("merge_map", cm_map_k, dim3(gk), dim3(CM_THREADS), 0, s, (const int*)w.root,
               (const uint32_t*)w.rank, nclusters, out_map);
    if (labels && n > 0)
        PCH_LAUNCH("merge_relabel", cm_relabel_k, dim3(gl), dim3(CM_THREADS), 0, s, labels, n,
                   (const int32_t*)out_map, nclusters);
    return PCH_OK;
}
