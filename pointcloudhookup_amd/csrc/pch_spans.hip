// Conductor spans: per-cluster float64 sums over the grouped rows of pch_segment_by_label, the input of
// the sag-curve fit.  The rule is spelled out in include/pch_hip.h.  One segmented-reduction skeleton, two sets of terms:
//   sp_sweep_k<T>   every wave owns one block of SP_BLOCK consecutive entries of perm, whatever the cluster sizes.  It
//                   gathers the block's rows, searches offsets for the first cluster it touches, reduces every segment
//                   (cluster x block) it holds in the wave and writes one partial per segment to the workspace
//   sp_finish_k<T>  sixteen threads per cluster, one per term: adds the cluster's partials in ascending block order
// A cluster of ten million rows is swept by twenty thousand waves; nothing waits on another workgroup, no floating-point
// atomic is used, and the order of every sum is a function of offsets alone: the same bits on every run.
#include "pch_common.h"

#include <math.h>

namespace pch {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES   = SP_THREADS / 64;
constexpr int SP_ROUNDS  = 8;                         // rows per lane and block
constexpr int SP_BLOCK   = 64 * SP_ROUNDS;            // 512 entries of perm per wave
constexpr int SP_SLOT    = 16;                        // doubles per partial (128 bytes): sums first, then the extrema
constexpr int SP_AHEAD   = 16;                        // partials sp_finish_k reads ahead of its adds

struct SpRow { float x, y, z; };

// The partial of (block b, cluster k) lies in slot b + k.  Blocks and clusters both ascend along perm, so the pairs
// that hold rows form a staircase on which b + k strictly grows: no two share a slot, and the partials of cluster k
// are the consecutive slots first_block + k .. last_block + k.  No count, no scan, no atomic.
static inline int64_t sp_blocks(int64_t n_grouped) { return ceil_div(n_grouped > 0 ? n_grouped : 0, SP_BLOCK); }
static inline size_t  sp_slots(int64_t n_grouped, int32_t nclusters) {
    return (size_t)sp_blocks(n_grouped) + (size_t)(nclusters > 0 ? nclusters : 0) + 1;
}

__device__ __forceinline__ int64_t sp_lane_i64(int64_t v, int i) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, i);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), i);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double sp_lane_f64(double v, int i) { return __longlong_as_double(sp_lane_i64(__double_as_longlong(v), i)); }
__device__ __forceinline__ float  sp_lane_f32(float v, int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i)); }

// ---- the two sets of terms ------------------------------------------------------------------------------------------
// step 1: differences from the cluster's first row, the nine sums of pch_dbscan_shape_f32 in its order
struct SpMoments {
    static constexpr int NS = 9, NE = 0;
    struct Lane { float ox, oy, oz; };                 // what a lane holds for the cluster it looks up
    struct Par  { double ox, oy, oz; };                // the same for the segment the wave is in
    const float* origin;                               // [K,3]
    __device__ __forceinline__ Lane load(int64_t k) const {
        return Lane{origin[3 * k], origin[3 * k + 1], origin[3 * k + 2]};
    }
    __device__ __forceinline__ static Par pick(const Lane& a, int i) {
        return Par{(double)sp_lane_f32(a.ox, i), (double)sp_lane_f32(a.oy, i), (double)sp_lane_f32(a.oz, i)};
    }
    __device__ __forceinline__ static void terms(const SpRow& r, const Par& p, double (&t)[NS], double (&e)[2]) {
        const double dx = (double)r.x - p.ox, dy = (double)r.y - p.oy, dz = (double)r.z - p.oz;
        t[0] = dx; t[1] = dy; t[2] = dz;
        t[3] = dx * dx; t[4] = dy * dy; t[5] = dz * dz;
        t[6] = dx * dy; t[7] = dx * dz; t[8] = dy * dz;
        e[0] = e[1] = 0.0;
    }
};

// step 3: along-track coordinate s, across-track t and height dz in the cluster's frame; ten sums, four extrema
struct SpProfile {
    static constexpr int NS = 10, NE = 4;
    struct Lane { double f[6]; };
    struct Par  { double f[6]; };
    const double* frames;                              // [K,6]
    __device__ __forceinline__ Lane load(int64_t k) const {
        Lane a;
#pragma unroll
        for (int j = 0; j < 6; ++j) a.f[j] = frames[6 * k + j];
        return a;
    }
    __device__ __forceinline__ static Par pick(const Lane& a, int i) {
        Par p;
#pragma unroll
        for (int j = 0; j < 6; ++j) p.f[j] = sp_lane_f64(a.f[j], i);
        return p;
    }
    __device__ __forceinline__ static void terms(const SpRow& r, const Par& p, double (&t)[NS], double (&e)[2]) {
        const double dx = (double)r.x - p.f[0], dy = (double)r.y - p.f[1], dz = (double)r.z - p.f[2];
        const double s = ((dx * p.f[3]) + (dy * p.f[4])) * p.f[5];
        const double tt = (dy * p.f[3]) - (dx * p.f[4]);
        const double s2 = s * s;
        t[0] = s; t[1] = s2; t[2] = s2 * s; t[3] = s2 * s2;
        t[4] = dz; t[5] = s * dz; t[6] = s2 * dz; t[7] = dz * dz;
        t[8] = tt; t[9] = tt * tt;
        e[0] = s; e[1] = dz;
    }
};

// o_k = the first row of every cluster that has one, zeros for the others
__global__ __launch_bounds__(SP_THREADS) void sp_origin_k(const float* __restrict__ xyz, const int32_t* __restrict__ perm,
                                                          const int64_t* __restrict__ offsets, int64_t n_grouped,
                                                          int32_t nclusters, float* __restrict__ out_origin) {
    const int64_t k = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (k >= nclusters) return;
    const int64_t b = offsets[k], e = offsets[k + 1];
    SpRow o{0.0f, 0.0f, 0.0f};
    if (b >= 0 && e > b && b < n_grouped) o = reinterpret_cast<const SpRow*>(xyz)[perm[b]];
    out_origin[3 * k] = o.x; out_origin[3 * k + 1] = o.y; out_origin[3 * k + 2] = o.z;
}

template <class T>
__global__ __launch_bounds__(SP_THREADS) void sp_sweep_k(const float* __restrict__ xyz, const int32_t* __restrict__ perm,
                                                         const int64_t* __restrict__ offsets, int64_t n_grouped,
                                                         int32_t nclusters, T terms, double* __restrict__ partial) {
    constexpr int NS = T::NS, NE = T::NE;
    const int l = lane_id();
    const int64_t blk = (int64_t)blockIdx.x * SP_WAVES + wave_id();
    const int64_t j0 = blk * SP_BLOCK;
    if (j0 >= n_grouped) return;                                       // (uniform per wave)
    const int64_t j1 = (j0 + SP_BLOCK < n_grouped) ? j0 + SP_BLOCK : n_grouped;

    // the whole block's gather is issued before anything is waited for: perm, then the 12-byte rows it names.  No load
    // stands under a condition - a lane past the end reads the last entry again and adds nothing (cc_rows_of, cc_rows)
    int32_t p[SP_ROUNDS];
    SpRow r[SP_ROUNDS];
#pragma unroll
    for (int q = 0; q < SP_ROUNDS; ++q) {
        const int64_t j = j0 + q * 64 + l;
        p[q] = perm[j < n_grouped ? j : n_grouped - 1];
    }
#pragma unroll
    for (int q = 0; q < SP_ROUNDS; ++q) r[q] = reinterpret_cast<const SpRow*>(xyz)[p[q]];

    // first cluster that owns an entry at or behind j0: the smallest k with offsets[k + 1] > j0
    int64_t lo = 0, hi = nclusters;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (offsets[mid + 1] > j0) hi = mid; else lo = mid + 1;
    }
    // clusters are taken 64 at a time: lane i looks up the bounds and the parameters of cluster k0 + i
    for (int64_t k0 = lo; k0 < nclusters; k0 += 64) {
        const int64_t kl = (k0 + l < nclusters) ? k0 + l : (int64_t)nclusters - 1;
        const int64_t a_l = offsets[kl], b_l = offsets[kl + 1];
        const typename T::Lane par_l = terms.load(kl);
        bool done = false;
        for (int i = 0; i < 64; ++i) {
            const int64_t k = k0 + i;
            if (k >= nclusters) { done = true; break; }
            const int64_t a = sp_lane_i64(a_l, i), b = sp_lane_i64(b_l, i);
            if (a >= j1) { done = true; break; }
            const int64_t s0 = a > j0 ? a : j0, s1 = b < j1 ? b : j1;
            if (s1 <= s0) continue;                                    // an empty cluster, or offsets that read -1
            const typename T::Par par = T::pick(par_l, i);
            const int q_lo = (int)((s0 - j0) >> 6), q_hi = (int)((s1 - 1 - j0) >> 6);
            double acc[NS];
            double mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY};
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s] = 0.0;
#pragma unroll
            for (int q = 0; q < SP_ROUNDS; ++q) {
                if (q >= q_lo && q <= q_hi) {                          // (uniform: the rounds this segment reaches)
                    const int64_t j = j0 + q * 64 + l;
                    const bool in = j >= s0 && j < s1;
                    double t[NS], e[2];
                    T::terms(r[q], par, t, e);
#pragma unroll
                    for (int s = 0; s < NS; ++s) acc[s] = in ? acc[s] + t[s] : acc[s];
                    if (NE) {
#pragma unroll
                        for (int c = 0; c < 2; ++c) {
                            mn[c] = (in && e[c] < mn[c]) ? e[c] : mn[c];
                            mx[c] = (in && e[c] > mx[c]) ? e[c] : mx[c];
                        }
                    }
                }
            }
            // butterflies over the wave, two dwords per value; every lane ends with every total
            double out = 0.0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double v = wave_reduce_add(acc[s]);
                if (l == s) out = v;
            }
            if (NE) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const double vmin = wave_reduce_min(mn[c]), vmax = wave_reduce_max(mx[c]);
                    if (l == NS + 2 * c) out = -vmin;                   // (negated: sp_finish_k folds every extremum as a maximum)
                    if (l == NS + 2 * c + 1) out = vmax;
                }
            }
            if (l < NS + NE) partial[(blk + k) * SP_SLOT + l] = out;
        }
        if (done) break;
    }
}

// thread t of cluster k's sixteen folds term t of the cluster's partials, first block first.  Two register buffers of
// SP_AHEAD values take turns: while one is folded the other is in flight, under no condition - only the last, short
// batches read an index past the end (the last slot again) and fold under one.  A sum and an extremum differ in one
// select, so the sixteen threads do not diverge.  The chain of folds of one long cluster is this kernel's time.
template <bool TAIL>
__device__ __forceinline__ void sp_read(const double* __restrict__ ptr, int64_t left, double (&w)[SP_AHEAD]) {
#pragma unroll
    for (int u = 0; u < SP_AHEAD; ++u) {
        const int64_t at = TAIL ? (u < left ? u : (left > 0 ? left - 1 : 0)) : u;
        w[u] = ptr[at * SP_SLOT];
    }
}
template <bool TAIL>
__device__ __forceinline__ double sp_fold(double v, const double (&w)[SP_AHEAD], int64_t left, bool is_ext) {
#pragma unroll
    for (int u = 0; u < SP_AHEAD; ++u) {
        const double next = is_ext ? fmax(v, w[u]) : v + w[u];            // (fmax skips a NaN, as the sweep does)
        v = (!TAIL || u < left) ? next : v;
    }
    return v;
}

template <class T>
__global__ __launch_bounds__(SP_THREADS) void sp_finish_k(const int64_t* __restrict__ offsets, int64_t n_grouped,
                                                          int32_t nclusters, const double* __restrict__ partial,
                                                          int64_t nslots, int64_t* __restrict__ out_count,
                                                          double* __restrict__ out_sums, double* __restrict__ out_ext) {
    constexpr int NS = T::NS, NE = T::NE;
    const int64_t g = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    const int64_t k = g >> 4;
    const int t = (int)(g & 15);
    if (k >= nclusters) return;
    int64_t b = offsets[k], e = offsets[k + 1];
    if (b < 0) b = 0;
    if (e > n_grouped) e = n_grouped;
    const int64_t cnt = e > b ? e - b : 0;
    if (t == 0 && out_count) out_count[k] = cnt;
    if (t >= NS + NE) return;
    const bool is_ext = t >= NS, is_min = is_ext && ((t - NS) & 1) == 0;   // (a minimum arrives negated)
    double v = is_ext ? -(double)INFINITY : 0.0;
    const int64_t first = b / SP_BLOCK + k, last = (e - 1) / SP_BLOCK + k;  // slots
    if (cnt > 0 && last < nslots) {
        const double* ptr = partial + first * SP_SLOT + t;
        int64_t left = last - first + 1;
        double w0[SP_AHEAD], w1[SP_AHEAD];
        sp_read<true>(ptr, left, w0);
        while (left >= 3 * SP_AHEAD) {                     // both batches behind the one in w0 are whole
            sp_read<false>(ptr + SP_AHEAD * SP_SLOT, left, w1);
            __builtin_amdgcn_sched_barrier(0);             // (the scheduler would sink the reads behind the folds)
            v = sp_fold<false>(v, w0, left, is_ext);
            sp_read<false>(ptr + 2 * SP_AHEAD * SP_SLOT, left, w0);
            __builtin_amdgcn_sched_barrier(0);
            v = sp_fold<false>(v, w1, left, is_ext);
            ptr += 2 * SP_AHEAD * SP_SLOT;
            left -= 2 * SP_AHEAD;
        }
        while (left > 0) {                                 // at most three short trips
            const int64_t behind = left > SP_AHEAD ? left - SP_AHEAD : 0;
            sp_read<true>(behind ? ptr + SP_AHEAD * SP_SLOT : ptr, behind, w1);
            v = sp_fold<true>(v, w0, left, is_ext);
#pragma unroll
            for (int u = 0; u < SP_AHEAD; ++u) w0[u] = w1[u];
            ptr += SP_AHEAD * SP_SLOT;
            left -= SP_AHEAD;
        }
    }
    if (t < NS) out_sums[k * NS + t] = v;
    else out_ext[k * NE + (t - NS)] = is_min ? -v : v;
}

static double* sp_plan(Arena& a, int64_t n_grouped, int32_t nclusters) {
    return a.take<double>(sp_slots(n_grouped, nclusters) * SP_SLOT);
}

template <class T>
static int sp_run(const char* sweep_name, const char* finish_name, const float* xyz, const int32_t* perm,
                  const int64_t* offsets, int64_t n_grouped, int32_t nclusters, const T& terms, int64_t* out_count,
                  double* out_sums, double* out_ext, double* partial, hipStream_t s) {
    const int64_t nb = sp_blocks(n_grouped);
    if (nb > 0)
        PCH_LAUNCH(sweep_name, sp_sweep_k<T>, dim3((unsigned)ceil_div(nb, SP_WAVES)), dim3(SP_THREADS), 0, s, xyz, perm,
                   offsets, n_grouped, nclusters, terms, partial);
    PCH_LAUNCH(finish_name, sp_finish_k<T>, dim3((unsigned)ceil_div(16 * (int64_t)nclusters, SP_THREADS)),
               dim3(SP_THREADS), 0, s, offsets, n_grouped, nclusters, (const double*)partial,
               (int64_t)sp_slots(n_grouped, nclusters), out_count, out_sums, out_ext);
    return PCH_OK;
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_cluster_moments_ws_bytes(int64_t n_grouped, int32_t nclusters) {
    if (n_grouped < 0 || nclusters < 0) return 0;
    Arena a;
    sp_plan(a, n_grouped, nclusters);
    return a.off;
}

extern "C" int pch_cluster_moments_f32(const float* xyz, const int32_t* perm, const int64_t* offsets, int64_t n_grouped,
                                       int32_t nclusters, int64_t* out_count, float* out_origin, double* out_moments,
                                       void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(out_moments ? (const void*)out_moments : (const void*)offsets);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n_grouped >= 0 && n_grouped < (int64_t(1) << 31) && nclusters >= 0, "bad size");
    if (nclusters == 0) return PCH_OK;
    PCH_REQUIRE(offsets && out_count && out_origin && out_moments && ws, "null buffer");
    PCH_REQUIRE(n_grouped == 0 || (xyz && perm), "null rows");
    Arena a(ws, ws_bytes);
    double* partial = sp_plan(a, n_grouped, nclusters);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    PCH_LAUNCH("span_origin", sp_origin_k, dim3((unsigned)ceil_div(nclusters, SP_THREADS)), dim3(SP_THREADS), 0, s, xyz,
               perm, offsets, n_grouped, nclusters, out_origin);
    return sp_run("span_moments", "span_moments_finish", xyz, perm, offsets, n_grouped, nclusters,
                  SpMoments{out_origin}, out_count, out_moments, (double*)nullptr, partial, s);
}

extern "C" size_t pch_cluster_profile_ws_bytes(int64_t n_grouped, int32_t nclusters) {
    return pch_cluster_moments_ws_bytes(n_grouped, nclusters);
}

extern "C" int pch_cluster_profile_f32(const float* xyz, const int32_t* perm, const int64_t* offsets, int64_t n_grouped,
                                       int32_t nclusters, const double* frames, double* out_sums, double* out_ext,
                                       void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(out_sums ? (const void*)out_sums : (const void*)offsets);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n_grouped >= 0 && n_grouped < (int64_t(1) << 31) && nclusters >= 0, "bad size");
    if (nclusters == 0) return PCH_OK;
    PCH_REQUIRE(offsets && frames && out_sums && out_ext && ws, "null buffer");
    PCH_REQUIRE(n_grouped == 0 || (xyz && perm), "null rows");
    Arena a(ws, ws_bytes);
    double* partial = sp_plan(a, n_grouped, nclusters);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    return sp_run("span_profile", "span_profile_finish", xyz, perm, offsets, n_grouped, nclusters, SpProfile{frames},
                  (int64_t*)nullptr, out_sums, out_ext, partial, s);
}
