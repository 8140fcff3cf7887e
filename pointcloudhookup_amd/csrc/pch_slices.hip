// Tower profile: per (table, height slice) the row count and the horizontal extents of the grouped rows of
// pch_segment_by_label, in a frame per cluster.  The rule is spelled out in include/pch_hip.h; every output is a count
// or a minimum / maximum, so every output is the rule's, bit for bit.
//   sl_sweep_k   sp_sweep_k's skeleton: every wave owns one block of SL_BLOCK consecutive entries of perm, gathers the
//                block's rows, finds the first cluster it touches and walks its (cluster x block) segments.  A segment
//                is combined in the wave's own LDS table of B slices (a count and four 64-bit keys) with integer LDS
//                atomics; then the slices between the lowest and the highest one the segment touched are looked at,
//                and every occupied one issues its integer atomics on the global tables and is cleared again
//   sl_decode_k  one thread per (table, slice): the keys back to doubles, (+inf, -inf, +inf, -inf) where the count is 0
// No inline assembly, no floating-point atomic, no barrier, nothing waits on another workgroup; the same bits on every run.
#include "pch_common.h"

#include <math.h>

namespace pch {

constexpr int SL_THREADS = 256;
constexpr int SL_WAVES   = SL_THREADS / 64;
constexpr int SL_ROUNDS  = 8;                         // rows per lane and block
constexpr int SL_BLOCK   = 64 * SL_ROUNDS;            // 512 entries of perm per wave
constexpr int SL_KEYS    = 4;                         // min s, min t, max s, max t: the planes of the key tables
constexpr uint64_t SL_MIN_INIT = ~uint64_t(0), SL_MAX_INIT = 0;   // no finite double has either key

struct SlRow { float x, y, z; };

__device__ __forceinline__ int64_t sl_lane_i64(int64_t v, int i) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, i);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), i);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double sl_lane_f64(double v, int i) {
    return __longlong_as_double(sl_lane_i64(__double_as_longlong(v), i));
}

// the wave's table lies in dynamic LDS: SL_KEYS planes of B keys per wave first, then B counts per wave.  Four waves per
// SIMD is what 36 KiB of LDS per workgroup (B = 256) allows; the register budget is held to the same figure
__global__ __launch_bounds__(SL_THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) void sl_sweep_k(const float* __restrict__ xyz, const int32_t* __restrict__ perm,
                                                         const int64_t* __restrict__ offsets, int64_t n_grouped,
                                                         int32_t nclusters, const double* __restrict__ frames5,
                                                         const int32_t* __restrict__ slot, int32_t ntables, double dz,
                                                         int32_t B, int32_t* __restrict__ gcount,
                                                         unsigned long long* __restrict__ gkeys,
                                                         unsigned long long* __restrict__ goutside) {
    extern __shared__ unsigned long long sl_lds[];
    const int l = lane_id(), w = wave_id();
    const int64_t blk = (int64_t)blockIdx.x * SL_WAVES + w;
    const int64_t j0 = blk * SL_BLOCK;
    if (j0 >= n_grouped) return;                                       // (uniform per wave; the kernel has no barrier)
    const int64_t j1 = (j0 + SL_BLOCK < n_grouped) ? j0 + SL_BLOCK : n_grouped;
    unsigned long long* __restrict__ key = sl_lds + (size_t)w * SL_KEYS * B;                       // [SL_KEYS][B]
    uint32_t* __restrict__ cnt = reinterpret_cast<uint32_t*>(sl_lds + (size_t)SL_WAVES * SL_KEYS * B) + (size_t)w * B;
    const size_t plane = (size_t)ntables * (size_t)B;                  // entries of one global key plane

    // the whole block's gather is issued before anything is waited for: perm, then the 12-byte rows it names.  No load
    // stands under a condition - a lane past the end reads the last entry again and bins nothing (sp_sweep_k)
    int32_t p[SL_ROUNDS];
    SlRow r[SL_ROUNDS];
#pragma unroll
    for (int q = 0; q < SL_ROUNDS; ++q) {
        const int64_t j = j0 + q * 64 + l;
        p[q] = perm[j < n_grouped ? j : n_grouped - 1];
    }
#pragma unroll
    for (int q = 0; q < SL_ROUNDS; ++q) r[q] = reinterpret_cast<const SlRow*>(xyz)[p[q]];

    // the table starts empty and every flush leaves it empty again
    for (int b = l; b < B; b += 64) {
        cnt[b] = 0u;
        key[b] = SL_MIN_INIT; key[B + b] = SL_MIN_INIT;
        key[2 * B + b] = SL_MAX_INIT; key[3 * B + b] = SL_MAX_INIT;
    }

    // first cluster that owns an entry at or behind j0: the smallest k with offsets[k + 1] > j0
    int64_t lo = 0, hi = nclusters;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (offsets[mid + 1] > j0) hi = mid; else lo = mid + 1;
    }
    // clusters are taken 64 at a time: lane i looks up the bounds, the slot and the frame of cluster k0 + i
    for (int64_t k0 = lo; k0 < nclusters; k0 += 64) {
        const int64_t kl = (k0 + l < nclusters) ? k0 + l : (int64_t)nclusters - 1;
        const int64_t a_l = offsets[kl], b_l = offsets[kl + 1];
        const int32_t slot_l = slot[kl];
        double f_l[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) f_l[c] = frames5[5 * kl + c];
        const bool part_l = slot_l >= 0 && slot_l < ntables && isfinite(f_l[0]) && isfinite(f_l[1]) && isfinite(f_l[2]) &&
                            isfinite(f_l[3]) && isfinite(f_l[4]);
        const int32_t slot_or_none = part_l ? slot_l : -1;
        bool done = false;
        for (int i = 0; i < 64; ++i) {
            const int64_t k = k0 + i;
            if (k >= nclusters) { done = true; break; }
            const int64_t a = sl_lane_i64(a_l, i), b = sl_lane_i64(b_l, i);
            if (a >= j1) { done = true; break; }
            const int64_t s0 = a > j0 ? a : j0, s1 = b < j1 ? b : j1;
            if (s1 <= s0) continue;                                    // an empty cluster, or offsets that read -1
            const int32_t tab = __builtin_amdgcn_readlane(slot_or_none, i);
            if (tab < 0) continue;                                     // the cluster takes no part: no arithmetic
            const double cx = sl_lane_f64(f_l[0], i), cy = sl_lane_f64(f_l[1], i), z0 = sl_lane_f64(f_l[2], i);
            const double ux = sl_lane_f64(f_l[3], i), uy = sl_lane_f64(f_l[4], i);
            const int q_lo = (int)((s0 - j0) >> 6), q_hi = (int)((s1 - 1 - j0) >> 6);
            int bmin = B, bmax = -1;                                   // the slices this lane touched
            uint32_t below = 0, above = 0;                             // (wave-uniform tallies)
#pragma unroll
            for (int q = 0; q < SL_ROUNDS; ++q) {
                if (q >= q_lo && q <= q_hi) {                          // (uniform: the rounds this segment reaches)
                    const int64_t j = j0 + q * 64 + l;
                    const bool in = j >= s0 && j < s1;
                    const double dx = (double)r[q].x - cx, dy = (double)r[q].y - cy, h = (double)r[q].z - z0;
                    const double s = (dx * ux) + (dy * uy);
                    const double t = (dy * ux) - (dx * uy);
                    const double qv = floor(h / dz);                   // (a NaN fails every comparison below)
                    below += (uint32_t)__popcll(__ballot(in && qv < 0.0));
                    above += (uint32_t)__popcll(__ballot(in && qv >= (double)B));
                    if (in && qv >= 0.0 && qv < (double)B && isfinite(s) && isfinite(t)) {
                        const int bb = (int)qv;
                        const unsigned long long ks = f64_ordered(s), kt = f64_ordered(t);
                        atomicAdd(&cnt[bb], 1u);
                        atomicMin(&key[bb], ks);
                        atomicMin(&key[B + bb], kt);
                        atomicMax(&key[2 * B + bb], ks);
                        atomicMax(&key[3 * B + bb], kt);
                        bmin = bb < bmin ? bb : bmin;
                        bmax = bb > bmax ? bb : bmax;
                    }
                }
            }
            if (l == 0 && below) atomicAdd(&goutside[2 * (size_t)tab], (unsigned long long)below);
            if (l == 0 && above) atomicAdd(&goutside[2 * (size_t)tab + 1], (unsigned long long)above);
            bmin = wave_reduce_min(bmin);
            bmax = wave_reduce_max(bmax);
            // LDS operations of one wave complete in the order they were issued; the fence keeps the compiler from
            // moving the reads below in front of the atomics above
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            // only the slices between the lowest and the highest one touched are looked at: a segment of three rows
            // pays one step, not B / 64; what is occupied goes to the global tables and is cleared
            const size_t row = (size_t)tab * (size_t)B;
            for (int bb = bmin + l; bb <= bmax; bb += 64) {
                const uint32_t c = cnt[bb];
                if (c) {
                    atomicAdd(&gcount[row + bb], (int32_t)c);
                    atomicMin(&gkeys[row + bb], key[bb]);
                    atomicMin(&gkeys[plane + row + bb], key[B + bb]);
                    atomicMax(&gkeys[2 * plane + row + bb], key[2 * B + bb]);
                    atomicMax(&gkeys[3 * plane + row + bb], key[3 * B + bb]);
                    cnt[bb] = 0u;
                    key[bb] = SL_MIN_INIT; key[B + bb] = SL_MIN_INIT;
                    key[2 * B + bb] = SL_MAX_INIT; key[3 * B + bb] = SL_MAX_INIT;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        if (done) break;
    }
}

// out_ext[e] = (min s, max s, min t, max t) of entry e = table * B + slice
__global__ __launch_bounds__(SL_THREADS) void sl_decode_k(const int32_t* __restrict__ gcount,
                                                          const unsigned long long* __restrict__ gkeys, int32_t entries,
                                                          double* __restrict__ out_ext) {
    const int e = blockIdx.x * SL_THREADS + threadIdx.x;
    if (e >= entries) return;
    const bool has = gcount[e] > 0;
    const size_t plane = (size_t)entries;
    const unsigned long long smin = gkeys[e], tmin = gkeys[plane + e];
    const unsigned long long smax = gkeys[2 * plane + e], tmax = gkeys[3 * plane + e];
    double* __restrict__ o = out_ext + 4 * (size_t)e;
    o[0] = has ? f64_unordered(smin) : (double)INFINITY;
    o[1] = has ? f64_unordered(smax) : -(double)INFINITY;
    o[2] = has ? f64_unordered(tmin) : (double)INFINITY;
    o[3] = has ? f64_unordered(tmax) : -(double)INFINITY;
}

static bool sl_sizes_ok(int64_t n_grouped, int32_t nclusters, int32_t ntables, int32_t nslices) {
    return n_grouped >= 0 && n_grouped < (int64_t(1) << 31) && nclusters >= 0 && ntables >= 1 &&
           ntables <= PCH_SLICES_MAX_TABLES && nslices >= 1 && nslices <= PCH_SLICES_MAX &&
           (int64_t)ntables * (int64_t)nslices <= PCH_SLICES_MAX_ENTRIES;
}

// the two minimum planes first, then the two maximum planes: one fill each
static unsigned long long* sl_plan(Arena& a, int32_t ntables, int32_t nslices) {
    return a.take<unsigned long long>((size_t)SL_KEYS * (size_t)ntables * (size_t)nslices);
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_cluster_slices_ws_bytes(int64_t n_grouped, int32_t nclusters, int32_t ntables, int32_t nslices) {
    if (!sl_sizes_ok(n_grouped, nclusters, ntables, nslices)) return 0;
    Arena a;
    sl_plan(a, ntables, nslices);
    return a.off;
}

extern "C" int pch_cluster_slices_f32(const float* xyz, const int32_t* perm, const int64_t* offsets, int64_t n_grouped,
                                      int32_t nclusters, const double* frames5, const int32_t* slot, int32_t ntables,
                                      double dz, int32_t nslices, int32_t* out_count, double* out_ext,
                                      int64_t* out_outside, void* ws, size_t ws_bytes, void* stream) {
    PCH_REQUIRE(sl_sizes_ok(n_grouped, nclusters, ntables, nslices),
                "0 <= n_grouped < 2^31, nclusters >= 0, 1 <= ntables <= 4096, 1 <= nslices <= 256, ntables * nslices <= 2^20");
    PCH_REQUIRE(isfinite(dz) && dz > 0.0, "dz must be finite and > 0");
    PCH_REQUIRE(out_count && out_ext && out_outside, "null table buffer");
    PCH_REQUIRE(ws, "null workspace");
    const bool sweep = n_grouped > 0 && nclusters > 0;
    PCH_REQUIRE(nclusters == 0 || (offsets && frames5 && slot), "null cluster buffer");
    PCH_REQUIRE(!sweep || (xyz && perm), "null rows");
    PCH_DEVICE_GUARD(ws);
    // every buffer a launch would follow is looked up (a null one is skipped: what is needed was checked above)
    const void* follow[] = {out_count, out_ext, out_outside, sweep ? offsets : nullptr, sweep ? frames5 : nullptr,
                            sweep ? slot : nullptr, sweep ? xyz : nullptr, sweep ? perm : nullptr};
    for (const void* q : follow) {
        DeviceGuard in(q);
        if (in.rc != PCH_OK) return in.rc;
    }
    hipStream_t s = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    unsigned long long* keys = sl_plan(a, ntables, nslices);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    const size_t entries = (size_t)ntables * (size_t)nslices;
    PCH_HIP_TRY(hipMemsetAsync(keys, 0xFF, 2 * entries * sizeof(unsigned long long), s));
    PCH_HIP_TRY(hipMemsetAsync(keys + 2 * entries, 0, 2 * entries * sizeof(unsigned long long), s));
    PCH_HIP_TRY(hipMemsetAsync(out_count, 0, entries * sizeof(int32_t), s));
    PCH_HIP_TRY(hipMemsetAsync(out_outside, 0, 2 * (size_t)ntables * sizeof(int64_t), s));
    if (sweep) {
        const int64_t nb = ceil_div(n_grouped, SL_BLOCK);
        const size_t lds = (size_t)SL_WAVES * (size_t)nslices * (SL_KEYS * sizeof(unsigned long long) + sizeof(uint32_t));
        PCH_LAUNCH("cluster_slices", sl_sweep_k, dim3((unsigned)ceil_div(nb, SL_WAVES)), dim3(SL_THREADS), lds, s, xyz,
                   perm, offsets, n_grouped, nclusters, frames5, slot, ntables, dz, nslices, out_count, keys,
                   reinterpret_cast<unsigned long long*>(out_outside));
    }
    PCH_LAUNCH("cluster_slices_decode", sl_decode_k, dim3((unsigned)ceil_div((int64_t)entries, SL_THREADS)),
               dim3(SL_THREADS), 0, s, (const int32_t*)out_count, (const unsigned long long*)keys, (int32_t)entries,
               out_ext);
    return PCH_OK;
}
