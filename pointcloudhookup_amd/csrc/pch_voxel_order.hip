// Stage A, opt-in: the rows pch_voxel_downsample_f64 wrote, every chunk's slice sorted by (ix, iy, iz) - an order
// that is a function of the input alone (the stage's own order depends on its tuning constants).
// One reduction for the bit widths, one device-wide LSD sort on [chunk | ix | iy | iz] (two where that key is wider
// than 64 bits), one gather of the 40-byte rows.
#include "pch_common.h"
#include "pch_prims.h"

namespace pch {

constexpr int VO_THREADS = 256;
constexpr int VO_MAX_ROUNDS = 8;                       // rows per thread of the reduction
constexpr int VO_ROWS = 1024;                          // rows per workgroup of the gather

// meta[0..2] = largest index per axis (compared as uint32: a negative index reads as >= 2^31), meta[3] = 1 when
// chunk_offsets[0] == 0 and chunk_offsets[nchunks] == m
__global__ __launch_bounds__(VO_THREADS) void vo_max_k(const int32_t* __restrict__ idx, int64_t m,
                                                       const int64_t* __restrict__ offs, int64_t nchunks,
                                                       uint32_t* __restrict__ meta) {
    __shared__ uint32_t part[VO_THREADS / 64][3];
    uint32_t mx = 0, my = 0, mz = 0;
    const int64_t base = (int64_t)blockIdx.x * (VO_THREADS * VO_MAX_ROUNDS);
#pragma unroll
    for (int r = 0; r < VO_MAX_ROUNDS; ++r) {
        const int64_t i = base + r * VO_THREADS + threadIdx.x;
        if (i < m) {
            const uint32_t x = (uint32_t)idx[3 * i], y = (uint32_t)idx[3 * i + 1], z = (uint32_t)idx[3 * i + 2];
            mx = x > mx ? x : mx;
            my = y > my ? y : my;
            mz = z > mz ? z : mz;
        }
    }
    mx = wave_reduce_max(mx);
    my = wave_reduce_max(my);
    mz = wave_reduce_max(mz);
    if (lane_id() == 0) { part[wave_id()][0] = mx; part[wave_id()][1] = my; part[wave_id()][2] = mz; }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t v = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < VO_THREADS / 64; ++w) v = part[w][threadIdx.x] > v ? part[w][threadIdx.x] : v;
        atomicMax(&meta[threadIdx.x], v);
    }
    if (blockIdx.x == 0 && threadIdx.x == 3) meta[3] = (offs[0] == 0 && offs[nchunks] == m) ? 1u : 0u;
}

// which fields of the virtual key [chunk | ix | iy | iz] one sort takes, and their widths
struct VoKey { int bx, by, bz; int chunk, x, yz; };

// chunk of output row r: the number of chunk ends at or below it (empty chunks are stepped over)
__device__ __forceinline__ uint64_t vo_chunk_of(const int64_t* __restrict__ offs, int64_t nchunks, int64_t r) {
    int64_t lo = 0, hi = nchunks;                      // answer in [lo, hi): offs[lo] <= r < offs[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (offs[mid] <= r) lo = mid; else hi = mid;
    }
    return (uint64_t)lo;
}

// first sort (src == nullptr): key of row i, value i.  Second sort: key of row src[i]; the values stay where they are.
__global__ __launch_bounds__(VO_THREADS) void vo_keys_k(const int32_t* __restrict__ idx, int64_t m,
                                                        const int64_t* __restrict__ offs, int64_t nchunks, VoKey k,
                                                        const uint32_t* __restrict__ src, uint64_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * VO_THREADS + threadIdx.x;
    if (i >= m) return;
    const int64_t r = src ? (int64_t)src[i] : i;
    uint64_t key = 0;
    if (k.chunk) key = vo_chunk_of(offs, nchunks, r);
    if (k.x) key = (key << k.bx) | (uint64_t)(uint32_t)idx[3 * r];
    if (k.yz) {
        key = (key << k.by) | (uint64_t)(uint32_t)idx[3 * r + 1];
        key = (key << k.bz) | (uint64_t)(uint32_t)idx[3 * r + 2];
    }
    keys[i] = key;
    if (!src) vals[i] = (uint32_t)i;
}

// out row i = in row perm[i].  A workgroup owns VO_ROWS consecutive OUTPUT rows, i.e. three contiguous stretches of
// the output arrays, and writes them as 16-byte stores in lane order; the reads are the scattered side (12 and 24
// contiguous bytes per source row).  The tile's first element is a multiple of 4 in every array, so only the last
// tile meets a ragged vector.
__global__ __launch_bounds__(VO_THREADS) void vo_gather_k(const uint32_t* __restrict__ perm, int64_t m,
                                                          const int32_t* __restrict__ idx,
                                                          const double* __restrict__ mean,
                                                          const int32_t* __restrict__ count,
                                                          int32_t* __restrict__ out_idx, double* __restrict__ out_mean,
                                                          int32_t* __restrict__ out_count,
                                                          int32_t* __restrict__ out_perm) {
    __shared__ uint32_t src[VO_ROWS];
    const int64_t row0 = (int64_t)blockIdx.x * VO_ROWS;
    const int rows = (int)((m - row0) < VO_ROWS ? (m - row0) : VO_ROWS);
    for (int j = threadIdx.x; j < rows; j += VO_THREADS) {
        const uint32_t p = perm[row0 + j];
        src[j] = p;
        if (out_perm) out_perm[row0 + j] = (int32_t)p;
    }
    __syncthreads();
    const int elems = 3 * rows;
    // idx: 3 int32 per row, four elements per store
    for (int e = 4 * threadIdx.x; e < elems; e += 4 * VO_THREADS) {
        int32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = e + j;
            v[j] = t < elems ? idx[3 * (int64_t)src[t / 3] + t % 3] : 0;
        }
        int32_t* dst = out_idx + 3 * row0 + e;
        if (e + 4 <= elems) *reinterpret_cast<int4*>(dst) = make_int4(v[0], v[1], v[2], v[3]);
        else for (int j = 0; e + j < elems; ++j) dst[j] = v[j];
    }
    // mean: 3 float64 per row, two elements per store
    for (int e = 2 * threadIdx.x; e < elems; e += 2 * VO_THREADS) {
        const double a = mean[3 * (int64_t)src[e / 3] + e % 3];
        double* dst = out_mean + 3 * row0 + e;
        if (e + 2 <= elems) {
            const double b = mean[3 * (int64_t)src[(e + 1) / 3] + (e + 1) % 3];
            *reinterpret_cast<double2*>(dst) = make_double2(a, b);
        } else dst[0] = a;
    }
    // count: one int32 per row, four rows per store
    for (int e = 4 * threadIdx.x; e < rows; e += 4 * VO_THREADS) {
        int32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = e + j < rows ? count[src[e + j]] : 0;
        int32_t* dst = out_count + row0 + e;
        if (e + 4 <= rows) *reinterpret_cast<int4*>(dst) = make_int4(v[0], v[1], v[2], v[3]);
        else for (int j = 0; e + j < rows; ++j) dst[j] = v[j];
    }
}

struct VoWs {
    uint32_t* meta;
    uint64_t* k[2];
    uint32_t* v[2];
    uint32_t* radix;
};

static void order_plan(Arena& a, int64_t m, VoWs& w) {
    const int64_t mm = m > 0 ? m : 1;
    w.meta = a.take<uint32_t>(4);
    w.k[0] = a.take<uint64_t>(mm);
    w.k[1] = a.take<uint64_t>(mm);
    w.v[0] = a.take<uint32_t>(mm);
    w.v[1] = a.take<uint32_t>(mm);
    w.radix = a.take<uint32_t>(radix_ws_u32(mm));
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_voxel_canonical_order_ws_bytes(int64_t m, int64_t nchunks) {
    if (m < 0 || m >= (int64_t(1) << 31) || nchunks < 0) return 0;
    Arena a;
    VoWs w;
    order_plan(a, m, w);
    return a.off;
}

extern "C" int pch_voxel_canonical_order(const int32_t* idx, const double* mean, const int32_t* count,
                                         const int64_t* chunk_offsets, int64_t nchunks, int64_t m,
                                         int32_t* out_idx, double* out_mean, int32_t* out_count, int32_t* out_perm,
                                         void* ws, size_t ws_bytes, void* stream) {
    PCH_REQUIRE(m >= 0 && nchunks >= 1 && nchunks < (int64_t(1) << 31), "m < 0 or nchunks outside [1, 2^31)");
    if (m >= (int64_t(1) << 31)) { set_error("m out of range [0, 2^31)"); return PCH_ERR_RANGE; }
    if (m == 0) return PCH_OK;
    PCH_DEVICE_GUARD(idx);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(idx && mean && count && chunk_offsets && out_idx && out_mean && out_count && ws, "null buffer");
    PCH_REQUIRE((const void*)out_idx != (const void*)idx && (const void*)out_mean != (const void*)mean &&
                (const void*)out_count != (const void*)count, "outputs must not alias the inputs");
    PCH_REQUIRE((((uintptr_t)out_idx | (uintptr_t)out_mean | (uintptr_t)out_count) & 15) == 0,
                "output buffers must be 16-byte aligned");
    Arena a(ws, ws_bytes);
    VoWs w;
    order_plan(a, m, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }

    PCH_HIP_TRY(hipMemsetAsync(w.meta, 0, sizeof(uint32_t) * 4, s));
    PCH_LAUNCH("voxel_order_max", vo_max_k, dim3((unsigned)ceil_div(m, VO_THREADS * VO_MAX_ROUNDS)), dim3(VO_THREADS),
               0, s, idx, m, chunk_offsets, nchunks, w.meta);
    uint32_t meta[4];                                                  // the one host read: the sort's pass count
    PCH_TRY(peek_enqueue(w.meta, sizeof(meta), s));
    PCH_TRY(peek_wait(meta, sizeof(meta)));
    PCH_REQUIRE(meta[0] <= 0x7fffffffu && meta[1] <= 0x7fffffffu && meta[2] <= 0x7fffffffu, "negative voxel index");
    PCH_REQUIRE(meta[3] == 1u, "chunk_offsets must run from 0 to m");

    const int bx = bits_for((uint64_t)meta[0] + 1), by = bits_for((uint64_t)meta[1] + 1),
              bz = bits_for((uint64_t)meta[2] + 1), cb = bits_for((uint64_t)nchunks);
    const unsigned grid = (unsigned)ceil_div(m, VO_THREADS);
    int res;                                                           // buffer that holds the sorted permutation
    if (cb + bx + by + bz <= 64) {
        const VoKey all = {bx, by, bz, 1, 1, 1};
        PCH_LAUNCH("voxel_order_keys", vo_keys_k, dim3(grid), dim3(VO_THREADS), 0, s, idx, m, chunk_offsets, nchunks,
                   all, (const uint32_t*)nullptr, w.k[0], w.v[0]);
        PCH_TRY(radix_sort_pairs(w.k[0], w.v[0], w.k[1], w.v[1], m, cb + bx + by + bz, w.radix, s));
        res = radix_sort_result_buffer(cb + bx + by + bz);
    } else {
        // the low fields first, then the high fields of the permuted rows: the sort is stable.  Three axes of an
        // int32 index are at most 93 bits, so x moves to the second sort where the three do not fit one key.
        const int x_low = bx + by + bz <= 64;
        const VoKey low = {bx, by, bz, 0, x_low, 1}, high = {bx, by, bz, 1, !x_low, 0};
        const int nlow = (x_low ? bx : 0) + by + bz, nhigh = cb + (x_low ? 0 : bx);
        PCH_LAUNCH("voxel_order_keys", vo_keys_k, dim3(grid), dim3(VO_THREADS), 0, s, idx, m, chunk_offsets, nchunks,
                   low, (const uint32_t*)nullptr, w.k[0], w.v[0]);
        PCH_TRY(radix_sort_pairs(w.k[0], w.v[0], w.k[1], w.v[1], m, nlow, w.radix, s));
        const int r1 = radix_sort_result_buffer(nlow);
        PCH_LAUNCH("voxel_order_keys", vo_keys_k, dim3(grid), dim3(VO_THREADS), 0, s, idx, m, chunk_offsets, nchunks,
                   high, (const uint32_t*)w.v[r1], w.k[r1], (uint32_t*)nullptr);
        PCH_TRY(radix_sort_pairs(w.k[r1], w.v[r1], w.k[1 - r1], w.v[1 - r1], m, nhigh, w.radix, s));
        res = r1 ^ radix_sort_result_buffer(nhigh);
    }
    PCH_LAUNCH("voxel_order_gather", vo_gather_k, dim3((unsigned)ceil_div(m, VO_ROWS)), dim3(VO_THREADS), 0, s,
               (const uint32_t*)w.v[res], m, idx, mean, count, out_idx, out_mean, out_count, out_perm);
    return PCH_OK;
}
