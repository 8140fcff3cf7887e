// Opt-in LAS-integer frame of stage B: the cloud is centred on the int32 LAS records BEFORE anything is rounded to
// float32 (the remedy of the reference's own test/pipei.py:68-79, restated on the integers).  The rule is written
// out in include/pch_hip.h (pch_ground_filter_las_i32); in short
//   C_j = floor(sum_i XYZ[i,j] / n)                       exact int64 sum, order free
//   p[i,j] = (float)((double)(XYZ[i,j] - C_j) * scale_j)  one float64 multiply, one rounding
//   base = np.percentile(p[:,2], pct) in float32; keep p_z > base + offset, or + fallback_offset when fewer than
//   min_keep rows are kept.
// Z -> p_z is non-decreasing, so the two order statistics of the percentile are the images of the order statistics of
// the Z integers: the select runs on the integers and never sees a float.
// Launch sequence (nothing reads back to the host, no grid depends on data, no copy of the cloud is made):
//   fr_sum_k -> fr_hist_k<0> -> fr_hist_k<1> -> fr_hist_k<2> -> fr_thr_k -> fr_filter_k<0> -> fr_filter_k<1> -> fr_finish_k
// Every sweep reads the 12-byte rows once; a histogram pass whose bits the range of Z does not need returns at once.
#include "pch_compact.h"
#include "pch_select.h"

namespace pch {

constexpr int FR_THREADS = 256;
constexpr int FR_CHUNK   = 1024;                        // rows per workgroup trip of the element sweeps: 768 16-byte words
constexpr int FR_GRID    = 2048;                        // workgroups of an element sweep at most (grid-stride beyond)
constexpr int FR_BINS    = 4096;                        // 12 bits per histogram pass
constexpr int FR_ROUNDS  = 8;
constexpr int FR_TILE    = FR_THREADS * FR_ROUNDS;      // 2048 rows per workgroup of the filter sweep
constexpr int FR_WROWS   = 64 * FR_ROUNDS;              // rows of one wave of it

struct FrScale { double v[3]; };
struct FrSel { unsigned long long rank; uint32_t prefix, pad; };   // rank inside the prefix, resolved high bits of the key

struct FrState {
    long long sum[3];                                   // S_j
    uint32_t  zlo, zhi;                                 // max of ~biased(Z) / biased(Z): 0 is the neutral start
    FrSel     sel[2][2];                                // [rank][p]: the state in front of histogram pass p + 1
    long long C[3];
    float     base, thr[2];
    uint32_t  pad0;
    long long cnt[2];                                   // count words of the two sweeps (oc_count_update)
    uint32_t  ticket[2], pad1[2];
    uint32_t  slots[2][OC_SLOTS][6];
};

// the one carve-up of the workspace (size query and call); everything in it starts as zeros
struct FrWs {
    int64_t   nt;
    FrState*  st;
    uint32_t* hist;                                     // pass 0 (both ranks), then passes 1, 2 of rank 0, of rank 1
    uint64_t* status;                                   // [2][nt] look-back words of the two sweeps
    FrWs(Arena& a, int64_t n) : nt(ceil_div(n > 0 ? n : 1, FR_TILE)) {
        st = a.take<FrState>(1);
        hist = a.take<uint32_t>(6 * FR_BINS);
        status = a.take<uint64_t>(2 * nt);
    }
};
__host__ __device__ __forceinline__ uint32_t* fr_hist_of(uint32_t* hist, int rank, int pass) {
    return hist + ((pass == 0 ? 0 : rank) * 3 + pass) * FR_BINS;
}

__device__ __forceinline__ uint32_t fr_biased(int32_t z) { return (uint32_t)z ^ 0x80000000u; }   // order preserving

// ---- every element of the [n,3] int32 array once, in no particular order: f(column, value).  Whole chunks of 1024
// rows are read as 768 aligned 16-byte words, thread t takes words t, 256 + t, 512 + t of the chunk; word w of a chunk
// starts at element 4 w, column (4 w) mod 3 = w mod 3 = (k + t) mod 3 for w = 256 k + t.  The rows behind the last
// whole chunk (and every row of a base that is not 16-byte aligned) go element by element.
template <class F>
__device__ __forceinline__ void fr_each(const int32_t* __restrict__ X, int64_t n, F&& f) {
    const bool vec = (reinterpret_cast<uintptr_t>(X) & 15u) == 0;
    const int64_t nfull = vec ? n / FR_CHUNK : 0;
    const int c0 = (int)(threadIdx.x % 3);
    for (int64_t chunk = blockIdx.x; chunk < nfull; chunk += gridDim.x) {
        const uint4* __restrict__ w4 = reinterpret_cast<const uint4*>(X + chunk * (3 * FR_CHUNK));
        uint4 q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = w4[k * FR_THREADS + threadIdx.x];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int c = (c0 + k) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            f(c, (int32_t)q[k].x);
            f(c1, (int32_t)q[k].y);
            f(c2, (int32_t)q[k].z);
            f(c, (int32_t)q[k].w);
        }
    }
    const int64_t total = 3 * n;
    for (int64_t e = nfull * (3 * FR_CHUNK) + (int64_t)blockIdx.x * FR_THREADS + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * FR_THREADS)
        f((int)(e % 3), X[e]);
}
static_assert(FR_THREADS % 3 == 1 && (3 * FR_CHUNK) % 4 == 0 && (3 * FR_CHUNK / 4) % 3 == 0, "fr_each's column rule");

// ---- sweep 1: the three int64 column sums and the range of Z.  Per-lane accumulators, a wave reduce, then one 64-bit
// integer atomic per workgroup and column: integer adds are order free, so the sums are exact and reproducible.
__global__ __launch_bounds__(FR_THREADS) void fr_sum_k(const int32_t* __restrict__ X, int64_t n,
                                                       FrState* __restrict__ st) {
    __shared__ long long sum_sh[OC_WAVES][3];
    __shared__ uint32_t z_sh[OC_WAVES][2];
    long long s[3] = {0, 0, 0};
    uint32_t lo = 0u, hi = 0u;
    fr_each(X, n, [&](int c, int32_t v) {
        s[0] += c == 0 ? (long long)v : 0ll;
        s[1] += c == 1 ? (long long)v : 0ll;
        s[2] += c == 2 ? (long long)v : 0ll;
        const uint32_t k = fr_biased(v);
        if (c == 2) { hi = k > hi ? k : hi; lo = ~k > lo ? ~k : lo; }
    });
#pragma unroll
    for (int a = 0; a < 3; ++a) s[a] = wave_reduce_add(s[a]);
    lo = wave_reduce_max(lo);
    hi = wave_reduce_max(hi);
    if (lane_id() == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) sum_sh[wave_id()][a] = s[a];
        z_sh[wave_id()][0] = lo;
        z_sh[wave_id()][1] = hi;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        long long t = 0;
        for (int w = 0; w < OC_WAVES; ++w) t += sum_sh[w][threadIdx.x];
        atomicAdd(reinterpret_cast<unsigned long long*>(&st->sum[threadIdx.x]), (unsigned long long)t);
    } else if (threadIdx.x < 5) {
        const int j = threadIdx.x - 3;
        uint32_t t = 0u;
        for (int w = 0; w < OC_WAVES; ++w) t = z_sh[w][j] > t ? z_sh[w][j] : t;
        atomicMax(j == 0 ? &st->zlo : &st->zhi, t);
    }
}

// ---- the select's key: Z - zmin as uint32, cut into at most three digits from the top of the bits the RANGE of Z
// needs (a cloud spans a few 10^4 counts: the top 12 bits of a raw 32-bit key would be one bin).  Digit p is
// (key >> s[p]) & (2^w[p] - 1); w = 12, 12, 8 at the full int32 range, and a digit of width 0 has nothing to resolve.
struct FrGeom { uint32_t zmin; int s[3], w[3]; };
__device__ __forceinline__ FrGeom fr_geom(const FrState* __restrict__ st) {
    FrGeom g;
    const uint32_t bmin = ~st->zlo, bmax = st->zhi;     // biased minimum and maximum of Z
    g.zmin = bmin ^ 0x80000000u;                        // (uint32)zmin
    const uint32_t range = bmax - bmin;
    int bits = range ? 32 - __clz((int)range) : 0;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        g.w[p] = bits < 12 ? bits : 12;
        bits -= g.w[p];
        g.s[p] = bits;
    }
    return g;                                           // bits <= 32: 12 + 12 + 8 cover it, s[2] == 0
}

// the pick behind a histogram pass (every thread of the workgroup calls; barriers): the bin that holds the rank
__device__ __forceinline__ FrSel fr_pick(const FrSel& in, const uint32_t* __restrict__ hist, int width) {
    __shared__ unsigned long long wsum[OC_WAVES];
    __shared__ uint32_t found_bin;
    __shared__ unsigned long long found_below;
    if (width == 0) return in;                          // workgroup-uniform
    constexpr int per = FR_BINS / FR_THREADS;
    unsigned long long loc[per], tsum = 0;
#pragma unroll
    for (int j = 0; j < per; ++j) { loc[j] = hist[threadIdx.x * per + j]; tsum += loc[j]; }
    const unsigned long long incl = wave_scan_incl(tsum);
    __syncthreads();                                    // a previous call may still be reading the shared words
    if (lane_id() == 63) wsum[wave_id()] = incl;
    if (threadIdx.x == 0) { found_bin = 0u; found_below = 0ull; }
    __syncthreads();
    unsigned long long before = incl - tsum;
    for (int w = 0; w < wave_id(); ++w) before += wsum[w];
    if (in.rank >= before && in.rank < before + tsum) { // the one thread whose bins hold the rank
        unsigned long long b = before;
#pragma unroll
        for (int j = 0; j < per; ++j) {
            if (in.rank >= b && in.rank < b + loc[j]) { found_bin = threadIdx.x * per + j; found_below = b; }
            b += loc[j];
        }
    }
    __syncthreads();
    FrSel out;
    out.rank = in.rank - found_below;
    out.prefix = (in.prefix << width) | found_bin;
    out.pad = 0u;
    return out;
}

// ---- sweeps 2..4: histogram pass PASS of both ranks (k0 and k1 = k0 + 1, or k0 twice) over the Z of the rows.  The
// pick of the pass in front runs as this kernel's prologue in every workgroup (workgroup 0 records it), as sel_hist_k
// does; pass 0 has no prefix, so both ranks share its histogram.
template <int PASS>
__global__ __launch_bounds__(FR_THREADS) void fr_hist_k(const int32_t* __restrict__ X, int64_t n,
                                                        unsigned long long k0, unsigned long long k1,
                                                        FrState* __restrict__ st, uint32_t* __restrict__ hist) {
    constexpr int NH = PASS == 0 ? 1 : 2;
    __shared__ uint32_t hh[NH][FR_BINS];
    const FrGeom g = fr_geom(st);
    FrSel in[2] = {{k0, 0u, 0u}, {k1, 0u, 0u}};
    if (PASS >= 1) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (PASS == 2) in[r] = st->sel[r][0];
            in[r] = fr_pick(in[r], fr_hist_of(hist, r, PASS - 1), g.w[PASS >= 1 ? PASS - 1 : 0]);
            if (blockIdx.x == 0 && threadIdx.x == 0) st->sel[r][PASS - 1] = in[r];
        }
    }
    const int width = g.w[PASS];
    if (width == 0) return;                             // the digits in front resolved the key: nothing to count
    for (int j = threadIdx.x; j < NH * FR_BINS; j += FR_THREADS) (&hh[0][0])[j] = 0u;
    __syncthreads();
    const int shift = g.s[PASS], up = PASS >= 1 ? g.s[PASS - 1] : 0;
    const uint32_t mask = (1u << width) - 1u;
    fr_each(X, n, [&](int c, int32_t v) {
        if (c != 2) return;
        const uint32_t key = (uint32_t)v - g.zmin;
        if (PASS == 0) {
            atomicAdd(&hh[0][key >> shift], 1u);
        } else {
#pragma unroll
            for (int r = 0; r < NH; ++r)
                if ((key >> up) == in[r].prefix) atomicAdd(&hh[r][(key >> shift) & mask], 1u);
        }
    });
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NH; ++r) {
        uint32_t* out = fr_hist_of(hist, r, PASS);
        for (int j = threadIdx.x; j < FR_BINS; j += FR_THREADS) {
            const uint32_t t = hh[r][j];
            if (t) atomicAdd(&out[j], t);
        }
    }
}

// a centred coordinate: the int64 difference is exact, then ONE float64 multiply and ONE rounding to float32
__device__ __forceinline__ float fr_centred(int32_t v, long long c, double scale) {
    return (float)((double)((long long)v - c) * scale);
}

// ---- one workgroup: the last pick, the floor division, the percentile's interpolation and the two thresholds
__global__ __launch_bounds__(FR_THREADS) void fr_thr_k(int64_t n, FrScale sc, int same, float gamma, float offset,
                                                       float fallback_offset, FrState* __restrict__ st,
                                                       uint32_t* __restrict__ hist) {
    const FrGeom g = fr_geom(st);
    FrSel fin[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) fin[r] = fr_pick(st->sel[r][1], fr_hist_of(hist, r, 2), g.w[2]);
    if (threadIdx.x != 0) return;
    long long C[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const long long S = st->sum[a];
        long long q = S / n;
        if (S % n != 0 && S < 0) --q;                   // floor, Python's //, not C truncation
        C[a] = q;
        st->C[a] = q;
    }
    const int32_t z0 = (int32_t)(g.zmin + fin[0].prefix), z1 = (int32_t)(g.zmin + fin[1].prefix);
    const float a = fr_centred(z0, C[2], sc.v[2]);
    const float b = same ? a : fr_centred(z1, C[2], sc.v[2]);
    const float base = sel_lerp_f32(a, b, gamma);
    st->base = base;
    st->thr[0] = base + offset;
    st->thr[1] = base + fallback_offset;
}

// ---- sweeps 5 (and 6): the register-resident ordered compaction of pch_compact.h on the integer rows, modelled on
// pl_filter_k.  A wave brings its 512 rows into LDS as 384 aligned 16-byte words and reads them back a row per lane.
// WHICH = 1 is the fallback threshold: its workgroups return at once unless sweep 0 kept fewer than min_keep rows.
template <int WHICH>
__global__ __launch_bounds__(FR_THREADS) void fr_filter_k(const int32_t* __restrict__ X, int64_t n, FrScale sc,
                                                          long long min_keep, FrState* __restrict__ st,
                                                          uint64_t* __restrict__ status,
                                                          float* __restrict__ out_points,
                                                          int32_t* __restrict__ out_index) {
    __shared__ __attribute__((aligned(16))) int32_t rows[OC_WAVES][3 * FR_WROWS];
    __shared__ uint32_t box[OC_WAVES][6];
    if (WHICH == 1) {
        const long long kept = st->cnt[0];
        if (kept < 0 || kept >= min_keep) return;       // the first threshold stands (or its sweep failed)
    }
    const int64_t tile = oc_take_tile(&st->ticket[WHICH]);
    const long long C[3] = {st->C[0], st->C[1], st->C[2]};
    const float thr = st->thr[WHICH];
    const int l = lane_id();
    const int64_t seg = tile * FR_TILE + (int64_t)wave_id() * FR_WROWS;
    const int64_t left = n - seg;                       // rows of this wave's share that exist (may be <= 0)
    int32_t* mine = rows[wave_id()];
    if (left >= FR_WROWS && (reinterpret_cast<uintptr_t>(X) & 15u) == 0) {      // wave-uniform
        const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(X + 3 * seg);   // seg * 12 is a multiple of 16
        uint4* t4 = reinterpret_cast<uint4*>(mine);
#pragma unroll
        for (int i = 0; i < 3 * FR_WROWS / 4 / 64; ++i) t4[i * 64 + l] = s4[i * 64 + l];
    } else {
        for (int e = l; e < 3 * FR_WROWS; e += 64) mine[e] = (int64_t)e < 3 * left ? X[3 * seg + e] : 0;
    }
    __builtin_amdgcn_wave_barrier();
    unsigned long long m[FR_ROUNDS];
#pragma unroll
    for (int r = 0; r < FR_ROUNDS; ++r) {
        const int row = r * 64 + l;
        const float pz = fr_centred(mine[3 * row + 2], C[2], sc.v[2]);
        m[r] = __ballot(row < left && pz > thr);
    }
    const uint32_t woff = oc_place(m, status, tile, reinterpret_cast<int64_t*>(&st->cnt[WHICH]));
    if (woff == OC_NONE) return;
    const float zero[3] = {0.0f, 0.0f, 0.0f};           // the rows are centred already
    uint32_t lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};
    oc_visit(m, woff, [&](int r, int64_t o) {
        const int row = r * 64 + l;
        oc_emit(fr_centred(mine[3 * row], C[0], sc.v[0]), fr_centred(mine[3 * row + 1], C[1], sc.v[1]),
                fr_centred(mine[3 * row + 2], C[2], sc.v[2]), zero, o, seg + row, out_points, out_index, lo, hi);
    });
    oc_fold_box(st->slots[WHICH], tile, lo, hi, box);
}
static_assert((3 * FR_WROWS) % (4 * 64) == 0 && (12 * FR_WROWS) % 16 == 0, "fr_filter_k's 16-byte words");

// ---- the record of the call
__global__ void fr_finish_k(const FrState* __restrict__ st, long long min_keep, PchLasFrame* __restrict__ out) {
    const long long kept = st->cnt[0];
    const uint32_t use_b = kept >= 0 && kept < min_keep ? 1u : 0u;
    if (threadIdx.x == 0) {
        for (int a = 0; a < 3; ++a) out->centroid[a] = st->C[a];
        out->count = st->cnt[use_b];                    // negative after a look-back wait that ran out
        out->count_at_offset = kept;
        out->base = st->base;
        out->threshold = st->thr[use_b];
        out->used_fallback = use_b;
        out->reserved = 0u;
    }
    if (threadIdx.x < 6) out->aabb[threadIdx.x] = oc_box_word(st->slots[use_b], threadIdx.x);
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_ground_filter_las_ws_bytes(int64_t n) {
    if (n < 0) return 0;
    Arena a;
    FrWs w(a, n);
    (void)w;
    return a.off;
}

extern "C" int pch_ground_filter_las_i32(const int32_t* XYZ, int64_t n, const double* scale3_host, double pct,
                                         float offset, float fallback_offset, int64_t min_keep, float* out_points,
                                         int32_t* out_index, PchLasFrame* out_frame_dev, void* ws, size_t ws_bytes,
                                         void* stream) {
    PCH_REQUIRE(n >= 1 && n < (int64_t(1) << 31), "n out of range [1, 2^31)");
    PCH_REQUIRE(scale3_host, "null scale");
    FrScale sc;
    for (int a = 0; a < 3; ++a) {
        sc.v[a] = scale3_host[a];
        PCH_REQUIRE(sc.v[a] > 0.0 && sc.v[a] < INFINITY, "a scale must be finite and > 0");
    }
    PCH_REQUIRE(pct >= 0.0 && pct <= 100.0, "Percentiles must be in the range [0, 100]");
    PCH_REQUIRE(XYZ && out_points && out_frame_dev && ws, "null buffer");
    PCH_DEVICE_GUARD(XYZ);
    hipStream_t s = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    const FrWs w(a, n);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    PCH_HIP_TRY(hipMemsetAsync(ws, 0, a.off, s));
    const PctIndex pi = pct_index(n, pct);
    const unsigned long long k0 = (unsigned long long)pi.k0, k1 = pi.same ? k0 : k0 + 1;
    int64_t gb = ceil_div(n, FR_CHUNK);
    if (gb > FR_GRID) gb = FR_GRID;
    const dim3 sweep((unsigned)gb), tiles((unsigned)w.nt), blk(FR_THREADS);
    PCH_LAUNCH("fr_sum", fr_sum_k, sweep, blk, 0, s, XYZ, n, w.st);
    PCH_LAUNCH("fr_hist0", fr_hist_k<0>, sweep, blk, 0, s, XYZ, n, k0, k1, w.st, w.hist);
    PCH_LAUNCH("fr_hist1", fr_hist_k<1>, sweep, blk, 0, s, XYZ, n, k0, k1, w.st, w.hist);
    PCH_LAUNCH("fr_hist2", fr_hist_k<2>, sweep, blk, 0, s, XYZ, n, k0, k1, w.st, w.hist);
    PCH_LAUNCH("fr_thr", fr_thr_k, dim3(1), blk, 0, s, n, sc, pi.same, pi.gamma, offset, fallback_offset, w.st, w.hist);
    PCH_LAUNCH("fr_filter", fr_filter_k<0>, tiles, blk, 0, s, XYZ, n, sc, (long long)min_keep, w.st, w.status,
               out_points, out_index);
    PCH_LAUNCH("fr_filter_fb", fr_filter_k<1>, tiles, blk, 0, s, XYZ, n, sc, (long long)min_keep, w.st,
               w.status + w.nt, out_points, out_index);
    PCH_LAUNCH("fr_finish", fr_finish_k, dim3(1), dim3(64), 0, s, (const FrState*)w.st, (long long)min_keep,
               out_frame_dev);
    return PCH_OK;
}
