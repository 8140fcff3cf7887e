// Crop of a cloud by MANY boxes in one sweep (axis-aligned and oriented): what the viewer does per tower with one
// boolean mask over the whole cloud (test/kuangxuan.py:60-79, the scaled oriented boxes of ui/extract.py:345-420).
//   sweep   : tiles of 2048 rows by ticket, every row tested against the boxes whose cull bounds meet the tile's own
//             bounding box (the box, the bitmap of those boxes and its walk: pch_tilecull.h); the hits leave as
//             (box, row) pairs in (row, box) order (one look-back per tile, as crop_aabb_k), the tile adds its hits
//             per box to the box's count
//   offsets : exclusive scan of the per-box counts, the total
//   group   : stable radix sort of the pairs by box (pch_prims.h) - rows stay ascending inside a box
//   gather  : the points (and rows) of the grouped pairs
#include <math.h>

#include <vector>

#include "pch_lookback.h"
#include "pch_prims.h"
#include "pch_tilecull.h"

namespace pch {

constexpr int CB_THREADS = 256;
constexpr int CB_ROUNDS  = 8;
constexpr int CB_TILE    = CB_THREADS * CB_ROUNDS;          // 2048 rows per workgroup
constexpr int CB_WAVES   = CB_THREADS / 64;
constexpr int CB_MAXBOX  = 4096;
constexpr int CB_WORDS   = CB_MAXBOX / 64;                  // words of the active-box bitmap

struct CbRow { double x, y, z; };
// a box as the device sees it: the cull bounds (pch_crop_box_bounds_f64) in front of the caller's record
struct CbBox { double cull[6]; PchCropBox b; };
struct CbState { uint32_t ticket, failed, pad[2]; };

// ---- the cull bounds (host).  Kind 0: the box itself.  Kind 1, R orthonormal: the predicate accepts p iff
// |u_k| <= half_k for u = R^T d, d = p - center, and then d = R u gives |d_j| <= r_j = sum_k |R[j][k]| * half_k.
// What is returned is center_j -+ w_j, w_j = (r_j + CB_SLACK * hmax) * (1 + 1e-9), moved two floats outwards, where
// hmax = max_k |half_k|.  The slack absorbs
//   (a) an R that is orthonormal only to delta = max |R^T R - I| <= CB_ORTHO: d = R (R^T R)^-1 u, and the entries
//       of (R^T R)^-1 - I are below 1.01 delta, so |d_j| <= r_j + sum_k |R[j][k]| * 3.03 delta hmax
//       <= r_j + 5.3e-6 hmax (a row of R has 1-norm <= sqrt(3 (1 + delta)));
//   (b) the rounding of the predicate: the subtraction and the three products and two sums of u_k make a relative
//       error below 5 * 2^-53 on sum_j |d_j R[j][k]| <= 3 * 1.01 * sqrt(3) hmax, so an accepted row has
//       |u_k| <= half_k + 2e-15 hmax - nothing beside (a);
// the factor (1 + 1e-9) the few roundings of r_j and w_j themselves (relative 2^-52 each), and the two floats the
// rounding of center_j -+ w_j (half a unit of the result, which is what counts next to a centre of 3e6 and a half
// extent of 1e-3).  An R further from orthonormal than CB_ORTHO, or any NaN / inf among center, axes and half, gives
// bounds of -inf / +inf (or NaN): a box whose bounds are not all finite is never culled.
constexpr double CB_ORTHO = 1e-6;
constexpr double CB_SLACK = 8e-6;

static void cb_bounds_one(const PchCropBox& b, double* out6) {
    if (b.kind == 0) {
        for (int j = 0; j < 3; ++j) { out6[j] = b.lo[j]; out6[3 + j] = b.hi[j]; }
        return;
    }
    const double* R = b.axes;
    bool ortho = true;                                   // NaN fails the comparison
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) {
            const double g = R[a] * R[c] + R[3 + a] * R[3 + c] + R[6 + a] * R[6 + c] - (a == c ? 1.0 : 0.0);
            if (!(fabs(g) <= CB_ORTHO)) ortho = false;
        }
    double hmax = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (!isfinite(b.half[k]) || !isfinite(b.center[k])) ortho = false;
        hmax = fmax(hmax, fabs(b.half[k]));
    }
    for (int j = 0; j < 3; ++j) {
        if (!ortho) { out6[j] = -INFINITY; out6[3 + j] = INFINITY; continue; }
        const double r = fabs(R[3 * j]) * fabs(b.half[0]) + fabs(R[3 * j + 1]) * fabs(b.half[1]) +
                         fabs(R[3 * j + 2]) * fabs(b.half[2]);
        const double w = (r + CB_SLACK * hmax) * (1.0 + 1e-9);
        out6[j] = nextafter(nextafter(b.center[j] - w, -INFINITY), -INFINITY);
        out6[3 + j] = nextafter(nextafter(b.center[j] + w, INFINITY), INFINITY);
    }
}

// ---- the two predicates.  Kind 0: crop_aabb_k's six inclusive comparisons.  Kind 1: float64 without contraction,
// d = p - center, u_k = (d_x R[0][k] + d_y R[1][k]) + d_z R[2][k], inside iff -half_k <= u_k <= half_k (k = 0, 1, 2).
__device__ __forceinline__ bool cb_inside(const CbRow& q, const PchCropBox& b) {
    if (b.kind == 0)
        return q.x >= b.lo[0] && q.x <= b.hi[0] && q.y >= b.lo[1] && q.y <= b.hi[1] && q.z >= b.lo[2] && q.z <= b.hi[2];
    const double dx = q.x - b.center[0], dy = q.y - b.center[1], dz = q.z - b.center[2];
    const double u0 = (dx * b.axes[0] + dy * b.axes[3]) + dz * b.axes[6];
    const double u1 = (dx * b.axes[1] + dy * b.axes[4]) + dz * b.axes[7];
    const double u2 = (dx * b.axes[2] + dy * b.axes[5]) + dz * b.axes[8];
    return u0 >= -b.half[0] && u0 <= b.half[0] && u1 >= -b.half[1] && u1 <= b.half[1] && u2 >= -b.half[2] &&
           u2 <= b.half[2];
}

__global__ __launch_bounds__(CB_THREADS) void cb_sweep_k(const double* __restrict__ xyz, int64_t n,
                                                         const CbBox* __restrict__ boxes, int nboxes,
                                                         CbState* __restrict__ st, uint64_t* __restrict__ status,
                                                         int64_t cap, uint64_t* __restrict__ out_box,
                                                         uint32_t* __restrict__ out_row,
                                                         unsigned long long* __restrict__ box_count) {
    __shared__ uint64_t active[CB_WORDS];
    __shared__ uint32_t hist[CB_MAXBOX];
    __shared__ double wlo[CB_WAVES][3], whi[CB_WAVES][3];
    __shared__ uint32_t wtot[CB_WAVES];
    __shared__ uint32_t tile_sh, excl_sh;
    if (threadIdx.x == 0) tile_sh = atomicAdd(&st->ticket, 1u);
    for (int j = threadIdx.x; j < nboxes; j += CB_THREADS) hist[j] = 0;
    __syncthreads();
    const int64_t tile = tile_sh;
    const int w = wave_id(), l = lane_id();
    const int nwords = (nboxes + 63) >> 6;
    const int64_t seg = tile * CB_TILE + (int64_t)w * (64 * CB_ROUNDS);
    const CbRow* __restrict__ rows = reinterpret_cast<const CbRow*>(xyz);
    CbRow q[CB_ROUNDS];
#pragma unroll
    for (int r = 0; r < CB_ROUNDS; ++r) {
        const int64_t i = seg + r * 64 + l;
        q[r] = rows[i < n ? i : 0];
    }
    // the tile's bounding box over its finite rows (a row holding NaN or inf cannot be inside a finite box)
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int r = 0; r < CB_ROUNDS; ++r) {
        const int64_t i = seg + r * 64 + l;
        if (i < n && isfinite(q[r].x) && isfinite(q[r].y) && isfinite(q[r].z)) {
            lo[0] = fmin(lo[0], q[r].x); hi[0] = fmax(hi[0], q[r].x);
            lo[1] = fmin(lo[1], q[r].y); hi[1] = fmax(hi[1], q[r].y);
            lo[2] = fmin(lo[2], q[r].z); hi[2] = fmax(hi[2], q[r].z);
        }
    }
    // the boxes this tile has to test: every box takes part
    cull_tile_box(lo, hi, wlo, whi);
    cull_tile_bitmap<CB_WAVES>(active, nboxes, lo, hi, [&](int t, const double*& blo, const double*& bhi) {
        blo = boxes[t].cull;
        bhi = boxes[t].cull + 3;
        return true;
    });
    // first pass: hits per row and round, hits per box
    uint32_t cnt[CB_ROUNDS];
#pragma unroll
    for (int r = 0; r < CB_ROUNDS; ++r) cnt[r] = 0;
    uint32_t run = 0;
    {
        int word = -1;
        uint64_t bits = 0;
        for (int t = cull_next_bit(active, nwords, word, bits); t >= 0; t = cull_next_bit(active, nwords, word, bits)) {
            const PchCropBox& b = boxes[t].b;
            uint32_t got = 0;
#pragma unroll
            for (int r = 0; r < CB_ROUNDS; ++r) {
                const bool keep = seg + r * 64 + l < n && cb_inside(q[r], b);
                cnt[r] += keep ? 1u : 0u;
                got += (uint32_t)__popcll(__ballot(keep));
            }
            if (got && l == 0) atomicAdd(&hist[t], got);
            run += got;
        }
    }
    if (l == 0) wtot[w] = run;
    __syncthreads();
    uint32_t T = 0;
#pragma unroll
    for (int w2 = 0; w2 < CB_WAVES; ++w2) T += wtot[w2];
    if (w == 0) {
        const uint32_t e0 = gf_lookback(status, tile, T);
        const bool lb_failed = e0 == GF_LB_FAILED;
        if (l == 0) {
            excl_sh = lb_failed ? 0u : e0;               // prefix 0 keeps the writes below inside the pair list
            if (lb_failed) atomicOr(&st->failed, 1u);    // cb_offsets_k turns it into the sign bit of the count word
        }
    }
    for (int j = threadIdx.x; j < nboxes; j += CB_THREADS)
        if (hist[j]) atomicAdd(&box_count[j], (unsigned long long)hist[j]);
    __syncthreads();
    if (run == 0) return;
    // second pass: the pairs, in (row, box) order.  Only boxes that counted a hit in this tile are tested again, and
    // only against the rounds of this wave that hold one.
    uint32_t woff = excl_sh;
    for (int w2 = 0; w2 < w; ++w2) woff += wtot[w2];
    uint32_t pos[CB_ROUNDS];
    uint32_t some = 0;                                   // rounds of this wave with a hit (wave-uniform)
#pragma unroll
    for (int r = 0; r < CB_ROUNDS; ++r) {
        const uint32_t incl = wave_scan_incl(cnt[r]);
        pos[r] = woff + incl - cnt[r];
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        woff += tot;
        some |= tot ? 1u << r : 0u;
    }
    int word = -1;
    uint64_t bits = 0;
    for (int t = cull_next_bit(active, nwords, word, bits); t >= 0; t = cull_next_bit(active, nwords, word, bits)) {
        if (__builtin_amdgcn_readfirstlane((int)hist[t]) == 0) continue;
        const PchCropBox& b = boxes[t].b;
#pragma unroll
        for (int r = 0; r < CB_ROUNDS; ++r) {
            if (!((some >> r) & 1u)) continue;
            const int64_t i = seg + r * 64 + l;
            if (cnt[r] && i < n && cb_inside(q[r], b)) {
                if ((int64_t)pos[r] < cap) { out_box[pos[r]] = (uint64_t)t; out_row[pos[r]] = (uint32_t)i; }
                ++pos[r];
            }
        }
    }
}

// out_offsets = exclusive scan of the per-box counts (one workgroup; 16 boxes per thread cover CB_MAXBOX), the count
// word = the total, with the sign bit when a tile's look-back gave up
__global__ __launch_bounds__(CB_THREADS) void cb_offsets_k(const unsigned long long* __restrict__ box_count,
                                                           int nboxes, const CbState* __restrict__ st,
                                                           int64_t* __restrict__ out_offsets,
                                                           int64_t* __restrict__ out_count) {
    constexpr int PER = CB_MAXBOX / CB_THREADS;
    __shared__ unsigned long long wsum[CB_WAVES];
    const int w = wave_id(), l = lane_id();
    const int t0 = threadIdx.x * PER;
    unsigned long long c[PER], mine = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { c[k] = t0 + k < nboxes ? box_count[t0 + k] : 0ull; mine += c[k]; }
    const unsigned long long incl = wave_scan_incl(mine);
    if (l == 63) wsum[w] = incl;
    __syncthreads();
    unsigned long long run = incl - mine, total = 0;
#pragma unroll
    for (int w2 = 0; w2 < CB_WAVES; ++w2) { if (w2 < w) run += wsum[w2]; total += wsum[w2]; }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (t0 + k < nboxes) out_offsets[t0 + k] = (int64_t)run;
        run += c[k];
    }
    if (threadIdx.x == 0) {
        out_offsets[nboxes] = (int64_t)total;
        *out_count = (int64_t)(st->failed ? total | (1ull << 63) : total);
    }
}

__global__ __launch_bounds__(CB_THREADS) void cb_gather_k(const double* __restrict__ xyz,
                                                          int64_t n, const uint32_t* __restrict__ row, int64_t cap,
                                                          const int64_t* __restrict__ count,
                                                          double* __restrict__ out_points,
                                                          int64_t* __restrict__ out_index) {
    const int64_t j = (int64_t)blockIdx.x * CB_THREADS + threadIdx.x;
    const int64_t m = *count;                            // negative (a look-back gave up): nothing is gathered
    if (j >= cap || j >= m) return;
    const uint32_t i = row[j];
    if ((int64_t)i >= n) return;                         // cannot happen below 2^31 hits; keeps the read inside xyz
    reinterpret_cast<CbRow*>(out_points)[j] = reinterpret_cast<const CbRow*>(xyz)[i];
    if (out_index) out_index[j] = (int64_t)i;
}

struct CbWs {
    CbState* st;
    uint64_t* status;
    CbBox* boxes;
    unsigned long long* box_count;
    uint64_t *k0, *k1;
    uint32_t *v0, *v1, *radix_ws;
};
static void cb_plan(Arena& a, int64_t n, int32_t nboxes, int64_t cap, CbWs& w) {
    // state, status words and box counts in front: one fill zeroes them
    w.st = a.take<CbState>(1);
    w.status = a.take<uint64_t>(ceil_div(n > 0 ? n : 1, CB_TILE));
    w.box_count = a.take<unsigned long long>(nboxes > 0 ? nboxes : 1);
    w.boxes = a.take<CbBox>(nboxes > 0 ? nboxes : 1);
    w.k0 = a.take<uint64_t>(cap);
    w.v0 = a.take<uint32_t>(cap);
    w.k1 = a.take<uint64_t>(cap);
    w.v1 = a.take<uint32_t>(cap);
    w.radix_ws = a.take<uint32_t>(radix_ws_u32(cap));
}
static bool cb_sizes_ok(int64_t n, int32_t nboxes, int64_t cap) {
    return n >= 0 && n < (int64_t(1) << 32) && nboxes >= 0 && nboxes <= CB_MAXBOX && cap >= 0;
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_crop_boxes_ws_bytes(int64_t n, int32_t nboxes, int64_t cap) {
    if (!cb_sizes_ok(n, nboxes, cap) || cap >= (int64_t(1) << 31)) return 0;
    Arena a;
    CbWs w;
    cb_plan(a, n, nboxes, cap, w);
    return a.off;
}

extern "C" int pch_crop_box_bounds_f64(const PchCropBox* boxes_host, int32_t nboxes, double* out_lo3_hi3) {
    PCH_REQUIRE(nboxes >= 0 && nboxes <= CB_MAXBOX, "0 <= nboxes <= 4096");
    PCH_REQUIRE(nboxes == 0 || (boxes_host && out_lo3_hi3), "null buffer");
    for (int32_t t = 0; t < nboxes; ++t) PCH_REQUIRE(boxes_host[t].kind == 0 || boxes_host[t].kind == 1, "unknown box kind");
    for (int32_t t = 0; t < nboxes; ++t) cb_bounds_one(boxes_host[t], out_lo3_hi3 + 6 * (size_t)t);
    return PCH_OK;
}

extern "C" int pch_crop_boxes_f64(const double* xyz, int64_t n, const PchCropBox* boxes_host, int32_t nboxes,
                                  int64_t cap, double* out_points, int64_t* out_index, int64_t* out_offsets,
                                  int64_t* out_count, void* ws, size_t ws_bytes, void* stream) {
    PCH_REQUIRE(cb_sizes_ok(n, nboxes, cap) && out_offsets && out_count, "bad argument");
    PCH_REQUIRE(nboxes == 0 || boxes_host, "null box table");
    for (int32_t t = 0; t < nboxes; ++t) PCH_REQUIRE(boxes_host[t].kind == 0 || boxes_host[t].kind == 1, "unknown box kind");
    if (cap >= (int64_t(1) << 31)) { set_error("pch_crop_boxes_f64: cap must stay below 2^31 hits"); return PCH_ERR_RANGE; }
    PCH_DEVICE_GUARD(out_count);
    hipStream_t s = (hipStream_t)stream;
    PCH_HIP_TRY(hipMemsetAsync(out_offsets, 0, sizeof(int64_t) * ((size_t)nboxes + 1), s));
    PCH_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(int64_t), s));
    if (n == 0 || nboxes == 0) return PCH_OK;
    PCH_REQUIRE(xyz && ws && (cap == 0 || out_points), "null buffer");
    Arena a(ws, ws_bytes);
    CbWs w;
    cb_plan(a, n, nboxes, cap, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    std::vector<CbBox> table((size_t)nboxes);
    for (int32_t t = 0; t < nboxes; ++t) {
        table[t].b = boxes_host[t];
        cb_bounds_one(boxes_host[t], table[t].cull);
    }
    PCH_HIP_TRY(hipMemsetAsync(ws, 0, (size_t)(reinterpret_cast<char*>(w.boxes) - static_cast<char*>(ws)), s));
    // pageable source: the runtime has staged the table when the call returns
    PCH_HIP_TRY(hipMemcpyAsync(w.boxes, table.data(), sizeof(CbBox) * (size_t)nboxes, hipMemcpyHostToDevice, s));
    // the box of a slot no hit reaches reads as all ones: behind every box in the sort below
    const int nbits = nboxes > 1 ? bits_for((uint64_t)nboxes + 1) : 0;
    if (nbits && cap) PCH_HIP_TRY(hipMemsetAsync(w.k0, 0xFF, sizeof(uint64_t) * (size_t)cap, s));
    const int64_t nt = ceil_div(n, CB_TILE);
    PCH_LAUNCH("crop_sweep", cb_sweep_k, dim3((unsigned)nt), dim3(CB_THREADS), 0, s, xyz, n, (const CbBox*)w.boxes,
               (int)nboxes, w.st, w.status, cap, w.k0, w.v0, w.box_count);
    PCH_LAUNCH("crop_offsets", cb_offsets_k, dim3(1), dim3(CB_THREADS), 0, s, (const unsigned long long*)w.box_count,
               (int)nboxes, (const CbState*)w.st, out_offsets, out_count);
    if (cap == 0) return PCH_OK;
    PCH_TRY(radix_sort_pairs(w.k0, w.v0, w.k1, w.v1, cap, nbits, w.radix_ws, s));      // one box: already grouped
    const uint32_t* grouped = radix_sort_result_buffer(nbits) == 1 ? w.v1 : w.v0;
    PCH_LAUNCH("crop_gather", cb_gather_k, dim3((unsigned)ceil_div(cap, CB_THREADS)), dim3(CB_THREADS), 0, s, xyz,
               n, grouped, cap, (const int64_t*)out_count, out_points, out_index);
    return PCH_OK;
}
