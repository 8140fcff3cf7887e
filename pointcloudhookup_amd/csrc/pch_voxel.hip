// Stage A: per-chunk voxel-grid downsample (Open3D VoxelDownSample semantics): the rows of every
// chunk are sorted by voxel index (one MSD partition in HBM, the rest inside LDS) and reduced in
// file order, one float64 running sum per voxel.
// Reference call site: ui/import_PC.py:8-13 inside the chunk loop ui/import_PC.py:45-58.
#include "pch_prims.h"
#ifdef PCH_VX_STAMPS
#define PCH_LB_COUNT
namespace pch { __device__ unsigned long long g_lb_polls = 0, g_lb_windows = 0; }
#endif
#include "pch_lookback.h"

namespace pch {

constexpr int VX_THREADS = 256;
constexpr int VX_MM_ROUNDS = 8;

// ---- per-chunk float64 min / max (ordered-uint64 atomics) ---------------------------
// A thread takes two rows per round as three 16-byte loads (a chunk starts on a 16-byte boundary
// when chunk_size is even; odd chunk sizes and the last row use the scalar path).
__global__ __launch_bounds__(VX_THREADS) void vx_minmax_k(const double* __restrict__ xyz,
                                                          int64_t n, int64_t chunk_size,
                                                          int64_t blocks_per_chunk,
                                                          unsigned long long* __restrict__ mm) {
    __shared__ unsigned long long sm[VX_THREADS / 64][6];
    const int64_t chunk = blockIdx.x / blocks_per_chunk;
    const int64_t tile  = blockIdx.x % blocks_per_chunk;
    const int64_t cbeg = chunk * chunk_size;
    const int64_t cend = (cbeg + chunk_size < n) ? cbeg + chunk_size : n;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool nan = false;
    auto take = [&](int a, double v) {
        lo[a] = v < lo[a] ? v : lo[a];
        hi[a] = v > hi[a] ? v : hi[a];
        nan |= v != v;
    };
    const bool vec = ((cbeg & 1) == 0) && ((reinterpret_cast<uintptr_t>(xyz) & 15u) == 0);
    const int64_t t0 = cbeg + tile * (VX_THREADS * VX_MM_ROUNDS);
    if (vec) {
        double2 q[VX_MM_ROUNDS / 2][3];
#pragma unroll
        for (int r = 0; r < VX_MM_ROUNDS / 2; ++r) {
            const int64_t i = t0 + 2 * (r * VX_THREADS + threadIdx.x);        // rows i, i+1
            const bool both = i + 1 < cend;
            const double2* p = reinterpret_cast<const double2*>(xyz + 3 * (both ? i : cbeg));
            q[r][0] = p[0]; q[r][1] = p[1]; q[r][2] = p[2];
        }
#pragma unroll
        for (int r = 0; r < VX_MM_ROUNDS / 2; ++r) {
            const int64_t i = t0 + 2 * (r * VX_THREADS + threadIdx.x);
            if (i + 1 < cend) {
                take(0, q[r][0].x); take(1, q[r][0].y); take(2, q[r][1].x);
                take(0, q[r][1].y); take(1, q[r][2].x); take(2, q[r][2].y);
            } else if (i < cend) {
                take(0, xyz[3 * i + 0]); take(1, xyz[3 * i + 1]); take(2, xyz[3 * i + 2]);
            }
        }
    } else {
        for (int r = 0; r < VX_MM_ROUNDS; ++r) {
            const int64_t i = t0 + r * VX_THREADS + threadIdx.x;
            if (i < cend) { take(0, xyz[3 * i + 0]); take(1, xyz[3 * i + 1]); take(2, xyz[3 * i + 2]); }
        }
    }
    unsigned long long klo[3], khi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        // a NaN anywhere must reach the bounds kernel (it rejects the call): it is carried in the max slot
        klo[a] = wave_reduce_min(f64_ordered(lo[a]));
        khi[a] = wave_reduce_max(nan ? f64_ordered(__longlong_as_double(0x7FF8000000000000ll)) : f64_ordered(hi[a]));
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { sm[wave_id()][a] = klo[a]; sm[wave_id()][3 + a] = khi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        unsigned long long v = sm[0][a];
        for (int w = 1; w < VX_THREADS / 64; ++w) {
            const unsigned long long o = sm[w][a];
            v = (a < 3) ? (o < v ? o : v) : (o > v ? o : v);
        }
        if (a < 3) atomicMin(&mm[chunk * 6 + a], v);
        else       atomicMax(&mm[chunk * 6 + a], v);
    }
}

// one thread per chunk: grid origin, largest voxel index per axis, Open3D's range check
__global__ void vx_bounds_k(const unsigned long long* __restrict__ mm, int64_t nchunks,
                            double voxel, double* __restrict__ minb, int* __restrict__ gmeta) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    double ext = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = f64_unordered(mm[c * 6 + a]);
        const double hi = f64_unordered(mm[c * 6 + 3 + a]);
        const double mb = lo - voxel * 0.5;           // voxel_min_bound
        const double xb = hi + voxel * 0.5;           // voxel_max_bound
        minb[c * 3 + a] = mb;
        const double e = xb - mb;
        ext = e > ext ? e : ext;
        const double q = floor((hi - mb) / voxel);
        int qi = (q >= 0.0 && q < 2147483647.0) ? (int)q : 2147483647;
        if (!(q == q)) qi = 2147483647;               // NaN coordinates
        atomicMax(&gmeta[a], qi);
        if (!(fabs(lo) < INFINITY) || !(fabs(hi) < INFINITY)) atomicMax(&gmeta[3], 1);   // NaN / inf coordinates
    }
    if (voxel * 2147483647.0 < ext || !(ext == ext)) atomicMax(&gmeta[3], 1);
}

// =====================================================================================
// Sorting the rows of every chunk by voxel index WITHOUT a key/index stream and without a final
// gather (a 24-byte gather through a sorted index costs a whole cache line per point):
//
//   level 1  one stable MSD partition of each chunk by the top D1 <= 9 bits of the packed voxel
//            index [ix|iy|iz]: what moves is the row itself (three doubles).  Three launches:
//            per-tile digit histograms, a per-chunk scan, the scatter (tile-local stable ranks from
//            wave ballots, as db_chunksort_k).  Runs of a tile are ~8 rows per bin: coalesced enough.
//   finish   the (chunk, digit) units are taken in order by persistent workgroups (tickets).  A unit
//            of <= VF_CAP rows is sorted inside LDS - only (key, row) words move there, the rows stay
//            in L2 where the unit was just read - and reduced straight from there: one thread per
//            voxel adds its rows in file order (the level-1 partition and the LDS sort are stable),
//            which is Open3D's AccumulatedPoint::AddPoint order, so the means are bit-exact.
//            A larger unit (tower cores, degenerate inputs) is sorted by its workgroup with LSD passes
//            in global memory first.  The first output slot of a unit comes from a decoupled
//            look-back over the units in front of it.
// HBM traffic per point: 24 (min/max) + 24 (histogram) + 48 (scatter) + 24 (finish) + 40 per voxel.
// =====================================================================================
constexpr int VP_THREADS = 512;
constexpr int VP_WAVES   = VP_THREADS / 64;
constexpr int VP_ROUNDS  = 8;                        // rows per thread and tile
constexpr int VP_TILE    = VP_THREADS * VP_ROUNDS;   // 4096 rows
constexpr int VP_MAXBITS = 9;
constexpr int VP_MAXBINS = 1 << VP_MAXBITS;
constexpr int VF_THREADS = 512;                      // finisher workgroup (two per CU)
constexpr int VF_WAVES   = VF_THREADS / 64;
constexpr int VF_CAP     = VF_THREADS * VP_ROUNDS;   // 4096 rows: what one LDS sort takes
constexpr int VF_DIGBITS = 8;                        // a batch spans at most 256 level-1 digits
constexpr int VG_ROUNDS  = 4;                        // general (global-memory) path: rows per thread and tile

struct Row { double x, y, z; };

struct VoxelPlan {
    int64_t n, chunk_size, nchunks, tiles_per_chunk;
    double  voxel, rvoxel;   // voxel size and fl(1 / voxel)
    int     bx, by, bz;      // bits per axis
    int     T;               // bx + by + bz
    int     d1;              // level-1 digit bits
    int     nb;              // 1 << d1
    int     rem;             // T - d1: bits the finisher sorts on
};

// floor((p - voxel_min_bound) / voxel_size) exactly as IEEE float64 subtraction + DIVISION + floor give it
// (Open3D: ref_coord = (p - min_bound) / voxel_size; floor), without paying for a division per coordinate:
// q = d * fl(1/v) differs from fl(d / v) by less than q * 2^-51 (three roundings of 2^-53 each), so whenever q
// is further than q * 2^-49 from the integers on both sides, both have the same floor; otherwise (a coordinate
// on a voxel face to within rounding - common for quantised LAS data) the real division decides.
__device__ __forceinline__ uint64_t vx_index(double p, double mb, double v, double rv) {
    const double d = p - mb;                            // >= v/2: min_bound is half a voxel below the smallest point
    const double q = d * rv;
    const double fq = floor(q);
    const double fr = q - fq, tol = q * 0x1p-49;
    // indices are < 2^31 (vx_bounds_k rejects larger grids): one v_cvt_i32_f64 instead of the 64-bit conversion
    if (fr > tol && (1.0 - fr) > tol) return (uint64_t)(uint32_t)(int32_t)fq;
    return (uint64_t)(uint32_t)(int32_t)floor(d / v);
}
__device__ __forceinline__ uint64_t vx_key(const VoxelPlan& g, const double* __restrict__ mb, const Row& q) {
    const uint64_t ix = vx_index(q.x, mb[0], g.voxel, g.rvoxel);
    const uint64_t iy = vx_index(q.y, mb[1], g.voxel, g.rvoxel);
    const uint64_t iz = vx_index(q.z, mb[2], g.voxel, g.rvoxel);
    return (((ix << g.by) | iy) << g.bz) | iz;
}

// Rank of this lane's digit d among the valid lanes of its wave with the same digit, after the wave_cnt[d] rows the
// wave ranked before; the first lane of every digit then moves wave_cnt[d] past the wave's rows of that digit.
template <int BITS>
__device__ __forceinline__ uint32_t wave_rank(uint32_t* wave_cnt, uint32_t d, bool valid) {
    uint32_t peers;
    const uint32_t rk = wave_match<BITS>(d, valid, peers);
    const uint32_t prior = wave_cnt[d];
    __builtin_amdgcn_wave_barrier();
    if (valid && rk == 0) wave_cnt[d] = prior + peers;
    __builtin_amdgcn_wave_barrier();
    return prior + rk;
}

// Workgroup-wide exclusive scan of one value per thread; all THREADS threads call it, and all get the sum in `total`.
// Barriers: one BEFORE wsum is written - so a call may follow another on the same wsum, and what the callers wrote to
// LDS before the call is visible to all threads after it - and one between the write of wsum and its reads.  None
// at the end: wsum is still being read when the call returns.
template <int THREADS>
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* wsum, uint32_t& total) {
    const uint32_t incl = wave_scan_incl(v);
    __syncthreads();
    if (lane_id() == 63) wsum[wave_id()] = incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        const uint32_t s = wsum[w];
        if (w < wave_id()) before += s;
        tot += s;
    }
    total = tot;
    return before + incl - v;
}

// "Per digit: the waves in order": the per-wave counts cnt[0 .. WAVES)[d] of a ranked digit pass become the offsets
// of every wave's first row of digit d, counted on from `start`; returns where the last wave's rows end.
template <int WAVES, int BINS>
__device__ __forceinline__ uint32_t vx_wave_offsets(uint32_t (*cnt)[BINS], uint32_t d, uint32_t start) {
    uint32_t run = start;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t cc = cnt[w][d];
        cnt[w][d] = run;
        run += cc;
    }
    return run;
}

// ---- level 1: one workgroup per tile of VP_TILE rows of a chunk -------------------------------------
struct VxTile { int64_t c, cbeg, cend, t0; };      // chunk, its rows [cbeg, cend), the tile's first row
__device__ __forceinline__ VxTile vx_tile(const VoxelPlan& g) {
    const int64_t c = blockIdx.x / g.tiles_per_chunk, t = blockIdx.x % g.tiles_per_chunk, cbeg = c * g.chunk_size;
    return {c, cbeg, (cbeg + g.chunk_size < g.n) ? cbeg + g.chunk_size : g.n, cbeg + t * VP_TILE};
}
// the chunk's grid origin and VP_ROUNDS rows per thread: row i0 + r * STRIDE + j in round r (rows past the chunk read
// its first)
template <int STRIDE>
__device__ __forceinline__ void vx_tile_load(const double* __restrict__ xyz, const double* __restrict__ minb,
                                             const VxTile& k, int64_t i0, int j, double (&mb)[3], Row (&q)[VP_ROUNDS]) {
    mb[0] = minb[3 * k.c + 0]; mb[1] = minb[3 * k.c + 1]; mb[2] = minb[3 * k.c + 2];
    const Row* __restrict__ rows = reinterpret_cast<const Row*>(xyz);
#pragma unroll
    for (int r = 0; r < VP_ROUNDS; ++r) {
        const int64_t i = i0 + r * STRIDE + j;
        q[r] = rows[i < k.cend ? i : k.cbeg];
    }
}

// ---- level 1a: digit histogram of every tile ------------------------------------------------
__global__ __launch_bounds__(VP_THREADS) void vx_tilehist_k(const double* __restrict__ xyz, VoxelPlan g,
                                                            const double* __restrict__ minb,
                                                            uint32_t* __restrict__ tile_hist) {
    __shared__ uint32_t hist[VP_MAXBINS];
    const VxTile k = vx_tile(g);
    for (int j = threadIdx.x; j < g.nb; j += VP_THREADS) hist[j] = 0;
    __syncthreads();
    double mb[3];
    Row q[VP_ROUNDS];
    vx_tile_load<VP_THREADS>(xyz, minb, k, k.t0, threadIdx.x, mb, q);
#pragma unroll
    for (int r = 0; r < VP_ROUNDS; ++r) {
        const int64_t i = k.t0 + r * VP_THREADS + threadIdx.x;
        if (i < k.cend) atomicAdd(&hist[(uint32_t)(vx_key(g, mb, q[r]) >> g.rem)], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < g.nb; j += VP_THREADS) tile_hist[(int64_t)blockIdx.x * g.nb + j] = hist[j];
}

// ---- level 1b: one workgroup per chunk: tile_hist -> exclusive offsets inside every bin, bin starts;
// consecutive units are then grouped into BATCHES of at most VF_CAP rows (one LDS sort each); a unit
// that is larger on its own is a batch of one (sorted in global memory by its workgroup)
struct alignas(8) VoxelBatch {  // 24 bytes: the workspace is carved in these
    uint32_t row0;        // first row (absolute, in the partitioned buffer) of the units this batch reads
    uint32_t rows;        // rows this batch sorts (0: nothing to do)
    uint32_t span;        // == rows; for the reserved slots of an oversize unit (before vx_split_k): the unit's rows
    uint16_t digit0;      // first level-1 digit of the batch
    uint16_t ndigits;     // level-1 digits covered (>= 1)
    uint32_t from_b;      // 1: the batch's rows lie in the second row buffer (a part of an oversize unit, vx_split_k)
};
static_assert(sizeof(VoxelBatch) == 24, "pch_voxel_downsample_ws_bytes depends on it");
struct VoxelOversize { uint32_t slot, nsub; };             // a unit above VF_CAP rows and its reserved batch slots

__global__ __launch_bounds__(VP_MAXBINS) void vx_binscan_k(VoxelPlan g, uint32_t* __restrict__ tile_hist,
                                                           uint32_t* __restrict__ unit_start,
                                                           VoxelBatch* __restrict__ batches,
                                                           uint32_t* __restrict__ nbatch,
                                                           VoxelOversize* __restrict__ over,
                                                           uint32_t* __restrict__ nover) {
    __shared__ uint32_t wsum[VP_MAXBINS / 64];
    __shared__ __attribute__((aligned(16))) uint32_t ucount[VP_MAXBINS];
    __shared__ uint32_t ustart[VP_MAXBINS];
    const int64_t c = blockIdx.x;
    const int b = threadIdx.x;
    uint32_t run = 0;
    if (b < g.nb) {
        constexpr int U = 32;                              // loads of 32 tiles in flight (a chunk of 500 000 rows has 123:
                                                           // four round trips instead of sixteen - the kernel is one
                                                           // workgroup per chunk and nothing but these round trips)
        for (int64_t t0 = 0; t0 < g.tiles_per_chunk; t0 += U) {
            uint32_t h[U];
#pragma unroll
            for (int k = 0; k < U; ++k)
                h[k] = t0 + k < g.tiles_per_chunk ? tile_hist[(c * g.tiles_per_chunk + t0 + k) * g.nb + b] : 0u;
#pragma unroll
            for (int k = 0; k < U; ++k) {
                if (t0 + k < g.tiles_per_chunk) tile_hist[(c * g.tiles_per_chunk + t0 + k) * g.nb + b] = run;
                run += h[k];
            }
        }
    }
    uint32_t chunk_rows;
    const uint32_t base = block_scan_excl<VP_MAXBINS>(run, wsum, chunk_rows);
    if (b < g.nb) {
        const uint32_t st = (uint32_t)(c * g.chunk_size) + base;
        unit_start[c * g.nb + b] = st;
        ucount[b] = run;
        ustart[b] = st;
    } else {
        ucount[b] = 0;                                     // (the grouping below reads the counts four at a time)
    }
    const uint32_t nonempty = (uint32_t)__syncthreads_count(b < g.nb && run != 0);
    if (b == 0) {                                          // greedy grouping, in digit order
        VoxelBatch* out = batches + c * VP_MAXBINS;
        uint32_t nbt = 0, rows = 0, first = 0;
        const uint32_t maxdig = (g.rem >= 32) ? 1u : (g.rem + VF_DIGBITS > 32 ? (1u << (32 - g.rem)) : (1u << VF_DIGBITS));
        auto emit = [&](uint32_t r0, uint32_t nrows, uint32_t d0, uint32_t nd) {
            VoxelBatch v;
            v.row0 = r0; v.rows = nrows; v.span = nrows; v.digit0 = (uint16_t)d0; v.ndigits = (uint16_t)nd;
            v.from_b = 0;
            out[nbt++] = v;
        };
        // a batch covers the digits [first, last] of its first and last NON-EMPTY unit (empty units in between
        // cost nothing but would widen the sort key)
        uint32_t last = 0, seen = 0;
        // (one thread, in digit order: the counts come four per LDS read - one dependent read per digit was most of
        // this kernel's 70 us, which every call waits for whatever its size)
        for (uint32_t d4 = 0; d4 < (uint32_t)g.nb; d4 += 4) {
          const uint4 c4 = *reinterpret_cast<const uint4*>(&ucount[d4]);
          const uint32_t cq[4] = {c4.x, c4.y, c4.z, c4.w};
          if ((c4.x | c4.y | c4.z | c4.w) == 0u) continue;
#pragma unroll
          for (uint32_t dd = 0; dd < 4; ++dd) {
            const uint32_t d = d4 + dd;
            const uint32_t cnt = cq[dd];
            if (cnt == 0) continue;
            ++seen;
            if (rows && (rows + cnt > (uint32_t)VF_CAP || d - first >= maxdig)) {   // close the open batch
                emit(ustart[first], rows, first, last - first + 1);
                rows = 0;
            }
            if (rows == 0) first = d;
            rows += cnt;
            last = d;
            if (rows > (uint32_t)VF_CAP) {                 // a single unit above VF_CAP (rows == cnt here)
                // split by its next digit into <= 2*ceil(rows/CAP)+1 parts (filled in by vx_split_k), unless
                // batch slots or the 16-bit position field run out: then one batch, sorted in global memory
                const uint32_t nsub = 2 * ((rows + VF_CAP - 1) / VF_CAP) + 1;
                const uint32_t left = nonempty - seen;                    // units still to come need <= 1 slot each
                if (g.rem > 0 && g.rem <= 32 && nbt + nsub + left <= (uint32_t)VP_MAXBINS) {
                    const uint32_t o = atomicAdd(nover, 1u);
                    over[o].slot = (uint32_t)(c * VP_MAXBINS) + nbt;
                    over[o].nsub = nsub;
                    for (uint32_t k = 0; k < nsub; ++k) {
                        emit(ustart[d], 0, d, 1);
                        out[nbt - 1].span = rows;
                    }
                } else {
                    emit(ustart[d], rows, d, 1);
                }
                rows = 0;
            }
          }
        }
        if (rows) emit(ustart[first], rows, first, last - first + 1);
        nbatch[c] = nbt;
    }
}

// one workgroup per oversize unit (a tower core: thousands of rows in one level-1 cell): a SECOND partition, by the
// unit's next 8-bit digit, into the second row buffer (stable: histogram, then ranked scatter tile by tile); the parts of
// <= VF_CAP rows that come out of it are contiguous there and are finished like any other batch.  (Until round 4 every
// part swept the whole unit twice and picked its rows: 12 sweeps of a 20 000-row unit that was cut into six.)
constexpr int VS_THREADS = 1024, VS_WAVES = VS_THREADS / 64, VS_ROUNDS = 4, VS_TILE = VS_THREADS * VS_ROUNDS;

// Stable scatter of the R rows src[0, R) of a chunk (grid origin mb) to dst by the digit ((key & remmask) >> shift) & 255,
// given base[d] = where digit d's rows start in dst: tile by tile, the rows of every wave are ranked per digit, the
// waves are taken in order and their rows carried into base.
template <int THREADS, int ROUNDS>
__device__ __forceinline__ void vx_ranked_scatter(const VoxelPlan& g, const double (&mb)[3], uint64_t remmask, int shift,
                                                  const Row* __restrict__ src, Row* __restrict__ dst, uint32_t R,
                                                  uint32_t* base, uint32_t (*cnt)[256]) {
    constexpr int WAVES = THREADS / 64, TILE = THREADS * ROUNDS;
    static_assert(THREADS >= 256, "one thread per digit");
    const int tid = threadIdx.x, w = wave_id(), l = lane_id();
    for (uint32_t t0 = 0; t0 < R; t0 += TILE) {
        for (int j = tid; j < WAVES * 256; j += THREADS) (&cnt[0][0])[j] = 0;
        __syncthreads();
        const uint32_t segb = t0 + w * (64 * ROUNDS);     // wave w owns 64 * ROUNDS consecutive rows of the tile
        Row q[ROUNDS];
        uint32_t dig[ROUNDS], rank[ROUNDS];
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const uint32_t i = segb + r * 64 + l;
            q[r] = src[i < R ? i : 0];
        }
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            dig[r] = (uint32_t)((vx_key(g, mb, q[r]) & remmask) >> shift) & 255u;
            rank[r] = wave_rank<8>(cnt[w], dig[r], segb + r * 64 + l < R);
        }
        __syncthreads();
        if (tid < 256) base[tid] = vx_wave_offsets<WAVES>(cnt, tid, base[tid]);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r)
            if (segb + r * 64 + l < R) dst[cnt[w][dig[r]] + rank[r]] = q[r];
        __syncthreads();
    }
}

__global__ __launch_bounds__(VS_THREADS, 8) void vx_split_k(VoxelPlan g, const double* __restrict__ minb,
                                                       const Row* __restrict__ rows, Row* __restrict__ rows_b,
                                                       VoxelBatch* __restrict__ batches,
                                                       const VoxelOversize* __restrict__ over,
                                                       const uint32_t* __restrict__ nover) {
    __shared__ uint32_t hist[256], base[256];
    __shared__ uint32_t cnt[VS_WAVES][256];
    __shared__ uint32_t wsum[VS_WAVES];
    __shared__ uint32_t okflag;
    const uint32_t total = *nover;
    const int tid = threadIdx.x;
    for (uint32_t o = blockIdx.x; o < total; o += gridDim.x) {
        const VoxelOversize ov = over[o];
        VoxelBatch* bt = batches + ov.slot;
        const uint32_t s = bt[0].row0, R = bt[0].span;
        const int64_t c = ov.slot / VP_MAXBINS;
        const double mb[3] = {minb[3 * c + 0], minb[3 * c + 1], minb[3 * c + 2]};
        const int sh2 = g.rem > 8 ? g.rem - 8 : 0;
        const uint64_t remmask = (1ull << g.rem) - 1;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (uint32_t i0 = 0; i0 < R; i0 += VS_TILE) {
            Row q[VS_ROUNDS];
#pragma unroll
            for (int k = 0; k < VS_ROUNDS; ++k) {
                const uint32_t i = i0 + k * VS_THREADS + tid;
                q[k] = rows[s + (i < R ? i : 0)];
            }
#pragma unroll
            for (int k = 0; k < VS_ROUNDS; ++k)
                if (i0 + k * VS_THREADS + tid < R)
                    atomicAdd(&hist[(uint32_t)((vx_key(g, mb, q[k]) & remmask) >> sh2) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t k = 0, acc = 0, first = 0, run = 0;
            bool ok = true;
            for (uint32_t d = 0; d < 256 && ok; ++d) {
                const uint32_t h = hist[d];
                if (h > (uint32_t)VF_CAP) { ok = false; break; }
                if (acc + h > (uint32_t)VF_CAP) {
                    bt[k].row0 = s + first; bt[k].rows = acc; bt[k].span = acc; bt[k].from_b = 1u; ++k;
                    first = run; acc = 0;
                }
                acc += h;
                run += h;
            }
            if (ok) {
                if (acc) { bt[k].row0 = s + first; bt[k].rows = acc; bt[k].span = acc; bt[k].from_b = 1u; ++k; }
                for (uint32_t j = k; j < ov.nsub; ++j) { bt[j].rows = 0; bt[j].span = 0; }
            } else {                                       // one voxel column alone exceeds the LDS capacity:
                for (uint32_t j = 0; j < ov.nsub; ++j) { bt[j].rows = 0; bt[j].from_b = 0; }
                bt[0].rows = R;                            // the whole unit as one batch, sorted in global memory
            }
            okflag = ok ? 1u : 0u;
        }
        __syncthreads();
        if (okflag) {                                      // workgroup-uniform
            // exclusive scan of the digit histogram -> where every digit's rows start in the second buffer
            uint32_t unit_rows;
            const uint32_t ex = block_scan_excl<VS_THREADS>(tid < 256 ? hist[tid] : 0u, wsum, unit_rows);
            if (tid < 256) base[tid] = s + ex;
            __syncthreads();
            vx_ranked_scatter<VS_THREADS, VS_ROUNDS>(g, mb, remmask, sh2, rows + s, rows_b, R, base, cnt);
        }
        __syncthreads();
    }
}

// exclusive scan of the per-chunk batch counts (one workgroup); prefix[nchunks] = total
__global__ __launch_bounds__(1024) void vx_batchscan_k(const uint32_t* __restrict__ nbatch, int64_t nchunks,
                                                       uint32_t* __restrict__ prefix) {
    __shared__ uint32_t wsum[16];
    uint32_t carry = 0;                                    // batches of the chunks in front (every thread keeps it)
    for (int64_t base = 0; base < nchunks; base += 1024) {
        const int64_t i = base + threadIdx.x;
        uint32_t tot;
        const uint32_t ex = block_scan_excl<1024>(i < nchunks ? nbatch[i] : 0u, wsum, tot);
        if (i < nchunks) prefix[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) prefix[nchunks] = carry;
}

// ---- level 1c: stable scatter of the rows into their (chunk, digit) units -----------------------
// What both forms of the scatter start with.  cnt is cleared, base[d] becomes where the tile's run of digit d starts
// in HBM; wave w owns rows [w*512, w*512+512) of the tile, 64 per round ((wave, round, lane) order = file order):
// it loads them and ranks them per digit inside the wave (cnt[w][d]: the wave's rows of digit d).  Ends with a
// barrier.  False (for the whole workgroup, before any barrier): the tile lies past the chunk's rows.
struct VxScatterRows {
    VxTile   k;
    int64_t  seg;                                 // the wave's first row
    Row      q[VP_ROUNDS];
    uint32_t dig[VP_ROUNDS], rank[VP_ROUNDS];
    __device__ __forceinline__ bool valid(int r) const { return seg + r * 64 + lane_id() < k.cend; }
};
__device__ __forceinline__ bool vx_scatter_prologue(const double* __restrict__ xyz, const VoxelPlan& g,
                                                    const double* __restrict__ minb, const uint32_t* __restrict__ tile_hist,
                                                    const uint32_t* __restrict__ unit_start, uint32_t (*cnt)[VP_MAXBINS],
                                                    uint32_t* base, VxScatterRows& t) {
    t.k = vx_tile(g);
    if (t.k.t0 >= t.k.cend) return false;
    const int w = wave_id();
    for (int j = threadIdx.x; j < VP_WAVES * g.nb; j += VP_THREADS) cnt[j / g.nb][j % g.nb] = 0;
    for (int j = threadIdx.x; j < g.nb; j += VP_THREADS)
        base[j] = unit_start[t.k.c * g.nb + j] + tile_hist[(int64_t)blockIdx.x * g.nb + j];
    __syncthreads();
    t.seg = t.k.t0 + (int64_t)w * (64 * VP_ROUNDS);
    double mb[3];
    vx_tile_load<64>(xyz, minb, t.k, t.seg, lane_id(), mb, t.q);
#pragma unroll
    for (int r = 0; r < VP_ROUNDS; ++r) {
        t.dig[r] = (uint32_t)(vx_key(g, mb, t.q[r]) >> g.rem);
        t.rank[r] = wave_rank<VP_MAXBITS>(cnt[w], t.dig[r], t.valid(r));
    }
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(VP_THREADS) void vx_scatter_k(const double* __restrict__ xyz, VoxelPlan g,
                                                           const double* __restrict__ minb,
                                                           const uint32_t* __restrict__ tile_hist,
                                                           const uint32_t* __restrict__ unit_start,
                                                           Row* __restrict__ out) {
    __shared__ uint32_t cnt[VP_WAVES][VP_MAXBINS];
    __shared__ uint32_t base[VP_MAXBINS];
    VxScatterRows t;
    if (!vx_scatter_prologue(xyz, g, minb, tile_hist, unit_start, cnt, base, t)) return;
    for (int d = threadIdx.x; d < g.nb; d += VP_THREADS) vx_wave_offsets<VP_WAVES>(cnt, d, base[d]);
    __syncthreads();
    const int w = wave_id();
#pragma unroll
    for (int r = 0; r < VP_ROUNDS; ++r)
        if (t.valid(r)) out[cnt[w][t.dig[r]] + t.rank[r]] = t.q[r];
}

// The same scatter with the tile staged through LDS: the rows of a tile are first put in digit order INSIDE the tile
// (LDS), then copied out - a (tile, digit) run of ~8 rows (192 bytes) leaves in one store instruction of adjacent lanes
// instead of reaching the L2 as eight 24-byte stores of eight waves at eight different times.
struct VsShared {
    Row      rows[VP_TILE];                       // 96 KB
    uint16_t dig[VP_TILE];                        // 8 KB: digit of the row at that LDS position
    uint32_t cnt[VP_WAVES][VP_MAXBINS];           // 16 KB
    uint32_t gbase[VP_MAXBINS];                   // where the tile's run of a digit starts in HBM
    uint32_t lstart[VP_MAXBINS];                  // ... and inside the tile
    uint32_t wsum[VP_WAVES];
};
__global__ __launch_bounds__(VP_THREADS) void vx_scatter_lds_k(const double* __restrict__ xyz, VoxelPlan g,
                                                               const double* __restrict__ minb,
                                                               const uint32_t* __restrict__ tile_hist,
                                                               const uint32_t* __restrict__ unit_start,
                                                               Row* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vs_raw[];
    VsShared& sh = *reinterpret_cast<VsShared*>(vs_raw);
    VxScatterRows t;
    if (!vx_scatter_prologue(xyz, g, minb, tile_hist, unit_start, sh.cnt, sh.gbase, t)) return;
    const uint32_t tn = (uint32_t)((t.k.cend - t.k.t0) < VP_TILE ? (t.k.cend - t.k.t0) : VP_TILE);
    const int tid = threadIdx.x, w = wave_id();
    // per digit (one thread each, g.nb <= VP_THREADS): the waves in order -> offsets inside the digit's run; the runs
    // in digit order -> where each starts inside the tile
    const uint32_t tot = tid < g.nb ? vx_wave_offsets<VP_WAVES>(sh.cnt, tid, 0u) : 0u;
    uint32_t tile_rows;
    const uint32_t ex = block_scan_excl<VP_THREADS>(tot, sh.wsum, tile_rows);
    if (tid < g.nb) sh.lstart[tid] = ex;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < VP_ROUNDS; ++r)
        if (t.valid(r)) {
            const uint32_t at = sh.lstart[t.dig[r]] + sh.cnt[w][t.dig[r]] + t.rank[r];
            sh.rows[at] = t.q[r];
            sh.dig[at] = (uint16_t)t.dig[r];
        }
    __syncthreads();
    for (uint32_t j = tid; j < tn; j += VP_THREADS) {
        const uint32_t d = sh.dig[j];
        out[sh.gbase[d] + (j - sh.lstart[d])] = sh.rows[j];
    }
}

// ---- finish ------------------------------------------------------------------------------------
// One batch per workgroup iteration.  LDS sort: what is sorted is a 32-bit key
//   ((level-1 digit - first digit of the batch) << rem) | (low `rem` bits of the voxel key)
// together with the row's position in the batch (uint16); the rows themselves stay in L2.
constexpr uint32_t VQ_SLOTS = 2 * VF_CAP;            // hash-set slots of a batch (load factor <= 1/2)
constexpr uint32_t VQ_MAXRUN = 32;                   // rows per voxel the grouping path takes (else: the stable sort)
constexpr uint32_t VQ_NONE = 0xFFFFFFFFu;            // empty hash slot / no row in this round
struct VfShared {
    union {
        struct {
            uint32_t key[2][VF_CAP];             // 32 KB
            uint16_t perm[2][VF_CAP];            // 16 KB
        };
        struct {                                 // grouping path (vf_group): hash set, per-slot row counts (one BYTE
            uint32_t hset[VQ_SLOTS];             // per slot, four to a word), first position of every slot's rows,
            uint32_t hcnt[VQ_SLOTS / 4];         // the rows' positions grouped by slot, and one bit per position that
            uint16_t sstart[VQ_SLOTS];           // is the first row of its voxel
            uint16_t pos[VF_CAP];
            unsigned long long headbits[VF_CAP / 64];
            uint32_t headpre[VF_CAP / 64];
        } q;
        uint32_t hist[8][256];                   // general path: digit histograms of every LSD pass
    };
    uint32_t cnt[VF_WAVES][256];                 // per-wave digit counters / offsets (16 KB)
    uint32_t base[256];
    uint32_t wsum[VF_WAVES];
    uint32_t ticket, vbase, lb_failed, overflow;
};

// The batch a workgroup is working on (vf_take_batch).
struct VfBatch {
    uint32_t   t;                 // its ticket = its place in the look-back chain
    int64_t    c;                 // chunk
    VoxelBatch bt;
    bool       first_of_chunk;
    const Row* src;               // where its rows are: src[0, bt.rows)
    double     mb[3];             // the chunk's grid origin
    uint64_t   d0;                // first level-1 digit
    uint64_t   remmask;           // the low g.rem key bits
    int        sortbits;          // bits of the relative key: g.rem + bits of the digit span
};
// How a batch is put in voxel order; decided once per batch in vx_finish_k.
enum VfPath {
    VF_EMPTY,                     // a reserved slot that was not needed: publishes zero voxels
    VF_GROUPED,                   // rows grouped by hash slot (vf_group), reduced by vf_reduce_grouped
    VF_SORT_LDS,                  // stable LSD passes over (key, position) in LDS (vf_sort_lds)
    VF_SORT_GLOBAL                // LSD passes over the rows in global memory (vf_sort_global)
};
// What a sort leaves for vf_reduce_runs: voxel v is the items [vst[v], vst[v + 1]) of the sorted batch.
struct VfRuns {
    uint32_t        nvox = 0;
    const uint32_t* vst = nullptr;
    const uint32_t* skey = nullptr;   // LDS sort: relative keys and batch positions of the sorted items
    const uint16_t* sperm = nullptr;
    const Row*      rows = nullptr;   // global sort: the sorted rows
};
struct VfOut { int32_t* __restrict__ idx; double* __restrict__ mean; int32_t* __restrict__ count; };

__device__ __forceinline__ void vf_emit(const VoxelPlan& g, uint64_t key, double ax, double ay, double az,
                                        uint32_t count, int64_t slot, const VfOut& out) {
    const double cnt = (double)count;
    out.mean[3 * slot + 0] = ax / cnt;                  // GetAveragePoint
    out.mean[3 * slot + 1] = ay / cnt;
    out.mean[3 * slot + 2] = az / cnt;
    out.count[slot] = (int32_t)count;
    out.idx[3 * slot + 2] = (int32_t)(key & ((1ull << g.bz) - 1));
    out.idx[3 * slot + 1] = (int32_t)((key >> g.bz) & ((1ull << g.by) - 1));
    out.idx[3 * slot + 0] = (int32_t)((key >> (g.bz + g.by)) & ((1ull << g.bx) - 1));
}
// the voxel key of a relative 32-bit key
__device__ __forceinline__ uint64_t vf_abs_key(const VoxelPlan& g, const VfBatch& b, uint64_t sk) {
    return ((b.d0 + (sk >> g.rem)) << g.rem) | (sk & b.remmask);
}

// tuning builds only (-DPCH_VX_STAMPS): where one workgroup's time goes, phase by phase
#ifdef PCH_VX_STAMPS
struct VfClock {
    unsigned long long acc[12] = {}, t_last = wall_clock64();
    __device__ __forceinline__ void stamp(int k) {
        __syncthreads();
        if (threadIdx.x == 0) { const unsigned long long t = wall_clock64(); acc[k] += t - t_last; t_last = t; }
    }
};
#define VX_STAMP(k) ck.stamp(k)
#else
struct VfClock {};
#define VX_STAMP(k)
#endif

// The next batch in ticket order (the look-back in vf_publish follows the tickets); false: none is left.
__device__ __forceinline__ bool vf_take_batch(VfShared& sh, const VoxelPlan& g, const double* __restrict__ minb,
                                              const VoxelBatch* __restrict__ batches, const uint32_t* __restrict__ batch_prefix,
                                              uint32_t nbatches, const Row* bufA, const Row* bufB,
                                              uint32_t* __restrict__ ticket, VfBatch& b) {
    __syncthreads();                                   // previous batch's LDS reads are done
    if (threadIdx.x == 0) sh.ticket = atomicAdd(ticket, 1u);
    __syncthreads();
    b.t = sh.ticket;
    if (b.t >= nbatches) return false;
    // chunk of batch t: last c with batch_prefix[c] <= t
    int64_t lo = 0, hi = g.nchunks - 1;
    while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (batch_prefix[mid] <= b.t) lo = mid; else hi = mid - 1; }
    b.c = lo;
    b.bt = batches[b.c * VP_MAXBINS + (b.t - batch_prefix[b.c])];
    b.first_of_chunk = b.t == batch_prefix[b.c];
    b.src = (b.bt.from_b ? bufB : bufA) + b.bt.row0;
    b.d0 = b.bt.digit0; b.remmask = (1ull << g.rem) - 1;        // rem <= 54
    b.mb[0] = minb[3 * b.c + 0]; b.mb[1] = minb[3 * b.c + 1]; b.mb[2] = minb[3 * b.c + 2];
    int dbits = 0;
    while ((1u << dbits) < (uint32_t)b.bt.ndigits) ++dbits;
    b.sortbits = g.rem + dbits;
    return true;
}

// A batch that fits in LDS with keys of <= 32 bits: the relative key of row r * VF_THREADS + tid goes to kreg[r]
__device__ __forceinline__ void vf_load_keys(const VoxelPlan& g, const VfBatch& b, uint32_t (&kreg)[VP_ROUNDS]) {
    const uint32_t R = b.bt.rows;
#pragma unroll
    for (int h = 0; h < 2; ++h) {                       // four rows per thread in flight
        Row q[VP_ROUNDS / 2];
#pragma unroll
        for (int r = 0; r < VP_ROUNDS / 2; ++r) {
            const uint32_t i = (h * (VP_ROUNDS / 2) + r) * VF_THREADS + threadIdx.x;
            q[r] = b.src[i < R ? i : 0];
        }
#pragma unroll
        for (int r = 0; r < VP_ROUNDS / 2; ++r) {
            const uint64_t k = vx_key(g, b.mb, q[r]);
            kreg[h * (VP_ROUNDS / 2) + r] = (uint32_t)((((k >> g.rem) - b.d0) << g.rem) | (k & b.remmask));
        }
    }
}

// ---------------- grouping path: rows grouped by HASH SLOT, not sorted by key ----------------
// The exact hash set that counts the batch's voxels already says which rows belong together; what Open3D's
// accumulation needs on top is the FILE ORDER inside a voxel, not an order between voxels (its own output
// order is unordered_map iteration order).  So: every row takes a ticket on its slot's counter (arrival
// order, arbitrary), the slots' counts are scanned, the rows' positions are scattered to their slot's run, and
// the thread of the row that arrived FIRST sorts that run (1-3 positions as a rule) and adds the rows in
// ascending position = file order.  Voxels leave the batch in the order of their first rows (a bit per
// position + prefix popcounts): deterministic, whatever the arrival order was.  One pass over the rows for
// the keys, no radix pass at all (the stable LDS sort costs 3-4 passes of a ballot per key bit).
//
// vf_count_voxels: the hash set and the tickets (hs[r]: slot | arrival ticket << 16, VQ_NONE past the batch).  Returns
// the batch's voxel count and announces it to the batches behind - before any sort: the batch's own prefix is only
// fetched in vf_publish.  sh.overflow: some voxel holds more than VQ_MAXRUN rows.
__device__ __forceinline__ uint32_t vf_count_voxels(VfShared& sh, const VfBatch& b, const uint32_t (&kreg)[VP_ROUNDS],
                                                    uint32_t (&hs)[VP_ROUNDS], uint64_t* __restrict__ status, VfClock& ck) {
    const int tid = threadIdx.x;
    for (uint32_t j = tid; j < VQ_SLOTS; j += VF_THREADS) sh.q.hset[j] = VQ_NONE;
    for (uint32_t j = tid; j < VQ_SLOTS / 4; j += VF_THREADS) sh.q.hcnt[j] = 0u;
    if (tid == 0) sh.overflow = 0u;
    __syncthreads();
    uint32_t fresh = 0;
#pragma unroll
    for (int rr = 0; rr < VP_ROUNDS; ++rr) {
        const uint32_t i = rr * VF_THREADS + tid;
        hs[rr] = VQ_NONE;
        if (i < b.bt.rows) {
            uint32_t slot = (kreg[rr] * 2654435761u) >> (32 - 13);
            for (;;) {
                const uint32_t old = atomicCAS(&sh.q.hset[slot], VQ_NONE, kreg[rr]);
                if (old == VQ_NONE) { ++fresh; break; }
                if (old == kreg[rr]) break;
                slot = (slot + 1) & (VQ_SLOTS - 1);
            }
            const uint32_t sft = (slot & 3u) * 8u;
            const uint32_t tk = (atomicAdd(&sh.q.hcnt[slot >> 2], 1u << sft) >> sft) & 255u;
            if (tk >= VQ_MAXRUN) sh.overflow = 1u;
            hs[rr] = slot | (tk << 16);
        }
    }
    VX_STAMP(8);
    uint32_t nvox;
    block_scan_excl<VF_THREADS>(fresh, sh.wsum, nvox);     // (its barriers also publish the counters and the flag)
    if (tid == 0) gf_announce(status, (int64_t)b.t, nvox);
    return nvox;
}

// the slot of the voxel this thread reduces in round r (its row arrived first there), or VQ_NONE
__device__ __forceinline__ uint32_t vf_owned_slot(uint32_t hs) {
    return (hs != VQ_NONE && (hs >> 16) == 0u) ? (hs & 0xFFFFu) : VQ_NONE;
}
__device__ __forceinline__ uint32_t vf_slot_rows(const VfShared& sh, uint32_t slot) {
    return (sh.q.hcnt[slot >> 2] >> (8 * (slot & 3u))) & 255u;
}

// vf_group: every slot's rows side by side in sh.q.pos, in file order, and the voxels numbered by their first rows
__device__ __forceinline__ void vf_group(VfShared& sh, const uint32_t (&hs)[VP_ROUNDS], VfClock& ck) {
    const int tid = threadIdx.x, w = wave_id(), l = lane_id();
    // ---- exclusive scan of the slots' counts: 16 slots (16 count bytes) per thread
    {
        const uint4 c4 = reinterpret_cast<const uint4*>(sh.q.hcnt)[tid];
        const uint32_t cw[4] = {c4.x, c4.y, c4.z, c4.w};
        uint32_t pre[16], run = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) { pre[j] = run; run += (cw[j >> 2] >> (8 * (j & 3))) & 255u; }
        uint32_t tot;
        const uint32_t ex = block_scan_excl<VF_THREADS>(run, sh.wsum, tot);
        uint4 o0, o1;
        o0.x = (ex + pre[0]) | ((ex + pre[1]) << 16);   o0.y = (ex + pre[2]) | ((ex + pre[3]) << 16);
        o0.z = (ex + pre[4]) | ((ex + pre[5]) << 16);   o0.w = (ex + pre[6]) | ((ex + pre[7]) << 16);
        o1.x = (ex + pre[8]) | ((ex + pre[9]) << 16);   o1.y = (ex + pre[10]) | ((ex + pre[11]) << 16);
        o1.z = (ex + pre[12]) | ((ex + pre[13]) << 16); o1.w = (ex + pre[14]) | ((ex + pre[15]) << 16);
        reinterpret_cast<uint4*>(sh.q.sstart)[2 * tid] = o0;
        reinterpret_cast<uint4*>(sh.q.sstart)[2 * tid + 1] = o1;
    }
    __syncthreads();
    VX_STAMP(9);
    // ---- positions to their slot's run (arrival order)
#pragma unroll
    for (int r = 0; r < VP_ROUNDS; ++r)
        if (hs[r] != VQ_NONE)
            sh.q.pos[sh.q.sstart[hs[r] & 0xFFFFu] + (hs[r] >> 16)] = (uint16_t)(r * VF_THREADS + tid);
    __syncthreads();
    VX_STAMP(10);
    // ---- every run in ascending position (insertion sort by the thread that owns the voxel)
#pragma unroll
    for (int r = 0; r < VP_ROUNDS; ++r) {
        const uint32_t slot = vf_owned_slot(hs[r]);
        if (slot != VQ_NONE) {
            const uint32_t a0 = sh.q.sstart[slot];
            const uint32_t cn = vf_slot_rows(sh, slot);
            for (uint32_t a = 1; a < cn; ++a) {
                const uint16_t v = sh.q.pos[a0 + a];
                uint32_t b = a;
                while (b > 0 && sh.q.pos[a0 + b - 1] > v) { sh.q.pos[a0 + b] = sh.q.pos[a0 + b - 1]; --b; }
                sh.q.pos[a0 + b] = v;
            }
        }
    }
    __syncthreads();
    // ---- one bit per position: is this row the first of its voxel?  Position r * 512 + tid sits in word
    // r * 8 + wave: a ballot per round, no atomics (64 lanes of a wave would hit one word)
#pragma unroll
    for (int r = 0; r < VP_ROUNDS; ++r) {
        const bool head = hs[r] != VQ_NONE && sh.q.pos[sh.q.sstart[hs[r] & 0xFFFFu]] == (uint16_t)(r * VF_THREADS + tid);
        const unsigned long long m = __ballot(head);
        if (l == 0) sh.q.headbits[r * VF_WAVES + w] = m;
    }
    static_assert(VF_THREADS == 64 * VF_WAVES && VF_CAP == VP_ROUNDS * VF_THREADS, "position -> word");
    __syncthreads();
    if (tid < 64) {                                         // voxels in front of every 64-position word
        const uint32_t c = tid < (int)(VF_CAP / 64) ? (uint32_t)__popcll(sh.q.headbits[tid]) : 0u;
        const uint32_t incl = wave_scan_incl(c);
        if (tid < (int)(VF_CAP / 64)) sh.q.headpre[tid] = incl - c;
    }
    static_assert(VF_CAP / 64 <= 64, "one wave scans the head words");
}

// The thread whose row arrived first on a slot reduces that voxel (slot and key are still in its registers).
// The first rows of all (up to eight) voxels of a thread are requested together; further rows of a voxel
// follow one after the other (file order), which few voxels need.
__device__ __forceinline__ void vf_reduce_grouped(const VfShared& sh, const VoxelPlan& g, const VfBatch& b,
                                                  const uint32_t (&kreg)[VP_ROUNDS], const uint32_t (&hs)[VP_ROUNDS],
                                                  int64_t vbase, const VfOut& out) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {                           // four voxels' first rows in flight per thread
        constexpr int HV = VP_ROUNDS / 2;
        uint32_t a0[HV], cn[HV], p0[HV];
        Row q0[HV];
#pragma unroll
        for (int j = 0; j < HV; ++j) {
            const uint32_t own = vf_owned_slot(hs[h * HV + j]);
            const uint32_t slot = own != VQ_NONE ? own : 0u;
            a0[j] = sh.q.sstart[slot];
            cn[j] = own != VQ_NONE ? vf_slot_rows(sh, slot) : 0u;
            p0[j] = own != VQ_NONE ? sh.q.pos[a0[j]] : 0u;
        }
#pragma unroll
        for (int j = 0; j < HV; ++j) q0[j] = b.src[p0[j]];
#pragma unroll
        for (int j = 0; j < HV; ++j) {
            if (cn[j] != 0u) {
                double ax = 0.0 + q0[j].x, ay = 0.0 + q0[j].y, az = 0.0 + q0[j].z;   // AddPoint starts from +0.0
                for (uint32_t a = 1; a < cn[j]; ++a) {
                    const Row q = b.src[sh.q.pos[a0[j] + a]];
                    ax += q.x; ay += q.y; az += q.z;
                }
                const uint32_t v = sh.q.headpre[p0[j] >> 6] +
                                   (uint32_t)__popcll(sh.q.headbits[p0[j] >> 6] & ((1ull << (p0[j] & 63u)) - 1ull));
                vf_emit(g, vf_abs_key(g, b, kreg[h * HV + j]), ax, ay, az, cn[j], vbase + v, out);
            }
        }
    }
}

// ---------------- LDS sort: stable LSD passes over (key, position) ----------------
__device__ __forceinline__ VfRuns vf_sort_lds(VfShared& sh, const VfBatch& b, const uint32_t (&kreg)[VP_ROUNDS],
                                              VfClock& ck) {
    const int tid = threadIdx.x, w = wave_id(), l = lane_id();
    const uint32_t R = b.bt.rows;
    const int passes = (b.sortbits + 7) / 8;
    const uint32_t per = ((R + VF_WAVES * 64 - 1) / (VF_WAVES * 64)) * 64;   // items per wave: multiple of 64, <= 512
    const int rounds = (int)(per / 64);
#pragma unroll
    for (int r = 0; r < VP_ROUNDS; ++r) {
        const uint32_t i = r * VF_THREADS + tid;
        if (i < R) { sh.key[0][i] = kreg[r]; sh.perm[0][i] = (uint16_t)i; }
    }
    __syncthreads();
    VX_STAMP(1);
    int cur = 0;
    for (int p = 0; p < passes; ++p) {
        const int shift = 8 * p;
        for (int j = tid; j < VF_WAVES * 256; j += VF_THREADS) (&sh.cnt[0][0])[j] = 0;
        __syncthreads();
        uint32_t kk[VP_ROUNDS], rank[VP_ROUNDS];
        uint16_t pp[VP_ROUNDS];
#pragma unroll
        for (int r = 0; r < VP_ROUNDS; ++r) {
            if (r < rounds) {                      // wave-uniform
                const uint32_t i = w * per + r * 64 + l;
                const bool valid = i < R;
                kk[r] = valid ? sh.key[cur][i] : 0u;
                pp[r] = valid ? sh.perm[cur][i] : (uint16_t)0;
                rank[r] = wave_rank<8>(sh.cnt[w], (kk[r] >> shift) & 255u, valid);
            }
        }
        __syncthreads();
        uint32_t tot = 0;                          // items of digit `tid`; the digits in order, then the waves in order
        if (tid < 256) {
#pragma unroll
            for (int w2 = 0; w2 < VF_WAVES; ++w2) tot += sh.cnt[w2][tid];
        }
        uint32_t all;
        const uint32_t ex = block_scan_excl<VF_THREADS>(tot, sh.wsum, all);
        if (tid < 256) vx_wave_offsets<VF_WAVES>(sh.cnt, tid, ex);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < VP_ROUNDS; ++r) {
            if (r < rounds) {
                const uint32_t i = w * per + r * 64 + l;
                if (i < R) {
                    const uint32_t at = sh.cnt[w][(kk[r] >> shift) & 255u] + rank[r];
                    sh.key[cur ^ 1][at] = kk[r];
                    sh.perm[cur ^ 1][at] = pp[r];
                }
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    VX_STAMP(2);
    // ---- voxel heads of the sorted keys; voxel v starts at item key[cur^1][v]
    VfRuns s;
    uint32_t heads = 0;
    const uint32_t i0 = tid * VP_ROUNDS;            // 8 consecutive items per thread
    bool hd[VP_ROUNDS];
#pragma unroll
    for (int j = 0; j < VP_ROUNDS; ++j) {
        const uint32_t i = i0 + j;
        hd[j] = i < R && (i == 0 || sh.key[cur][i] != sh.key[cur][i - 1]);
        heads += hd[j];
    }
    uint32_t vi = block_scan_excl<VF_THREADS>(heads, sh.wsum, s.nvox);
#pragma unroll
    for (int j = 0; j < VP_ROUNDS; ++j)
        if (hd[j]) sh.key[cur ^ 1][vi++] = i0 + j;
    __syncthreads();
    s.skey = sh.key[cur]; s.sperm = sh.perm[cur]; s.vst = sh.key[cur ^ 1];
    return s;
}

// ---------------- general path (one oversize unit, or keys above 32 bits): LSD passes over the rows in global
// memory, between the batch's place in the first row buffer and the same place in the second ----------------
__device__ __forceinline__ VfRuns vf_sort_global(VfShared& sh, const VoxelPlan& g, const VfBatch& b, Row* bufA, Row* bufB,
                                                 uint32_t* __restrict__ vstart_g) {
    const int tid = threadIdx.x;
    const uint32_t s = b.bt.row0, R = b.bt.rows;
    const int passes = (g.rem + 7) / 8;
    for (int j = tid; j < 8 * 256; j += VF_THREADS) (&sh.hist[0][0])[j] = 0;
    __syncthreads();
    const int np = passes > 8 ? 8 : passes;
    for (uint32_t i = tid; i < R; i += VF_THREADS) {
        const uint64_t k = vx_key(g, b.mb, bufA[s + i]) & b.remmask;
        for (int p = 0; p < np; ++p) atomicAdd(&sh.hist[p][(k >> (8 * p)) & 255u], 1u);
    }
    __syncthreads();
    Row* from = bufA + s;
    Row* to = bufB + s;
    for (int p = 0; p < np; ++p) {
        uint32_t all;
        const uint32_t ex = block_scan_excl<VF_THREADS>(tid < 256 ? sh.hist[p][tid] : 0u, sh.wsum, all);
        if (tid < 256) sh.base[tid] = ex;
        __syncthreads();
        vx_ranked_scatter<VF_THREADS, VG_ROUNDS>(g, b.mb, b.remmask, 8 * p, from, to, R, sh.base, sh.cnt);
        __threadfence_block();
        __syncthreads();                             // this pass' rows are visible to the whole workgroup
        Row* tswap = from; from = to; to = tswap;
    }
    const Row* fin = from;
    // ---- voxel heads: vstart_g[s + v] = first row of voxel v (rows are physically sorted now)
    uint32_t carry = 0;
    for (uint32_t t0 = 0; t0 < R; t0 += VF_THREADS * VP_ROUNDS) {
        const uint32_t i0 = t0 + tid * VP_ROUNDS;
        uint64_t prevk = 0;
        if (i0 > 0 && i0 < R) prevk = vx_key(g, b.mb, fin[i0 - 1]);
        bool hd[VP_ROUNDS];
        uint32_t heads = 0;
#pragma unroll
        for (int j = 0; j < VP_ROUNDS; ++j) {
            const uint32_t i = i0 + j;
            uint64_t k = prevk;
            if (i < R) k = vx_key(g, b.mb, fin[i]);
            hd[j] = i < R && (i == 0 || k != prevk);
            heads += hd[j];
            prevk = k;
        }
        uint32_t tot;
        uint32_t vi = carry + block_scan_excl<VF_THREADS>(heads, sh.wsum, tot);
#pragma unroll
        for (int j = 0; j < VP_ROUNDS; ++j)
            if (hd[j]) vstart_g[s + vi++] = i0 + j;
        carry += tot;
    }
    __threadfence_block();
    __syncthreads();
    VfRuns r;
    r.nvox = carry; r.vst = vstart_g + s; r.rows = fin;
    return r;
}

// First output slot of the batch: look-back over the batches in front (ticket order).  Also the chunk's offset, the
// total, and the failure mark of a wait that ran out of its budget.
__device__ __forceinline__ int64_t vf_publish(VfShared& sh, const VoxelPlan& g, const VfBatch& b, uint32_t nvox,
                                              bool announced, uint32_t nbatches, uint64_t* __restrict__ status,
                                              int64_t* __restrict__ out_chunk_offsets, int64_t* __restrict__ out_m,
                                              VfClock& ck) {
    if (wave_id() == 0) {
        const uint32_t e0 = gf_lookback(status, (int64_t)b.t, nvox, announced);
        if (lane_id() == 0) {
            sh.vbase = e0 == GF_LB_FAILED ? 0u : e0;     // slot 0 keeps the writes of the reduce inside the output
            sh.lb_failed = e0 == GF_LB_FAILED ? 1u : 0u;
        }
    }
    __syncthreads();
    const int64_t vbase = sh.vbase;
    VX_STAMP(4);
    if (threadIdx.x == 0) {
        // *out_m starts at 0: the last batch adds the total (< 2^62), a batch whose wait ran out of its budget
        // sets the sign bit (idempotent: every batch behind a poisoned one fails too) - the word reads negative
        // iff some batch failed, in whatever order the two happen
        unsigned long long* om = reinterpret_cast<unsigned long long*>(out_m);
        if (sh.lb_failed) atomicOr(om, 1ull << 63);
        if (b.first_of_chunk && out_chunk_offsets) out_chunk_offsets[b.c] = vbase;
        if (b.t == nbatches - 1 && !sh.lb_failed) {
            atomicAdd(om, (unsigned long long)(vbase + nvox));
            if (out_chunk_offsets) out_chunk_offsets[g.nchunks] = vbase + nvox;
        }
    }
    return vbase;
}

// One thread per voxel of a sorted batch adds its rows in file order (AccumulatedPoint::AddPoint); row_at(i): the
// i-th row in sorted order, key_of(i): its voxel key.
template <class RowAt, class KeyOf>
__device__ __forceinline__ void vf_reduce_runs(const VoxelPlan& g, const VfRuns& s, uint32_t R, RowAt row_at, KeyOf key_of,
                                               int64_t vbase, const VfOut& out) {
    for (uint32_t v = threadIdx.x; v < s.nvox; v += VF_THREADS) {
        const uint32_t a0 = s.vst[v], a1 = v + 1 < s.nvox ? s.vst[v + 1] : R;
        double ax = 0.0, ay = 0.0, az = 0.0;
        for (uint32_t i = a0; i < a1; ++i) {
            const Row q = row_at(i);
            ax += q.x; ay += q.y; az += q.z;
        }
        vf_emit(g, key_of(a0), ax, ay, az, a1 - a0, vbase + v, out);
    }
}

__global__ __launch_bounds__(VF_THREADS, (2 * VF_THREADS) / 256) void vx_finish_k(
    VoxelPlan g, const double* __restrict__ minb, const VoxelBatch* __restrict__ batches,
    const uint32_t* __restrict__ batch_prefix, Row* __restrict__ bufA, Row* __restrict__ bufB,
    uint32_t* __restrict__ vstart_g, uint64_t* __restrict__ status, uint32_t* __restrict__ ticket,
    int32_t* __restrict__ out_idx, double* __restrict__ out_mean, int32_t* __restrict__ out_count,
    int64_t* __restrict__ out_chunk_offsets, int64_t* __restrict__ out_m, unsigned long long* __restrict__ stamps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vf_raw[];
    VfShared& sh = *reinterpret_cast<VfShared*>(vf_raw);
    const uint32_t nbatches = batch_prefix[g.nchunks];
    const VfOut out = {out_idx, out_mean, out_count};
    VfClock ck;
    VfBatch b;
    while (vf_take_batch(sh, g, minb, batches, batch_prefix, nbatches, bufA, bufB, ticket, b)) {
        VX_STAMP(0);
        const uint32_t R = b.bt.rows;
        // in LDS go the batches of <= VF_CAP rows whose relative keys fit 32 bits; with a bit to spare, the hash set
        // counts the voxels first and announces them (VQ_NONE is no key then)
        const bool fits = R != 0 && R <= (uint32_t)VF_CAP && b.sortbits <= 32;
        const bool announced = fits && b.sortbits <= 31;
        uint32_t kreg[VP_ROUNDS], hs[VP_ROUNDS];
        uint32_t nvox = 0;
        if (fits) vf_load_keys(g, b, kreg);
        if (announced) nvox = vf_count_voxels(sh, b, kreg, hs, status, ck);
        // The grouping path pays where most voxels hold one or two rows (0.1 m voxels on 100 points / m^2: 0.86 voxels
        // per row, 2.55 against 2.93 ms per 100 M rows); where rows share voxels (0.2 m: 0.45 voxels per row) the
        // stable sort is the faster of the two (0.30 against 0.34 ms per 10 M rows) - measured, both exact.
        const VfPath path = R == 0 ? VF_EMPTY
                          : !fits ? VF_SORT_GLOBAL
                          : (announced && sh.overflow == 0u && 10u * nvox >= 7u * R) ? VF_GROUPED : VF_SORT_LDS;
        if (path == VF_GROUPED) vf_group(sh, hs, ck);
        if (announced) { __syncthreads(); VX_STAMP(11); }
        VfRuns runs;
        if (path == VF_SORT_LDS) runs = vf_sort_lds(sh, b, kreg, ck);
        if (path == VF_SORT_GLOBAL) runs = vf_sort_global(sh, g, b, bufA, bufB, vstart_g);
        if (path == VF_SORT_LDS || path == VF_SORT_GLOBAL) nvox = runs.nvox;
#ifdef PCH_VX_STAMPS
        if (threadIdx.x == 0) { ck.acc[6] += path == VF_SORT_GLOBAL ? 1 : 0; ck.acc[7] += path == VF_EMPTY ? 1 : 0; }
#endif
        VX_STAMP(3);
        const int64_t vbase = vf_publish(sh, g, b, nvox, announced, nbatches, status, out_chunk_offsets, out_m, ck);
        if (path == VF_GROUPED) {
            vf_reduce_grouped(sh, g, b, kreg, hs, vbase, out);
        } else if (path == VF_SORT_LDS) {
            vf_reduce_runs(g, runs, R, [&](uint32_t i) { return b.src[runs.sperm[i]]; },
                           [&](uint32_t i) { return vf_abs_key(g, b, runs.skey[i]); }, vbase, out);
        } else if (path == VF_SORT_GLOBAL) {
            vf_reduce_runs(g, runs, R, [&](uint32_t i) { return runs.rows[i]; },
                           [&](uint32_t i) { return vx_key(g, b.mb, runs.rows[i]); }, vbase, out);
        }
        VX_STAMP(5);
    }
#ifdef PCH_VX_STAMPS
    if (threadIdx.x == 0) for (int k = 0; k < 12; ++k) atomicAdd(&stamps[k], ck.acc[k]);
#endif
}

struct VoxelWs {
    unsigned long long* mm;
    double*   minb;
    int*      gmeta;
    Row      *bufA, *bufB;
    uint32_t *tile_hist, *unit_start, *nbatch, *batch_prefix, *vstart, *ticket;
    VoxelBatch* batches;
    VoxelOversize* over;
    uint32_t* nover;
    uint64_t* status;
    size_t    clear_bytes;       // ticket .. end of status: zeroed before the finisher
};

// a kernel's dynamic LDS above the default limit: set once per device
template <auto kernel>
static int set_max_lds(size_t bytes) {
    static bool done[PCH_MAX_DEVICES] = {};
    const int slot = current_device_slot();
    if (!done[slot]) {
        PCH_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)bytes));
        done[slot] = true;
    }
    return PCH_OK;
}

static int64_t voxel_nchunks(int64_t n, int64_t& chunk_size) {
    if (chunk_size <= 0 || chunk_size > n) chunk_size = n > 0 ? n : 1;
    return n > 0 ? ceil_div(n, chunk_size) : 1;
}

static void voxel_workspace(Arena& a, int64_t n, int64_t nchunks, int64_t chunk_size, VoxelWs& w) {
    const int64_t nn = n > 0 ? n : 1;
    const int64_t tiles = nchunks * ceil_div(chunk_size, VP_TILE);
    w.mm = a.take<unsigned long long>(nchunks * 6);
    w.minb = a.take<double>(nchunks * 3);
    w.gmeta = a.take<int>(4);
    w.bufA = a.take<Row>(nn);
    w.bufB = a.take<Row>(nn);
    w.vstart = a.take<uint32_t>(nn);
    w.tile_hist = a.take<uint32_t>(tiles * VP_MAXBINS);
    w.unit_start = a.take<uint32_t>(nchunks * VP_MAXBINS);
    w.batches = a.take<VoxelBatch>(nchunks * VP_MAXBINS);
    w.nbatch = a.take<uint32_t>(nchunks + 1);
    w.batch_prefix = a.take<uint32_t>(nchunks + 1);
    w.over = a.take<VoxelOversize>(nchunks * VP_MAXBINS);
    const size_t off0 = a.off;
    w.ticket = a.take<uint32_t>(64);                       // [0] ticket, [1] oversize units, [8..24) stamp sums (tuning builds)
    w.nover = w.ticket + 1;
    w.status = a.take<uint64_t>(nchunks * VP_MAXBINS);
    w.clear_bytes = a.off - off0;
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_voxel_downsample_ws_bytes(int64_t n, int64_t chunk_size) {
    if (n < 0) return 0;
    const int64_t nchunks = voxel_nchunks(n, chunk_size);
    Arena a;
    VoxelWs w;
    voxel_workspace(a, n, nchunks, chunk_size, w);
    return a.off;
}

// The grid of the call from what vx_bounds_k found (gmeta: largest index per axis, range flag), or the range error
static int voxel_make_plan(const int (&gmeta)[4], int64_t n, int64_t chunk_size, int64_t nchunks, double voxel_size,
                           VoxelPlan& g) {
    if (gmeta[3] != 0) {   // Open3D: "[VoxelDownSample] voxel_size is too small."
        set_error("voxel_size is too small (or non-finite coordinates)");
        return PCH_ERR_RANGE;
    }
    g.n = n; g.chunk_size = chunk_size; g.nchunks = nchunks; g.tiles_per_chunk = ceil_div(chunk_size, VP_TILE);
    g.voxel = voxel_size; g.rvoxel = 1.0 / voxel_size;
    g.bx = bits_for((uint64_t)gmeta[0] + 1); g.by = bits_for((uint64_t)gmeta[1] + 1); g.bz = bits_for((uint64_t)gmeta[2] + 1);
    g.T = g.bx + g.by + g.bz;
    if (g.T > 63) {
        set_error("voxel grid needs %d key bits (> 63): reduce chunk extent or enlarge voxel", g.T);
        return PCH_ERR_RANGE;
    }
    g.d1 = g.T < VP_MAXBITS ? g.T : VP_MAXBITS; g.nb = 1 << g.d1; g.rem = g.T - g.d1;
    return PCH_OK;
}

// level 1: the rows of every chunk partitioned by their first digit into w.bufA, the units grouped into batches
static int voxel_launch_partition(const double* xyz, const VoxelPlan& g, const VoxelWs& w, hipStream_t s) {
    const unsigned gt = (unsigned)(g.nchunks * g.tiles_per_chunk);
    PCH_LAUNCH("voxel_tilehist", vx_tilehist_k, dim3(gt), dim3(VP_THREADS), 0, s, xyz, g, (const double*)w.minb,
               w.tile_hist);
    PCH_LAUNCH("voxel_binscan", vx_binscan_k, dim3((unsigned)g.nchunks), dim3(VP_MAXBINS), 0, s, g, w.tile_hist,
               w.unit_start, w.batches, w.nbatch, w.over, w.nover);
    PCH_LAUNCH("voxel_batchscan", vx_batchscan_k, dim3(1), dim3(1024), 0, s, (const uint32_t*)w.nbatch, g.nchunks,
               w.batch_prefix);
    // staged through LDS where the partitioned rows do not stay in the Infinity Cache (256 MB): 100 M rows 1.39 -> 1.20 ms;
    // below that the direct form is the faster one (10 M rows: 0.125 against 0.134 ms).  PCH_VX_SCATTER=direct|lds: tuning
    static const int scatter_mode = [] {
        const char* e = getenv("PCH_VX_SCATTER");
        return e == nullptr ? 0 : (strcmp(e, "lds") == 0 ? 1 : (strcmp(e, "direct") == 0 ? 2 : 0));
    }();
    if (scatter_mode == 1 || (scatter_mode == 0 && g.n * (int64_t)sizeof(Row) > (int64_t(384) << 20))) {
        PCH_TRY(set_max_lds<vx_scatter_lds_k>(sizeof(VsShared)));
        PCH_LAUNCH("voxel_scatter", vx_scatter_lds_k, dim3(gt), dim3(VP_THREADS), sizeof(VsShared), s, xyz, g,
                   (const double*)w.minb, (const uint32_t*)w.tile_hist, (const uint32_t*)w.unit_start, w.bufA);
    } else {
        PCH_LAUNCH("voxel_scatter", vx_scatter_k, dim3(gt), dim3(VP_THREADS), 0, s, xyz, g, (const double*)w.minb,
                   (const uint32_t*)w.tile_hist, (const uint32_t*)w.unit_start, w.bufA);
    }
    return PCH_OK;
}

// persistent finisher: two 512-thread workgroups per CU draw the batches in order; fg: how many were launched
static int voxel_launch_finish(const VoxelPlan& g, const VoxelWs& w, int32_t* out_idx, double* out_mean,
                               int32_t* out_count, int64_t* out_chunk_offsets, int64_t* out_m, hipStream_t s,
                               int64_t& fg) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    fg = (int64_t)cus * 2;
    if (fg > g.nchunks * g.nb) fg = g.nchunks * g.nb;
    PCH_TRY(set_max_lds<vx_finish_k>(sizeof(VfShared)));
    PCH_LAUNCH("voxel_finish", vx_finish_k, dim3((unsigned)fg), dim3(VF_THREADS), sizeof(VfShared), s, g,
               (const double*)w.minb, (const VoxelBatch*)w.batches, (const uint32_t*)w.batch_prefix, w.bufA, w.bufB,
               w.vstart, w.status, w.ticket, out_idx, out_mean, out_count, out_chunk_offsets, out_m,
               reinterpret_cast<unsigned long long*>(w.ticket + 8));
    return PCH_OK;
}

#ifdef PCH_VX_STAMPS
static int voxel_print_stamps(const VoxelWs& w, int64_t nchunks, int64_t fg, hipStream_t s) {
    unsigned long long t[12];
    uint32_t nb_tot = 0, nov = 0;
    PCH_HIP_TRY(hipStreamSynchronize(s));
    PCH_HIP_TRY(hipMemcpy(t, w.ticket + 8, sizeof(t), hipMemcpyDeviceToHost));
    PCH_HIP_TRY(hipMemcpy(&nb_tot, w.batch_prefix + nchunks, 4, hipMemcpyDeviceToHost));
    PCH_HIP_TRY(hipMemcpy(&nov, w.nover, 4, hipMemcpyDeviceToHost));
    const char* nm[6] = {"ticket+lookup", "load+keys", "sort passes", "heads", "look-back", "reduce"};
    fprintf(stderr, "voxel finisher: %u batches, %u oversize units; per-workgroup average (us):", nb_tot, nov);
    for (int k = 0; k < 6; ++k) fprintf(stderr, "  %s %.1f", nm[k], (double)t[k] / 100.0 / (double)fg);
    fprintf(stderr, "  | global-path batches %llu, empty slots %llu", t[6], t[7]);
    fprintf(stderr, "  | grouping path: init+keys+insert %.1f, announce+slot scan %.1f, scatter %.1f, sort+heads %.1f",
            (double)t[8] / 100.0 / (double)fg, (double)t[9] / 100.0 / (double)fg, (double)t[10] / 100.0 / (double)fg,
            (double)t[11] / 100.0 / (double)fg);
    unsigned long long polls = 0, wins = 0;
    (void)hipMemcpyFromSymbol(&polls, HIP_SYMBOL(g_lb_polls), 8);
    (void)hipMemcpyFromSymbol(&wins, HIP_SYMBOL(g_lb_windows), 8);
    fprintf(stderr, "  | look-back totals so far: %llu windows, %llu failed polls\n", wins, polls);
    return PCH_OK;
}
#endif

extern "C" int pch_voxel_downsample_f64(const double* xyz, int64_t n, double voxel_size,
                                        int64_t chunk_size, int32_t* out_idx, double* out_mean,
                                        int32_t* out_count, int64_t* out_chunk_offsets,
                                        int64_t* out_m, void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(xyz ? (const void*)xyz : (const void*)out_m);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "n out of range [0, 2^31)");
    PCH_REQUIRE(voxel_size > 0.0, "voxel_size must be > 0");
    PCH_REQUIRE(out_m != nullptr, "out_m is null");
    const int64_t nchunks = voxel_nchunks(n, chunk_size);
    if (n == 0) {
        PCH_HIP_TRY(hipMemsetAsync(out_m, 0, sizeof(int64_t), s));
        if (out_chunk_offsets) PCH_HIP_TRY(hipMemsetAsync(out_chunk_offsets, 0, 2 * sizeof(int64_t), s));
        return PCH_OK;
    }
    PCH_REQUIRE(xyz && out_idx && out_mean && out_count && ws, "null buffer");
    Arena a(ws, ws_bytes);
    VoxelWs w;
    voxel_workspace(a, n, nchunks, chunk_size, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }

    // per-chunk bounds: [chunk][min3,max3]; min slots start at all-ones, max slots at zero
    PCH_HIP_TRY(hipMemsetAsync(w.mm, 0, sizeof(unsigned long long) * nchunks * 6, s));
    PCH_HIP_TRY(hipMemset2DAsync(w.mm, 48, 0xFF, 24, nchunks, s));
    PCH_HIP_TRY(hipMemsetAsync(w.gmeta, 0, sizeof(int) * 4, s));
    PCH_HIP_TRY(hipMemsetAsync(out_m, 0, sizeof(int64_t), s));           // the finisher ADDS to it (see vf_publish)
    const int64_t bpc = ceil_div(chunk_size, VX_THREADS * VX_MM_ROUNDS);
    PCH_LAUNCH("voxel_minmax", vx_minmax_k, dim3((unsigned)(bpc * nchunks)), dim3(VX_THREADS), 0, s,
               xyz, n, chunk_size, bpc, w.mm);
    PCH_LAUNCH("voxel_bounds", vx_bounds_k, dim3((unsigned)ceil_div(nchunks, 256)), dim3(256), 0, s,
               (const unsigned long long*)w.mm, nchunks, voxel_size, w.minb, w.gmeta);
    int gmeta[4];
    PCH_TRY(peek_enqueue(w.gmeta, sizeof(gmeta), s));
    PCH_HIP_TRY(hipMemsetAsync(w.ticket, 0, w.clear_bytes, s));      // overlaps the host's wait
    PCH_TRY(peek_wait(gmeta, sizeof(gmeta)));

    VoxelPlan g;
    int64_t fg = 0;
    PCH_TRY(voxel_make_plan(gmeta, n, chunk_size, nchunks, voxel_size, g));
    PCH_TRY(voxel_launch_partition(xyz, g, w, s));
    // units above the LDS capacity (dense columns): split by their next digit, one workgroup each (one unit per workgroup
    // as a rule: 512 of them are resident at a time)
    PCH_LAUNCH("voxel_split", vx_split_k, dim3((unsigned)(nchunks * g.nb < 2048 ? nchunks * g.nb : 2048)), dim3(VS_THREADS), 0, s, g,
               (const double*)w.minb, (const Row*)w.bufA, w.bufB, w.batches, (const VoxelOversize*)w.over,
               (const uint32_t*)w.nover);
    PCH_TRY(voxel_launch_finish(g, w, out_idx, out_mean, out_count, out_chunk_offsets, out_m, s, fg));
#ifdef PCH_VX_STAMPS
    PCH_TRY(voxel_print_stamps(w, nchunks, fg, s));
#endif
    return PCH_OK;
}
