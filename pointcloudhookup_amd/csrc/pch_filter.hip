// Stage B: float32 centroid (numpy sequential-sum semantics), centring, numpy 'linear'
// percentile by radix select, and the order-preserving height-filter compaction.
// Reference: utils/tower_extraction.py:62-64 (centroid, centring), :82-89 (percentile filter).
#include "pch_prims.h"
#include "pch_mean.h"
#include "pch_compact.h"
#include "pch_select.h"

namespace pch {

// =====================================================================================
// B2: k-th order statistics of v[i] = base[i*stride] - sub by 12/12/8-bit radix select on the
// order-preserving uint32 image of the float.  NaN sorts last (as numpy's partition).
// x -> fl(x - sub) is monotone non-decreasing, so the k-th smallest of v is fl(k-th smallest of
// base - sub): the select runs on the raw values and the subtraction is applied to the two
// selected order statistics only.
// =====================================================================================
constexpr int SEL_BINS = 4096;
constexpr int SEL_REP0 = 4;             // histogram copies in the first pass
constexpr int SEL_TILE = 4096;          // values per workgroup trip in the histogram passes

struct SelState {
    unsigned long long rank;       // remaining rank inside the current prefix
    unsigned long long less;       // elements strictly below the current prefix
    uint32_t prefix;               // resolved high bits
    uint32_t need_next;            // 1: k1 is not inside the final bin of k0
    uint32_t v0key;                // the selected key (after the last pick)
    uint32_t pad;
};

// (sel_key, the order-preserving key of a value, lives in pch_mean.h: the summary pass brackets with it too)

// adds 1 to h[bin] for every active lane; lanes of a wave that share a bin are merged into one
// LDS atomic (z values of a flat corridor fall into a handful of bins)
template <int ROUNDS>
__device__ __forceinline__ void sel_hist_add(uint32_t* h, bool active, uint32_t bin) {
    // up to ROUNDS rounds of 'merge every lane that shares the first pending lane's bin into one
    // LDS atomic' while many lanes are pending, plain atomics for the rest
    bool pending = active;
#pragma unroll
    for (int round = 0; round < ROUNDS; ++round) {
        const unsigned long long todo = __ballot(pending);
        if (__popcll(todo) < 8) break;
        const int leader = (int)__builtin_ctzll(todo);
        const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
        const unsigned long long same = __ballot(pending && bin == b0);
        if (lane_id() == leader) atomicAdd(&h[b0], (uint32_t)__popcll(same));
        pending = pending && bin != b0;
    }
    if (pending) atomicAdd(&h[bin], 1u);
}

// Source switch of the bracketed select (below): when *ok is set the kernel works on the candidate buffer
// (alt_base, *alt_n values, contiguous) instead of the column it was launched for - one launch serves either case.
struct SelGate { const uint32_t* ok; const float* alt_base; const uint32_t* alt_n; };
__device__ __forceinline__ void sel_gate(const SelGate& g, const float*& base, int64_t& n, int64_t& stride) {
    if (g.ok && *g.ok) { base = g.alt_base; n = (int64_t)*g.alt_n; stride = 1; }
}

__device__ __forceinline__ float sel_key_to_float(uint32_t k) {
    return (k == 0xFFFFFFFFu) ? __uint_as_float(0x7FC00000u) : f32_unordered(k);
}

// (the interpolation itself is numpy's _lerp in float32: a + (b-a)*t, and b - (b-a)*(1-t) where t >= 0.5,
// numpy/lib/_function_base_impl.py:4639-4660; NaN anywhere -> NaN.  scal: [0] = percentile,
// [1] = percentile + add1, [2] = percentile + add2 - see sel_lerp_k)

// ---- the select, with every pick folded into its consumer ----------------------------------------
// A kernel of a few microseconds still costs a launch slot (~5 us each on this stream), and a percentile used
// to be 9 of them (27 with the sample bracket below).  Here the single-workgroup pick of pass p runs as the
// prologue of whatever needs its result - histogram pass p+1, the "next key" pass, the bracket sweep, the final
// interpolation: every workgroup repeats it from the finished histogram of pass p (16 KB, L2), workgroup 0 stores
// the new state for the kernels behind.  Histograms of the three passes live side by side and are cleared once.
// NR = 2 selects two ranks of the same data in the same sweeps (the two ends of the sample bracket).
struct SelRun {
    SelState st[4];                 // st[p]: state in front of histogram pass p; st[3]: after the last pick
    unsigned long long nan_count;
    uint32_t next_min, pad;
};
__host__ __device__ __forceinline__ uint32_t* sel_hist_of(uint32_t* hist, int run, int pass) {
    return hist + ((pass == 0 ? 0 : run) * 3 + pass) * SEL_BINS;        // pass 0 has no prefix: one histogram for all runs
}

template <int PASS>
__device__ __forceinline__ SelState sel_pick_block(const SelState& in, const uint32_t* __restrict__ hist) {
    __shared__ unsigned long long wsum[4];
    __shared__ int found_bin;
    __shared__ unsigned long long found_below, found_cnt;
    constexpr int nb = (PASS == 2) ? 256 : SEL_BINS;
    constexpr int per = nb / 256;                   // bins per thread (16 or 1)
    const unsigned long long rank = in.rank;
    unsigned long long loc[per];
    unsigned long long tsum = 0;
#pragma unroll
    for (int j = 0; j < per; ++j) { loc[j] = hist[threadIdx.x * per + j]; tsum += loc[j]; }
    const unsigned long long incl = wave_scan_incl(tsum);
    __syncthreads();                                // a previous call may still be reading the shared words
    if (lane_id() == 63) wsum[wave_id()] = incl;
    if (threadIdx.x == 0) found_bin = -1;
    __syncthreads();
    unsigned long long before = incl - tsum;
    for (int w = 0; w < wave_id(); ++w) before += wsum[w];
    if (rank >= before && rank < before + tsum) {   // the thread whose bins hold the rank
        unsigned long long b = before;
#pragma unroll
        for (int j = 0; j < per; ++j) {
            if (rank >= b && rank < b + loc[j]) { found_bin = threadIdx.x * per + j; found_below = b; found_cnt = loc[j]; }
            b += loc[j];
        }
    }
    __syncthreads();
    SelState out = in;
    const bool hit = found_bin >= 0;                // (an empty input never gets here)
    const uint32_t bin = hit ? (uint32_t)found_bin : 0u;
    const unsigned long long below = hit ? found_below : 0ull;
    out.less = in.less + below;
    out.rank = rank - below;
    if (PASS == 0) out.prefix = bin;
    else if (PASS == 1) out.prefix = (in.prefix << 12) | bin;
    else {
        out.v0key = (in.prefix << 8) | bin;
        out.need_next = (hit && rank + 1 < found_below + found_cnt) ? 0u : 1u;   // is rank+1 in this final bin too?
    }
    return out;
}

// PICK = false: no pick prologue, the prefix is taken as the caller left it in run[r].st[PASS] (the passes one at a
// time, pch_select_hist_f32)
template <int PASS, int NR, bool PICK = true>
__global__ __launch_bounds__(256) void sel_hist_k(const float* __restrict__ base_in, int64_t n, int64_t stride,
                                                   SelRun* __restrict__ run, uint32_t* __restrict__ hist,
                                                   SelGate gate) {
    const float* base = base_in;
    sel_gate(gate, base, n, stride);
    // the grid is sized for the column the launch names; on the gated source (the bracket's candidates: ~1 % of it) most
    // workgroups have no tile - they leave before the pick and the 16 KB of LDS zeroing (workgroup 0 stays: it records
    // the pick)
    if (blockIdx.x != 0 && (int64_t)blockIdx.x * SEL_TILE >= n) return;
    // pass 0 sees a handful of hot bins (z of a flat corridor): SEL_REP0 copies of the histogram, picked by lane,
    // divide the same-address serialisation of the LDS atomics
    constexpr int REP = PASS == 0 ? SEL_REP0 : 1;
    constexpr int NH = PASS == 0 ? 1 : NR;
    __shared__ uint32_t hh[NH][REP][SEL_BINS];
    uint32_t prefix[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        prefix[r] = 0;
        if (PASS >= 1 && PICK) {
            const SelState st = sel_pick_block<(PASS >= 1 ? PASS - 1 : 0)>(run[r].st[PASS >= 1 ? PASS - 1 : 0],
                                                                             sel_hist_of(hist, r, PASS >= 1 ? PASS - 1 : 0));
            if (blockIdx.x == 0 && threadIdx.x == 0) run[r].st[PASS] = st;
            prefix[r] = st.prefix;
        } else if (PASS >= 1) {
            prefix[r] = run[r].st[PASS].prefix;
        }
    }
    for (int j = threadIdx.x; j < NH * REP * SEL_BINS; j += 256) (&hh[0][0][0])[j] = 0;
    __syncthreads();
    const int rep = lane_id() & (REP - 1);
    unsigned long long nans = 0;
    auto take = [&](bool in, float v) {
        const uint32_t k = sel_key(v);
        if (PASS == 0) {
            if (in) atomicAdd(&hh[0][rep][k >> 20], 1u);
            nans += (in && v != v);
        } else {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                if (PASS == 1) sel_hist_add<1>(hh[r < NH ? r : 0][0], in && (k >> 20) == prefix[r], (k >> 8) & 0xFFFu);
                else sel_hist_add<1>(hh[r < NH ? r : 0][0], in && (k >> 8) == prefix[r], k & 0xFFu);
            }
        }
    };
    // a workgroup takes tiles of 4096 values; on a contiguous, 16-byte aligned column every thread keeps four float4
    // loads in flight (the histogram update behind a load is a dependent chain)
    const int64_t span = (int64_t)gridDim.x * SEL_TILE;
    const bool vec = stride == 1 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0;
    for (int64_t t0 = (int64_t)blockIdx.x * SEL_TILE; t0 < n; t0 += span) {    // wave-uniform trip count
        if (vec && t0 + SEL_TILE <= n) {
            const float4* b4 = reinterpret_cast<const float4*>(base + t0);
            float4 q[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) q[r] = b4[r * 256 + threadIdx.x];
#pragma unroll
            for (int r = 0; r < 4; ++r) { take(true, q[r].x); take(true, q[r].y); take(true, q[r].z); take(true, q[r].w); }
        } else {
#pragma unroll 4
            for (int r = 0; r < SEL_TILE / 256; ++r) {
                const int64_t i = t0 + r * 256 + threadIdx.x;
                const bool in = i < n;
                take(in, in ? base[i * stride] : 0.0f);
            }
        }
    }
    __syncthreads();
    constexpr int nb = (PASS == 2) ? 256 : SEL_BINS;
#pragma unroll
    for (int r = 0; r < NH; ++r) {
        uint32_t* out = sel_hist_of(hist, r, PASS);
        for (int j = threadIdx.x; j < nb; j += 256) {
            uint32_t t = 0;
#pragma unroll
            for (int c = 0; c < REP; ++c) t += hh[r][c][j];
            if (t) atomicAdd(&out[j], t);
        }
    }
    if (PASS == 0) {
        nans = wave_reduce_add(nans);
        if (lane_id() == 0 && nans) atomicAdd(&run[0].nan_count, nans);
    }
}

// smallest key strictly above the selected one (only when rank+1 lies beyond its final bin); the last pick first
// (PICK = false: the key and need_next as the caller left them in run->st[3], pch_select_min_above_f32)
template <bool PICK = true>
__global__ __launch_bounds__(256) void sel_next_k(const float* __restrict__ base_in, int64_t n, int64_t stride,
                                                   SelRun* __restrict__ run, uint32_t* __restrict__ hist, SelGate gate) {
    const float* base = base_in;
    sel_gate(gate, base, n, stride);
    if (blockIdx.x != 0 && (int64_t)blockIdx.x * SEL_TILE >= n) return;      // no tile (see sel_hist_k)
    SelState st = run->st[3];
    if (PICK) {
        st = sel_pick_block<2>(run->st[2], sel_hist_of(hist, 0, 2));
        if (blockIdx.x == 0 && threadIdx.x == 0) run->st[3] = st;
    }
    if (st.need_next == 0) return;
    const uint32_t v0 = st.v0key;
    uint32_t best = 0xFFFFFFFFu;
    auto take = [&](float v) {
        const uint32_t k = sel_key(v);
        if (k > v0 && k < best) best = k;
    };
    const int64_t span = (int64_t)gridDim.x * SEL_TILE;
    const bool vec = stride == 1 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0;
    for (int64_t t0 = (int64_t)blockIdx.x * SEL_TILE; t0 < n; t0 += span) {
        if (vec && t0 + SEL_TILE <= n) {
            const float4* b4 = reinterpret_cast<const float4*>(base + t0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float4 q = b4[r * 256 + threadIdx.x];
                take(q.x); take(q.y); take(q.z); take(q.w);
            }
        } else {
            for (int r = 0; r < SEL_TILE / 256; ++r) {
                const int64_t i = t0 + r * 256 + threadIdx.x;
                if (i < n) take(base[i * stride]);
            }
        }
    }
    best = wave_reduce_min(best);
    if (lane_id() == 0 && best != 0xFFFFFFFFu) atomicMin(&run->next_min, best);
}

// the final interpolation; picked = 0: the last pick has not run yet (there was no "next" pass)
__global__ __launch_bounds__(256) void sel_lerp_k(const SelRun* __restrict__ run, const uint32_t* __restrict__ hist2,
                                                   int picked, int same_index, float gamma,
                                                   const float* __restrict__ sub, float add1, float add2,
                                                   float* __restrict__ scal) {
    SelState st = run->st[3];
    if (!picked) st = sel_pick_block<2>(run->st[2], hist2);
    if (threadIdx.x != 0) return;
    const float c = sub ? *sub : 0.0f;
    const float a = sel_key_to_float(st.v0key) - c;
    float b = a;
    if (!same_index && st.need_next) b = sel_key_to_float(run->next_min) - c;
    float r = sel_lerp_f32(a, b, gamma);
    if (run->nan_count) r = __uint_as_float(0x7FC00000u);
    scal[0] = r;
    scal[1] = r + add1;
    scal[2] = r + add2;
}

// ---- bracketed select for large contiguous columns: ONE pass over the data instead of three ------------
// A sample (16 consecutive values out of every 1024) is selected exactly at two ranks around the wanted
// quantile; the keys L <= H found there bracket the wanted order statistics with overwhelming probability.
// One pass over the column counts the keys below L and collects the keys in [L, H] (a few per cent of the
// data); the exact three-pass select then runs on those candidates only, with the rank shifted by the count
// below L.  Whether the bracket really holds both order statistics is CHECKED on the device
// (sel_bracket_fix_k); if not, the same three passes read the whole column instead of the candidates.
// Either way the result is the exact order statistic - the sample only decides how much data is read.
constexpr int64_t SEL_BRACKET_MIN = int64_t(1) << 22;     // below this the three passes are cheap enough
constexpr int SEL_GROUP = 16, SEL_EVERY = 1024;

struct BrState {
    unsigned long long less;       // keys < L
    unsigned long long nan;        // NaN values seen by the bracket pass
    uint32_t count;                // candidates collected (keys in [L, H])
    uint32_t overflow;             // candidate buffer too small
    uint32_t ok;                   // 1: both order statistics lie inside the candidates
    uint32_t pad;
};

// four consecutive values per thread (SEL_GROUP is a multiple of 4, SEL_EVERY of 16: both sides 16-byte aligned when
// the column is)
__global__ void sel_sample_k(const float* __restrict__ base, int64_t ns, float* __restrict__ sample) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= ns) return;
    const int64_t src = (i / SEL_GROUP) * SEL_EVERY + (i % SEL_GROUP);
    float4 q;
    if ((reinterpret_cast<uintptr_t>(base) & 15u) == 0) {
        q = *reinterpret_cast<const float4*>(base + src);
    } else {
        q.x = base[src]; q.y = base[src + 1]; q.z = base[src + 2]; q.w = base[src + 3];
    }
    *reinterpret_cast<float4*>(sample + i) = q;
}
static_assert(SEL_GROUP % 4 == 0 && SEL_EVERY % 4 == 0, "sel_sample_k");

constexpr int SEL_STAGE = 2 * SEL_TILE;                  // candidates a workgroup stages in LDS before it reserves output

__global__ __launch_bounds__(256) void sel_bracket_k(const float* __restrict__ base, int64_t n,
                                                     const SelRun* __restrict__ lohi, uint32_t* __restrict__ hist,
                                                     int lo_is_min, int hi_is_max,
                                                     BrState* __restrict__ br, float* __restrict__ cand, uint32_t cap) {
    // candidates are staged in LDS and written out a few thousand at a time: one global atomic per flush (a
    // reservation per wave would be ~1.5 M atomics on one address for 100 M values - 13 ms, measured)
    __shared__ float stage[SEL_STAGE];
    __shared__ uint32_t nstage, gbase;
    // the last picks of the two sample selects; a bracket that reaches the bottom / top of the sample is open there
    const uint32_t Lk = sel_pick_block<2>(lohi[0].st[2], sel_hist_of(hist, 0, 2)).v0key;
    const uint32_t Hk = sel_pick_block<2>(lohi[1].st[2], sel_hist_of(hist, 1, 2)).v0key;
    const uint32_t L = lo_is_min ? 0u : Lk, H = hi_is_max ? 0xFFFFFFFFu : Hk;
    unsigned long long less = 0, nans = 0;
    const uint64_t lt = lanemask_lt();
    if (threadIdx.x == 0) nstage = 0;
    __syncthreads();
    auto flush = [&]() {                                   // workgroup-uniform call
        const uint32_t m = nstage;
        if (threadIdx.x == 0) gbase = m ? atomicAdd(&br->count, m) : 0u;
        __syncthreads();
        const uint32_t g0 = gbase;
        for (uint32_t i = threadIdx.x; i < m; i += 256) {
            if (g0 + i < cap) cand[g0 + i] = stage[i]; else br->overflow = 1u;
        }
        __syncthreads();
        if (threadIdx.x == 0) nstage = 0;
        __syncthreads();
    };
    auto take = [&](bool in, float v) {
        const uint32_t k = sel_key(v);
        less += (in && k < L) ? 1u : 0u;
        nans += (in && v != v) ? 1u : 0u;
        const bool keep = in && k >= L && k <= H;
        const unsigned long long m = __ballot(keep);
        if (m) {
            const int leader = (int)__builtin_ctzll(m);
            uint32_t at = 0;
            if (lane_id() == leader) at = atomicAdd(&nstage, (uint32_t)__popcll(m));      // LDS atomic
            at = (uint32_t)__builtin_amdgcn_readlane((int)at, leader);
            if (keep) stage[at + (uint32_t)__popcll(m & lt)] = v;                          // < SEL_STAGE: see the flush rule
        }
    };
    const int64_t span = (int64_t)gridDim.x * SEL_TILE;
    const bool vec = (reinterpret_cast<uintptr_t>(base) & 15u) == 0;
    for (int64_t t0 = (int64_t)blockIdx.x * SEL_TILE; t0 < n; t0 += span) {    // workgroup-uniform trip count
        __syncthreads();
        if (nstage > (uint32_t)(SEL_STAGE - SEL_TILE)) flush();                  // room for a whole tile of candidates
        if (vec && t0 + SEL_TILE <= n) {
            const float4* b4 = reinterpret_cast<const float4*>(base + t0);
            float4 q[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) q[r] = b4[r * 256 + threadIdx.x];
#pragma unroll
            for (int r = 0; r < 4; ++r) { take(true, q[r].x); take(true, q[r].y); take(true, q[r].z); take(true, q[r].w); }
        } else {
            for (int r = 0; r < SEL_TILE / 256; ++r) {
                const int64_t i = t0 + r * 256 + threadIdx.x;
                const bool in = i < n;
                take(in, in ? base[i] : 0.0f);
            }
        }
    }
    __syncthreads();
    flush();
    less = wave_reduce_add(less);
    nans = wave_reduce_add(nans);
    if (lane_id() == 0) {
        if (less) atomicAdd(&br->less, less);
        if (nans) atomicAdd(&br->nan, nans);
    }
}

// The same BrState from what the centroid summary left (MsBracket, pch_mean.h) instead of a sweep over a z column:
// per 1024-row block one record (keys below L, NaN values, values inside the bracket) and those values at the front
// of the block's segment.  A workgroup takes SEL_CBLKS blocks, one record per thread; the counts are known before a
// value is read, so the output offsets come from a scan and ONE reservation per workgroup (382 at 100 M rows; see
// sel_bracket_k for the price of reserving more often) and the values go straight from the segments to `cand` -
// item k of the workgroup finds its block by a search over the scanned counts, so every lane copies and consecutive
// lanes write consecutive words.  An invalid bracket raises `overflow`: the device check behind (sel_bracket_fix_k)
// then fails as it does for a full buffer or a rank outside the bracket, and the select reads the rows.
constexpr int SEL_CBLKS = 256;
__global__ __launch_bounds__(SEL_CBLKS) void sel_collect_k(const MsBracket* __restrict__ brk,
                                                           const MsBrRec* __restrict__ brec, int64_t nblk,
                                                           const float* __restrict__ zseg, BrState* __restrict__ br,
                                                           float* __restrict__ cand, uint32_t cap) {
    __shared__ uint32_t first[SEL_CBLKS];                  // values of the workgroup in front of block t
    __shared__ uint32_t wtot[SEL_CBLKS / 64];
    __shared__ uint32_t gbase;
    if ((brk->valid[0] & brk->valid[1]) == 0u) {
        if (blockIdx.x == 0 && threadIdx.x == 0) br->overflow = 1u;
        return;
    }
    const int64_t b0 = (int64_t)blockIdx.x * SEL_CBLKS;
    const int64_t b = b0 + threadIdx.x;
    MsBrRec r = {0u, 0u};
    if (b < nblk) r = brec[b];
    const uint32_t c = r.count_less & 0xFFFFu;
    const uint32_t incl = wave_scan_incl(c);
    if (lane_id() == 63) wtot[wave_id()] = incl;
    unsigned long long less = wave_reduce_add((unsigned long long)(r.count_less >> 16));
    unsigned long long nans = wave_reduce_add((unsigned long long)r.nan);
    if (lane_id() == 0) {
        if (less) atomicAdd(&br->less, less);
        if (nans) atomicAdd(&br->nan, nans);
    }
    __syncthreads();
    uint32_t before = incl - c, T = 0;
    for (int w = 0; w < SEL_CBLKS / 64; ++w) { before += w < wave_id() ? wtot[w] : 0u; T += wtot[w]; }
    first[threadIdx.x] = before;
    if (threadIdx.x == 0) gbase = T ? atomicAdd(&br->count, T) : 0u;
    __syncthreads();
    if (T == 0) return;                                    // workgroup-uniform
    const uint32_t g0 = gbase;
    if (g0 + T > cap || g0 + T < g0) {                     // (the sum of all counts is below 2^31: n is)
        if (threadIdx.x == 0) br->overflow = 1u;
        return;                                            // the candidates will not be used
    }
#pragma unroll 4
    for (uint32_t k = threadIdx.x; k < T; k += SEL_CBLKS) {
        int t = 0;                                         // largest block with first[t] <= k
#pragma unroll
        for (int step = SEL_CBLKS / 2; step > 0; step >>= 1)
            if (first[t + step] <= k) t += step;
        cand[g0 + k] = zseg[(b0 + t) * 1024 + (k - first[t])];
    }
}

// decides whether the candidates hold both order statistics and prepares the state of whichever select runs next
__global__ void sel_bracket_fix_k(BrState* __restrict__ br, SelRun* __restrict__ run, unsigned long long k0, int same) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long less = br->less, cnt = br->count;
    const bool ok = br->overflow == 0 && less <= k0 && (k0 - less) < cnt && (same || (k0 + 1 - less) < cnt);
    br->ok = ok ? 1u : 0u;
    SelState z;
    z.rank = ok ? k0 - less : k0;
    z.less = 0; z.prefix = 0; z.need_next = 0; z.v0key = 0; z.pad = 0;
    run->st[0] = z;
    run->nan_count = ok ? br->nan : 0ull;                  // (the full passes count NaN themselves)
}

// one launch in front of a select: clears the histograms (and the bracket state), sets the ranks of up to 3 runs
__global__ __launch_bounds__(256) void sel_init_k(uint32_t* __restrict__ hist, int nwords, SelRun* __restrict__ runs,
                                                   int nruns, unsigned long long r0, unsigned long long r1,
                                                   unsigned long long r2, BrState* __restrict__ br,
                                                   uint32_t* __restrict__ also_zero, int64_t also_words) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nwords) hist[i] = 0;
    // words of the caller that must be zero before a LATER kernel of the same call (the fused filter's sweep state and
    // look-back words: a fill of their own sat on the critical path between the interpolation and the sweep)
    for (int64_t j = i; j < also_words; j += (int64_t)gridDim.x * 256) also_zero[j] = 0u;
    if (i < nruns) {
        SelRun z;
        memset(&z, 0, sizeof(z));
        z.st[0].rank = i == 0 ? r0 : (i == 1 ? r1 : r2);
        z.next_min = 0xFFFFFFFFu;
        runs[i] = z;
    }
    if (i == 0 && br) { BrState b; memset(&b, 0, sizeof(b)); *br = b; }
}

struct SelWs {
    float*    scal;     // 4 floats
    SelRun*   run;      // [0], [1]: the two ends of the sample bracket, [2]: the select proper
    uint32_t* hist;     // [3 runs][3 passes][SEL_BINS]
    // bracketed select (n >= SEL_BRACKET_MIN)
    BrState*  br;
    float    *sample, *cand;
    int64_t   ns;       // sample size
    uint32_t  cap;      // candidate capacity
    uint32_t* also_zero;   // optional: words sel_init clears for the caller (see sel_init_k)
    int64_t   also_words;
};
// a select over a plain column of n values: with its own sample bracket from SEL_BRACKET_MIN values on
static void sel_plan(Arena& a, SelWs& w, int64_t n = 0) {
    w.scal = a.take<float>(4);
    w.run = a.take<SelRun>(3);
    w.hist = a.take<uint32_t>(9 * SEL_BINS);
    w.br = nullptr; w.sample = w.cand = nullptr; w.ns = 0; w.cap = 0;
    w.also_zero = nullptr; w.also_words = 0;
    if (n >= SEL_BRACKET_MIN) {
        w.br = a.take<BrState>(1);
        w.ns = SEL_GROUP * (n / SEL_EVERY);
        w.sample = a.take<float>(w.ns);
        w.cap = (uint32_t)(n / 16) + 1024u;
        w.cand = a.take<float>(w.cap);
    }
}
// The fused filter's select where the centroid summary brackets the percentile (sel_collect_k): no sample, and larger
// candidate buffers - one sample per 1024 rows makes a wider bracket than sixteen in 1024 (bracket_ranks): a tenth of
// the column at 4 M rows and the 25th percentile, a third at 400 000.  Hence n/2 below 4 M rows and n/4 above; the
// 2 M values in between keep the plan monotone in n (a grow-only workspace is sized by it).
static void sel_plan_from_summary(Arena& a, SelWs& w, int64_t n) {
    sel_plan(a, w);
    const int64_t half = n / 2, quarter = n / 4, flat = SEL_BRACKET_MIN / 2;
    w.br = a.take<BrState>(1);
    w.cap = (uint32_t)(half < flat ? half : (quarter > flat ? quarter : flat)) + 1024u;
    w.cand = a.take<float>(w.cap);
}

// (np.percentile's index arithmetic, pct_index, lives in pch_select.h: the LAS-integer frame selects with it too)

// three histogram passes (+ the "next key" pass) on one SelRun; run and histograms are prepared by the caller
static int select_rounds(const float* base, int64_t n, int64_t stride, bool with_next, SelRun* run, uint32_t* hist,
                         hipStream_t s, SelGate gate, int64_t grid_n) {
    int64_t gb = ceil_div(grid_n, SEL_TILE);
    if (gb > 2048) gb = 2048;
    if (gb < 1) gb = 1;
    const dim3 grid((unsigned)gb), blk(256);
    PCH_LAUNCH("sel_hist0", (sel_hist_k<0, 1>), grid, blk, 0, s, base, n, stride, run, hist, gate);
    PCH_LAUNCH("sel_hist1", (sel_hist_k<1, 1>), grid, blk, 0, s, base, n, stride, run, hist, gate);
    PCH_LAUNCH("sel_hist2", (sel_hist_k<2, 1>), grid, blk, 0, s, base, n, stride, run, hist, gate);
    if (with_next) PCH_LAUNCH("sel_next", sel_next_k<>, grid, blk, 0, s, base, n, stride, run, hist, gate);
    return PCH_OK;
}

struct SelBracket { int64_t r_lo, r_hi; };
// bracket from a sample of ns values drawn in runs of `group` consecutive ones: ranks around k0 * ns / n, six sigma
// of the binomial rank error for ns / group independent draws + 0.2 % + 16
static SelBracket bracket_ranks(int64_t ns, int group, int64_t n, const PctIndex& pi) {
    const double p = (double)pi.k0 / (double)(n > 1 ? n - 1 : 1);
    const double sigma = sqrt(p * (1.0 - p) * (double)ns * (double)group);
    const int64_t margin = (int64_t)(6.0 * sigma) + ns / 500 + 16;
    const int64_t mid = (int64_t)(p * (double)(ns - 1));
    SelBracket r;
    r.r_lo = mid - margin < 0 ? 0 : mid - margin;
    r.r_hi = mid + margin > ns - 1 ? ns - 1 : mid + margin;
    return r;
}
static SelBracket select_bracket_ranks(const SelWs& w, int64_t n, const PctIndex& pi) {
    return bracket_ranks(w.ns, SEL_GROUP, n, pi);
}
// First half of the bracketed select of a plain column (>= SEL_BRACKET_MIN values, sample buffer planned): the sample
// and the two order statistics of it that bracket the ranks.
static int select_sample_passes(const float* base, int64_t n, double q_percent, SelWs& w, hipStream_t s) {
    const PctIndex pi = pct_index(n, q_percent);
    const SelGate always = {nullptr, nullptr, nullptr};
    const SelBracket br = select_bracket_ranks(w, n, pi);
    const int64_t ns = w.ns;
    PCH_LAUNCH("sel_init", sel_init_k, dim3((unsigned)ceil_div(9 * SEL_BINS, 256)), dim3(256), 0, s, w.hist,
               9 * SEL_BINS, w.run, 3, (unsigned long long)br.r_lo, (unsigned long long)br.r_hi, 0ull, w.br,
               w.also_zero, w.also_words);
    PCH_LAUNCH("sel_sample", sel_sample_k, dim3((unsigned)ceil_div(ns, 1024)), dim3(256), 0, s, base, ns, w.sample);
    int64_t gs = ceil_div(ns, SEL_TILE);                   // both ends of the bracket in the same three sweeps
    if (gs > 2048) gs = 2048;
    if (gs < 1) gs = 1;
    const dim3 grid((unsigned)gs), blk(256);
    PCH_LAUNCH("sel_hist0", (sel_hist_k<0, 2>), grid, blk, 0, s, (const float*)w.sample, ns, (int64_t)1, w.run, w.hist, always);
    PCH_LAUNCH("sel_hist1", (sel_hist_k<1, 2>), grid, blk, 0, s, (const float*)w.sample, ns, (int64_t)1, w.run, w.hist, always);
    PCH_LAUNCH("sel_hist2", (sel_hist_k<2, 2>), grid, blk, 0, s, (const float*)w.sample, ns, (int64_t)1, w.run, w.hist, always);
    return PCH_OK;
}

// the histogram / next passes (need only the raw values) ...
static int select_passes(const float* base, int64_t n, int64_t stride, double q_percent, SelWs& w, hipStream_t s) {
    const PctIndex pi = pct_index(n, q_percent);
    const SelGate always = {nullptr, nullptr, nullptr};
    SelRun* fin = w.run + 2;
    uint32_t* hfin = w.hist + 6 * SEL_BINS;
    if (!w.sample || stride != 1) {                          // (a sample is planned from SEL_BRACKET_MIN values on)
        PCH_LAUNCH("sel_init", sel_init_k, dim3((unsigned)ceil_div(9 * SEL_BINS, 256)), dim3(256), 0, s, w.hist,
                   9 * SEL_BINS, w.run, 3, 0ull, 0ull, (unsigned long long)pi.k0, (BrState*)nullptr, w.also_zero,
                   w.also_words);
        return select_rounds(base, n, stride, !pi.same, fin, hfin, s, always, n);
    }
    PCH_TRY(select_sample_passes(base, n, q_percent, w, s));
    const SelBracket br = select_bracket_ranks(w, n, pi);
    const int64_t ns = w.ns;
    // one resident round of workgroups: 32 KB of LDS each, five per CU (a 2048-workgroup grid ran as 1280 + 768:
    // 0.191 -> 0.177 ms).  Tried and dropped (round 3): one ballot per four values and 32-bit counters (no change: the
    // sweep is not bound by its arithmetic); per-wave staging without barriers + register prefetch (0.194 ms);
    // 2 KB of staging per wave for 8 workgroups per CU (0.266 ms: more waves streaming shorter runs each)
    int64_t gb = ceil_div(n, SEL_TILE);
    {
        static int per_round[PCH_MAX_DEVICES] = {};
        const int slot = current_device_slot();
        if (!per_round[slot]) {
            int dev = 0, cus = 256;
            if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
            per_round[slot] = cus * 5;
        }
        if (gb > per_round[slot]) gb = per_round[slot];
    }
    PCH_LAUNCH("sel_bracket", sel_bracket_k, dim3((unsigned)gb), dim3(256), 0, s, base, n, (const SelRun*)w.run, w.hist,
               br.r_lo == 0 ? 1 : 0, br.r_hi == ns - 1 ? 1 : 0, w.br, w.cand, w.cap);
    PCH_LAUNCH("sel_bracket_fix", sel_bracket_fix_k, dim3(1), dim3(64), 0, s, w.br, fin, (unsigned long long)pi.k0,
               pi.same);
    // exact select: on the candidates when the bracket holds, else over the whole column - the same launches either
    // way, the kernels pick their source from br->ok
    const SelGate src = {&w.br->ok, w.cand, &w.br->count};
    return select_rounds(base, n, stride, !pi.same, fin, hfin, s, src, n);
}
// The second half when the centroid summary bracketed the z of the rows (MsBracket, pch_mean.h; the caller has run
// sel_init_k): gather what it left, check it, and select - from the candidates, or if the check fails from the z of the
// (n,3) rows themselves (three passes over 12 B per row: exact and rare).
static int select_from_summary(const float* raw, int64_t n, double q_percent, const MsCand& mc, SelWs& w,
                               hipStream_t s) {
    const PctIndex pi = pct_index(n, q_percent);
    SelRun* fin = w.run + 2;
    const int64_t nblk = ceil_div(n, 1024);
    PCH_LAUNCH("sel_collect", sel_collect_k, dim3((unsigned)ceil_div(nblk, SEL_CBLKS)), dim3(SEL_CBLKS), 0, s,
               (const MsBracket*)mc.bracket, (const MsBrRec*)mc.brec, nblk, (const float*)mc.zseg, w.br, w.cand, w.cap);
    PCH_LAUNCH("sel_bracket_fix", sel_bracket_fix_k, dim3(1), dim3(64), 0, s, w.br, fin, (unsigned long long)pi.k0,
               pi.same);
    const SelGate src = {&w.br->ok, w.cand, &w.br->count};
    return select_rounds(raw + 2, n, 3, !pi.same, fin, w.hist + 6 * SEL_BINS, s, src, n);
}
// ... and the final interpolation, which is where `sub` (the centroid) enters
static int select_lerp(int64_t n, const float* sub, double q_percent, float add1, float add2, SelWs& w,
                       hipStream_t s) {
    const PctIndex pi = pct_index(n, q_percent);
    PCH_LAUNCH("sel_lerp", sel_lerp_k, dim3(1), dim3(256), 0, s, (const SelRun*)(w.run + 2),
               (const uint32_t*)(w.hist + 8 * SEL_BINS), pi.same ? 0 : 1, pi.same, pi.gamma, sub, add1, add2, w.scal);
    return PCH_OK;
}
static int select_percentile(const float* base, int64_t n, int64_t stride, const float* sub,
                             double q_percent, SelWs& w, hipStream_t s) {
    PCH_TRY(select_passes(base, n, stride, q_percent, w, s));
    return select_lerp(n, sub, q_percent, 0.0f, 0.0f, w, s);
}

// per-thread side stream + events: the fused filter's select only needs the raw z values (and what the summary left),
// so it runs beside the centroid's level 2 and 3-wave walk
struct SideStream { hipStream_t s; hipEvent_t ev_fork, ev_join, ev_start; bool ok; };
struct SideStreams {                                    // one per device this thread has used; gone with the thread
    SideStream ss[PCH_MAX_DEVICES];
    SideStreams() { for (auto& x : ss) x = {nullptr, nullptr, nullptr, nullptr, false}; }
    ~SideStreams() {
        if (!may_release_hip_objects()) return;
        for (auto& x : ss)
            if (x.ok) {
                (void)hipEventDestroy(x.ev_fork); (void)hipEventDestroy(x.ev_join);
                (void)hipEventDestroy(x.ev_start);
                (void)hipStreamDestroy(x.s);
            }
    }
};
static SideStream& side_stream() {
    static thread_local SideStreams all;
    SideStream& ss = all.ss[current_device_slot()];
    if (!ss.ok) {
        if (hipStreamCreateWithFlags(&ss.s, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&ss.ev_fork, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&ss.ev_join, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&ss.ev_start, hipEventDisableTiming) == hipSuccess)
            ss.ok = true;
    }
    return ss;
}

// =====================================================================================
// B2/B3: keep = (z - cz) > thr, order preserving, in ONE sweep over the z of the rows: every
// workgroup counts its tile, publishes the count and obtains its output offset by a decoupled
// look-back over the tiles in front of it (status word = 2-bit flag + 32-bit value, one 64-bit
// relaxed atomic), then writes the centred survivors and folds their bounding box into one of
// 64 slot sets.  The sweep runs with the first threshold (offset); only if that keeps fewer than
// min_keep points (utils/tower_extraction.py:87-89) a second sweep with the fallback threshold
// overwrites the output - its workgroups return at once otherwise (the last tile of the first sweep
// sets the switch).
// =====================================================================================
constexpr int GF_THREADS = 256;
constexpr int GF_ROUNDS  = 64;
constexpr int GF_TILE    = GF_THREADS * GF_ROUNDS;   // 16 384 points per workgroup: few enough tiles for the look-back

struct GfState {
    uint32_t total[2];                     // kept with threshold A (offset) / B (fallback)
    uint32_t use_b;
    uint32_t failed;                       // a look-back wait ran out of its budget (pch_lookback.h): count -> -1
    uint32_t ticket[2];                    // next logical tile of either sweep (order of arrival, see gf_compact_k)
    uint32_t pad2[2];
    uint32_t slots[2][OC_SLOTS][6];        // per sweep: ~min xyz (complemented) / max xyz as ordered uint32,
                                           // all folded with atomicMax so that 0 is the neutral start
};

// ---- the candidate rows of the summary pass (MsCand, pch_mean.h) -------------------------------------------------
// May the sweep read the candidate slots instead of the tile?  Only if no survivor can be missing from them.  A row
// survives iff fl(z - cz) > thr; the slots hold every row with z > tcand.  If tcand <= thr + cz (as real numbers: the
// double sum is exact while the two exponents are within 29 bits, and the test takes one step below it for when they
// are not), a row with z <= tcand has z - cz <= thr, and rounding is monotone with fl(thr) = thr, so
// fl(z - cz) <= thr: it does not survive.  The same test, on the same device words, decides in gf_cand_k (go) and in
// gf_compact_k (stand down), for both thresholds at once; a NaN anywhere fails it.
__device__ __forceinline__ bool gf_cand_ok(const float* __restrict__ tcand, const float* __restrict__ centroid,
                                           const float* __restrict__ scal) {
    if (!tcand) return false;
    if (reinterpret_cast<const uint32_t*>(tcand)[1] != 0u) return false;      // a slot overflowed (pch_mean.h)
    const double cz = (double)centroid[2];
    const double ta = (double)scal[1] + cz, tb = (double)scal[2] + cz;
    const double t = (double)*tcand;
    // the two sums are exact in double unless the exponents of threshold and centroid lie more than 29 bits apart;
    // one step below the (then rounded) sum is at or below the real sum either way
    return t <= nextafter(ta, -INFINITY) && t <= nextafter(tb, -INFINITY);
}

// ---- what the two sweeps share (gf_compact_k over the rows, gf_cand_k over the candidate slots): the tile order,
// the tile's output offset and what becomes of a survivor (its store and the fold of the tile's bounding box are those
// of pch_compact.h).  The logical tile is a ticket drawn on arrival, for the reason given at oc_take_tile.
// false: this sweep does not run (the fallback sweep without use_b).  The caller's next barrier publishes *tile_sh.
template <int WHICH>
__device__ __forceinline__ bool gf_take_tile(GfState* __restrict__ st, uint32_t* tile_sh) {
    if (WHICH == 1 && st->use_b == 0) return false;
    if (threadIdx.x == 0) *tile_sh = atomicAdd(&st->ticket[WHICH], 1u);
    return true;
}
// Wave 0 obtains the tile's exclusive prefix (T = the tile's count) and leaves it in *excl_sh for the caller's next
// barrier; the last tile records the sweep's total.
template <int WHICH>
__device__ __forceinline__ void gf_tile_prefix(GfState* __restrict__ st, uint64_t* __restrict__ status, int64_t tile,
                                               uint32_t T, long long min_keep, uint32_t* excl_sh) {
    if (wave_id() != 0) return;
    const uint32_t e0 = gf_lookback(status, tile, T);
    const bool lb_failed = e0 == GF_LB_FAILED;
    const uint32_t e = lb_failed ? 0u : e0;                  // prefix 0 keeps the survivors' writes inside the output
    if (lane_id() == 0) {
        *excl_sh = e;
        if (lb_failed) {
            atomicOr(&st->failed, 1u);
        } else if (tile == (int64_t)gridDim.x - 1) {         // the last tile knows the total: it also decides
            st->total[WHICH] = e + T;                        // whether the fallback threshold applies
            if (WHICH == 0) st->use_b = ((long long)(e + T) < min_keep) ? 1u : 0u;
        }
    }
}

template <int WHICH>
__global__ __launch_bounds__(GF_THREADS) void gf_compact_k(
    const float* __restrict__ raw, int64_t n, const float* __restrict__ centroid, const float* __restrict__ scal, GfState* __restrict__ st,
    uint64_t* __restrict__ status, long long min_keep, float* __restrict__ out_points,
    int32_t* __restrict__ out_index, const float* __restrict__ tcand) {
    if (gf_cand_ok(tcand, centroid, scal)) return;         // gf_cand_k does this sweep from the candidate slots
    __shared__ uint32_t wtot[GF_THREADS / 64];
    __shared__ uint32_t excl_sh;
    __shared__ uint32_t box[GF_THREADS / 64][6];
    __shared__ unsigned long long masks[GF_THREADS / 64][GF_ROUNDS];      // survivors of every 64-point round
    __shared__ uint32_t cum[GF_THREADS / 64][GF_ROUNDS + 1];
    __shared__ uint32_t tile_sh;
    if (!gf_take_tile<WHICH>(st, &tile_sh)) return;
    __syncthreads();
    const int64_t tile = tile_sh;
    const float cen[3] = {centroid[0], centroid[1], centroid[2]};
    const float cz = cen[2], thr = scal[1 + WHICH];
    const int w = wave_id(), l = lane_id();
    const int64_t seg = tile * GF_TILE + (int64_t)w * (64 * GF_ROUNDS);
    // ---- sweep over the z of the rows: survivor masks and the tile's count
    uint32_t run = 0;
#pragma unroll 8
    for (int r = 0; r < GF_ROUNDS; ++r) {
        const int64_t i = seg + r * 64 + l;
        const float z = i < n ? raw[3 * i + 2] : 0.0f;
        const bool keep = i < n && (z - cz) > thr;       // points = raw_points - centroid (float32)
        const unsigned long long m = __ballot(keep);
        if (l == 0) masks[w][r] = m;
        run += (uint32_t)__popcll(m);
    }
    if (l == 0) wtot[w] = run;
    {   // survivors in the rounds in front of round l (cum[w][64] = the wave's total)
        __builtin_amdgcn_wave_barrier();
        const uint32_t c = (uint32_t)__popcll(masks[w][l]);
        const uint32_t incl = wave_scan_incl(c);
        cum[w][l] = incl - c;
        if (l == 63) cum[w][64] = incl;
    }
    __syncthreads();
    const uint32_t T = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    gf_tile_prefix<WHICH>(st, status, tile, T, min_keep, &excl_sh);
    __syncthreads();
    if (T == 0) return;                                       // workgroup-uniform
    // ---- survivors: the row (one 12-byte load) is only fetched for them.  The wave's survivors are taken
    // DENSELY - lane j of pass d handles survivor 64 d + j of the wave, found through the per-round counts
    // and the position of its bit in the round's mask - so that every lane has a row in flight and
    // consecutive lanes write consecutive output rows (a pass over the 64 rounds with the ~10 % surviving
    // lanes active would leave most lanes idle and scatter the writes)
    struct Row3 { float x, y, z; };
    const uint32_t woff = oc_wave_offset(excl_sh, wtot, w);
    uint32_t lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};
    const uint32_t nw = wtot[w];
#pragma unroll 2
    for (uint32_t j = l; j < nw; j += 64) {
        int r = 0;                                             // largest round with cum[r] <= j
#pragma unroll
        for (int step = 32; step > 0; step >>= 1)
            if (cum[w][r + step] <= j) r += step;
        unsigned long long m = masks[w][r];
        uint32_t k = j - cum[w][r];                            // the k-th set bit of that round's mask
        int bit = 0;
        uint32_t word = (uint32_t)m;
        {
            const uint32_t c = (uint32_t)__popc(word);
            if (k >= c) { k -= c; word = (uint32_t)(m >> 32); bit = 32; }
        }
#pragma unroll
        for (int half = 16; half > 0; half >>= 1) {
            const uint32_t c = (uint32_t)__popc(word & ((1u << half) - 1u));
            if (k >= c) { k -= c; word >>= half; bit += half; }
        }
        const int64_t i = seg + r * 64 + bit;
        const Row3 q = reinterpret_cast<const Row3*>(raw)[i];
        oc_emit(q.x, q.y, q.z, cen, (int64_t)woff + j, i, out_points, out_index, lo, hi);
    }
    oc_fold_box(st->slots[WHICH], tile, lo, hi, box);
}

// The same sweep from the candidate slots (MsCand, pch_mean.h: four planes per 1024-row block): a workgroup takes 64
// slots, a wave 16 of them, round-major.  ~12 % of the rows are candidates and they lie contiguously, so the sweep
// reads 4 B per candidate to count and 16 B per candidate for the rows, instead of the z column plus one memory
// line per survivor.
constexpr int GF_CBLK = 1024;                          // rows per block of the summary
constexpr int GF_CSLOT = MS_CAND_SLOT;                 // candidate rows a slot holds
constexpr int GF_CT_BLKS = 64;                         // slots per workgroup: 65 536 rows of the tile (32 measured no
                                                       // faster; the ticket word hands out ~88 tiles per microsecond)
constexpr int GF_CW_BLKS = GF_CT_BLKS / (GF_THREADS / 64);     // 16 slots per wave

template <int WHICH>
__global__ __launch_bounds__(GF_THREADS, 6) void gf_cand_k(     // six waves per SIMD: every tile of a 100 M-point call resident
    const float* __restrict__ slots, const uint32_t* __restrict__ counts, const float* __restrict__ tcand,
    int64_t nblk, const float* __restrict__ centroid, const float* __restrict__ scal, GfState* __restrict__ st,
    uint64_t* __restrict__ status, long long min_keep, float* __restrict__ out_points,
    int32_t* __restrict__ out_index) {
    constexpr int NR = GF_CSLOT / 64;                      // rounds of 64 rows in a slot
    constexpr int64_t SLOT_WORDS = 4 * GF_CSLOT;           // planes x | y | z | row-in-block (MsCand, pch_mean.h)
    constexpr int NE = GF_CW_BLKS * NR;                    // (slot, round) pairs of a wave
    __shared__ uint32_t wtot[GF_THREADS / 64];
    __shared__ uint32_t excl_sh;
    __shared__ uint32_t box[GF_THREADS / 64][6];
    __shared__ unsigned long long masks[GF_THREADS / 64][NE];        // survivors of every (slot, round): 4 KB
    __shared__ uint32_t cum[GF_THREADS / 64][NE];                     // survivors of the wave in front of that pair
    __shared__ uint32_t tile_sh;
    static_assert(NE == 128, "two (slot, round) pairs per lane in the prefix below");
    if (!gf_cand_ok(tcand, centroid, scal)) return;        // gf_compact_k runs instead
    if (!gf_take_tile<WHICH>(st, &tile_sh)) return;
    const int w = wave_id(), l = lane_id();
    masks[w][2 * l] = 0ull;
    masks[w][2 * l + 1] = 0ull;
    __syncthreads();
    const int64_t tile = tile_sh;
    const float cen[3] = {centroid[0], centroid[1], centroid[2]};
    const float cz = cen[2], thr = scal[1 + WHICH];
    const int64_t b0 = tile * GF_CT_BLKS + (int64_t)w * GF_CW_BLKS;
    // Candidates come in runs: blocks next to a tower hold hundreds, most blocks fewer than 64 or none.  A slot after
    // the other is a chain of dependent memory round trips (the kernel waited 86 % of its wave cycles that way), so
    // the wave goes ROUND-major: round r of all its 16 slots at once - 16 independent loads in flight, of the z PLANE
    // alone in the counting phase (a quarter of the slot's bytes) - and usually one or two rounds are all there is.
    uint32_t ncs[GF_CW_BLKS];
    uint32_t maxnc = 0;
#pragma unroll
    for (int kb = 0; kb < GF_CW_BLKS; ++kb) {
        ncs[kb] = (b0 + kb) < nblk ? counts[b0 + kb] : 0u;
        maxnc = ncs[kb] > maxnc ? ncs[kb] : maxnc;
    }
    maxnc = (uint32_t)__builtin_amdgcn_readfirstlane((int)maxnc);      // (every lane read the same words)
    uint32_t run = 0;
#pragma unroll 1
    for (int r = 0; r < NR; ++r) {
        if ((uint32_t)(r * 64) >= maxnc) break;            // wave-uniform
        const uint32_t i = r * 64 + l;
        float z[GF_CW_BLKS];
#pragma unroll
        for (int kb = 0; kb < GF_CW_BLKS; ++kb) {
            z[kb] = 0.0f;
            if (i < ncs[kb]) z[kb] = slots[(b0 + kb) * SLOT_WORDS + 2 * GF_CSLOT + i];
        }
#pragma unroll
        for (int kb = 0; kb < GF_CW_BLKS; ++kb) {
            const bool keep = i < ncs[kb] && (z[kb] - cz) > thr;        // points = raw_points - centroid (float32)
            const unsigned long long m = __ballot(keep);
            if (l == 0 && m) masks[w][kb * NR + r] = m;
            run += (uint32_t)__popcll(m);
        }
    }
    if (l == 0) wtot[w] = run;
    __syncthreads();
    const uint32_t T = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    // eight slots at a time: with all sixteen rows in registers the kernel needs 130 VGPRs, and at three waves per
    // SIMD only half of the tiles are resident - two rounds of workgroups that each wait on the look-back
    constexpr int HB = GF_CW_BLKS / 2;
    const uint64_t lt = lanemask_lt();
    uint32_t lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};
    auto load_half = [&](int r, int half, float4 (&q)[HB], unsigned long long (&ms)[HB]) {
        const uint32_t i = r * 64 + l;
#pragma unroll
        for (int k = 0; k < HB; ++k) {                     // the four planes, survivors only
            const int kb = half * HB + k;
            ms[k] = masks[w][kb * NR + r];
            q[k].x = q[k].y = q[k].z = q[k].w = 0.0f;
            if ((ms[k] >> l) & 1ull) {
                const float* __restrict__ sp = slots + (b0 + kb) * SLOT_WORDS + i;
                q[k].x = sp[0]; q[k].y = sp[GF_CSLOT]; q[k].z = sp[2 * GF_CSLOT]; q[k].w = sp[3 * GF_CSLOT];
            }
        }
    };
    auto emit_half = [&](int r, int half, const float4 (&q)[HB], const unsigned long long (&ms)[HB], uint32_t woff) {
#pragma unroll
        for (int k = 0; k < HB; ++k) {
            const int kb = half * HB + k;
            const unsigned long long m = ms[k];
            if ((m >> l) & 1ull) {
                const float4 c4 = q[k];
                oc_emit(c4.x, c4.y, c4.z, cen, (int64_t)woff + cum[w][kb * NR + r] + (uint32_t)__popcll(m & lt),
                        (b0 + kb) * GF_CBLK + (int64_t)__float_as_uint(c4.w), out_points, out_index, lo, hi);
            }
        }
    };
    // the rows of the first half-batch are requested BEFORE the look-back: the loads need no output offset (only the
    // stores do), and a tile waits ~30 us for the tiles in front of it with nothing of its own in flight otherwise
    float4 q0[HB];
    unsigned long long ms0[HB];
    if (T != 0 && maxnc != 0) load_half(0, 0, q0, ms0);
    gf_tile_prefix<WHICH>(st, status, tile, T, min_keep, &excl_sh);
    {   // survivors of the wave in front of every (slot, round) pair, in file order = slot-major
        const uint32_t c0 = (uint32_t)__popcll(masks[w][2 * l]), c1 = (uint32_t)__popcll(masks[w][2 * l + 1]);
        const uint32_t incl = wave_scan_incl(c0 + c1);
        cum[w][2 * l] = incl - c0 - c1;
        cum[w][2 * l + 1] = incl - c1;
    }
    __syncthreads();
    if (T == 0) return;                                    // workgroup-uniform
    const uint32_t woff = oc_wave_offset(excl_sh, wtot, w);
    if (maxnc != 0) {
        emit_half(0, 0, q0, ms0, woff);
        {
            float4 q[HB];
            unsigned long long ms[HB];
            load_half(0, 1, q, ms);
            emit_half(0, 1, q, ms, woff);
        }
#pragma unroll 1
        for (int r = 1; r < NR; ++r) {
            if ((uint32_t)(r * 64) >= maxnc) break;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                float4 q[HB];
                unsigned long long ms[HB];
                load_half(r, half, q, ms);
                emit_half(r, half, q, ms, woff);
            }
        }
    }
    oc_fold_box(st->slots[WHICH], tile, lo, hi, box);
}

// publishes the scalars, the count and the bounding box of the sweep that counts
__global__ void gf_finalize_k(const GfState* __restrict__ st, const float* __restrict__ centroid,
                              const float* __restrict__ scal, float* __restrict__ out_scalars,
                              int64_t* __restrict__ out_count, float* __restrict__ out_aabb) {
    if (blockIdx.x != 0) return;
    const uint32_t use_b = st->use_b;
    if (threadIdx.x == 0) {
        out_scalars[0] = centroid[0];
        out_scalars[1] = centroid[1];
        out_scalars[2] = centroid[2];
        out_scalars[3] = scal[0];
        out_scalars[4] = scal[1 + use_b];
        out_scalars[5] = use_b ? 1.0f : 0.0f;
        out_scalars[6] = __uint_as_float(st->total[0]);   // kept at the first threshold: the uint32 count's BITS
        out_scalars[7] = 0.0f;
        *out_count = st->failed ? (int64_t)-1 : (int64_t)st->total[use_b];
    }
    if (threadIdx.x < 6 && out_aabb) out_aabb[threadIdx.x] = oc_box_word(st->slots[use_b], threadIdx.x);
}

struct GfWs {
    float*    centroid;
    MsWs      ms;
    SelWs     sel;
    GfState*  st;
    uint64_t* status;            // [2][tiles] look-back words of the two sweeps
    size_t    clear_bytes;       // st .. end of status: zeroed before the sweeps
    MsCand    cand;              // candidate rows and the percentile's bracket, emitted by the summary pass
};
// The percentile's bracket comes from the summary (MsBracket) wherever it emits candidate slots (ms_makes_cand); a
// cloud without them has the select read the z of the rows.  PCH_GF_BRACKET_INVALID fails the bracket's device check,
// so that the select of a large cloud reads the rows too.
static void gf_plan(Arena& a, int64_t n, GfWs& w) {
    const int64_t nb = ceil_div(n > 0 ? n : 1, GF_TILE);
    const bool bracket = ms_makes_cand(n);
    w.centroid = a.take<float>(4);
    ms_plan(a, n, w.ms);
    w.cand.zseg = bracket ? a.take<float>(n) : nullptr;    // one 1024-float segment per block of the summary
    if (bracket) sel_plan_from_summary(a, w.sel, n);
    else sel_plan(a, w.sel);
    const size_t st_off = a.off;
    w.st = a.take<GfState>(1);
    w.status = a.take<uint64_t>(2 * nb);
    w.clear_bytes = a.off - st_off;
    const int64_t nblk = ceil_div(n > 0 ? n : 1, GF_CBLK);
    w.cand.tcand = a.take<float>(4);
    w.cand.counts = a.take<uint32_t>(nblk);
    w.cand.zsample = a.take<float>(nblk);
    w.cand.slots = a.take<float>(nblk * 4 * MS_CAND_SLOT); // 8 KB per 1024-row block: four planes (MsCand)
    w.cand.pct = 0.0;
    w.cand.add = 0.0f;
    w.cand.bracket = bracket ? a.take<MsBracket>(1) : nullptr;
    w.cand.brec = bracket ? a.take<MsBrRec>(nblk) : nullptr;
    w.cand.r_lo = w.cand.r_hi = 0;
    w.cand.force_invalid = 0;
}

}  // namespace pch

using namespace pch;

extern "C" size_t pch_percentile_f32_ws_bytes(int64_t n) {
    Arena a;
    SelWs w;
    sel_plan(a, w, n);
    return a.off;
}

extern "C" int pch_percentile_f32(const float* base, int64_t n, int64_t stride, const float* sub,
                                  double q_percent, float* out, void* ws, size_t ws_bytes,
                                  void* stream) {
    PCH_DEVICE_GUARD(base);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n >= 1, "percentile of an empty array (numpy raises IndexError)");
    PCH_REQUIRE(base && out && ws && stride >= 1, "bad argument");
    PCH_REQUIRE(q_percent >= 0.0 && q_percent <= 100.0, "Percentiles must be in the range [0, 100]");
    Arena a(ws, ws_bytes);
    SelWs w;
    sel_plan(a, w, n);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    PCH_TRY(select_percentile(base, n, stride, sub, q_percent, w, s));
    PCH_HIP_TRY(hipMemcpyAsync(out, w.scal, sizeof(float), hipMemcpyDeviceToDevice, s));
    return PCH_OK;
}

// ---- the select passes one at a time, for a percentile over values that are spread over several GPUs
// (tiles.shared_percentile: every rank histograms its part, the histograms are all-reduced, the host picks
// the bin).  They launch the kernels of pch_percentile_f32 without the pick prologue (PICK = false; the host
// does the picks): same kernels, same arithmetic, same result as pch_percentile_f32 over the concatenation.
extern "C" int pch_select_hist_f32(const float* base, int64_t n, int64_t stride, int32_t pass, uint32_t prefix,
                                   uint32_t* out_hist, unsigned long long* out_nan, void* ws, size_t ws_bytes,
                                   void* stream) {
    PCH_DEVICE_GUARD(out_hist);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n >= 0 && stride >= 1 && pass >= 0 && pass <= 2 && out_hist && ws, "bad argument");
    PCH_REQUIRE(n == 0 || base, "null input");
    Arena a(ws, ws_bytes);
    SelWs w;
    sel_plan(a, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    SelRun h;
    memset(&h, 0, sizeof(h));
    h.st[pass].prefix = prefix;                          // (pass 0 has no prefix)
    uint32_t* hist = sel_hist_of(w.hist, 0, pass);
    PCH_HIP_TRY(hipMemcpyAsync(w.run, &h, sizeof(h), hipMemcpyHostToDevice, s));
    PCH_HIP_TRY(hipMemsetAsync(hist, 0, sizeof(uint32_t) * SEL_BINS, s));
    if (n > 0) {
        int64_t gb = ceil_div(n, SEL_TILE);
        if (gb > 2048) gb = 2048;
        const dim3 grid((unsigned)gb), blk(256);
        const SelGate always = {nullptr, nullptr, nullptr};
        if (pass == 0)
            PCH_LAUNCH("sel_hist0", (sel_hist_k<0, 1>), grid, blk, 0, s, base, n, stride, w.run, w.hist, always);
        else if (pass == 1)
            PCH_LAUNCH("sel_hist1", (sel_hist_k<1, 1, false>), grid, blk, 0, s, base, n, stride, w.run, w.hist, always);
        else
            PCH_LAUNCH("sel_hist2", (sel_hist_k<2, 1, false>), grid, blk, 0, s, base, n, stride, w.run, w.hist, always);
    }
    PCH_HIP_TRY(hipMemcpyAsync(out_hist, hist, sizeof(uint32_t) * SEL_BINS, hipMemcpyDeviceToDevice, s));
    if (out_nan)
        PCH_HIP_TRY(hipMemcpyAsync(out_nan, &w.run->nan_count, sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    PCH_HIP_TRY(hipStreamSynchronize(s));               // `h` lives on this stack frame
    return PCH_OK;
}

extern "C" int pch_select_min_above_f32(const float* base, int64_t n, int64_t stride, uint32_t key,
                                        uint32_t* out_key, void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(out_key);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n >= 0 && stride >= 1 && out_key && ws, "bad argument");
    PCH_REQUIRE(n == 0 || base, "null input");
    Arena a(ws, ws_bytes);
    SelWs w;
    sel_plan(a, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    SelRun h;
    memset(&h, 0, sizeof(h));
    h.st[3].need_next = 1;
    h.st[3].v0key = key;
    h.next_min = 0xFFFFFFFFu;
    PCH_HIP_TRY(hipMemcpyAsync(w.run, &h, sizeof(h), hipMemcpyHostToDevice, s));
    if (n > 0) {
        int64_t gb = ceil_div(n, SEL_TILE);
        if (gb > 2048) gb = 2048;
        const SelGate always = {nullptr, nullptr, nullptr};
        PCH_LAUNCH("sel_next", sel_next_k<false>, dim3((unsigned)gb), dim3(256), 0, s, base, n, stride, w.run, w.hist,
                   always);
    }
    PCH_HIP_TRY(hipMemcpyAsync(out_key, &w.run->next_min, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    PCH_HIP_TRY(hipStreamSynchronize(s));
    return PCH_OK;
}

// ---- keep = (z - cz) > threshold with GIVEN centroid and threshold (the shared values of a tiled run);
// same sweep and same finish as the fused filter
constexpr int FGT_FLOATS = 16;    // first block of the workspace: centroid[4], scal[4], gf_finalize_k's scalars[8]
extern "C" size_t pch_filter_gt_ws_bytes(int64_t n) {
    if (n < 0) return 0;
    Arena a;
    a.take<float>(FGT_FLOATS);
    a.take<GfState>(1);
    a.take<uint64_t>(2 * ceil_div(n > 0 ? n : 1, GF_TILE));
    return a.off;
}

extern "C" int pch_filter_gt_f32(const float* raw, int64_t n, const float* centroid3_host, float threshold,
                                 float* out_points, int32_t* out_index, int64_t* out_count, float* out_aabb,
                                 void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(out_count);
    hipStream_t s = (hipStream_t)stream;
    PCH_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && centroid3_host && out_count && ws, "bad argument");
    if (n == 0) {
        PCH_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(int64_t), s));
        return PCH_OK;
    }
    PCH_REQUIRE(raw && out_points, "null buffer");
    Arena a(ws, ws_bytes);
    float* f = a.take<float>(FGT_FLOATS);
    const size_t st_off = a.off;
    GfState* st = a.take<GfState>(1);
    const int64_t nb = ceil_div(n, GF_TILE);
    uint64_t* status = a.take<uint64_t>(2 * nb);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    // the words the fused filter computes on the device: centroid[3], -, then scal = base, threshold A, threshold B, -.
    // With min_keep 0 sweep A never raises use_b, so gf_finalize_k reports sweep A; its scalars land in the workspace
    const float hs[8] = {centroid3_host[0], centroid3_host[1], centroid3_host[2], 0.0f, 0.0f, threshold, threshold, 0.0f};
    PCH_HIP_TRY(hipMemcpyAsync(f, hs, sizeof(hs), hipMemcpyHostToDevice, s));
    PCH_HIP_TRY(hipMemsetAsync(st, 0, a.off - st_off, s));
    const float* centroid = f;
    const float* scal = f + 4;
    // the sweep reads z straight from the rows (a pass that first copied the z column out - 16 B per point of traffic
    // for a 12 B per point sweep - is gone)
    PCH_LAUNCH("gf_compact", gf_compact_k<0>, dim3((unsigned)nb), dim3(GF_THREADS), 0, s, raw, n, centroid, scal, st, status, (long long)0, out_points, out_index, (const float*)nullptr);
    PCH_LAUNCH("gf_finalize", gf_finalize_k, dim3(1), dim3(64), 0, s, (const GfState*)st, centroid, scal,
               f + 8, out_count, out_aabb);
    PCH_HIP_TRY(hipStreamSynchronize(s));               // `hs` lives on this stack frame
    return PCH_OK;
}

extern "C" size_t pch_ground_filter_ws_bytes(int64_t n) {
    if (n < 0) return 0;
    Arena a;
    GfWs w;
    gf_plan(a, n, w);
    return a.off;
}

extern "C" int pch_ground_filter_f32(const float* raw, int64_t n, double pct, float offset,
                                     float fallback_offset, int64_t min_keep, float* out_points,
                                     int32_t* out_index, float* out_scalars, int64_t* out_count,
                                     float* out_aabb, void* ws, size_t ws_bytes, void* stream) {
    PCH_DEVICE_GUARD(raw);
    return pch::ground_filter_run(raw, n, pct, offset, fallback_offset, min_keep, out_points, out_index, out_scalars,
                                  out_count, out_aabb, ws, ws_bytes, (hipStream_t)stream, nullptr);
}

int pch::ground_filter_run(const float* raw, int64_t n, double pct, float offset, float fallback_offset,
                           int64_t min_keep, float* out_points, int32_t* out_index, float* out_scalars,
                           int64_t* out_count, float* out_aabb, void* ws, size_t ws_bytes, hipStream_t s,
                           GfFollowUp* early) {
    PCH_REQUIRE(n >= 1 && n < (int64_t(1) << 31), "n out of range [1, 2^31) (numpy raises on empty input)");
    PCH_REQUIRE(raw && out_points && out_scalars && out_count && ws, "null buffer");
    PCH_REQUIRE(pct >= 0.0 && pct <= 100.0, "Percentiles must be in the range [0, 100]");
    Arena a(ws, ws_bytes);
    GfWs w;
    gf_plan(a, n, w);
    if (a.overflow) { set_error("workspace too small: need %zu bytes", a.off); return PCH_ERR_WORKSPACE; }
    const int64_t nb = ceil_div(n, GF_TILE);

    // candidate rows for the sweep: raw z above (estimated percentile + the smaller offset - 0.5 m), emitted by the summary
    w.cand.pct = pct;
    w.cand.add = (offset < fallback_offset ? offset : fallback_offset) - 0.5f;
    bool cand_made = false;
    // the sweep's state and look-back words are cleared by the select's init kernel (first thing on the side stream)
    w.sel.also_zero = reinterpret_cast<uint32_t*>(w.st);
    w.sel.also_words = (int64_t)(w.clear_bytes / 4);
    SideStream& ss = side_stream();
    // Two strands.  `s`: summary, level 2, walk - no cross-stream hop inside the chain (a large cloud's summary comes
    // in slices, and the walk of all but the last slice runs on a third stream beside it: mean_seq_launch).  Side
    // stream: at once the select's init kernel, then - behind the summary - the exact select; joined in front of the interpolation
    // (measured: the other assignment, select on `s` and walk on the side stream, loses 45 us to the hops).  Without a
    // side stream the select follows the walk on `s`.
    // Where the summary emits candidate slots it brackets the percentile too (MsBracket, pch_mean.h) and the select
    // gathers the blocks' values (sel_collect_k); a cloud without them has the three passes read the z of the rows.
    const bool bracket = ms_makes_cand(n);
    const PctIndex pi = pct_index(n, pct);
    static const bool invalid = getenv("PCH_GF_BRACKET_INVALID") != nullptr;       // tuning toggle
    const int64_t nblk = ceil_div(n, GF_CBLK);
    const SelBracket r = bracket_ranks(ceil_div(nblk, ms_bracket_stride(nblk)), 1, n, pi);   // (used with the bracket)
    w.cand.r_lo = r.r_lo;
    w.cand.r_hi = r.r_hi;
    w.cand.force_invalid = invalid ? 1 : 0;
    const hipStream_t sel_s = ss.ok ? ss.s : s;
    if (ss.ok) {
        PCH_HIP_TRY(hipEventRecord(ss.ev_start, s));            // everything the caller queued before this call
        PCH_HIP_TRY(hipStreamWaitEvent(ss.s, ss.ev_start, 0));   // (the rows; the previous user of the workspace)
    }
    // (the rank is that of the rows' select; with the bracket sel_bracket_fix_k sets it again)
    PCH_LAUNCH("sel_init", sel_init_k, dim3((unsigned)ceil_div(9 * SEL_BINS, 256)), dim3(256), 0, sel_s, w.sel.hist,
               9 * SEL_BINS, w.sel.run, 3, 0ull, 0ull, (unsigned long long)pi.k0, w.sel.br, w.sel.also_zero,
               w.sel.also_words);
    MsLaunch ml;
    ml.ev_summary = ss.ok ? ss.ev_fork : nullptr;
    ml.cand = &w.cand;
    ml.cand_made = &cand_made;
    ml.may_slice = true;
    PCH_TRY(mean_seq_launch(raw, n, w.centroid, w.ms, nullptr, s, ml));
    PCH_REQUIRE(!bracket || cand_made, "bracket route without candidate slots");
    if (ss.ok) PCH_HIP_TRY(hipStreamWaitEvent(ss.s, ss.ev_fork, 0));
    if (bracket) {
        PCH_TRY(select_from_summary(raw, n, pct, w.cand, w.sel, sel_s));
    } else {
        const SelGate always = {nullptr, nullptr, nullptr};
        PCH_TRY(select_rounds(raw + 2, n, 3, !pi.same, w.sel.run + 2, w.sel.hist + 6 * SEL_BINS, sel_s, always, n));
    }
    if (ss.ok) {
        PCH_HIP_TRY(hipEventRecord(ss.ev_join, ss.s));
        PCH_HIP_TRY(hipStreamWaitEvent(s, ss.ev_join, 0));
    }
    PCH_TRY(select_lerp(n, w.centroid + 2, pct, offset, fallback_offset, w.sel, s));
    const dim3 grid((unsigned)nb), blk(GF_THREADS);
    const float* tcand = cand_made ? (const float*)w.cand.tcand : (const float*)nullptr;
    // Sweep A (first threshold) from the candidate slots when the device-side guard allows it (gf_cand_ok), else over
    // the tile - one of the two kernels returns at once; same tiles, same tickets, same look-back words.  Then the
    // results are published ONCE ALREADY (gf_finalize; and queued for the host if the caller asked): they are final
    // unless the last tile of sweep A raised use_b.  Sweep B (fallback threshold) and the second gf_finalize follow;
    // without use_b they return at once, and the host is by then preparing the next stage.
    const dim3 cgrid((unsigned)ceil_div(nblk, GF_CT_BLKS));
    if (cand_made)
        PCH_LAUNCH("gf_cand", gf_cand_k<0>, cgrid, blk, 0, s, (const float*)w.cand.slots, (const uint32_t*)w.cand.counts,
                   tcand, nblk, (const float*)w.centroid, (const float*)w.sel.scal, w.st, w.status, (long long)min_keep,
                   out_points, out_index);
    PCH_LAUNCH("gf_compact", gf_compact_k<0>, grid, blk, 0, s, raw, n, (const float*)w.centroid,
               (const float*)w.sel.scal, w.st, w.status, (long long)min_keep, out_points, out_index, tcand);
    GfFollowUp fu = {cand_made, cgrid, grid, (const float*)w.cand.slots, (const uint32_t*)w.cand.counts, tcand, nblk, raw, n,
                     (const float*)w.centroid, (const float*)w.sel.scal, w.st, w.status + nb, (long long)min_keep,
                     out_points, out_index, out_scalars, out_count, out_aabb};
    if (early) {                                        // the caller queues the rest when the first results ask for it
        PCH_LAUNCH("gf_finalize", gf_finalize_k, dim3(1), dim3(64), 0, s, (const GfState*)w.st,
                   (const float*)w.centroid, (const float*)w.sel.scal, out_scalars, out_count, out_aabb);
        *early = fu;
        return PCH_OK;
    }
    return ground_filter_follow_up(fu, s);
}

int pch::ground_filter_follow_up(const GfFollowUp& f, hipStream_t s) {
    const dim3 blk(GF_THREADS);
    GfState* const st = static_cast<GfState*>(f.st);
    if (f.cand_made)
        PCH_LAUNCH("gf_cand_fb", gf_cand_k<1>, f.cgrid, blk, 0, s, f.slots, f.counts, f.tcand, f.nblk, f.centroid, f.scal,
                   st, f.status_fb, f.min_keep, f.out_points, f.out_index);
    PCH_LAUNCH("gf_compact_fb", gf_compact_k<1>, f.grid, blk, 0, s, f.raw, f.n, f.centroid, f.scal, st, f.status_fb,
               f.min_keep, f.out_points, f.out_index, f.tcand);
    PCH_LAUNCH("gf_finalize", gf_finalize_k, dim3(1), dim3(64), 0, s, (const GfState*)st, f.centroid, f.scal,
               f.out_scalars, f.out_count, f.out_aabb);
    return PCH_OK;
}
