// Bit-exact parallel evaluation of numpy's sequential float32 column mean (pch_mean.hip).
#pragma once
#include "pch_common.h"

namespace pch {

struct MsHdr;
struct MsRec;
struct MsPred;
// Candidate rows for the height filter, emitted by the summary pass while it has the rows in LDS anyway (pch_filter.hip,
// gf_cand_k): rows whose RAW z exceeds `tcand`, a deliberately low estimate of the filter's threshold.
//   slots  [nb][4][MS_CAND_SLOT] words: four PLANES per block - x, y, z and the bits of the row's index inside its
//          1024-row block - file order inside a block.  Planes, not float4 rows: the sweep first counts survivors
//          from the z plane alone (a quarter of the bytes) and then reads the rows once; as rows it pulled every line
//          twice (0.55 GB for 0.35 GB of necessary traffic).  A slot holds half of its block: typical data keeps ~10 % of the rows (a block next to a tower in
//          flight-line order more), and slots that are 8 KB apart instead of 16 KB are what makes their reads and writes stream; a block with more candidates
//          raises the overflow word and the sweep then reads the tile as before
//   counts [nb]       rows used in every slot
//   tcand  [2]        [0] the threshold that was used (device; written before the summary runs), [1] overflow word
constexpr int MS_CAND_SLOT = 512;
// The percentile's bracket, taken from the same samples in front of the summary (ms_prefix_k, ms_zbracket): two exact
// order statistics of every `stride`-th sampled z as sel_key keys L <= H.  With it the summary keeps, per block, the
// z values whose key lies in [L, H] packed at the front of the block's own 1024-float segment of MsCand::zseg
// (zseg[1024 * blk ...]: as large as the block, so it cannot overflow; order inside a block is not kept) and one
// MsBrRec.  sel_collect_k (pch_filter.hip) gathers them; whether they hold the wanted order statistics is checked on
// the device there, so the keys only decide how much is read.
struct MsBracket {
    uint32_t L, H;               // as used: 0 / 0xFFFFFFFF at an open end
    uint32_t lo_is_min, hi_is_max;
    uint32_t valid[2];           // one word per end (two workgroups write them): a NaN sample or none clears it
    uint32_t pad[2];
};
struct MsBrRec { uint32_t count_less, nan; };       // count | less << 16 (both <= 1024), NaN values of the block
constexpr int MS_BR_PER = 16;                       // samples a thread of ms_zbracket holds in registers
__host__ __device__ inline int64_t ms_bracket_stride(int64_t ns) {      // every stride-th sample: at most 16 384 of them
    const int64_t s = (ns + 1024 * MS_BR_PER - 1) / (1024 * MS_BR_PER);
    return s < 1 ? 1 : s;
}
// order-preserving key of the select (NaN sorts last, as in numpy's partition)
__device__ __forceinline__ uint32_t sel_key(float v) {
    return (v != v) ? 0xFFFFFFFFu : f32_ordered(v);
}
struct MsCand {
    float*    slots;
    uint32_t* counts;
    float*    tcand;
    float*    zsample;           // [nb] one sampled z per block (scratch of the estimate)
    double    pct;               // the percentile the filter will ask for
    float     add;               // tcand = (estimated percentile of z) + add
    // bracket emission (optional: bracket == nullptr emits none)
    MsBracket* bracket;
    MsBrRec*   brec;             // [nb], every record rewritten by every call
    float*     zseg;             // [n] the blocks' segments: what lies behind a block's front is stale and never read
    int64_t    r_lo, r_hi;       // ranks of L and H among the ceil(nb / ms_bracket_stride(nb)) samples used
    int        force_invalid;    // tuning toggle: valid = 0, whatever the sample holds
};
struct MsWs {
    MsPred*    pred;             // [3][nb2] estimated running sum in front of every level-2 row (candidate windows)
    int*       stats;            // [3][4]: level-2 batches, -, exactly added blocks, descents
    MsRec*     rec;              // [3][nb] level-1 records (three 128-byte lines per column and block)
    MsHdr*     hdr2;
    long long* rows2;
};
void ms_plan(Arena& a, int64_t n, MsWs& w);
// centroid[3] = np.mean(xyz, axis=0) (float32).  zcol (optional, n floats) receives a copy of
// the z column, written by the same pass that reads the tile.
// ev_summary (optional) is recorded on `s` right behind the summary, the pass that writes zcol and the candidates.
// sum_in (optional, device float[3]): running sum to continue instead of +0.0; divide_n: MS_DIVIDE_BY_N (the
// mean of these n rows), MS_NO_DIVIDE (out = the running sum after the rows) or the row count to divide by.
// phase: both kernels groups (default), only the tables (summary + level 2: they do not depend on sum_in), or only
// the walk over tables an earlier call left in `w`.
constexpr int64_t MS_DIVIDE_BY_N = -1, MS_NO_DIVIDE = -2;
constexpr int MS_PHASE_BOTH = 0, MS_PHASE_TABLES = 1, MS_PHASE_WALK = 2;
// cand (optional): emit the candidate rows described above; *cand_made says whether they were (needs the sampled
// estimate, i.e. more than 65 536 rows - a second group of 64 blocks - and prediction enabled): ms_makes_cand(n) tells
// beforehand.
// With cand->bracket the z values inside the bracket go to the fronts of cand->zseg's segments.
// may_slice (phase both, no sum_in): a large cloud - or any, with pch_mean_set_slices - is summarised in file-order
// slices, and level 2 and the walk of every slice but the last run on a stream of their own beside the summary of
// the next one (pch_mean.hip, "the centroid in file-order slices").  ev_summary is then recorded behind the last
// slice.  Same tables, same result.
bool ms_makes_cand(int64_t n);
struct MsLaunch {                // the optional arguments described above
    hipEvent_t    ev_summary = nullptr;
    const float*  sum_in = nullptr;
    int64_t       divide_n = MS_DIVIDE_BY_N;
    int           phase = MS_PHASE_BOTH;
    const MsCand* cand = nullptr;
    bool*         cand_made = nullptr;
    bool          may_slice = false;
};
int mean_seq_launch(const float* xyz, int64_t n, float* out, MsWs& w, float* zcol, hipStream_t s,
                    const MsLaunch& opt = MsLaunch());

}  // namespace pch
