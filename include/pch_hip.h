/*
 * pch_hip.h -- C ABI of libpch_hip.so: the MI355X (gfx950) implementation of the
 * pointcloudhookup ground-removal + tower-clustering hot path.
 *
 * The reference (Daniel-Starr/pointcloudhookup) is pure Python; the arithmetic of its
 * hot path lives in library calls (Open3D, numpy, scikit-learn).  Every entry point
 * below replaces exactly one of those call sites (cited as reference file:line), so the
 * reference's Python modules can bind them with ctypes.
 *
 * Conventions
 *  - plain C: pointers, sizes, scalars.  No torch/HIP types in signatures
 *    (`stream` is a hipStream_t passed as void*; NULL = default stream).
 *  - every `const T*` / `T*` argument is a DEVICE pointer unless its name ends in
 *    `_host`.  Buffers are caller-owned.  Every entry point looks up the device that owns
 *    its first buffer (hipPointerGetAttributes), makes it current for the call
 *    (hipSetDevice) and restores the caller's device on return; a host pointer where a
 *    device pointer is expected gives PCH_ERR_ARG.
 *  - return value: 0 = ok, <0 = PCH_ERR_*.  pch_last_error() gives a thread-local text.
 *  - the library never allocates device memory: scratch is a caller-provided workspace
 *    whose size comes from the matching *_ws_bytes() (a pure host function).
 *  - entry points enqueue work on `stream` and return without synchronising, except the
 *    ones documented "synchronises" (they must read a device-side count to size the next
 *    launch).
 *  - results are bit-exact restatements of the reference's arithmetic: the library is
 *    built with -ffp-contract=off; float64 division is IEEE.
 */
#ifndef PCH_HIP_H
#define PCH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCH_VERSION 300

#define PCH_OK               0
#define PCH_ERR_ARG         -1   /* bad argument (null pointer, negative size, eps<=0 ...) */
#define PCH_ERR_WORKSPACE   -2   /* workspace too small */
#define PCH_ERR_HIP         -3   /* a HIP runtime call failed */
#define PCH_ERR_RANGE       -4   /* grid does not fit the 64-bit cell/voxel key */
#define PCH_ERR_NODEVICE    -5   /* no gfx950 device visible */
#define PCH_ERR_TIMEOUT     -6   /* a device-side wait between workgroups ran out of its budget (see below) */

/* Device-side waits are bounded.  The order-preserving compactions (pch_ground_filter_f32, pch_filter_gt_f32,
 * pch_filter_plane_f32, pch_crop_aabb_f64, pch_crop_boxes_f64) and the voxel finisher (pch_voxel_downsample_f64) chain their workgroups by a single-pass
 * look-back: a workgroup polls the status words of the workgroups in front of it.  Every such poll loop has a
 * wall-clock budget (4 s); a workgroup that exceeds it gives up, the kernel drains, and the call's count word
 * (*out_count / *out_m, device memory) reads NEGATIVE instead of holding a count - the outputs are then
 * undefined.  Entry points that read the count on the host themselves (pch_tower_clusters_f32) return
 * PCH_ERR_TIMEOUT; callers of the asynchronous entry points must test the sign when they read the count
 * (pointcloudhookup_amd/ops.py does and raises).  Nothing in normal operation comes near the budget: it exists
 * so that a GPU shared with other processes can never be left with a resident spinning grid. */

int         pch_version(void);
const char* pch_last_error(void);
/* number of visible HIP devices (0 if none); does not initialise a context */
int         pch_device_count(void);

/* ------------------------------------------------------------------ stage A
 * Open3D PointCloud.voxel_down_sample applied per file-order chunk.
 * Replaces: ui/import_PC.py:8-13 (process_chunk) inside the loop ui/import_PC.py:45-58
 *           (twin: ui/Sampling.py:10-18,46-60).
 * xyz        [n,3] float64, row-major
 * chunk_size points per chunk (<=0: one chunk); every chunk has its own grid origin
 *            min(chunk) - voxel/2; duplicates across chunks are kept (as the reference).
 * out_idx    [n,3] int32   voxel index triplets   } capacity n rows, the first *out_m rows
 * out_mean   [n,3] float64 sum(points in order)/count } are valid; rows are grouped by chunk
 * out_count  [n]   int32                           } (order inside a chunk: see below)
 * Order inside a chunk: Open3D emits unordered_map iteration order, i.e. unspecified; parity is the SET of
 * (index, mean, count) per chunk.  This library emits coarse grid cells (the top bits of [ix|iy|iz]) in ascending
 * order and, inside a cell, the voxels in the order of their first points - or sorted by (ix,iy,iz) where a cell
 * takes the sorting path (dense cells, wide keys).  Deterministic for a given input and build, but not stable across
 * versions of this library; pch_voxel_canonical_order below gives an order that depends on the input alone.
 * out_chunk_offsets [nchunks+1] int64 (may be NULL): slice of each chunk in the output
 * out_m      [1] int64 number of voxels
 */
size_t pch_voxel_downsample_ws_bytes(int64_t n, int64_t chunk_size);
int pch_voxel_downsample_f64(const double* xyz, int64_t n, double voxel_size,
                             int64_t chunk_size,
                             int32_t* out_idx, double* out_mean, int32_t* out_count,
                             int64_t* out_chunk_offsets, int64_t* out_m,
                             void* ws, size_t ws_bytes, void* stream);

/* Opt-in canonical order: the rows pch_voxel_downsample_f64 wrote, with every chunk's slice sorted ascending by
 * (ix, iy, iz) - the order of oracle/voxel.py, a function of the input alone.  Everything downstream that depends on
 * row order (the sequential float32 centroid and the DBSCAN chunk split of stage B/C, read from point_2.las) is then
 * the same for every version and tuning of the voxel stage.
 * idx [m,3] int32 (every index >= 0), mean [m,3] float64, count [m] int32, chunk_offsets [nchunks+1] int64 with
 * chunk_offsets[0] == 0 and chunk_offsets[nchunks] == m (anything else: PCH_ERR_ARG), nchunks >= 1.
 * out_idx / out_mean / out_count: the same rows reordered; buffers distinct from the inputs, 16-byte aligned.
 * out_perm [m] int32 (may be NULL): source row of every output row.  chunk_offsets holds for the outputs unchanged.
 * No voxel index repeats inside a chunk of the stage's output; if one does, the repeats keep their input order.
 * One device-wide stable radix sort on the bits in use of [chunk | ix | iy | iz]; two sorts (the voxel fields, then
 * the chunk of the permuted rows) where that key is wider than 64 bits.  m == 0 is success; m >= 2^31 is
 * PCH_ERR_RANGE.  Host reads: ONE - four words behind the reduction over idx (the largest index per axis, which
 * fixes the number of sort passes, and the check of chunk_offsets); the host waits for that copy only, everything
 * behind it is enqueued without synchronising. */
size_t pch_voxel_canonical_order_ws_bytes(int64_t m, int64_t nchunks);
int pch_voxel_canonical_order(const int32_t* idx, const double* mean, const int32_t* count,
                              const int64_t* chunk_offsets, int64_t nchunks, int64_t m,
                              int32_t* out_idx, double* out_mean, int32_t* out_count,
                              int32_t* out_perm /* may be NULL: source row of every output row */,
                              void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ LAS files (native reader / writer)
 * What laspy does for the reference on the hot path, done by the library itself (host C++ + one decode
 * kernel): read the public header block; read the X, Y, Z integers of a record range straight into a
 * DEVICE buffer (memory-mapped file -> pinned double buffer -> H2D copy overlapped with the decode);
 * write a LAS file whose records carry X, Y, Z and zeros elsewhere (what laspy writes for a LasData whose
 * only assigned dimensions are x, y, z).  LAS 1.0-1.4, point formats 0-10, uncompressed; VLRs, extra bytes
 * and padding in front of the point data are skipped through header_size / offset_to_points /
 * record_length.
 * Replaces: laspy.read(...) / laspy.open(...).read() (ui/import_PC.py:28, utils/tower_extraction.py:60-61,
 *           ui/extract.py:114-115); LasHeader / LasData(...).write (ui/import_PC.py:35-42,64-65,
 *           utils/tower_extraction.py:243-257).  Both synchronise `stream` before returning. */
typedef struct PchLasHeader {
    uint8_t  version_major, version_minor, point_format, reserved0;
    uint16_t header_size, record_length;
    uint32_t offset_to_points, num_vlrs;
    uint64_t point_count;
    double   scales[3], offsets[3], mins[3], maxs[3];
} PchLasHeader;
int    pch_las_read_header(const char* path_host, PchLasHeader* out_host);
size_t pch_las_read_ws_bytes(void);
/* out_XYZ [count,3] int32 (device): records first .. first+count-1;  ws: device scratch */
int    pch_las_read_xyz_i32(const char* path_host, int64_t first, int64_t count, int32_t* out_XYZ,
                            void* ws, size_t ws_bytes, void* stream);
/* hdr_host: point_format, version, scales, offsets are used; XYZ [n,3] int32 (device) */
int    pch_las_write_xyz_i32(const char* path_host, const PchLasHeader* hdr_host, const int32_t* XYZ,
                             int64_t n, void* stream);

/* LAS point records -> X,Y,Z: gathers the three little-endian int32 at the start of every
 * `record_len`-byte record (LAS 1.0-1.4 point formats 0-10 all start with X,Y,Z).
 * Replaces: laspy's record parsing behind las.X/.Y/.Z (ui/import_PC.py:28,
 *           utils/tower_extraction.py:60-61).  records: raw bytes [n*record_len] on the device. */
int pch_las_records_xyz_i32(const uint8_t* records, int64_t n, int32_t record_len,
                            int32_t* out_XYZ, void* stream);

/* laspy scaled view, stage A0: out = (double)X * scale + offset (no FMA).
 * Replaces: the chunk.x/.y/.z reads at ui/import_PC.py:47-48 and las.x/.y/.z at
 *           utils/tower_extraction.py:62.  XYZ [n,3] int32 (LAS record ints, AoS). */
int pch_las_scale_i32_f64(const int32_t* XYZ, int64_t n, const double* scale3_host,
                          const double* offset3_host, double* out_xyz, void* stream);
/* laspy coordinate setter, stage A3: out = (int32) rint((v - offset) / scale).
 * Replaces: downsampled.x/.y/.z = ... at ui/import_PC.py:61-63 and
 *           utils/tower_extraction.py:254-256. */
int pch_las_unscale_f64_i32(const double* xyz, int64_t n, const double* scale3_host,
                            const double* offset3_host, int32_t* out_XYZ, void* stream);

/* ------------------------------------------------------------------ stage B
 * .astype(np.float32) of utils/tower_extraction.py:62 */
int pch_cast_f64_f32(const double* in, int64_t count, float* out, void* stream);

/* np.mean(raw_points, axis=0) for a C-order [n,3] float32 array, bit-exact: a
 * SEQUENTIAL float32 running sum per column divided by float32(n).
 * Replaces: utils/tower_extraction.py:63.   out_centroid [3] float32. */
size_t pch_mean_seq_f32_ws_bytes(int64_t n);
int pch_mean_seq_f32(const float* xyz, int64_t n, float* out_centroid,
                     void* ws, size_t ws_bytes, void* stream);
/* Slices of pch_mean_seq_f32 and of the centroid inside pch_ground_filter_f32 / the fused call: the summary pass is
 * cut into k launches over consecutive row ranges, and the serial walk of every slice but the last runs on a stream
 * of the library's own beside the summary of the next slice.  0 (default) = automatic: one launch below 2^26 rows,
 * two equal slices from there; 1..8 = forced, equal shares, clamped to the number of 65 536-row groups.  Per thread;
 * the result does not depend on it (tests slice small clouds with it).  pch_mean_seq_partial_f32 ignores it. */
void pch_mean_set_slices(int k);
/* One file-order SHARD of that sequential sum (config 4: every rank holds a consecutive slice of the rows and the
 * three running sums travel down the line, 12 bytes per hop): continues the float32 running sums sum_in3 (device
 * float[3]; NULL = +0.0, the first shard) over these n rows, exactly as numpy's loop would.
 *   total_n == 0: out3 = the running sums AFTER the rows (hand them to the next shard);
 *   total_n  > 0: out3 = running sums / float32(total_n) - the centroid of all total_n rows (last shard).
 * Shards chained in file order give np.mean(concatenation, axis=0) bit for bit; n == 0 passes the sums through.
 * phase: 0 = everything; 1 = only the summary tables of these rows (they do not depend on sum_in3: every rank
 * builds them at once, sum_in3 / out3 are ignored); 2 = only the short serial walk over the tables a phase-1 call
 * left in the SAME workspace (the caller keeps that workspace untouched in between) - so that along a chain of
 * shards only the walks (~0.1-0.3 ms each) are serial, not the passes over the rows.
 * zcol_out (optional, [n] float32): receives a contiguous copy of the z column, written by the table pass that
 * reads the rows anyway (phases 0 and 1) - what the percentile passes of stage B2 then read instead of the rows.
 * Workspace: pch_mean_seq_f32_ws_bytes(n).  Replaces: utils/tower_extraction.py:63 on a sharded array. */
int pch_mean_seq_partial_f32(const float* xyz, int64_t n, const float* sum_in3, int64_t total_n,
                             float* out3, float* zcol_out, int32_t phase, void* ws, size_t ws_bytes, void* stream);
/* same result from one workgroup adding element by element (O(n) serial; kept only to
 * cross-check the parallel algorithm above) */
int pch_mean_seq_serial_f32(const float* xyz, int64_t n, float* out_centroid, void* stream);

/* np.percentile(v, q) (method 'linear', numpy 2.x float32 semantics) of the strided
 * float32 column v[i] = base[i*stride] - (sub ? *sub : 0).
 * Replaces: utils/tower_extraction.py:82-83 (z_values = points[:,2]; percentile 25).
 * out [1] float32. */
size_t pch_percentile_f32_ws_bytes(int64_t n);
int pch_percentile_f32(const float* base, int64_t n, int64_t stride, const float* sub,
                       double q_percent, float* out,
                       void* ws, size_t ws_bytes, void* stream);

/* The three histogram passes of the radix select and the "smallest key above" pass one at a time, for a
 * percentile over values that are spread over several GPUs (pointcloudhookup_amd/tiles.py::shared_percentile:
 * every rank histograms its part, the histograms are all-reduced, the host picks the bin).  They run the same
 * kernels as pch_percentile_f32, so the tiled threshold is the one pch_percentile_f32 gives.  Keys are the
 * order-preserving uint32 images of the floats (sign bit flipped / complemented; NaN = 0xFFFFFFFF).
 * pass 0: bins = key >> 20 (4096), pass 1: (key >> 8) & 0xFFF among keys with key >> 20 == prefix,
 * pass 2: key & 0xFF among keys with key >> 8 == prefix.  out_hist [4096] uint32 (device), out_nan [1] uint64
 * (device, may be NULL; filled by pass 0).  ws: pch_percentile_f32_ws_bytes.  Both synchronise. */
int pch_select_hist_f32(const float* base, int64_t n, int64_t stride, int32_t pass, uint32_t prefix,
                        uint32_t* out_hist, unsigned long long* out_nan, void* ws, size_t ws_bytes, void* stream);
int pch_select_min_above_f32(const float* base, int64_t n, int64_t stride, uint32_t key, uint32_t* out_key,
                             void* ws, size_t ws_bytes, void* stream);

/* keep = (z - centroid[2]) > threshold, points = raw - centroid, order preserving: the sweep of the fused filter
 * with GIVEN centroid and threshold (utils/tower_extraction.py:64,84 once both are known - the shared values of
 * a tiled run).  out_points [n,3] capacity, out_index [n] int32 (may be NULL), out_count [1] int64, out_aabb [6]
 * float32 (may be NULL).  Synchronises. */
size_t pch_filter_gt_ws_bytes(int64_t n);
int pch_filter_gt_f32(const float* raw, int64_t n, const float* centroid3_host, float threshold,
                      float* out_points, int32_t* out_index, int64_t* out_count, float* out_aabb,
                      void* ws, size_t ws_bytes, void* stream);

/* Fused stage B: centroid, centring, percentile threshold, order-preserving compaction.
 * Replaces: utils/tower_extraction.py:63-64,82-89
 *   centroid = mean(raw); points = raw - centroid; base = percentile(points[:,2], pct);
 *   keep = z > base + offset; if kept < min_keep: keep = z > base + fallback_offset.
 * raw          [n,3] float32
 * out_points   [n,3] float32 capacity; first *out_count rows = points[keep] (file order)
 * out_index    [n]   int32 (may be NULL): original row of each kept point
 * out_scalars  [8]   float32: centroid xyz, base, threshold, used_fallback(0/1),
 *                    [6] = the BITS of the uint32 count kept at `offset` (an integer in a
 *                    float slot - reinterpret, do not convert), [7] = 0
 * out_count    [1]   int64
 * out_aabb     [6]   float32 (may be NULL): min xyz, max xyz of the kept points
 */
size_t pch_ground_filter_ws_bytes(int64_t n);
int pch_ground_filter_f32(const float* raw, int64_t n, double pct, float offset,
                          float fallback_offset, int64_t min_keep,
                          float* out_points, int32_t* out_index, float* out_scalars,
                          int64_t* out_count, float* out_aabb,
                          void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ stage B, opt-in: the LAS-integer frame
 * The reference casts world coordinates to float32 BEFORE it centres them (utils/tower_extraction.py:62-64): at
 * projected-CRS scale that is a 0.25 m grid in y.  This frame centres on the int32 LAS records first (the remedy of
 * the reference's own test/pipei.py:68-79, restated on the integers) and applies the reference's height rule to the
 * result.  XYZ [n,3] int32 (device), scale3_host [3] float64 (host; `offset` of the LAS header does not enter):
 *   1 centroid: S_j = sum_i XYZ[i,j] in int64 (exact: |S| < 2^62); C_j = floor(S_j / n) (Python's //, not C
 *     truncation).  World centroid, for the caller: (double)C_j * scale_j + offset_j, a multiply, then an add.
 *   2 rows: p[i,j] = (float)((double)((int64)XYZ[i,j] - C_j) * scale_j) - an exact difference, one float64 multiply,
 *     one rounding to float32, no FMA.
 *   3 threshold: base = np.percentile(p[:,2], pct) under numpy's float32 'linear' rule (the arithmetic of
 *     pch_percentile_f32); threshold = base + offset; keep p_z > threshold (strict), order preserving; if fewer than
 *     min_keep rows are kept, keep p_z > base + fallback_offset instead.  p_z is non-decreasing in Z, so the two order
 *     statistics are taken on the integers (an exact radix select on Z - min Z, digits cut from the range of Z).
 *   4 outputs: out_points [n,3] float32 capacity, the first count rows = the kept p rows in file order; out_index [n]
 *     int32 (may be NULL): their rows; out_frame_dev: the DEVICE record below - aabb is the box of the finite kept
 *     rows (zeros if none), count_at_offset the rows kept at `offset`, count those of the threshold that stands;
 *     count reads negative after a bounded wait that ran out (above).
 * Asynchronous: enqueues and returns, no host read; three to six sweeps over the 12-byte rows (sums and range of Z,
 * one histogram pass per 12 bits of that range, the compaction, its repeat for the fallback), every launch sized from
 * n alone, no float copy of the cloud.  n <= 0, n >= 2^31, a scale that is not finite or <= 0, pct outside [0, 100]
 * or NaN: PCH_ERR_ARG; ws_bytes below pch_ground_filter_las_ws_bytes(n): PCH_ERR_WORKSPACE.  The size query is host
 * arithmetic and gives 0 for n < 0. */
typedef struct PchLasFrame {
    int64_t  centroid[3];     /* C, in LAS counts */
    int64_t  count;           /* kept rows; negative: PCH_ERR_TIMEOUT */
    int64_t  count_at_offset; /* kept at base + offset */
    float    base, threshold;
    float    aabb[6];         /* min xyz, max xyz of the finite kept rows */
    uint32_t used_fallback;   /* 1: threshold = base + fallback_offset */
    uint32_t reserved;
} PchLasFrame;                /* 80 bytes */
size_t pch_ground_filter_las_ws_bytes(int64_t n);
int pch_ground_filter_las_i32(const int32_t* XYZ, int64_t n, const double* scale3_host, double pct, float offset,
                              float fallback_offset, int64_t min_keep, float* out_points, int32_t* out_index,
                              PchLasFrame* out_frame_dev, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ stage B, opt-in: one RANSAC ground plane
 * The second ground rule, for sloped terrain: a plane z = a x + b y + c fitted by RANSAC on z ~ (x, y) instead of one
 * global percentile.  Replaces: test/main_ground.py:8-32 (remove_ground_ransac; RANSACRegressor with
 * residual_threshold 0.1).  Frame: P = fl32(raw - centroid) as in stage B; everything below is float64 on (double)P
 * in exactly the written association, without FMA.
 *   plane of hypothesis h from p0, p1, p2 = P[rows[h]]:  u = p1 - p0, v = p2 - p0,
 *     nx = u.y v.z - u.z v.y, ny = u.z v.x - u.x v.z, nz = u.x v.y - u.y v.x, nn = (nx nx + ny ny) + nz nz;
 *     valid iff nn is finite, nz != 0 and nz nz >= cos2_max_slope nn (the slope gate: a tower face is no ground);
 *     a = -nx / nz, b = -ny / nz, c = p0.z - (a p0.x + b p0.y); a non-finite a, b or c invalidates it too, and so does
 *     a row outside [0, n).  Repeats in a triple are not rejected: such a triple is degenerate, hence invalid.
 *   residual of row i: r = z - ((a x + b y) + c); inlier iff |r| <= residual_threshold (a NaN row never is)
 *   best: the valid hypothesis with the most inliers, the smallest h on a tie; -1 if none is valid.  No refit.
 * pch_plane_fit_f32 (test/main_ground.py:21-28):
 *   raw [n,3] float32, 0 <= n < 2^31; centroid3_dev [3] float32 (DEVICE: what pch_mean_seq_f32 wrote);
 *   rows_dev [nhyp,3] int64 (device), 1 <= nhyp <= 4096
 *   out_planes [nhyp,4] float64: a, b, c, valid (1.0 / 0.0); an invalid hypothesis is four zeros
 *   out_counts [nhyp] int64: inliers over all n rows, 0 for an invalid hypothesis
 *   out_best_dev: DEVICE record; a = b = c = 0, count = 0, best = -1 when no hypothesis is valid (always so for n == 0)
 *   Asynchronous: enqueues and returns, fit and filter chain through out_best_dev without a host read.  The inlier
 *   count takes the cloud in passes of 1024 rows per workgroup.  The workspace is reserved (0 bytes today).
 * pch_filter_plane_f32 (test/main_ground.py:28-30): the order-preserving compaction of pch_filter_gt_f32 with the
 *   plane of best_dev as the rule - keep_mode 0: keep r > offset_or_threshold (height above the fitted ground, the
 *   analogue of z > base + offset); keep_mode 1: keep !(|r| <= offset_or_threshold), i.e. ~inlier_mask_, NaN rows
 *   included.  best < 0 keeps nothing.  Outputs as pch_filter_gt_f32 (out_aabb over the finite kept rows, zeros if
 *   there are none); *out_count reads negative after a bounded wait that ran out (above).  Asynchronous. */
typedef struct PchPlaneBest {
    double  a, b, c;          /* z = a x + b y + c in the centred frame */
    int64_t count;            /* inliers of the best hypothesis */
    int32_t best;             /* its index, -1: no valid hypothesis */
    int32_t nvalid;           /* valid hypotheses */
} PchPlaneBest;
size_t pch_plane_fit_ws_bytes(int64_t n, int32_t nhyp);
int pch_plane_fit_f32(const float* raw, int64_t n, const float* centroid3_dev, const int64_t* rows_dev, int32_t nhyp,
                      double residual_threshold, double cos2_max_slope, double* out_planes /*[nhyp,4]: a,b,c,valid*/,
                      int64_t* out_counts /*[nhyp]*/, PchPlaneBest* out_best_dev, void* ws, size_t ws_bytes,
                      void* stream);
size_t pch_filter_plane_ws_bytes(int64_t n);
int pch_filter_plane_f32(const float* raw, int64_t n, const float* centroid3_dev, const PchPlaneBest* best_dev,
                         int32_t keep_mode, double offset_or_threshold, float* out_points, int32_t* out_index,
                         int64_t* out_count, float* out_aabb, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ stage B, opt-in: one RANSAC plane per xy tile
 * The third ground rule, for rolling terrain (a corridor that crosses ridges and valleys): the rule above run once per
 * tile of an xy grid.  Replaces: test/main_ground.py:77-115 (remove_ground_tiled_ransac, "for complex terrain").
 * Frame and arithmetic as above: P = fl32(raw - centroid), then float64 on (double)P in exactly the written
 * association, no FMA, IEEE division.
 *   1 grid: PchPlaneGrid, given by the caller; tile > 0 and finite, nx, ny >= 1, nx * ny <= 65536 (else PCH_ERR_ARG).
 *     fx = floor((x - x0) / tile), fy = floor((y - y0) / tile); the row is in the grid iff 0 <= fx < nx and
 *     0 <= fy < ny (NaN and inf fail the comparisons); then t = fy * nx + fx, otherwise the row has no tile (t = -1).
 *   2 members: list_t = the rows of tile t in ascending row order, n_t its length.
 *   3 hypotheses: ONE table draws [nhyp,3] int64 with entries >= 0 for all tiles, 1 <= nhyp <= 4096 and
 *     nx * ny * nhyp <= 2^22 (else PCH_ERR_ARG).  The triple of (t, h) is list_t[draws[h][k] mod n_t], k = 0, 1, 2;
 *     validity and a, b, c as for pch_plane_fit_f32 (a repeated row is degenerate, then the slope gate, then
 *     finiteness).  A tile with n_t < min_tile_rows (>= 1) has no valid hypothesis (the reference skips tiles under 10
 *     rows); a negative draw invalidates its hypothesis.
 *   4 counts[t][h] = the rows OF TILE t with |r| <= residual_threshold; 0 for an invalid hypothesis.
 *   5 best per tile: the valid hypothesis with the most inliers, the smallest h on a tie; none valid: best = -1.
 *   6 filter, order preserving over the whole cloud in FILE order (the reference emits tile by tile; file order is kept
 *     because the sequential centroid and the 50 000-row DBSCAN chunks depend on it): a row uses its tile's plane when
 *     that tile has one, otherwise the fallback record (a tile without a plane, a row without a tile); fallback_dev is
 *     a PchPlaneBest on the device as pch_plane_fit_f32 writes it and may be NULL.  A row with no plane at all is not
 *     kept, in either keep mode.
 * pch_plane_tiles_fit_f32: out_best_dev [ntiles] device records (ntiles = nx * ny); optional outputs out_tile_rows
 *   [ntiles] int64 (n_t), out_planes [ntiles,nhyp,4] float64 and out_counts [ntiles,nhyp] int64 (NULL: the tables live
 *   in the workspace).  n == 0 succeeds with every tile at best = -1.  Asynchronous, no host read: the rows are grouped
 *   by a stable radix sort of (tile, row) on the bits in use, the inlier count takes every tile in passes of at most
 *   1024 grouped rows that never straddle two tiles, and every launch is sized from n and ntiles alone (surplus
 *   workgroups return).  Workspace: 24 bytes per row for the sort's two key / row buffers, its digit tables, and the
 *   two tables above.
 * pch_filter_plane_tiles_f32: keep modes, outputs, the box of the finite kept rows and the negative count word after
 *   a bounded wait that ran out are those of pch_filter_plane_f32; best_dev [ntiles] is what the fit wrote.
 *   Asynchronous. */
typedef struct PchPlaneGrid {
    double  x0, y0, tile;     /* origin and tile edge in the centred frame */
    int32_t nx, ny;           /* tiles along x and y; tile t = fy * nx + fx */
} PchPlaneGrid;
size_t pch_plane_tiles_fit_ws_bytes(int64_t n, int32_t ntiles, int32_t nhyp);
int pch_plane_tiles_fit_f32(const float* raw, int64_t n, const float* centroid3_dev, const PchPlaneGrid* grid_host,
                            const int64_t* draws_dev /*[nhyp,3]*/, int32_t nhyp, int32_t min_tile_rows,
                            double residual_threshold, double cos2_max_slope,
                            PchPlaneBest* out_best_dev /*[ntiles]*/, int64_t* out_tile_rows /*[ntiles], may be NULL*/,
                            double* out_planes /*[ntiles,nhyp,4], may be NULL*/,
                            int64_t* out_counts /*[ntiles,nhyp], may be NULL*/, void* ws, size_t ws_bytes,
                            void* stream);
size_t pch_filter_plane_tiles_ws_bytes(int64_t n, int32_t ntiles);
int pch_filter_plane_tiles_f32(const float* raw, int64_t n, const float* centroid3_dev, const PchPlaneGrid* grid_host,
                               const PchPlaneBest* best_dev /*[ntiles]*/, const PchPlaneBest* fallback_dev /*may be NULL*/,
                               int32_t keep_mode, double offset_or_threshold, float* out_points, int32_t* out_index,
                               int64_t* out_count, float* out_aabb, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ stage C
 * sklearn.cluster.DBSCAN(eps, min_samples, algorithm='ball_tree').fit(chunk).labels_ for
 * every consecutive chunk_size-row chunk, with the reference's label offsetting.
 * Replaces: the loop utils/tower_extraction.py:96-117.
 * xyz        [n,3] float32 (n known on the host)
 * chunk_size rows per fit (reference: 50000); <=0: one global fit
 * labels     [n] int32: -1 noise, else cluster id, ids dense and ordered exactly as the
 *            reference's all_labels
 * core       [n] uint8 (may be NULL): 1 for core samples
 * out_nclusters [1] int32
 * A chunk that contains NaN/inf is left at -1 and does not advance the label counter (sklearn
 * raises ValueError for it and the reference catches that, utils/tower_extraction.py:118-119).
 * Exact rule implemented (equals sklearn's sweep): neighbours are
 * sum_j((double)x_j-(double)y_j)^2 <= eps*eps; core = >= min_samples neighbours incl.
 * self; clusters = components of the core graph numbered by smallest core index;
 * border point -> smallest cluster id among its core neighbours.
 * Synchronises once (reads the bounding box to size the cell grid) unless aabb_host
 * (min xyz, max xyz of the input, any superset box) is given.
 * Cell sort: one workgroup per chunk or one global radix sort, chosen by the chunk count;
 * environment PCH_DBSCAN_SORT=chunk|global (read once per process) or
 * pch_dbscan_set_sort_mode(0 auto | 1 chunk | 2 global) force one - same results either way.
 */
void   pch_dbscan_set_sort_mode(int mode);
size_t pch_dbscan_ws_bytes(int64_t n);
int pch_dbscan_f32(const float* xyz, int64_t n, double eps, int32_t min_samples,
                   int64_t chunk_size, const float* aabb_host,
                   int32_t* labels, uint8_t* core, int32_t* out_nclusters,
                   void* ws, size_t ws_bytes, void* stream);

/* Relabels the result of the pch_dbscan_f32 call this thread made last, on the SAME workspace (which still
 * holds the cell grid, the core flags and the sorted points): core points take map[old cluster id],
 * every non-core point is assigned again as "smallest NEW id among its core neighbours within eps, else
 * -1" (border points must be re-decided: the order of the ids may have changed).  Used by the cross-tile
 * reconciliation (pointcloudhookup_amd/tiles.py): clusters cut by a tile edge are united and renumbered
 * globally, which generalises the per-chunk label offsets of utils/tower_extraction.py:113-116.
 * map [nmap] int32 (device): new id per old id (-1 = drop).  labels [n] int32: in/out.
 * Workspace rule: the library remembers, per thread, the workspace of the last pch_dbscan_f32 call; ANY pch_*
 * call of that thread whose workspace overlaps it forgets it again, and this call then returns PCH_ERR_ARG
 * ("must follow pch_dbscan_f32 ... untouched workspace") rather than following overwritten indices.  Give the
 * fit a workspace of its own if other calls run between the fit and the relabel (ops.DbscanFit does). */
int pch_dbscan_relabel_i32(const int32_t* map, int32_t nmap, int64_t n, int32_t* labels,
                           void* ws, size_t ws_bytes, void* stream);
/* Smallest core row of every cluster of that same last call (the row that gives a cluster its number in
 * sklearn's sweep): out_rows [nclusters] int32, ascending.  Same workspace rule as the relabel call. */
int pch_dbscan_first_core_rows_i32(int64_t n, int32_t* out_rows, void* ws, size_t ws_bytes, void* stream);

/* Measurement of the radius kernel in the currency that bounds it ("pair-tests/s").  With counting
 * enabled (per thread) pch_dbscan_f32 runs the radius-count kernel in a variant with the SAME control flow that
 * tallies its distance tests; pch_dbscan_pair_stats then reads, from the fit's untouched workspace,
 *   out4_host[0] useful pair tests (a real query point against a real candidate point),
 *   out4_host[1] issued lane slots (64 per wave instruction group: padding and idle lanes included),
 *   out4_host[2] cells that reached the distance-test path, out4_host[3] LDS candidate tiles staged.
 * The counting variant is slower: time the plain kernel, count with this one (bench.py does).  Synchronises. */
void pch_dbscan_set_pair_counting(int enable);
int pch_dbscan_pair_stats(int64_t n, uint64_t* out4_host, void* ws, size_t ws_bytes, void* stream);

/* The (row, cluster) pairs a tile publishes to its neighbour for the cross-tile reconciliation (config 4,
 * pointcloudhookup_amd/tiles.py): of that same last fit, ONE pair per grid cell that holds a core point with
 * x_lo <= x < x_hi - the cell's smallest such row and the cell's cluster id.  All core points of a cell lie within
 * eps of each other, so they share a cluster in any tile that sees them: a pair per cell carries what a pair per
 * point would (a tower on a tile edge: hundreds of pairs instead of hundreds of thousands).  Call it BEFORE
 * pch_dbscan_relabel_i32 (it reports the fit's own ids).  out_pairs [cap,2] int32 in no particular order;
 * *out_count (device int32) = number of such cells, which may exceed cap (then only cap pairs were stored: call
 * again with a larger buffer).  Same workspace rule as the relabel call.
 * Generalises: the per-chunk label offsets of utils/tower_extraction.py:113-116 to tiles that share points. */
int pch_dbscan_strip_pairs_i32(int64_t n, float x_lo, float x_hi, int32_t cap, int32_t* out_pairs,
                               int32_t* out_count, void* ws, size_t ws_bytes, void* stream);

/* Assigns points that were NOT part of the fit to the clusters of that same last fit: "which rows of my original
 * cloud belong to tower k?" - a second flight line, the rows the height filter removed (tower feet), the cloud before
 * it was thinned.  The rule is the one the fit applies to its own non-core rows:
 *   q = fl32(query[i] - sub3) per component (a float32 subtraction, the arithmetic of raw - centroid; sub3_host ==
 *       NULL: no subtraction);
 *   out_labels[i] = the smallest label among the fit's core points p within eps of q under the library's predicate
 *       (float64 sum_j((double)q_j - (double)p_j)^2 <= eps*eps behind the float32 guard-band pre-filter), -1 if no
 *       core point is in reach; a query holding NaN or +-inf gets -1.
 * Applied to the fit's own rows it reproduces the fit's labels, core rows included (core points within eps of each
 * other share a cluster).
 * query [nq,3] float32, out_labels [nq] int32 (device); sub3_host 3 floats on the host or NULL.
 * query_chunk [nq] int32 (device): the chunk whose fit query i is held against (one fit per chunk, as sklearn is
 *       called); an index outside [0, nchunks) or a chunk that held NaN/inf gives -1 for that query.  NULL is allowed
 *       only for a single-chunk fit (else PCH_ERR_ARG).
 * n, ws, ws_bytes name the fit (same workspace rule as the relabel call: PCH_ERR_ARG, "untouched workspace").  The
 * fit's workspace and labels are only read, so the call may be repeated, before or after pch_dbscan_relabel_i32; after
 * a relabel it reports the new ids, and a cell whose cluster was dropped attracts nothing.
 * qws: a query workspace of its own, >= pch_dbscan_assign_ws_bytes(nq) bytes (smaller: PCH_ERR_WORKSPACE); it must
 * not overlap ws (PCH_ERR_ARG - the fit stays remembered).  nq == 0 is success, nq >= 2^31 PCH_ERR_ARG.
 * A fit that took the compressed-coordinate path (grid beyond the 64-bit cell key) keeps no map from a coordinate to
 * a cell: PCH_ERR_RANGE.  Per-chunk refits and all-noise early returns leave no grid: PCH_ERR_ARG, as for the other
 * continuation calls.  Enqueues its work and returns; no host reads. */
size_t pch_dbscan_assign_ws_bytes(int64_t nq);
int pch_dbscan_assign_f32(const float* query, int64_t nq, const float* sub3_host, const int32_t* query_chunk,
                          int64_t n, int32_t* out_labels, void* qws, size_t qws_bytes,
                          void* ws, size_t ws_bytes, void* stream);

/* The k-distance of points against that same last fit: for every query the squared distance to its k-th nearest row of
 * the fit, exactly - the sorted k-distance plot is the instrument DBSCAN's authors give for choosing eps, and
 * pch_dbscan_f32 itself stops counting neighbours at min_samples.  For query i:
 *   q = fl32(query[i] - sub3) per component (sub3_host == NULL: no subtraction), c = query_chunk[i];
 *   d2(q, p) = (dx*dx + dy*dy) + dz*dz in float64 on the float64 images of the float32 coordinates, accumulated in x,
 *       y, z order without FMA - the library's predicate, sklearn's euclidean_rdist;
 *   R = { d2(q, p) : p a row of the fit in chunk c, core or not, d2 <= eps*eps } as a multiset (the fit's own eps*eps);
 *   out_count[i] = |R|; out_d2[i] = the k-th smallest element of R (1-based, equal values counted separately) if
 *       |R| >= k, else +inf.
 * A query holding NaN or +-inf, a chunk index outside [0, nchunks) and a chunk that held NaN/inf give count 0 and +inf.
 * Applied to the fit's own rows (query_chunk[i] = i / chunk_size) the row itself is in R with d2 = 0, so
 * core[i] == (out_count[i] >= min_samples), and with k = min_samples also core[i] == (out_d2[i] <= eps*eps).
 * The answer is truncated at the fit's eps (the grid reaches two cells): for k-distances up to 16 m fit at eps = 16 with
 * any min_samples; one fit then serves every k.  Answers do not depend on labels: before or after a relabel alike.
 * query [nq,3] float32, query_chunk [nq] int32 or NULL (single-chunk fits only), out_d2 [nq] float64, out_count [nq]
 * int32 or NULL - all device; sub3_host 3 floats on the host or NULL.  k < 1: PCH_ERR_ARG.
 * n, ws, ws_bytes, qws (>= pch_dbscan_kdist_ws_bytes(nq) bytes) and every other status: as for pch_dbscan_assign_f32.
 * Enqueues its work and returns; no host reads; the fit is only read, so the call may be repeated. */
size_t pch_dbscan_kdist_ws_bytes(int64_t nq);
int pch_dbscan_kdist_f32(const float* query, int64_t nq, const float* sub3_host, const int32_t* query_chunk,
                         int32_t k, int64_t n, double* out_d2, int32_t* out_count, void* qws, size_t qws_bytes,
                         void* ws, size_t ws_bytes, void* stream);

/* The k nearest rows of points against that same last fit: WHICH rows the neighbours are, where pch_dbscan_kdist_f32
 * gives one distance - the input of statistical outlier removal, normals, a kNN graph.  For query i:
 *   q, c, d2(q, p) and the set of rows in reach are exactly those of pch_dbscan_kdist_f32: q = fl32(query[i] - sub3),
 *       c = query_chunk[i], d2 the float64 sum in x, y, z order without FMA, and
 *   R = the rows of the fit in chunk c, core or not, with d2 <= eps*eps for the fit's own eps (the float32 guard band
 *       comes first, as everywhere in stage C);
 *   R is ordered by (d2, row) ascending, row being the original file-order row of the fit - the GLOBAL row, not a
 *       chunk-local one.  Rows are unique, so the order is total, and the answer depends neither on the sorted copy's
 *       order nor on PCH_DBSCAN_SORT;
 *   out_rows[i, j] and out_d2[i, j] are element j of that order for j < min(k, |R|); every further slot holds -1 and
 *       +inf; out_count[i] = |R|, and out_count may be NULL.
 * A query holding NaN or +-inf, a chunk index outside [0, nchunks) and a chunk that held NaN/inf give count 0 and k empty
 * slots.  On the fit's own rows slot 0 is the row itself at 0.0, unless a duplicate with a smaller row exists: then that
 * duplicate comes first - the order decides, not identity.
 * query [nq,3] float32, query_chunk [nq] int32 or NULL (single-chunk fits only), out_rows [nq,k] int32, out_d2 [nq,k]
 * float64, out_count [nq] int32 or NULL - all device; sub3_host 3 floats on the host or NULL.
 * 1 <= k <= PCH_KNN_MAX_K, anything else is PCH_ERR_ARG: the bound lets the answer of one query sit in a wave's LDS while
 * it is ordered.
 * n, ws, ws_bytes, qws (>= pch_dbscan_knn_ws_bytes(nq) bytes: too small PCH_ERR_WORKSPACE, overlapping the fit's
 * PCH_ERR_ARG), nq == 0 (success), nq >= 2^31 (PCH_ERR_ARG), compressed-coordinate fits (PCH_ERR_RANGE), refits,
 * all-noise fits and retired fits (PCH_ERR_ARG, the fit stays remembered): exactly as for pch_dbscan_kdist_f32.
 * Labels play no part.  The answer is truncated at the fit's eps, so fit at the radius of interest; cost follows the
 * fit's eps.  Enqueues its work and returns; no host reads; the fit is only read, so the call may be repeated. */
#define PCH_KNN_MAX_K 256
size_t pch_dbscan_knn_ws_bytes(int64_t nq);
int pch_dbscan_knn_f32(const float* query, int64_t nq, const float* sub3_host, const int32_t* query_chunk,
                       int32_t k, int64_t n, int32_t* out_rows /* [nq,k] */, double* out_d2 /* [nq,k] */,
                       int32_t* out_count, void* qws, size_t qws_bytes, void* ws, size_t ws_bytes, void* stream);

/* What a neighbourhood looks like, against that same last fit: for every query the number of rows of the fit within
 * `radius` and their first and second moments about the query - the input of the covariance features that tell a
 * conductor (a line) from vegetation (a blob) and from a tower.  For query i:
 *   q = fl32(query[i] - sub3) per component (sub3_host == NULL: no subtraction), c = query_chunk[i], exactly as for
 *       pch_dbscan_kdist_f32;
 *   d = (double)p - (double)q per component (dx, dy, dz); these differences are exact;
 *   d2 = (dx*dx + dy*dy) + dz*dz in float64, accumulated in x, y, z order without FMA - the library's predicate;
 *   R = the rows p of the fit in chunk c, core or not, with d2 <= radius*radius;
 *   out_count[i] = |R|;
 *   out_moments[i] = (Σdx, Σdy, Σdz, Σdx², Σdy², Σdz², Σdx·dy, Σdx·dz, Σdy·dz) over R, in float64.
 * The moments are taken about the query, not the origin, so a covariance formed from them loses nothing at the scale
 * of projected coordinates.  count is exact.  The order of summation is the library's own: with u = 2^-53 and n = count,
 * each of the first three moments lies within 2(n+1)·u·n·radius and each of the six second moments within
 * 2(n+1)·u·n·radius² of the sum taken in any other order.  Membership of R is decided by the float32 guard-band
 * pre-filter and the float64 test, as everywhere else in stage C.
 * radius must be finite, > 0 and <= the fit's eps (the grid reaches two cells): anything else is PCH_ERR_ARG.
 * A query holding NaN or +-inf, a chunk index outside [0, nchunks) and a chunk that held NaN/inf give count 0 and nine
 * zeros.  Labels play no part: before or after a relabel alike.
 * query [nq,3] float32, query_chunk [nq] int32 or NULL (single-chunk fits only), out_count [nq] int32, out_moments
 * [nq,9] float64 - all device; sub3_host 3 floats on the host or NULL.
 * n, ws, ws_bytes, qws (>= pch_dbscan_shape_ws_bytes(nq) bytes), nq == 0, nq >= 2^31, compressed-coordinate fits
 * (PCH_ERR_RANGE), refits and all-noise fits (PCH_ERR_ARG): as for pch_dbscan_assign_f32.
 * Enqueues its work and returns; no host reads; the fit is only read, so the call may be repeated. */
size_t pch_dbscan_shape_ws_bytes(int64_t nq);
int pch_dbscan_shape_f32(const float* query, int64_t nq, const float* sub3_host, const int32_t* query_chunk,
                         double radius, int64_t n, int32_t* out_count, double* out_moments /* [nq,9] */,
                         void* qws, size_t qws_bytes, void* ws, size_t ws_bytes, void* stream);

/* Covariance eigenvalues from those moments, one query per thread: n = max(count, 1), mu = M[0:3]/n,
 * C = M2/n - mu mu^T (symmetric, not clamped: rounding may leave a tiny negative eigenvalue), eigen-decomposed by
 * cyclic Jacobi in float64 (six sweeps over (0,1), (0,2), (1,2)).  out4[i] = (l1, l2, l3, v) with l1 >= l2 >= l3 and
 * v = |e1.z|, the z component of the unit eigenvector of l1; for the zero matrix (count 0) e1 = (1,0,0) and v = 0.
 * count [nq] int32, moments [nq,9] float64, out4 [nq,4] float64 - all device.  Needs no fit.  nq == 0 is success. */
int pch_shape_features_f64(const int32_t* count, const double* moments, int64_t nq, double* out4 /* [nq,4] */,
                           void* stream);

/* One representative per LATTICE cell of up to two strips of a tile: the smallest row among the core points of the
 * cell whose x lies in the strip.  The lattice is shared by all ranks (cell = floor(coordinate / side) per axis, side =
 * eps / sqrt(3) * (1 - 2^-16), anchored at the origin of the common frame), so the two tiles on either side of an edge
 * name the SAME rows for the strip around it - the join on the row links their cluster pieces (tiles.cluster_tiled).
 * xyz [n,3] float32, rows [n] int64 (global row of every point, ascending), labels [n] int32 (-1 = noise), core [n]
 * uint8 - all device; strips_host [nstrips][2] float32 = x_from, x_to per strip (nstrips <= 2, disjoint).
 * out_rows [2][cap] int64, out_labels [2][cap] int32: the pairs of strip k in row k, in no particular order;
 * out_count [4] int32 (device): [k] = cells of strip k (may exceed cap: call again with a larger cap), [2] = flags
 * (1: a coordinate beyond 2^20 cells from the origin, 2: table full - both make the result unusable), [3] = 0.
 * Generalises: the per-chunk label offsets of utils/tower_extraction.py:113-116 to tiles that share points. */
size_t pch_strip_lattice_reps_ws_bytes(int32_t cap);
int pch_strip_lattice_reps_f32(const float* xyz, const int64_t* rows, const int32_t* labels, const uint8_t* core,
                               int64_t n, int32_t nstrips, const float* strips_host, double eps, int32_t cap,
                               int64_t* out_rows, int32_t* out_labels, int32_t* out_count,
                               void* ws, size_t ws_bytes, void* stream);

/* First row of xyz [n,3] float32 that holds NaN or +-inf, -1 if every row is finite.
 * Replaces: sklearn's input validation inside DBSCAN.fit (check_array, ensure_all_finite), which
 * is what makes a chunk "fail" in the reference (utils/tower_extraction.py:107-119).
 * out_row [1] int64 (device). */
int pch_first_nonfinite_row_f32(const float* xyz, int64_t n, int64_t* out_row, void* stream);

/* ------------------------------------------------------------------ stage D0
 * Groups points by cluster label in one pass instead of the reference's K boolean
 * masks.  Replaces: utils/tower_extraction.py:125,131-134.
 * labels [n] int32 in [-1, nclusters)
 * out_perm    [n] int32: point rows ordered by (label, row); noise rows last
 * out_offsets [nclusters+1] int64: cluster k owns out_perm[offsets[k]:offsets[k+1]]
 * out_stats   [nclusters,8] float32 (may be NULL): min xyz, max xyz, 0, 0 per cluster; a cluster without rows
 *             reads +inf, -inf (also with n = 0).  A label outside [-1, nclusters) counts as noise.
 */
size_t pch_segment_by_label_ws_bytes(int64_t n, int32_t nclusters);
int pch_segment_by_label(const int32_t* labels, const float* xyz, int64_t n,
                         int32_t nclusters, int32_t* out_perm, int64_t* out_offsets,
                         float* out_stats, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ between C and D0, opt-in: merge of cluster pieces
 * Stage C fits once per file-order chunk, so a tower whose kept rows straddle a chunk boundary comes out as two or
 * more clusters, of which the 30 m centre de-dup (utils/tower_extraction.py:153-162) keeps the first piece only.  These
 * calls restate the remedy of the reference's own test/tttt.py:93-175 ("聚类后处理：合并相邻簇"): clusters whose
 * centres lie within merge_threshold (6.0 there) of each other, directly or through a chain of others, become one.
 *
 * The rule.  P: the kept, centred float32 rows [n,3]; labels in [-1, K); cluster k owns the rows with labels == k in
 * ascending row order, i.e. perm[offsets[k]:offsets[k+1]] as pch_segment_by_label writes them.
 *   1 centre: c_k = np.mean(P[labels == k], axis=0) (tttt.py:113): per column a sequential float32 running sum over the
 *     cluster's rows in that order, divided by float32(n_k) with a correctly rounded float32 division - the arithmetic
 *     of pch_mean_seq_f32.  A cluster without rows has centre NaN; non-finite rows propagate as in numpy.
 *   2 reach: clusters i, j are linked iff ((dx*dx + dy*dy) + dz*dz) <= r*r in float64 on (double)c_i - (double)c_j,
 *     accumulated in x, y, z order without FMA, r = merge_threshold: the predicate of sklearn's
 *     KDTree.query_radius (reduced distance against r*r).  A NaN centre is linked to nothing.
 *   3 components of that graph: the new id of a cluster is the rank of its component, components ordered by their
 *     smallest old id.  So map[0] == 0, map[k] <= max(map[:k]) + 1, and clusters that merge with nothing keep their
 *     relative order.  nmerged = number of components, empty clusters included as singletons.
 *   4 relabel: labels[i] = map[labels[i]] for labels[i] in [0, K), everything else becomes -1.
 * Two deliberate deviations from the script, neither of which changes the partition: it numbers the merged clusters
 * from max(label) + 1 and then iterates a Python set of those numbers (an order that wraps at the set's table size, so
 * which piece the later de-dup sees first depends on CPython internals); here they are numbered from 0 and iterated
 * ascending.
 *
 * pch_cluster_centers_f32: step 1.  xyz [*,3] float32; perm int32 and offsets [nclusters+1] int64 as written by
 * pch_segment_by_label (perm entries are trusted to be rows of xyz); out_centers [nclusters,3] float32; out_sizes
 * [nclusters] int64 (may be NULL).  One wave per cluster, so the time is linear in the LARGEST cluster (a cluster of
 * millions of rows - a global fit - is summed serially).  Enqueues and returns; no workspace, no host read.
 *
 * pch_cluster_merge_f32: steps 2-4.  centers [nclusters,3] float32; labels [n] int32 in/out (may be NULL: map only);
 * out_map [nclusters] int32; out_nmerged [1] int32 (device).  All pairs are tested, so nclusters > 65536 is
 * PCH_ERR_RANGE; merge_threshold not finite or < 0: PCH_ERR_ARG; nclusters == 0: success, nmerged = 0 (and every
 * label -1); ws_bytes below pch_cluster_merge_ws_bytes(nclusters): PCH_ERR_WORKSPACE.  Nothing in it waits on
 * another workgroup.  Enqueues and returns; no host read. */
int pch_cluster_centers_f32(const float* xyz, const int32_t* perm, const int64_t* offsets, int32_t nclusters,
                            float* out_centers, int64_t* out_sizes, void* stream);
size_t pch_cluster_merge_ws_bytes(int32_t nclusters);
int pch_cluster_merge_f32(const float* centers, int32_t nclusters, double merge_threshold, int32_t* labels, int64_t n,
                          int32_t* out_map, int32_t* out_nmerged, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ conductor spans, opt-in
 * The rows that the wire rule of section 5b marks are grouped into wire pieces (a global fit, then the grouping of
 * stage D0); these calls reduce every piece to the sums from which a sag curve dz = a + b s + c s^2 is fitted.
 *
 * The rule.  P: float32 rows [*,3].  perm (int32) and offsets (int64 [K+1]) as the grouping call writes them; cluster k
 * owns rows_k = perm[offsets[k]:offsets[k+1]], n_k = len(rows_k).  All arithmetic is float64 without FMA (the library
 * is built with -ffp-contract=off), with parentheses exactly as written here.
 *   1 moments (pch_cluster_moments_f32): o_k = P[rows_k[0]] in float32; d = (double)p - (double)o_k per component - this
 *     difference is exact; out_count[k] = n_k (int64); out_origin[k] = o_k; out_moments[k] = (Σdx, Σdy, Σdz, Σdx², Σdy²,
 *     Σdz², Σdx·dy, Σdx·dz, Σdy·dz) over rows_k, the order of terms of pch_dbscan_shape_f32.  An empty cluster gives
 *     count 0 and twelve zeros.  Non-finite rows propagate as IEEE arithmetic propagates them.
 *   2 frame (no kernel, float64 on K records; ops.span_frames): with n = max(n_k, 1): μ = M[0:3]/n; cxx = M[3]/n - μx²,
 *     cyy = M[4]/n - μy², cxy = M[6]/n - μx·μy; θ = ½·atan2(2cxy, cxx - cyy), (ux, uy) = (cos θ, sin θ), negated when
 *     ux < 0, or when ux == 0 and uy < 0; λ = ½(cxx + cyy) + hypot(½(cxx - cyy), cxy); h = sqrt(3·max(λ, 0)), and h = 1
 *     where that is 0 (for rows spread evenly along a line h is half the length);
 *     frame_k = (ox + μx, oy + μy, oz + μz, ux, uy, 1/h), six float64 values f0..f5.
 *   3 profile (pch_cluster_profile_f32), frames [K,6] float64 on the device.  Per row: dx = (double)px - f0,
 *     dy = (double)py - f1, dz = (double)pz - f2; s = ((dx*f3) + (dy*f4))*f5; t = (dy*f3) - (dx*f4); s2 = s*s;
 *     out_sums[k] = (Σs, Σs2, Σ(s2*s), Σ(s2*s2), Σdz, Σ(s*dz), Σ(s2*dz), Σ(dz*dz), Σt, Σ(t*t));
 *     out_ext[k] = (min s, max s, min dz, max dz) - exact: the per-row arithmetic is fixed and min/max do not round (a
 *     NaN is never smaller or larger than anything and so is skipped).  An empty cluster gives ten zeros and
 *     (+inf, -inf, +inf, -inf).
 *   4 fit (no kernel, float64 on K records; ops.span_fit): the normal equations G x = r of dz ≈ a + b·s + c·s² with
 *     G = [[n, S1, S2], [S1, S2, S3], [S2, S3, S4]], r = (Σdz, Σs·dz, Σs2·dz).
 * The order of summation is the library's own.  With u = 2^-53, every sum S of terms t lies within 2(n_k+1)·u·Σ|t| of
 * the same sum taken in any other order.  It is a function of offsets alone: the same input gives the same bits on
 * every run (no floating-point atomics, no waiting on another workgroup).
 *
 * How: perm is swept in fixed blocks of 512 entries, one wave each, whatever the cluster sizes - the sweep's time is
 * linear in the number of grouped rows, not in the largest cluster.  A wave reduces every (cluster, block) segment it
 * holds and writes one partial; a second kernel adds a cluster's partials in ascending block order, one thread per
 * term: that part IS a serial chain of n_k/512 additions for cluster k (about 0.2 ms for ten million rows).
 *
 * n_grouped = the number of entries of perm (< 2^31).  Entries at and behind offsets[K] - the noise rows of the
 * grouping - belong to nobody.  perm entries are trusted to be rows of xyz.  xyz [*,3] float32; out_count [K] int64,
 * out_origin [K,3] float32, out_moments [K,9] float64, frames [K,6] float64, out_sums [K,10] float64, out_ext [K,4]
 * float64 - all device.  ws: the caller's, at least the matching *_ws_bytes(n_grouped, nclusters) bytes (smaller:
 * PCH_ERR_WORKSPACE).  nclusters == 0 is success; a null output, negative sizes and host pointers are PCH_ERR_ARG.
 * Enqueue and return; no host read. */
size_t pch_cluster_moments_ws_bytes(int64_t n_grouped, int32_t nclusters);
int pch_cluster_moments_f32(const float* xyz, const int32_t* perm, const int64_t* offsets, int64_t n_grouped,
                            int32_t nclusters, int64_t* out_count, float* out_origin /* [K,3] */,
                            double* out_moments /* [K,9] */, void* ws, size_t ws_bytes, void* stream);
size_t pch_cluster_profile_ws_bytes(int64_t n_grouped, int32_t nclusters);
int pch_cluster_profile_f32(const float* xyz, const int32_t* perm, const int64_t* offsets, int64_t n_grouped,
                            int32_t nclusters, const double* frames /* [K,6] */, double* out_sums /* [K,10] */,
                            double* out_ext /* [K,4] */, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ conductor clearance, opt-in
 * The distance of every row of a cloud to the fitted span curves: what comes how close to the line.
 *
 * The rule.  All arithmetic is float64 without FMA (the library is built with -ffp-contract=off); parentheses are as
 * written.
 *   Curves (no kernel; ops.span_curves): float64 [K,10] = (cx, cy, cz, ux, uy, a, b, c, m0, m1).  The centre and the
 *     direction are the frame's (f0..f4 above); a, b, c are the span table's (metres along the track);
 *     m0 = ext[:,0]*h and m1 = ext[:,1]*h with h = 1.0 / f5: the piece's along-track interval in metres from its centre.
 *   Polyline (no kernel; ops.span_segments), S segments, 1 <= S <= 128: float64 [K,S,5] = (m_j, z_j, dm_j, dz_j, inv_j).
 *     step = (m1 - m0) / S; m_j = m0 + j*step for j < S, and m_S = m1; z_j = a + m_j*(b + c*m_j);
 *     dm_j = m_{j+1} - m_j and dz_j = z_{j+1} - z_j; len2 = (dm*dm) + (dz*dz); inv_j = 1/len2 where len2 > 0,
 *     otherwise 0.  The polyline lies within |c|*((m1 - m0)/S)^2/4 of the parabola, vertically, and above it for a
 *     hanging wire: clearances to objects below are over-estimated by at most that (chord_error).
 *   Per row and span (pch_clearance_f32).  xyz float32 [n,3]; an optional skip uint8 [n]; curves5 float64 [K,5] =
 *     (cx, cy, cz, ux, uy); segs float64 [K,S,5]; radius and limit, finite, with 0 < limit <= radius;
 *     r2 = radius*radius and l2 = limit*limit, taken in double on the host.  A span takes part if and only if all
 *     5 + 5*S of its values are finite.  For row i with skip[i] == 0, spans are visited in ascending k:
 *         dx = (double)px - cx;  dy = (double)py - cy;  w = (double)pz - cz
 *         m = (dx*ux) + (dy*uy);  t = (dy*ux) - (dx*uy)
 *         g = +inf
 *         for j ascending:
 *             rm = m - m_j;  rw = w - z_j
 *             q = ((rm*dm_j) + (rw*dz_j))*inv_j
 *             if q < 0: q = 0
 *             if q > 1: q = 1
 *             em = rm - (q*dm_j);  ew = rw - (q*dz_j)
 *             d = (em*em) + (ew*ew)
 *             if d < g: g = d
 *         d2 = g + (t*t)
 *         if d2 <= r2 and d2 < best: best = d2; who = k
 *     out_dist2[i] = best (+inf if no span is within the radius); out_span[i] = who (-1 if no span is within the
 *     radius).  A skipped row gets +inf and -1.  A row with a non-finite coordinate also gets +inf and -1: every
 *     comparison with a NaN fails.  Ties between spans go to the lowest index.
 *   Per span, over the rows with out_span[i] == k: out_count[k] (int64); out_violations[k] (int64): the rows with
 *     dist2 <= l2; out_min_dist2[k] (float64): +inf if there is no row; out_min_row[k] (int64): the lowest row index
 *     that attains out_min_dist2[k], or -1.
 * Every row is attributed to its NEAREST span only: a row within the radius of two spans counts for the nearer one (the
 * lower index on a tie) and is absent from the other's count, violations and minimum.
 *
 * How: a small kernel over the spans writes the "takes part" flag and conservative bounds of each polyline, widened
 * by the radius; a sweep over tiles of 1024 rows walks, in ascending order, the spans whose bounds meet the tile's
 * own bounding box; a finisher finds the lowest row of every minimum.  Culling skips only spans the rule cannot accept
 * within the radius: the outputs are the rule's, whatever is culled.  The tallies are integer atomics and the minimum
 * is an integer atomic on the bit pattern (non-negative doubles order as integers): the same input gives the same bits
 * on every run; nothing waits on another workgroup.
 *
 * 0 <= n < 2^32, 0 <= nspans <= 4096, 1 <= nsegments <= 128 (else PCH_ERR_ARG, as a radius or limit that is not
 * finite, limit <= 0, limit > radius, a null buffer that is needed and a host pointer).  All buffers device; skip may
 * be NULL (no row is skipped); out_loops (int64 [2], may be NULL): the (row, span) segment loops run and the (tile,
 * span) pairs walked - figures for measurement, not part of the rule.  ws: the caller's, at least
 * pch_clearance_ws_bytes(n, nspans, nsegments) bytes - pure host code, 0 for sizes out of range (smaller:
 * PCH_ERR_WORKSPACE).  n == 0 or nspans == 0: every row gets +inf / -1, the table is (0, 0, +inf, -1) per span, and no
 * launch reads a null pointer.  Enqueues on the caller's stream and returns; no host read. */
size_t pch_clearance_ws_bytes(int64_t n, int32_t nspans, int32_t nsegments);
int pch_clearance_f32(const float* xyz, const uint8_t* skip, int64_t n, const double* curves5 /* [K,5] */,
                      const double* segs /* [K,S,5] */, int32_t nspans, int32_t nsegments, double radius, double limit,
                      double* out_dist2, int32_t* out_span, int64_t* out_count, int64_t* out_violations,
                      double* out_min_dist2, int64_t* out_min_row, int64_t* out_loops, void* ws, size_t ws_bytes,
                      void* stream);

/* ------------------------------------------------------------------ terrain grid, opt-in
 * A ground model that can be sampled: the lowest return per cell of an xy grid, the cells that are ground by a
 * morphological opening, the rest filled from their neighbours; then the height of every row above that ground and the
 * ground under any position - what a sag curve's ground clearance is measured against.
 *
 * The rule.  All arithmetic is float64 without FMA (the library is built with -ffp-contract=off), with parentheses as
 * written.  tests/terrain_cases.py follows it literally in numpy.
 *   Grid.  PchTerrainGrid { double x0, y0, cell; int32_t nx, ny; }, host side, with the conventions of PchPlaneGrid.
 *     cell > 0 and finite; nx, ny >= 1; nx * ny <= 2^24.  Anything else is PCH_ERR_ARG.  Cell c = fy * nx + fx.
 *   Row frame.  P = fl32(xyz[i] - sub3) per component.  This is a float32 subtraction, the arithmetic of
 *     raw - centroid, as in pch_dbscan_assign_f32.  sub3_host == NULL means no subtraction.  X, Y, Z = (double)P.
 *   Cell of a row.  fx = floor((X - x0) / cell) and fy = floor((Y - y0) / cell).  The row is inside the grid iff
 *     0 <= fx < nx and 0 <= fy < ny.  NaN and inf fail these comparisons.  A row takes part iff it is inside the grid,
 *     Z is finite, and skip[i] == 0.  skip is an optional uint8 [n].
 *   Lowest return (pch_terrain_low_f32).  count[c] (int32) is the number of rows that take part in cell c.  low[c]
 *     (float32) is the row value P.z with the smallest key, where
 *         key(z) = bits(z) ^ (bits(z) >> 31 ? 0xFFFFFFFF : 0x80000000)
 *     This is the usual order-preserving map, so -0.0 sorts below +0.0.  low[c] is NaN where count[c] == 0.
 *   Ground cells and fill (pch_terrain_ground_f32), with window radius R in cells (0 <= R <= 64), dh >= 0 finite, and
 *     gap G in cells (0 <= G <= 256).
 *     Opening.  Erosion then dilation with the square window (2R+1)^2, clipped at the grid edge.  Both are separable:
 *       first along x, then along y.  Erosion is the minimum over the window's non-NaN cells, NaN if there is none.
 *       Dilation is the maximum over the eroded grid's non-NaN cells, NaN if there is none.  All four passes are in
 *       float32.  They are exact, since min and max round nothing.  A pass walks its window in ascending index and
 *       replaces what it holds only by a value that compares smaller (larger): of -0.0 and +0.0 the first met stays.
 *       The result is open[c].
 *     Ground.  Cell c is ground iff low[c] is not NaN and ((double)low[c] - (double)open[c]) <= dh.  With R == 0, every
 *       cell that has a row is ground.
 *     Fill.  A ground cell gets ground[c] = low[c].  Any other cell looks in the four directions, in the order
 *       -x, +x, -y, +y.  In each direction it walks d = 1..G and takes the first ground cell.  It stops at the grid
 *       edge.  Start with num = 0.0; den = 0.0.  For each direction that found a cell, in that order, add
 *           num = num + ((double)low_k / (double)d_k)   and   den = den + (1.0 / (double)d_k)
 *       ground[c] = (float)(num / den) if a cell was found, otherwise NaN.
 *     State.  state[c] (uint8) has bit 0 set for ground, bit 1 for filled from neighbours, and bit 2 when the cell had
 *       rows (low not NaN).  So 5 is a ground cell, 6 is a cell with rows that was rejected and filled (a roof, a
 *       crown), 2 is an empty cell that was filled, and 0 or 4 has no ground value.
 *   Ground under a position, g(X, Y) in doubles.  One __device__ function serves both entry points below.
 *     The position's cell is (fx, fy) by the cell rule.  Outside the grid, g is NaN.
 *         u = ((X - x0) / cell) - 0.5
 *         i0 = floor(u), clamped to [0, max(nx - 2, 0)];  i1 = min(i0 + 1, nx - 1)
 *         a = u - (double)i0;  if a < 0: a = 0;  if a > 1: a = 1
 *     v, j0, j1 and b are the same along y.  With g00 = ground[j0][i0], g10 = ground[j0][i1], g01 = ground[j1][i0] and
 *     g11 = ground[j1][i1] as doubles: if none of the four is NaN,
 *         g = (((g00*(1 - a)) + (g10*a))*(1 - b)) + (((g01*(1 - a)) + (g11*a))*b)
 *     Otherwise g = (double)ground[fy][fx], which may be NaN.
 *     pch_terrain_height_f32 works on rows: out_height[i] = (float)(Z - g(X, Y)); the optional out_ground[i] = (float)g.
 *     A row with a non-finite coordinate gets NaN in both.  There is no skip here: every row is answered.
 *     pch_terrain_sample_f64 takes xy as double [m,2] and writes out double [m] = g, with no subtraction.
 *   Span ground clearance.  This needs no kernel of its own: torch arithmetic on K*(S+1) records plus one
 *     pch_terrain_sample_f64 call (ops.span_ground_profile).  The vertices j = 0..S of a piece's polyline are exactly
 *     the m_j, z_j of the polyline above (m_S = m1).  X = cx + (m*ux), Y = cy + (m*uy), W = cz + z,
 *     clr = W - g(X, Y).  Per piece: clearance and ground ([K, S+1] float64; NaN where g is NaN), covered (int64: the
 *     vertices with a ground value), min_clearance (the smallest clr over the covered vertices, +inf if there is
 *     none), min_vertex (the lowest j that attains it, -1 if none), min_at ([K,3] = (X, Y, g) at that vertex, NaN
 *     without one) and violation (min_clearance <= limit).  The polyline lies above the parabola by at most
 *     chord_error, so a ground clearance is over-estimated by at most that.
 *
 * How: tiles of 1024 rows are combined in an open-addressed table of 2048 slots in LDS (cell id, smallest key, count;
 * 1024 rows give at most 1024 distinct cells, so it cannot fill), and every occupied slot then issues one integer
 * atomicMin on the key grid and one atomicAdd on the counts; a small kernel decodes the keys.  The opening is four
 * grid-sized passes of 2R+1 reads, the fill one walk of at most 4*G reads per cell.  Integer atomics only, nothing waits
 * on another workgroup: the same input gives the same bits on every run.
 *
 * 0 <= n < 2^31 and 0 <= m < 2^31 (else PCH_ERR_ARG, as a grid, R, dh or G outside the limits above, a null buffer that
 * is needed and a host pointer where a device pointer is needed).  xyz float32 [n,3], skip uint8 [n] or NULL, low /
 * ground / out_open float32 [nx*ny], out_count int32 [nx*ny], out_state uint8 [nx*ny], out_height / out_ground float32
 * [n] - all device; sub3_host 3 floats on the host or NULL; grid_host on the host.  out_stats (int64 [2], device, may
 * be NULL): the rows that took part and the (tile, cell) flushes - figures for measurement, not part of the rule.  ws:
 * the caller's, at least the matching *_ws_bytes bytes - pure host code, 0 for sizes out of range (smaller:
 * PCH_ERR_WORKSPACE).  With n == 0, every cell is NaN with count 0, ground is NaN, and state is 0.  No launch reads a
 * null pointer.  Every call enqueues on the caller's stream and returns; no host read. */
typedef struct PchTerrainGrid {
    double  x0, y0, cell;     /* origin and cell edge in the row frame */
    int32_t nx, ny;           /* cells along x and y; cell c = fy * nx + fx */
} PchTerrainGrid;
#define PCH_TERRAIN_MAX_CELLS  (1 << 24)
#define PCH_TERRAIN_MAX_WINDOW 64
#define PCH_TERRAIN_MAX_GAP    256
size_t pch_terrain_low_ws_bytes(int64_t n, int32_t ncells);
int pch_terrain_low_f32(const float* xyz, const uint8_t* skip, int64_t n, const float* sub3_host,
                        const PchTerrainGrid* grid_host, float* out_low, int32_t* out_count,
                        int64_t* out_stats /* [2], may be NULL */, void* ws, size_t ws_bytes, void* stream);
size_t pch_terrain_ground_ws_bytes(int32_t ncells);
int pch_terrain_ground_f32(const float* low, const PchTerrainGrid* grid_host, int32_t window_cells, double dh,
                           int32_t max_gap, float* out_open /* may be NULL */, float* out_ground,
                           uint8_t* out_state, void* ws, size_t ws_bytes, void* stream);
int pch_terrain_height_f32(const float* xyz, int64_t n, const float* sub3_host, const PchTerrainGrid* grid_host,
                           const float* ground, float* out_height, float* out_ground /* may be NULL */, void* stream);
int pch_terrain_sample_f64(const double* xy, int64_t m, const PchTerrainGrid* grid_host, const float* ground,
                           double* out, void* stream);

/* ------------------------------------------------------------------ tower profile, opt-in
 * Where a tower has its cross-arms and how high it stands: per (table, height slice) the row count and the horizontal
 * extents of the grouped rows, in a horizontal frame per cluster.  Every output is a count or a minimum / maximum, so
 * it is exact, free of any order and the same bits on every run.
 *
 * The rule.  All arithmetic is float64 without FMA (the library is built with -ffp-contract=off), with parentheses as
 * written.  tests/tower_profile_cases.py follows it literally in numpy.
 *   Grouping is as in pch_cluster_moments_f32: cluster k owns rows_k = perm[offsets[k]:offsets[k+1]].  Entries at and
 *     behind offsets[K] belong to nobody.
 *   frames5[k] = (cx, cy, z0, ux, uy).  slot[k] is the table row that cluster k writes to.  T = ntables, B = nslices.
 *   Cluster k takes part iff 0 <= slot[k] < T and all five frame values are finite.  A slot of -1 or out of range, or a
 *     non-finite frame, takes no part.  u need not be unit.
 *   Per row p of a cluster that takes part:
 *         dx = (double)px - cx;  dy = (double)py - cy;  h = (double)pz - z0
 *         s = (dx*ux) + (dy*uy);  t = (dy*ux) - (dx*uy);  q = floor(h / dz)
 *     If q < 0: out_outside[slot,0] += 1.
 *     If q >= B: out_outside[slot,1] += 1.
 *     A NaN q counts nowhere.
 *     The row is binned iff 0 <= q < B and s and t are finite, with b = (int)q.  Then:
 *         out_count[slot,b] += 1;
 *         out_ext[slot,b] = (min s, max s, min t, max t), where min and max are taken by the order-preserving key of
 *         the double's bit pattern, key(v) = bits(v) ^ (bits(v) >> 63 ? 0xFFFFFFFFFFFFFFFF : 0x8000000000000000), so
 *         -0.0 sorts below +0.0.
 *   A slice without a row holds (+inf, -inf, +inf, -inf) and count 0.
 *   Clusters that share a slot are combined as if they were one.
 *   Limits: 0 <= n_grouped < 2^31, nclusters >= 0, 1 <= T <= 4096, 1 <= B <= 256, T*B <= 2^20, dz finite and > 0.
 *   Anything else is PCH_ERR_ARG, as is a needed null buffer or a host pointer.
 *   A workspace that is too small is PCH_ERR_WORKSPACE.
 *   pch_cluster_slices_ws_bytes is pure host code and returns 0 for sizes out of range.
 *   A refused call writes nothing.
 *   With n_grouped == 0 or K == 0 the tables are still written (zeros and infinities).
 *   The call enqueues and returns, with no host read.
 *   Levels (no kernel; ops.tower_levels: float64 torch on [T,B] records).  With min_rows, arm_window, arm_excess,
 *     max_levels and G = ceil(arm_window / dz): occ[b] = count[b] >= min_rows; w[b] = max(ext[b,1] - ext[b,0],
 *     ext[b,3] - ext[b,2]) where occupied, else NaN; body[b] = the smallest w[b'] over the occupied b' with
 *     |b' - b| <= G; arm[b] = occ[b] and (w[b] - body[b]) >= arm_excess.  A level is a maximal run [b_lo, b_hi] of arm
 *     slices, the lowest first, at most max_levels kept: z_low = z0 + b_lo*dz, z_high = z0 + (b_hi + 1)*dz,
 *     width = max w over the run, rows = the sum of count over the run.  top = z0 + (b_top + 1)*dz for the highest
 *     occupied slice, NaN without one.  An arm thicker than 2G + 1 slices is not found.
 *
 * How: perm is swept in fixed blocks of 512 entries, one wave each, as pch_cluster_moments_f32 sweeps it - the time is
 * linear in the number of grouped rows, not in the largest cluster.  A wave combines each (cluster, block) segment it
 * holds in its own LDS table of B slices (a count and four 64-bit keys) with integer LDS atomics, then looks at the
 * slices between the lowest and the highest one the segment touched: every occupied one issues one integer atomicAdd
 * and four 64-bit atomicMin / atomicMax on the global tables and is cleared again.  A small kernel decodes the keys.
 * Integer atomics only, no barrier, nothing waits on another workgroup.
 *
 * xyz float32 [*,3], perm int32 [n_grouped], offsets int64 [K+1], frames5 float64 [K,5], slot int32 [K], out_count int32
 * [T,B], out_ext float64 [T,B,4], out_outside int64 [T,2] - all device; perm entries are trusted to be rows of xyz.
 * xyz and perm may be NULL when n_grouped == 0 or K == 0; offsets, frames5 and slot when K == 0.  ws: the caller's, at
 * least pch_cluster_slices_ws_bytes(n_grouped, nclusters, ntables, nslices) bytes. */
#define PCH_SLICES_MAX         256
#define PCH_SLICES_MAX_TABLES  4096
#define PCH_SLICES_MAX_ENTRIES (1 << 20)
size_t pch_cluster_slices_ws_bytes(int64_t n_grouped, int32_t nclusters, int32_t ntables, int32_t nslices);
int pch_cluster_slices_f32(const float* xyz, const int32_t* perm, const int64_t* offsets, int64_t n_grouped,
                           int32_t nclusters, const double* frames5 /* [K,5] */, const int32_t* slot /* [K] */,
                           int32_t ntables, double dz, int32_t nslices,
                           int32_t* out_count /* [T,B] */, double* out_ext /* [T,B,4] */,
                           int64_t* out_outside /* [T,2] */, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ tree fall, opt-in
 * Which vegetation, standing where it stands, reaches a conductor if it falls towards the line: the distance from every
 * row's ground foot to the fitted span curves, held against that row's own height above the ground.
 *
 * The rule.  All arithmetic is float64 without FMA (the library is built with -ffp-contract=off); parentheses are as
 * written.  tests/treefall_cases.py follows it literally in numpy.
 *   Inputs.  xyz float32 [n,3]; an optional skip uint8 [n]; sub3_host, 3 floats on the host, or NULL; grid_host
 *     (PchTerrainGrid) and ground float32 [nx*ny], exactly as pch_terrain_height_f32 takes them; curves5 float64 [K,5]
 *     and segs float64 [K,S,5], exactly as pch_clearance_f32 takes them; h_min, h_max, grow, limit: doubles, all
 *     finite, with 0 <= h_min <= h_max, grow >= 0 and limit >= 0.  Anything else is PCH_ERR_ARG.
 *   Span participation.  A span takes part iff all 5 + 5*S of its values are finite (the clearance rule).
 *   Row frame and ground.  P = fl32(xyz[i] - sub3) and X, Y, Z = (double)P (the terrain rule).  g = g(X, Y) by the
 *     terrain rule's bilinear function; one __device__ function serves terrain and this call.
 *         H = Z - g
 *   Row participation.  A row takes part iff skip[i] == 0, X, Y, Z are finite, g is not NaN, and
 *         h_min <= H and H <= h_max
 *     A row that fails only the g test is tallied as uncovered.
 *   Reach.
 *         reach = H + grow;  s2 = reach*reach
 *         R = reach + limit;  R2 = R*R
 *   Distance.  Spans that take part are visited in ascending k.  The measured point is the foot (X, Y, g):
 *         dx = X - cx;  dy = Y - cy;  w = g - cz
 *     m, t, the segment loop over j and d2 = gmin + (t*t) are exactly as in the clearance rule, with this w:
 *         m = (dx*ux) + (dy*uy);  t = (dy*ux) - (dx*uy)
 *         gmin = +inf
 *         for j ascending:
 *             rm = m - m_j;  rw = w - z_j
 *             q = ((rm*dm_j) + (rw*dz_j))*inv_j
 *             if q < 0: q = 0
 *             if q > 1: q = 1
 *             em = rm - (q*dm_j);  ew = rw - (q*dz_j)
 *             d = (em*em) + (ew*ew)
 *             if d < gmin: gmin = d
 *         d2 = gmin + (t*t)
 *         if d2 <= R2 and d2 < best: best = d2; who = k
 *     Ties go to the lowest k.
 *   Per-row outputs.  out_dist2[i] (float64) is best; +inf if there is none or the row takes no part.  out_span[i]
 *     (int32) is who, or -1.  out_height[i] (float32) is (float)H for every row with finite coordinates, whether it
 *     takes part or not; otherwise it is NaN.  It equals pch_terrain_height_f32's out_height bit for bit (NaN where g is
 *     NaN).  out_class[i] (uint8) is one of
 *         PCH_TREEFALL_CLEAR  = 0: no span within R, or the row takes no part
 *         PCH_TREEFALL_NEAR   = 1: best <= R2 and best > s2 - the row comes within limit of a conductor after falling
 *         PCH_TREEFALL_STRIKE = 2: best <= s2 - the row strikes
 *   Per-span outputs, over the rows with out_span[i] == k: out_count[k] (int64); out_strikes[k] (int64): the rows of
 *     class 2; out_min_dist2[k] (float64): +inf if there is no row; out_min_row[k] (int64): the lowest row that attains
 *     it, or -1; out_max_height[k] (float32): the largest out_height by the order-preserving key (key(z) of the terrain
 *     rule), NaN without a row; out_max_row[k] (int64): the lowest row that attains it, or -1.
 *   Statistics.  out_stats (int64 [4], may be NULL): [0] the rows that took part and [1] the uncovered rows are part of
 *     the rule; [2] the (row, span) segment loops run and [3] the (tile, span) pairs walked are figures for measurement
 *     only.
 * Every row is attributed to its NEAREST span within its own R only, by the distance of its FOOT: the row's own position
 * enters through H alone.
 *
 * How: pch_clearance_f32's bounds kernel runs at radius Rmax = (h_max + grow) + limit.  Rounding is monotone, so every
 * row that takes part has R <= Rmax and the bounds' derivation holds unchanged.  A sweep over tiles of 1024 rows samples
 * the ground under every row once, boxes the FEET (X, Y, g) of the rows that take part and walks, in ascending order,
 * the spans whose bounds meet that box; the tests in front of the segment loop use the row's own R2.  A finisher finds
 * the lowest rows of the two extremes.  Culling skips only what the rule cannot accept: the outputs are the rule's,
 * whatever is culled.  The tallies are integer atomics, the minimum an integer atomic on the bit pattern, the maximum
 * one on the key: the same input gives the same bits on every run; nothing waits on another workgroup.
 *
 * 0 <= n < 2^31, 0 <= nspans <= 4096, 1 <= nsegments <= 128; the grid limits are terrain's (else PCH_ERR_ARG, as a null
 * buffer that is needed and a host pointer).  All buffers device, except sub3_host and grid_host.  ws: the caller's, at
 * least pch_treefall_ws_bytes(n, nspans, nsegments) bytes - pure host code, 0 for sizes out of range (smaller:
 * PCH_ERR_WORKSPACE).  n == 0 or nspans == 0: every row gets +inf / -1 / class 0 and its height, the table is
 * (0, 0, +inf, -1, NaN, -1) per span, and no launch reads a null pointer.  Enqueues on the caller's stream and returns;
 * no host read. */
#define PCH_TREEFALL_CLEAR  0
#define PCH_TREEFALL_NEAR   1
#define PCH_TREEFALL_STRIKE 2
size_t pch_treefall_ws_bytes(int64_t n, int32_t nspans, int32_t nsegments);
int pch_treefall_f32(const float* xyz, const uint8_t* skip, int64_t n, const float* sub3_host,
                     const PchTerrainGrid* grid_host, const float* ground, const double* curves5 /* [K,5] */,
                     const double* segs /* [K,S,5] */, int32_t nspans, int32_t nsegments, double h_min, double h_max,
                     double grow, double limit, double* out_dist2, int32_t* out_span, float* out_height,
                     uint8_t* out_class, int64_t* out_count, int64_t* out_strikes, double* out_min_dist2,
                     int64_t* out_min_row, float* out_max_height, int64_t* out_max_row,
                     int64_t* out_stats /* [4], may be NULL */, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ wind swing clearance, opt-in
 * The distance of every row of a cloud to the conductors under the largest wind deviation: each wire swung sideways
 * about the line between its attachment points, towards the row, by at most the angle Theta.
 *
 * The rule.  All arithmetic is float64 without FMA (the library is built with -ffp-contract=off); parentheses are as
 * written.  The only other operations are / and sqrt, both IEEE correctly rounded.  There is no trigonometry on the
 * device: the host supplies sin Theta and cos Theta.  tests/swing_cases.py follows it literally in numpy.
 *   Model.  A wire point at station m hangs f(m) = zc(m) - z(m) below the chord, where the chord runs through the
 *     polyline's two ends.  Under wind this hanging vector turns about the horizontal along-track axis through the chord
 *     point, by an angle in [-Theta, Theta].  The swung point is (m, f*s, z + f*(1 - c)) in the span frame (along the
 *     track, lateral, height); (s, c) is the sine and cosine of the turn.  At rest s = 0 and c = 1, and the vertex is
 *     exactly (m, 0, z).  Insulator strings swinging with the wire are not modelled.
 *   Tables (no kernel; ops.swing_heads, ops.swing_segments), from ops.span_curves' [K,10].  The vertices m_j, z_j for
 *     j = 0..S are exactly those of ops.span_segments (the polyline of the clearance rule).
 *         kap = (z_S - z_0) / (m_S - m_0)
 *         zc_j = z_0 + ((m_j - m_0)*kap)
 *         f_j = zc_j - z_j
 *     Segment record, float64 [K,S,6] = (m_j, z_j, f_j, dm_j, dz_j, df_j), with dm_j = m_{j+1} - m_j,
 *     dz_j = z_{j+1} - z_j and df_j = f_{j+1} - f_j.  Head record, float64 [K,11] = (cx, cy, cz, ux, uy, mA, mB, zA, kap,
 *     sT, cT), with mA = m_0, mB = m_S, zA = z_0, sT = sin Theta and cT = cos Theta.
 *   Span participation.  A span takes part if and only if all 11 + 6*S values are finite, mB > mA, 0 <= sT <= 1,
 *     0 < cT <= 1 and |((sT*sT) + (cT*cT)) - 1| <= 1e-6.
 *   Per row and span (pch_swing_clearance_f32).  Rows, skip, radius, limit, r2 and l2 are exactly as in
 *     pch_clearance_f32.  Spans are visited in ascending k:
 *         dx, dy, w, m, t                       as in pch_clearance_f32
 *         mh = m;  if mh < mA: mh = mA;  if mh > mB: mh = mB
 *         bb = (zA + ((mh - mA)*kap)) - w                     # depth of the row below the chord at its own station
 *         if bb > 0 and (fabs(t)*cT) <= (bb*sT):              # inside the swing sector: the wire can point at the row
 *             rho = sqrt((t*t) + (bb*bb));  s = t/rho;  c = bb/rho
 *         else:                                               # the end of the sector on the row's side
 *             s = (t >= 0) ? sT : -sT;  c = cT
 *         e = 1.0 - c
 *         g = +inf
 *         for j ascending:
 *             py = f_j*s;  pw = z_j + (f_j*e);  ey = df_j*s;  ez = dz_j + (df_j*e)
 *             rm = m - m_j;  rt = t - py;  rw = w - pw
 *             len2 = ((dm_j*dm_j) + (ey*ey)) + (ez*ez)
 *             q = len2 > 0 ? (((rm*dm_j) + (rt*ey)) + (rw*ez)) / len2 : 0
 *             if q < 0: q = 0
 *             if q > 1: q = 1
 *             vm = rm - (q*dm_j);  vt = rt - (q*ey);  vw = rw - (q*ez)
 *             d = ((vm*vm) + (vt*vt)) + (vw*vw);  if d < g: g = d
 *         if g <= r2 and g < best: best = g; who = k; sin = s
 *   Row outputs.  out_dist2[i] (float64) = best, out_span[i] (int32) = who and out_sin[i] (float64) = sin: the sine of
 *     the angle at which the winning span is nearest; its sign tells the side.  A row without a span gets +inf, -1 and
 *     NaN.  So does a skipped row and a row with a non-finite coordinate.  Ties go to the lowest span index.
 *   Span outputs.  The same table as the clearance call, over each row's nearest span only: out_count, out_violations
 *     (dist2 <= l2), out_min_dist2, out_min_row.  out_loops is also as there.
 * One angle per (row, span): the angle is chosen in the row's own cross-section; distance is then measured to the whole
 * polyline swung to that angle.  With sT = 0, cT = 1 the call is the clearance call's geometry; the roundings differ (a
 * division per segment, a three-term sum), so agreement with pch_clearance_f32 is to rounding, not to the bit.
 *
 * How: a small kernel over the spans writes the "takes part" flag and conservative bounds of the whole swung family,
 * widened by the radius; a sweep over tiles of 1024 rows walks, in ascending order, the spans whose bounds meet the
 * tile's own bounding box; pch_clearance_f32's finisher finds the lowest row of every minimum.  Culling skips only what
 * the rule cannot accept: the outputs are the rule's, whatever is culled.  The same input gives the same bits on every
 * run; nothing waits on another workgroup.
 *
 * 0 <= n < 2^32, 0 <= nspans <= 4096, 1 <= nsegments <= 128 (else PCH_ERR_ARG, as a radius or limit that is not
 * finite, limit <= 0, limit > radius, a null buffer that is needed and a host pointer).  All buffers device; skip may
 * be NULL; out_loops (int64 [2]) may be NULL.  ws: the caller's, at least pch_swing_clearance_ws_bytes(n, nspans,
 * nsegments) bytes - pure host code, 0 for sizes out of range (smaller: PCH_ERR_WORKSPACE).  n == 0 or nspans == 0:
 * every row gets +inf / -1 / NaN, the table is (0, 0, +inf, -1) per span, and no launch reads a null pointer.  Enqueues
 * on the caller's stream and returns; no host read. */
size_t pch_swing_clearance_ws_bytes(int64_t n, int32_t nspans, int32_t nsegments);
int pch_swing_clearance_f32(const float* xyz, const uint8_t* skip, int64_t n, const double* heads /* [K,11] */,
                            const double* segs /* [K,S,6] */, int32_t nspans, int32_t nsegments, double radius,
                            double limit, double* out_dist2, int32_t* out_span, double* out_sin, int64_t* out_count,
                            int64_t* out_violations, double* out_min_dist2, int64_t* out_min_row,
                            int64_t* out_loops /* [2], may be NULL */, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ span sections, opt-in
 * The longitudinal section of every span: station by station along the wire, how many rows lie in the corridor under
 * it, how many of them within the vertical limit, how far below the wire the highest one is and which row that is; and
 * for every row the span and station where a wire hangs lowest above it.
 *
 * The rule.  All arithmetic is float64 without FMA (the library is built with -ffp-contract=off); parentheses are as
 * written.  The only other operations are one division, floor and the cast to float32.  tests/section_cases.py follows
 * it literally in numpy.
 *   Inputs.  xyz float32 [n,3]; an optional skip uint8 [n]; curves10 float64 [K,10] = (cx, cy, cz, ux, uy, a, b, c, m0,
 *     m1), exactly ops.span_curves' records; B stations, 1 <= B <= 128; half (the corridor's half width), depth and
 *     limit, all finite, with half > 0 and 0 < limit <= depth.
 *   Span participation.  A span takes part if and only if all ten of its values are finite and m1 > m0.  Its step is
 *     step = (m1 - m0) / (double)B.
 *   Per row and span (pch_span_section_f32).  For row i with skip[i] == 0, spans are visited in ascending k:
 *         dx = (double)px - cx;  dy = (double)py - cy;  w = (double)pz - cz
 *         m = (dx*ux) + (dy*uy);  t = (dy*ux) - (dx*uy)
 *         in the corridor iff  m >= m0 and m <= m1 and t >= -half and t <= half
 *         zw = a + (m*(b + (c*m)));  v = zw - w                 # the wire above the row: v > 0
 *         takes part iff in the corridor and v >= 0.0 and v <= depth
 *         j = (int)floor((m - m0) / step);  if j > B - 1: j = B - 1
 *         vf = fabsf((float)v)                                  # float32; the cast is monotone: min commutes with it
 *     A NaN fails every comparison.  A row with a non-finite coordinate, or a skipped row, takes part nowhere.
 *   The wire height is the parabola itself, not the polyline of pch_clearance_f32: the two differ, vertically, by at
 *     most that rule's chord_error.  v is a vertical distance, t a horizontal one: neither is the spatial clearance.
 *   Per cell (k, j), over EVERY row that takes part in span k - a row under three phases counts in all three; this is
 *     not the nearest-only attribution of pch_clearance_f32: out_count[k][j] (int64): the rows; out_violations[k][j]
 *     (int64): those with v <= limit, tested on the double; out_min_v[k][j] (float32): the smallest vf, +inf for an
 *     empty cell; out_min_row[k][j] (int64): the lowest row index that attains the smallest vf, or -1.
 *   Per row: out_v[i] (float32): the smallest vf over the spans the row takes part in, or +inf; out_span[i] (int32):
 *     the lowest k that attains it, or -1; out_station[i] (int32): its j in that span, or -1.
 *
 * How: a small kernel over the spans writes the "takes part" flag and a cull record - a world box around the corridor
 * rectangle and the heights a row under the wire can have, widened for the roundings of m, t and zw; a sweep over tiles
 * of 1024 rows walks, in ascending order, the spans whose record meets the tile's own bounding box.  Culling skips only
 * spans the rule cannot accept: the outputs are the rule's, whatever is culled.  A cell's smallest vf and its lowest row
 * travel in one 64-bit key (bits(vf) << 32) | i - vf >= 0, so its bits order as integers - folded with an integer
 * atomic minimum.  Every tile first combines its rows per station in LDS and adds each station that is not empty to the
 * cell once per (tile, span): a cell that thousands of rows fall into receives two atomics per tile - the key and the
 * packed tally -, not two per row.  A last kernel decodes the keys and the tallies.  Integer atomics only: the same
 * input gives the same bits on every run; nothing waits on another workgroup.
 *
 * 0 <= n < 2^32, 0 <= nspans <= 4096, 1 <= nstations <= 128 (else PCH_ERR_ARG, as a half_width, depth or limit that is
 * not finite, half_width <= 0, limit <= 0, limit > depth, a null buffer that is needed and a host pointer).  All
 * buffers device; the cell tables are [K,B], row-major; skip may be NULL (no row is skipped); out_stats (int64 [3], may
 * be NULL): the (row, span) pairs that took part, the (tile, span) pairs walked and the cell flushes (atomics on a
 * cell's key) - figures for measurement, not part of the rule.  ws: the caller's, at least
 * pch_span_section_ws_bytes(n, nspans, nstations) bytes - pure host code, 0 for sizes out of range (smaller:
 * PCH_ERR_WORKSPACE).  n == 0 or nspans == 0: every row gets +inf / -1 / -1, every cell (0, 0, +inf, -1), and no launch
 * reads a null pointer.  Enqueues on the caller's stream and returns; no host read. */
size_t pch_span_section_ws_bytes(int64_t n, int32_t nspans, int32_t nstations);
int pch_span_section_f32(const float* xyz, const uint8_t* skip, int64_t n, const double* curves10 /* [K,10] */,
                         int32_t nspans, int32_t nstations, double half_width, double depth, double limit,
                         float* out_v, int32_t* out_span, int32_t* out_station, int64_t* out_count /* [K,B] */,
                         int64_t* out_violations /* [K,B] */, float* out_min_v /* [K,B] */,
                         int64_t* out_min_row /* [K,B] */, int64_t* out_stats /* [3], may be NULL */, void* ws,
                         size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ canopy grid and tree crowns, opt-in
 * The vegetation as trees: the tallest return above the ground per cell of a fine xy grid (the canopy height model),
 * the cells that are tree tops, the crown of cells that belongs to every top, one table record per tree, and for every
 * row the tree it belongs to.
 *
 * The rule.  Arithmetic is float64 without FMA (the library is built with -ffp-contract=off), with parentheses as
 * written; comparisons of sm are float32 comparisons.  tests/canopy_cases.py follows it literally in numpy.
 *   Frames and participation.  The row frame, the cell rule and PchTerrainGrid are the terrain rule's.  Two grids take
 *     part: the terrain grid with its ground array, as pch_terrain_height_f32 takes them, and a canopy grid, a second
 *     PchTerrainGrid in the same frame, usually finer, with at most PCH_TERRAIN_MAX_CELLS cells.
 *         g = g(X, Y) on the terrain grid;  Hd = Z - g;  H = (float)Hd
 *     A row takes part iff skip[i] == 0, X, Y, Z are finite, it is inside the canopy grid, g is not NaN, and
 *         h_min <= Hd and Hd <= h_max
 *     tested on the double, as in the tree-fall rule.  0 <= h_min <= h_max, both finite.  One __device__ function
 *     decides this for pch_canopy_top_f32 and pch_canopy_rows_f32: the two never disagree.
 *   1. Canopy top (pch_canopy_top_f32).  Per canopy cell c: count[c] (int32) is the number of rows that take part;
 *     top[c] (float32) is the H with the largest key(H) of the terrain rule, so -0.0 sorts below +0.0, NaN where
 *     count[c] == 0; top_row[c] (int32) is the lowest row index that attains it, -1 without a row.  The optional
 *     out_height (float32 [n]) is H for every row with finite coordinates, whether it takes part or not, NaN where g is
 *     NaN and for a row that is not finite: pch_terrain_height_f32's out_height bit for bit.  The optional out_stats
 *     (int64 [2]): the rows that took part and the (tile, cell) flushes - figures for measurement, not part of the rule.
 *   2. Smoothing, with radius S in cells, 0 <= S <= PCH_CANOPY_MAX_SMOOTH.  sm[c] is NaN iff top[c] is NaN: empty cells
 *     are not filled.  Otherwise, over the square window (2S+1)^2 clipped at the grid edge, fy ascending outside and fx
 *     ascending inside: start with sum = 0.0; cnt = 0; for each non-NaN top[c'] in that order
 *         sum = sum + (double)top[c'];  cnt = cnt + 1
 *     and then sm[c] = (float)(sum / (double)cnt).  With S == 0, sm == top bit for bit.
 *   3. The order "beats", on cells whose sm is not NaN.
 *         c' beats c iff sm[c'] > sm[c], or sm[c'] == sm[c] and c' < c
 *     in float32, so -0.0 and +0.0 tie and the index decides.  A strict total order; "the greatest" of a set is the one
 *     that beats all others.
 *   4. Window of a cell.
 *         r = r0 + (r1 * (double)sm[c]);  W = (int)floor(r / cell), clamped to [1, PCH_CANOPY_MAX_WINDOW]
 *     with r0 >= 0 and r1 >= 0, both finite (W = 1 should r / cell be NaN).  The window of c is the set of cells
 *     c' != c inside the grid with integer dx*dx + dy*dy <= W*W whose sm is not NaN.
 *   5. Tree tops.  c is a top iff sm[c] is not NaN, (double)sm[c] >= top_min, and no cell of its window beats it.
 *     top_min is finite and >= 0.
 *   6. Parent, for every cell with non-NaN sm.  Let b be the greatest of its up to eight neighbours (clipped at the
 *     edge, non-NaN only).  If b exists and beats c, parent[c] = b.  Otherwise, if some cell of its window beats c,
 *     parent[c] is the greatest cell of the window.  Otherwise parent[c] = c.  Every step goes to a cell that beats the
 *     one before, so chains end in a fixed point root[c]: a top, or a cell below top_min.
 *   7. Crowns.  Tops are numbered t = 0, 1, ... in ascending cell index.  With the crown radius Rc in cells,
 *     1 <= Rc <= PCH_CANOPY_MAX_CROWN, and crown_frac in [0, 1]: tree[c] = t iff sm[c] is not NaN, root[c] is top t,
 *         (double)sm[c] >= (crown_frac * (double)sm[root[c]])
 *     and integer (64-bit) dx*dx + dy*dy <= Rc*Rc from the root cell.  Otherwise tree[c] = -1.
 *   8. Tree table, per tree t: top_cell (int32): the cell of the top; cells (int32): the crown cells, the top among
 *     them; rows (int64): the sum of count over the crown; max_height (float32): the largest top[c] over the crown by
 *     key(.); max_row (int32): the lowest top_row[c] among the crown cells that attain max_height.  The tables have
 *     tree_cap entries, 1 <= tree_cap <= PCH_TERRAIN_MAX_CELLS.  out_ntrees (int32 [1]) holds the true number of tops;
 *     trees >= tree_cap are not written to the tables, tree[] keeps the true ids.  Entries from the number of tops on
 *     read (-1, 0, 0, NaN, -1).
 *   9. Rows (pch_canopy_rows_f32).  out_tree[i] (int32) is tree[] of the row's canopy cell for a row that takes part,
 *     and -1 otherwise.
 *
 * How: step 1 sweeps tiles of 1024 rows (every row and skip load issued before anything is waited for), combining a
 * tile's rows in an open-addressed table of 2048 slots in LDS - cell id, the 64-bit key (key(H) << 32) | ~row, whose
 * largest value is the tallest return and among equals the lowest row, and a count; 0 is "empty" - and every occupied
 * slot then issues one 64-bit atomicMax on a key grid and one atomicAdd on count; a small kernel decodes the keys.  Only
 * rows that take part reach the table.  The grid-sized steps are one thread per cell: (2S+1)^2 reads for sm, the window
 * and the neighbours for tops and parents, ceil(log2(cells)) rounds of pointer doubling between two buffers for the
 * roots, a three-launch ordered count / scan / number of the top flags, then crown and table by integer atomics per
 * tree (max_height and max_row in one 64-bit atomicMax of the same packing).  Integer atomics only, nothing waits on
 * another workgroup: the same input gives the same bits on every run.
 *
 * 0 <= n < 2^31; the limits of both grids are terrain's (else PCH_ERR_ARG, as h_min, h_max, S, r0, r1, top_min,
 * crown_frac, Rc or tree_cap outside the limits above, a null buffer that is needed and a host pointer where a device
 * pointer is needed; an argument error writes nothing).  xyz float32 [n,3], skip uint8 [n] or NULL, ground float32 over
 * the terrain grid; top / out_smooth float32, top_row / count / tree int32 over the canopy grid; the five tables
 * [tree_cap] - all device; sub3_host 3 floats on the host or NULL; the grids on the host.  ws: the caller's, at least
 * the matching *_ws_bytes bytes - pure host code, 0 for sizes out of range (smaller: PCH_ERR_WORKSPACE);
 * pch_canopy_rows_f32 needs none.  With n == 0 every cell is (NaN, -1, 0) and no launch reads a null pointer.  Every call
 * enqueues on the caller's stream and returns; no host read. */
#define PCH_CANOPY_MAX_SMOOTH 8
#define PCH_CANOPY_MAX_WINDOW 32
#define PCH_CANOPY_MAX_CROWN  256
size_t pch_canopy_top_ws_bytes(int64_t n, int32_t ncells);
int pch_canopy_top_f32(const float* xyz, const uint8_t* skip, int64_t n, const float* sub3_host,
                       const PchTerrainGrid* terrain_host, const float* ground, const PchTerrainGrid* canopy_host,
                       double h_min, double h_max, float* out_top, int32_t* out_top_row, int32_t* out_count,
                       float* out_height /* [n], may be NULL */, int64_t* out_stats /* [2], may be NULL */, void* ws,
                       size_t ws_bytes, void* stream);
size_t pch_canopy_trees_ws_bytes(int32_t ncells, int32_t tree_cap);
int pch_canopy_trees_f32(const float* top, const int32_t* top_row, const int32_t* count,
                         const PchTerrainGrid* canopy_host, int32_t smooth, double r0, double r1, double top_min,
                         double crown_frac, int32_t crown_cells, int32_t tree_cap, float* out_smooth /* may be NULL */,
                         int32_t* out_tree, int32_t* out_ntrees /* [1] */, int32_t* out_top_cell, int32_t* out_cells,
                         int64_t* out_rows, float* out_max_height, int32_t* out_max_row, void* ws, size_t ws_bytes,
                         void* stream);
int pch_canopy_rows_f32(const float* xyz, const uint8_t* skip, int64_t n, const float* sub3_host,
                        const PchTerrainGrid* terrain_host, const float* ground, const PchTerrainGrid* canopy_host,
                        double h_min, double h_max, const int32_t* tree, int32_t* out_tree, void* stream);

/* ------------------------------------------------------------------ stage D1, fast mode
 * The reference boxes every cluster with trimesh (utils/tower_extraction.py:137-139:
 * trimesh.PointCloud(cluster_points).bounding_box_oriented): qhull's 3-D hull of the whole cluster, then a
 * search over the hull's facet normals.  These two calls take the bandwidth part and the candidate search
 * off the Python host; the hull itself stays with qhull (pointcloudhookup_amd/obb.py:boxes_fast).
 *
 * pch_obb_shell_f32: for every cluster of the grouped rows (perm / offsets as written by
 * pch_segment_by_label) marks the points that can be vertices of the cluster's convex hull: a point
 * strictly inside a tetrahedron spanned by points of the cluster (support points in 218 fixed directions
 * and their mean) is dropped, everything else - a superset of the hull's vertices, about 1 % - is kept.
 * Clusters of fewer than 2048 points are kept whole.
 * xyz [*,3] float32; perm [n_grouped] int32; offsets [nclusters+1] int64 (device), offsets[nclusters] ==
 * n_grouped; out_keep [n_grouped] uint8 in grouped order. */
size_t pch_obb_shell_ws_bytes(int32_t nclusters);
int pch_obb_shell_f32(const float* xyz, const int32_t* perm, const int64_t* offsets, int32_t nclusters,
                      int64_t n_grouped, uint8_t* out_keep, void* ws, size_t ws_bytes, void* stream);
/* HOST function (no device work): minimum-volume boxes of many convex hulls by trimesh's procedure
 * (bounds.oriented_bounds: facet normals folded to a hemisphere, de-duplicated at 0.1 rad in spherical
 * coordinates, per candidate the minimum-area rectangle of the projected vertices, smallest volume wins),
 * on `nthreads` C++ threads (0: all cores).  All pointers are HOST pointers.
 * verts [sum nv,3] float64 hull vertices, vert_offsets [nhulls+1]; tris [sum nt,3] int32 indices into the
 * hull's own vertices (qhull's simplices), tri_offsets [nhulls+1]; sorted_extents: 0 = [rect_long,
 * rect_short, normal_extent], 1 = ascending with permuted axes (current trimesh).
 * out_to_origin [nhulls,16] row-major 4x4 (world -> box frame), out_extents [nhulls,3],
 * out_status [nhulls]: 0 ok, 1 = no candidate (degenerate hull). */
int pch_obb_min_boxes_f64(const double* verts, const int64_t* vert_offsets, const int32_t* tris,
                          const int64_t* tri_offsets, int32_t nhulls, int32_t sorted_extents,
                          int32_t nthreads, double* out_to_origin, double* out_extents, int32_t* out_status);

/* ------------------------------------------------------------------ stage D1, upright mode (opt-in)
 * A transmission tower stands upright: the box its height, width and north angle presume has z as one axis and the
 * smallest rectangle around the footprint as the other two.  That box is minima and maxima only, so it is order-free
 * and can be stated in numpy and checked bit for bit (tests/upright_cases.py); it needs no hull and no host copy of the
 * clustered points.
 *
 * The rule.  Constants: PCH_UPRIGHT_COARSE = 128, PCH_UPRIGHT_FINE = 32, T = 4096 = 128 * 32.
 * Angle table: cs[j] = (cos th_j, sin th_j) with th_j = j * (pi/2) / T as float64, computed with numpy on the host and
 * passed in as a device array [T,2]; the kernels never evaluate a sine or a cosine, so device libm cannot enter the
 * result.
 * Input: P, the kept, centred float32 rows; cluster k owns perm[offsets[k]:offsets[k+1]] as written by
 * pch_segment_by_label.  For every cluster:
 *   1 status = 1 (no box) if the cluster has no rows or any coordinate of any of its rows is not finite; then
 *     j = j0 = -1 and the six bounds are NaN.  Otherwise status = 0.
 *   2 rectangle at table index j: x, y as float64 of the float32 coordinates, (c, s) = cs[j]; u = x*c + y*s and
 *     v = y*c - x*s (two products and one add or subtract each, no FMA); umin, umax, vmin, vmax are the minima and
 *     maxima over the cluster's rows; area(j) = (umax - umin) * (vmax - vmin) in float64, from the bounds of the WHOLE
 *     cluster.
 *   3 level 0: j0 is the index among {a * 32 : a = 0..127} with the smallest area; ties go to the smallest index.
 *   4 level 1: the candidates are {(j0 + d) mod T : d = -31..31} (63 of them, d = 0 among them; wrapping past 0 or T is
 *     the same rectangle with u and v exchanged); j is the candidate with the smallest area, ties go to the smallest
 *     table index.
 *   5 zmin, zmax are the extremes of the float32 z values, stored as float64.
 *   6 the record PchUprightBox (72 bytes), the four rectangle bounds taken at j.
 * Bounds are compared by value (-0.0 equals +0.0).
 * Quality: a set inside a du x dv rectangle has, at an angle delta away, widths at most du cos d + dv sin d and
 * dv cos d + du sin d; some coarse angle lies within h = pi/512 of the optimum and level 1 can only improve on level 0,
 * so the found area is at most A_opt * (1 + h (r + 1/r) + h^2) for a footprint of aspect r.
 *
 * pch_upright_boxes_f32: xyz [*,3] float32; perm [n_rows_cap] int32; offsets [nclusters+1] int64 (device); n_rows_cap
 * is the number of perm entries, an upper bound of offsets[nclusters], used only to size grids and the workspace
 * (offsets beyond it are clamped to it); cs_table_dev [4096,2] float64 (device); out_boxes [nclusters].  Enqueues and
 * returns: no host read, no float atomics, nothing that waits on another workgroup.  A cluster is spread over up to
 * min(1024, 16384 / nclusters) workgroups, so with very many clusters the time is linear in the largest one.
 * nclusters == 0: success, no work; negative counts or NULL pointers: PCH_ERR_ARG; ws_bytes below
 * pch_upright_boxes_ws_bytes(nclusters, n_rows_cap): PCH_ERR_WORKSPACE; a host pointer as the table: PCH_ERR_ARG. */
#define PCH_UPRIGHT_COARSE 128
#define PCH_UPRIGHT_FINE   32
typedef struct PchUprightBox {
    int32_t status, j, j0, reserved;
    int64_t n;
    double  umin, umax, vmin, vmax, zmin, zmax;
} PchUprightBox;
size_t pch_upright_boxes_ws_bytes(int32_t nclusters, int64_t n_rows_cap);
int pch_upright_boxes_f32(const float* xyz, const int32_t* perm, const int64_t* offsets, int32_t nclusters,
                          int64_t n_rows_cap, const double* cs_table_dev, PchUprightBox* out_boxes, void* ws,
                          size_t ws_bytes, void* stream);

/* HOST function: the search alone, for the exact mode. The caller (pointcloudhookup_amd/obb.py) lets qhull
 * build the hull of the FULL cluster and derives the candidate directions exactly as trimesh does; this call
 * evaluates the box volume of every candidate and names the winner, which the caller then evaluates once
 * more with the reference's own arithmetic - so the result is the python loop's, at 1/50 of its cost.
 * angles [sum nc,2] float64 (theta, phi) in evaluation order, angle_offsets [nhulls+1].
 * out_best [nhulls] int32: index of the first candidate of smallest volume (-1: none);
 * out_volumes [sum nc]: box volume per candidate (inf: no rectangle) - a caller that wants the python loop's
 * winner even when candidates tie in the last bits re-evaluates those that come within its tolerance of the
 * smallest. */
int pch_obb_search_f64(const double* verts, const int64_t* vert_offsets, const double* angles,
                       const int64_t* angle_offsets, int32_t nhulls, int32_t nthreads,
                       int32_t* out_best, double* out_volumes);

/* ------------------------------------------------------------------ viewer helpers
 * Axis-aligned crop, bounds INCLUSIVE, order preserving:
 *   points[(x>=x0)&(x<=x1)&(y>=y0)&(y<=y1)&(z>=z0)&(z<=z1)]
 * Replaces: the per-tower mask + gather of test/kuangxuan.py:69-79 (the box a tower's kuangxuan wire frame shows).
 * xyz [n,3] float64; out_points [n,3] float64 capacity; out_index [n] int64 (may be NULL): source rows;
 * out_count [1] int64.  Rows holding NaN fail the comparisons and are dropped, as in numpy. */
size_t pch_crop_aabb_ws_bytes(int64_t n);
int pch_crop_aabb_f64(const double* xyz, int64_t n, const double* min3_host, const double* max3_host,
                      double* out_points, int64_t* out_index, int64_t* out_count,
                      void* ws, size_t ws_bytes, void* stream);

/* Crop by MANY boxes in one sweep of the cloud, axis-aligned and oriented ones mixed: the points of every tower box of
 * a tile at once, instead of one pch_crop_aabb_f64 call (one sweep, one [n,3] buffer, one host read) per tower.
 * Replaces: the per-tower mask + gather of test/kuangxuan.py:60-79, and the same over the scaled oriented boxes of
 * ui/extract.py:345-420 (the tower dict's center / rotation / extent, which the non-default wire frame draws).
 *
 * kind 0  the predicate of pch_crop_aabb_f64: six inclusive comparisons of the raw float64 coordinates with lo / hi.  A
 *         row or a bound holding NaN fails them; lo > hi is an empty box, not an error.
 * kind 1  float64, no contraction, in exactly this order: d = p - center per component;
 *         u_k = (d_x*R[0][k] + d_y*R[1][k]) + d_z*R[2][k] with R = axes, row-major, whose COLUMNS are the box axes;
 *         inside iff -half_k <= u_k <= half_k for k = 0, 1, 2.  A NaN anywhere gives not inside.  We believe this is
 *         what Open3D's OrientedBoundingBox::GetPointIndicesWithinBoundingBox computes; Open3D was not at hand when
 *         this was written, so parity is with this formula, not with Open3D.
 * Output, grouped by box, boxes ascending, inside a box rows ascending (the order of points[mask]); a row inside
 * several boxes appears once in each:
 *   out_offsets [nboxes+1] int64 (device): box t owns [offsets[t], offsets[t+1]) of out_points / out_index
 *   out_points  [cap,3] float64, out_index [cap] int64 (may be NULL): the rows and their source rows
 *   out_count   [1] int64: the total number of hits
 * cap is a capacity, not a promise: if there are more hits than cap, *out_count still holds the true total and
 * out_offsets the complete, true table, nothing is written at or beyond cap, and what lies below cap is undefined -
 * call again with cap >= *out_count (pch_strip_lattice_reps_f32 works the same way; ops.crop_boxes retries once).
 * Limits: n < 2^32; nboxes <= 4096 - more, or a kind other than 0 and 1: PCH_ERR_ARG; n == 0 or nboxes == 0: success,
 * offsets and count zeroed.  The hits must number fewer than 2^31: cap >= 2^31 gives PCH_ERR_RANGE at once; the
 * call reads nothing back, so a total of 2^31 or more shows in *out_count only (offsets and count are kept in 64
 * bits and stay true), and whoever reads the count reports PCH_ERR_RANGE (ops.crop_boxes does).  A workspace
 * below the ws_bytes function's figure for the same (n, nboxes, cap): PCH_ERR_WORKSPACE.  Enqueues and returns: no host
 * read.  boxes_host has been copied when the call returns.  A bounded wait that ran out (above, PCH_ERR_TIMEOUT)
 * leaves *out_count negative, as pch_crop_aabb_f64 does.
 *
 * The sweep takes the cloud in tiles of 2048 rows and tests a tile only against the boxes whose cull bounds meet the
 * bounding box of the tile's finite rows.  pch_crop_box_bounds_f64 - a HOST function, no device work, all pointers
 * host pointers - returns those bounds, [nboxes,6] = lo xyz, hi xyz: for kind 0 the box itself; for kind 1
 * center_j -+ (sum_k |R[j][k]|*|half_k| + 8e-6*max|half|)*(1 + 1e-9), two floats further out (the margin is derived in
 * pch_crop.hip: every row the predicate accepts lies inside, for an R orthonormal to 1e-6), and -inf / +inf for an R
 * further from orthonormal or a box with NaN / inf fields.  A box whose bounds are not all finite is never skipped,
 * so the cull never changes the result.  A file-order LAS cloud is spatially coherent and most tiles meet no or few
 * boxes; a shuffled cloud tests every box for every tile. */
typedef struct PchCropBox {
    int32_t kind;        /* 0 = axis-aligned, 1 = oriented */
    int32_t reserved;
    double  lo[3], hi[3];   /* kind 0: inclusive bounds on the raw coordinates; kind 1: unused */
    double  center[3];      /* kind 1 */
    double  axes[9];        /* kind 1: row-major 3x3 R, COLUMNS are the box axes (the tower dict's 'rotation') */
    double  half[3];        /* kind 1: half extents */
} PchCropBox;
size_t pch_crop_boxes_ws_bytes(int64_t n, int32_t nboxes, int64_t cap);
int pch_crop_boxes_f64(const double* xyz, int64_t n, const PchCropBox* boxes_host, int32_t nboxes, int64_t cap,
                       double* out_points, int64_t* out_index, int64_t* out_offsets, int64_t* out_count,
                       void* ws, size_t ws_bytes, void* stream);
int pch_crop_box_bounds_f64(const PchCropBox* boxes_host, int32_t nboxes, double* out_lo3_hi3);

/* Self-test of the bounded wait: launches eight look-back tiles of which the second never publishes and returns
 * PCH_ERR_TIMEOUT when the six tiles behind it gave up within budget_ms (1..2000) as designed AND the count word they
 * marked (sign bit, as the data-path kernels mark theirs) reads negative; PCH_ERR_HIP when not.  dev_scratch: >= 256 bytes of device memory.  Synchronises.  Not part of the data path (tests only). */
int pch_selftest_lookback_timeout(int budget_ms, void* dev_scratch, size_t scratch_bytes, void* stream);

/* Self-test of the shared exclusive scans of uint32: out[i] = in[0] + ... + in[i-1] modulo 2^32, out_total [1] uint32
 * (device, may be NULL) = the sum of all n.  form selects the routine the stages call: 0 the three-launch scan, 1 the
 * same over the bit counts of the words of in (a row bitmap to ranks), 2 and 3 the one-launch look-back forms of 0 and
 * 1 (their status words and out_total are zeroed here; out_total reads 0xFFFFFFFF if a bounded wait gave up), 4 the
 * single-workgroup scan of n tile sums alone (in is copied to out and scanned there).  0 <= n < 2^31; in and out
 * 16-byte aligned; out may be in for forms 0, 2 and 4, never for 1 and 3, and may not overlap it otherwise.  n = 0
 * launches nothing and out_total reads 0.  A refused call (PCH_ERR_ARG, PCH_ERR_WORKSPACE) writes nothing.  Enqueues
 * and returns.  Not part of the data path (tests only). */
size_t pch_selftest_scan_u32_ws_bytes(int64_t n, int32_t form);
int pch_selftest_scan_u32(const uint32_t* in, uint32_t* out, int64_t n, int32_t form, uint32_t* out_total,
                          void* ws, size_t ws_bytes, void* stream);

/* Self-test of the shared stable LSD radix sort: out_keys / out_vals [n] = the pairs (keys[i], vals[i]) ordered by
 * the low nbits bits of the key (0 <= nbits <= 64), pairs that agree in those bits in input order; the bits above
 * nbits travel with the key and are not looked at, nbits = 0 copies.  The pairs are sorted inside the workspace and
 * the ping-pong buffer the sort names as its result is the one copied out.  0 <= n < 2^31.  A refused call writes
 * nothing.  Enqueues and returns.  Not part of the data path (tests only). */
size_t pch_selftest_radix_sort_ws_bytes(int64_t n);
int pch_selftest_radix_sort_pairs(const uint64_t* keys, const uint32_t* vals, int64_t n, int32_t nbits,
                                  uint64_t* out_keys, uint32_t* out_vals, void* ws, size_t ws_bytes, void* stream);

/* Preview decimation: k distinct rows chosen by a seeded pseudo-random bijection of the row range.
 * Replaces: points[np.random.choice(len(points), k, replace=False)] (pyGUI_towers_test.py:174-177 with k =
 * 200 000, ui/vtk_widget.py:115-118 with k = 500 000).  numpy's draw is unseeded there, so parity is a
 * property: exactly k rows, no row twice, every row from the input, order arbitrary.
 * out_points [k,3] float64 (may be NULL), out_index [k] int64 (may be NULL). */
int pch_decimate_f64(const double* xyz, int64_t n, int64_t k, uint64_t seed,
                     double* out_points, int64_t* out_index, void* stream);

/* ------------------------------------------------------- stages B + C + D0 in one call
 * The body of extract_towers between "points are loaded" and the per-label loop
 * (utils/tower_extraction.py:62-125): pch_ground_filter_f32, pch_dbscan_f32 on the kept points
 * (cell grid sized from the filter's bounding box) and pch_segment_by_label, back to back on
 * `stream` with one shared workspace.  Same results as the three calls.
 * out_points  [n,3] float32, out_index [n] int32 (may be NULL): as pch_ground_filter_f32
 * out_labels  [nf_cap] int32: labels of the kept points (first info->count entries)
 * out_perm    [nf_cap] int32, out_offsets [k_cap+1] int64, out_stats [k_cap,8] float32 (may be
 *             NULL): as pch_segment_by_label; pass out_perm = NULL to skip the grouping
 * nf_cap      upper bound on the kept points the caller is prepared for (<= n); if the filter
 *             keeps more: PCH_ERR_WORKSPACE, info->count says how many (retry with nf_cap >= it)
 * k_cap       capacity of out_offsets / out_stats; more clusters: PCH_ERR_RANGE (labels and
 *             info are valid, group with pch_segment_by_label)
 * info_host   HOST struct, filled on return.  Synchronises (two times: kept count together with the
 *             cell count, cluster count); the device outputs are complete once `stream` is.
 *             info->reserved is the route word: 1 = the head of stage C was planned on the device and
 *             ran without the host reading the kept count first, 0 = the host planned it (fallback
 *             threshold, nothing kept, another sort route, a grid the cell key does not hold, ...).
 */
typedef struct PchTowerClusters {
    float   centroid[3];      /* np.mean(raw.astype(f32), axis=0)            (:62-63) */
    float   base;             /* np.percentile(points[:,2], pct)             (:82)    */
    float   threshold;        /* base + offset, or base + fallback_offset    (:87-89) */
    int32_t used_fallback;
    int64_t count_at_offset;  /* points kept by the first threshold */
    float   aabb[6];          /* min xyz, max xyz of the kept (centred) points */
    int64_t count;            /* points kept */
    int32_t nclusters;
    int32_t reserved;         /* route word, see above */
} PchTowerClusters;
size_t pch_tower_clusters_ws_bytes(int64_t n, int64_t nf_cap, int32_t k_cap);
int pch_tower_clusters_f32(const float* raw, int64_t n, double pct, float offset,
                           float fallback_offset, int64_t min_keep, double eps,
                           int32_t min_samples, int64_t chunk_size,
                           float* out_points, int32_t* out_index, int32_t* out_labels,
                           int32_t* out_perm, int64_t* out_offsets, float* out_stats,
                           int64_t nf_cap, int32_t k_cap, PchTowerClusters* info_host,
                           void* ws, size_t ws_bytes, void* stream);

/* --------------------------------------------------------- profiling helpers
 * Last-call timings recorded with hipEvents on the caller's stream when
 * pch_set_profiling(1): fills up to `cap` (name, total ms, launch count) triples for the
 * kernels launched by this thread's pch_* calls since the previous pch_get_profile /
 * pch_set_profiling call.  Returns the number of entries.  (synchronises) */
void pch_set_profiling(int enable);
/* restrict the recording to a comma separated list of kernel names (NULL or "" = all): keeps the
 * host cost of the event records out of a timed region that only needs its heavy kernels */
void pch_set_profiling_filter(const char* names);
int  pch_get_profile(int cap, char names[][48], float* ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* PCH_HIP_H */
