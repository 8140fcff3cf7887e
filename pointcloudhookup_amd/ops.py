"""Tensor-level operators: PyTorch-ROCm tensors in, C-ABI calls underneath.

torch is used for device memory, streams and (in tiles.py) torch.distributed only; all
arithmetic happens in libpch_hip.so.  Every function requires CUDA(HIP) tensors and raises
if the extension or a GPU is missing - there is no CPU fallback here by design.

One function per reference library call:
  voxel_downsample  <- open3d voxel_down_sample per chunk   ui/import_PC.py:8-13,45-58
  mean_seq_f32      <- np.mean(raw, axis=0)                  utils/tower_extraction.py:63
  percentile_f32    <- np.percentile(z, 25)                  utils/tower_extraction.py:83
  ground_filter     <- centring + percentile filter          utils/tower_extraction.py:63-64,82-89
  ground_filter_plane <- RANSAC ground plane (opt-in)      test/main_ground.py:8-32
  ground_filter_plane_tiles <- the same per xy tile (opt-in) test/main_ground.py:77-115
  dbscan            <- chunked sklearn DBSCAN + label offset utils/tower_extraction.py:96-117
  segment_by_label  <- per-label boolean masks               utils/tower_extraction.py:125,131-134
  merge_clusters    <- merge of neighbouring clusters (opt-in) test/tttt.py:93-175
  upright_boxes     <- upright box per cluster (opt-in)      test/008.py:302-331 (axis-aligned there)
  crop_boxes        <- per-tower box masks over the cloud    test/kuangxuan.py:60-79, ui/extract.py:345-420
Beyond the reference, on a retained fit (DbscanFit): assign, kdist, shape (+ shape_features), knn (+ knn_mean_distance) -
DESIGN.md sections 5a, 5b, 5c; on a grouping: cluster_moments, span_frames, cluster_profile, span_fit - section 5d; on a cloud and the fitted
curves: span_curves, span_segments, clearance - section 5e; on a cloud and a grid: terrain_grid, terrain_low,
terrain_ground, terrain_height, terrain_sample, span_ground_profile - section 5f; on a cloud and the curves swung by
wind: swing_heads, swing_segments, swing_clearance - section 5i; on a cloud and the curves, station by station:
span_section - section 5j; on a cloud, a terrain grid and a canopy grid: canopy_grid, canopy_top, canopy_trees,
canopy_rows - section 5k.
"""
from __future__ import annotations

import threading

import torch

from . import _lib

_tls = threading.local()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _need_cuda(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA/HIP tensor (no CPU fallback in the product path)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def _workspace(nbytes, device):
    """Grow-only per-thread, per-device scratch buffer."""
    cache = getattr(_tls, "ws", None)
    if cache is None:
        cache = _tls.ws = {}
    key = device.index if device.index is not None else torch.cuda.current_device()
    buf = cache.get(key)
    if buf is None or buf.numel() < nbytes:
        cache[key] = None
        buf = None
        buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
        cache[key] = buf
    return buf


def release_workspace():
    _tls.ws = {}


def _double3(v):
    import ctypes as C
    return (C.c_double * 3)(*[float(x) for x in v])


def set_profiling(enable, only=None):
    """Enables per-kernel hipEvent timing inside the library; ``only`` (iterable of kernel names)
    restricts the recording so that the host cost of the event records stays negligible."""
    L = _lib.lib()
    L.pch_set_profiling_filter(",".join(only).encode() if only else None)
    L.pch_set_profiling(1 if enable else 0)


def get_profile():
    return _lib.get_profile()


# ---------------------------------------------------------------------------- stage A
def voxel_downsample(xyz, voxel_size, chunk_size=0, order="library"):
    """Per-chunk voxel-grid downsample.  Returns (idx int32 [m,3], mean f64 [m,3],
    count int32 [m], chunk_offsets int64 [nchunks+1]); rows grouped by chunk; the order inside a
    chunk is deterministic but not sorted (include/pch_hip.h; Open3D's own is unspecified).  Synchronises (reads m).
    ``order="canonical"`` sorts every chunk's rows by (ix, iy, iz) behind the stage (voxel_canonical_order): that
    order depends on the input alone, the default one also on the build."""
    if order not in ("library", "canonical"):
        raise ValueError(f"order must be 'library' or 'canonical', got {order!r}")
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float64, "xyz").reshape(-1, 3)
    n = xyz.shape[0]
    dev = xyz.device
    cs = int(chunk_size) if chunk_size and chunk_size > 0 else max(n, 1)
    nchunks = max(1, -(-n // cs))
    with torch.cuda.device(dev):
        idx = torch.empty((n, 3), dtype=torch.int32, device=dev)
        mean = torch.empty((n, 3), dtype=torch.float64, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        offs = torch.zeros((nchunks + 1,), dtype=torch.int64, device=dev)
        m_dev = torch.zeros((1,), dtype=torch.int64, device=dev)
        nb = L.pch_voxel_downsample_ws_bytes(n, cs)
        ws = _workspace(nb, dev)
        _lib.check(L.pch_voxel_downsample_f64(_ptr(xyz), n, float(voxel_size), cs, _ptr(idx), _ptr(mean),
                                              _ptr(count), _ptr(offs), _ptr(m_dev), _ptr(ws), ws.numel(),
                                              _stream()))
        m = _lib.check_count(m_dev.item(), "voxel_downsample")
    if order == "canonical":
        return voxel_canonical_order(idx[:m], mean[:m], count[:m], offs) + (offs,)
    return idx[:m], mean[:m], count[:m], offs


def voxel_canonical_order(idx, mean, count, chunk_offsets, want_perm=False):
    """The rows voxel_downsample returned, every chunk's slice sorted ascending by (ix, iy, iz): new tensors
    (idx, mean, count) and, with ``want_perm``, the source row of every output row (int32 [m]).  chunk_offsets holds
    for the result unchanged.  Runs on the current stream in the shared workspace."""
    L = _lib.lib()
    idx = _need_cuda(idx, torch.int32, "idx").reshape(-1, 3)
    mean = _need_cuda(mean, torch.float64, "mean").reshape(-1, 3)
    count = _need_cuda(count, torch.int32, "count").reshape(-1)
    offs = _need_cuda(chunk_offsets, torch.int64, "chunk_offsets").reshape(-1)
    m = idx.shape[0]
    if mean.shape[0] != m or count.shape[0] != m or offs.shape[0] < 2:
        raise ValueError("idx, mean and count must have the same number of rows; chunk_offsets at least two entries")
    dev = idx.device
    nchunks = offs.shape[0] - 1
    with torch.cuda.device(dev):
        out_idx, out_mean, out_count = torch.empty_like(idx), torch.empty_like(mean), torch.empty_like(count)
        perm = torch.empty((m,), dtype=torch.int32, device=dev) if want_perm else None
        if m:
            ws = _workspace(L.pch_voxel_canonical_order_ws_bytes(m, nchunks), dev)
            _lib.check(L.pch_voxel_canonical_order(_ptr(idx), _ptr(mean), _ptr(count), _ptr(offs), nchunks, m,
                                                   _ptr(out_idx), _ptr(out_mean), _ptr(out_count), _ptr(perm),
                                                   _ptr(ws), ws.numel(), _stream()))
    return (out_idx, out_mean, out_count, perm) if want_perm else (out_idx, out_mean, out_count)


def las_records_xyz(records_u8, n, record_len):
    """Raw LAS point records (uint8 device tensor) -> int32 [n,3] X,Y,Z."""
    L = _lib.lib()
    rec = _need_cuda(records_u8, torch.uint8, "records")
    if rec.numel() < int(n) * int(record_len):
        raise ValueError("record buffer shorter than n * record_len")
    out = torch.empty((int(n), 3), dtype=torch.int32, device=rec.device)
    with torch.cuda.device(rec.device):
        _lib.check(L.pch_las_records_xyz_i32(_ptr(rec), int(n), int(record_len), _ptr(out), _stream()))
    return out


def las_scale(XYZ_i32, scales, offsets):
    """laspy scaled view: int32 [n,3] -> float64 [n,3] (X*scale+offset)."""
    import ctypes as C
    L = _lib.lib()
    X = _need_cuda(XYZ_i32, torch.int32, "XYZ").reshape(-1, 3)
    out = torch.empty(X.shape, dtype=torch.float64, device=X.device)
    sc, of = _double3(scales), _double3(offsets)
    with torch.cuda.device(X.device):
        _lib.check(L.pch_las_scale_i32_f64(_ptr(X), X.shape[0], C.cast(sc, C.c_void_p),
                                           C.cast(of, C.c_void_p), _ptr(out), _stream()))
    return out


def las_unscale(xyz_f64, scales, offsets):
    """laspy coordinate setter: float64 [n,3] -> int32 [n,3] (rint((v-offset)/scale))."""
    import ctypes as C
    L = _lib.lib()
    x = _need_cuda(xyz_f64, torch.float64, "xyz").reshape(-1, 3)
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    sc, of = _double3(scales), _double3(offsets)
    with torch.cuda.device(x.device):
        _lib.check(L.pch_las_unscale_f64_i32(_ptr(x), x.shape[0], C.cast(sc, C.c_void_p),
                                             C.cast(of, C.c_void_p), _ptr(out), _stream()))
    return out


# ---------------------------------------------------------------------------- stage B
def cast_f32(x_f64):
    L = _lib.lib()
    x = _need_cuda(x_f64, torch.float64, "x")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.pch_cast_f64_f32(_ptr(x), x.numel(), _ptr(out), _stream()))
    return out


def mean_seq_f32(xyz, serial=False):
    """np.mean(xyz, axis=0) for C-order float32 [n,3], bit exact.  Returns float32 [3].
    ``serial`` selects the one-workgroup element-by-element variant (cross-check only)."""
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    out = torch.empty((3,), dtype=torch.float32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        if serial:
            _lib.check(L.pch_mean_seq_serial_f32(_ptr(xyz), xyz.shape[0], _ptr(out), _stream()))
            return out
        nb = L.pch_mean_seq_f32_ws_bytes(xyz.shape[0])
        ws = _workspace(nb, xyz.device)
        _lib.check(L.pch_mean_seq_f32(_ptr(xyz), xyz.shape[0], _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def mean_seq_partial_f32(xyz, sum_in=None, total_n=0):
    """One file-order shard of np.mean(., axis=0): continues the float32 running sums ``sum_in`` (float32 [3] device
    tensor, None = +0.0) over the rows of ``xyz``.  total_n == 0: returns the running sums after the rows (hand them
    to the next shard); total_n > 0: returns sums / float32(total_n), the centroid (last shard).  float32 [3]."""
    sh = MeanShard(xyz)
    return sh.walk(sum_in, total_n)


class MeanShard:
    """A file-order shard of the sequential float32 column sums, in two phases (pch_mean_seq_partial_f32): the
    constructor builds the shard's summary tables (the passes over the rows; independent of what comes before the
    shard, so every rank does this at once), ``walk`` then continues GIVEN running sums over them (the short serial
    part that is chained from rank to rank).  The tables live in a workspace that belongs to this object."""

    def __init__(self, xyz, want_zcol=False):
        L = _lib.lib()
        self.xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
        self.n, self.device = self.xyz.shape[0], self.xyz.device
        with torch.cuda.device(self.device):
            self.workspace = torch.empty(int(L.pch_mean_seq_f32_ws_bytes(self.n)) + 256, dtype=torch.uint8,
                                         device=self.device)
            # contiguous copy of the z column, written by the pass that reads the rows anyway
            self.zcol = torch.empty((self.n,), dtype=torch.float32, device=self.device) if want_zcol else None
            _lib.check(L.pch_mean_seq_partial_f32(_ptr(self.xyz), self.n, 0, 0, 0, _ptr(self.zcol), 1,
                                                  _ptr(self.workspace), self.workspace.numel(), _stream()))

    def walk(self, sum_in=None, total_n=0):
        L = _lib.lib()
        if sum_in is not None:
            sum_in = _need_cuda(sum_in, torch.float32, "sum_in").reshape(3)
        out = torch.empty((3,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.pch_mean_seq_partial_f32(_ptr(self.xyz), self.n, _ptr(sum_in), int(total_n), _ptr(out), 0, 2,
                                                  _ptr(self.workspace), self.workspace.numel(), _stream()))
        return out


def percentile_f32(values, q_percent, sub=None):
    """np.percentile(values - sub, q) for a float32 vector (any stride).  Returns float32 [1]."""
    L = _lib.lib()
    n, stride = _strided_1d(values)
    out = torch.empty((1,), dtype=torch.float32, device=values.device)
    with torch.cuda.device(values.device):
        nb = L.pch_percentile_f32_ws_bytes(n)
        ws = _workspace(nb, values.device)
        _lib.check(L.pch_percentile_f32(values.data_ptr(), n, stride, _ptr(sub), float(q_percent),
                                        _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def _strided_1d(values):
    if not values.is_cuda or values.dtype != torch.float32 or values.dim() != 1:
        raise TypeError("values must be a 1-D float32 CUDA tensor")
    n = values.shape[0]
    return n, (values.stride(0) if n > 1 else 1)


def select_hist(values, pass_no, prefix=0):
    """One histogram pass of the radix select over this tensor's values (see pch_select_hist_f32).
    Returns (hist int64 [4096] on the host, NaN count)."""
    L = _lib.lib()
    n, stride = _strided_1d(values)
    dev = values.device
    with torch.cuda.device(dev):
        hist = torch.empty((4096,), dtype=torch.int32, device=dev)
        nan = torch.zeros((1,), dtype=torch.int64, device=dev)
        ws = _workspace(L.pch_percentile_f32_ws_bytes(n), dev)
        _lib.check(L.pch_select_hist_f32(values.data_ptr() if n else 0, n, stride, int(pass_no), int(prefix) & 0xFFFFFFFF,
                                         _ptr(hist), _ptr(nan), _ptr(ws), ws.numel(), _stream()))
    return hist.cpu().numpy().view("<u4").astype("int64"), int(nan.item())


def select_min_above(values, key):
    """Smallest order-preserving key of this tensor's values that is > key (0xFFFFFFFF if none)."""
    L = _lib.lib()
    n, stride = _strided_1d(values)
    dev = values.device
    with torch.cuda.device(dev):
        out = torch.empty((1,), dtype=torch.int32, device=dev)
        ws = _workspace(L.pch_percentile_f32_ws_bytes(n), dev)
        _lib.check(L.pch_select_min_above_f32(values.data_ptr() if n else 0, n, stride, int(key) & 0xFFFFFFFF, _ptr(out),
                                              _ptr(ws), ws.numel(), _stream()))
    return int(out.cpu().numpy().view("<u4")[0])


def filter_gt(raw, centroid, threshold, want_index=True):
    """points = raw - centroid; keep z > threshold, order preserving, with GIVEN float32 centroid and threshold
    (utils/tower_extraction.py:64,84).  Returns dict(points, index | None, count, aabb).  Synchronises."""
    import ctypes as C
    import numpy as np
    L = _lib.lib()
    raw = _need_cuda(raw, torch.float32, "raw").reshape(-1, 3)
    n = raw.shape[0]
    dev = raw.device
    cen = (C.c_float * 3)(*[float(np.float32(v)) for v in centroid])
    with torch.cuda.device(dev):
        out_points, out_index, cnt, aabb = _filter_outputs(raw, want_index)
        ws = _workspace(L.pch_filter_gt_ws_bytes(n), dev)
        _lib.check(L.pch_filter_gt_f32(_ptr(raw), n, C.cast(cen, C.c_void_p), float(np.float32(threshold)), _ptr(out_points),
                                       _ptr(out_index), _ptr(cnt), _ptr(aabb), _ptr(ws), ws.numel(), _stream()))
        return _filter_result("filter_gt", out_points, out_index, cnt, aabb)


def _filter_outputs(raw, want_index):
    """the device buffers of filter_gt, filter_plane and filter_plane_tiles: out_points, out_index | None, count, aabb"""
    n, dev = raw.shape[0], raw.device
    return (torch.empty((n, 3), dtype=torch.float32, device=dev),
            torch.empty((n,), dtype=torch.int32, device=dev) if want_index else None,
            torch.zeros((1,), dtype=torch.int64, device=dev), torch.zeros((6,), dtype=torch.float32, device=dev))


def _filter_result(what, out_points, out_index, cnt, aabb):
    """the dict those three return; reads the count (synchronises)"""
    m = _lib.check_count(cnt.item(), what)
    return dict(points=out_points[:m], index=None if out_index is None else out_index[:m], count=m,
                aabb=aabb.cpu().numpy())


def _ground_result(points, index, nf, centroid, base, threshold, used_fallback, count_at_offset, aabb):
    """The stage-B result of ground_filter and tower_clusters: device rows, host scalars as numpy float32."""
    import numpy as np
    return dict(points=points[:nf], index=None if index is None else index[:nf],
                centroid=np.array(centroid, dtype=np.float32), base=np.float32(base), threshold=np.float32(threshold),
                used_fallback=bool(used_fallback), count_at_offset=int(count_at_offset),
                aabb=np.array(aabb, dtype=np.float32), count=nf)


def ground_filter(raw, pct=25.0, offset=3.0, fallback_offset=1.0, min_keep=1000, want_index=True):
    """Fused stage B on float32 [n,3].  Returns dict(points [n_f,3] f32 (centred, file
    order), index int32 [n_f] | None, centroid f32[3] (host np), base, threshold,
    used_fallback, aabb (host, 6 floats), count).  Synchronises (reads n_f)."""
    L = _lib.lib()
    raw = _need_cuda(raw, torch.float32, "raw").reshape(-1, 3)
    n = raw.shape[0]
    dev = raw.device
    with torch.cuda.device(dev):
        out_points = torch.empty((n, 3), dtype=torch.float32, device=dev)
        out_index = torch.empty((n,), dtype=torch.int32, device=dev) if want_index else None
        scal = torch.zeros((18,), dtype=torch.float32, device=dev)     # [0:8] scalars, [8:14] aabb, [16:18] count (int64)
        nb = L.pch_ground_filter_ws_bytes(n)
        ws = _workspace(nb, dev)
        _lib.check(L.pch_ground_filter_f32(_ptr(raw), n, float(pct), float(offset), float(fallback_offset),
                                           int(min_keep), _ptr(out_points), _ptr(out_index), _ptr(scal),
                                           scal.data_ptr() + 64, scal.data_ptr() + 32, _ptr(ws), ws.numel(),
                                           _stream()))
        host = scal.cpu().numpy()           # one D2H copy, synchronises the stream
        nf = _lib.check_count(host[16:18].view("<i8")[0], "ground_filter")
    return _ground_result(out_points, out_index, nf, host[0:3], host[3], host[4], host[5] != 0.0,
                          host[6:7].view("<u4")[0], host[8:14])


# ------------------------------------------------------------- stage B, opt-in: the LAS-integer frame
FRAME_TILE = 2048              # rows per workgroup of the frame's filter sweep (fr_filter_k): the sizes tests straddle


def frame_scales(scales):
    """the three LAS scales of the "las" frame as float64; ValueError unless every one is finite and > 0"""
    import numpy as np
    sc = np.asarray(scales, dtype=np.float64).reshape(-1)
    if sc.shape != (3,) or not np.all(np.isfinite(sc)) or not np.all(sc > 0.0):
        raise ValueError(f"the LAS scales must be three finite numbers > 0, got {scales!r}")
    return sc


def ground_filter_las(XYZ, scales, offsets, pct=25.0, offset=3.0, fallback_offset=1.0, min_keep=1000, want_index=True):
    """Stage B in the LAS-integer frame (opt-in; include/pch_hip.h, pch_ground_filter_las_i32) on the int32 [n,3] LAS
    records themselves: the centroid is the exact integer one, C = floor(sum / n), every row is centred on the integers
    and rounded to float32 once, p = float32(float64(XYZ - C) * scale), and the reference's percentile rule runs on p.
    No float64 or float32 copy of the cloud is made.  Returns the dict of ground_filter, where ``centroid`` is the
    float64 world centroid C * scale + offset (points.astype(float64) + centroid are world coordinates), plus
    ``centroid_int`` (int64 [3]) and ``frame`` = "las".  Synchronises (reads the record)."""
    import ctypes as C
    import numpy as np
    sc = frame_scales(scales)
    of = np.asarray(offsets, dtype=np.float64).reshape(3)
    L = _lib.lib()
    XYZ = _need_cuda(XYZ, torch.int32, "XYZ").reshape(-1, 3)
    n = XYZ.shape[0]
    dev = XYZ.device
    sc_c = _double3(sc)
    with torch.cuda.device(dev):
        out_points = torch.empty((n, 3), dtype=torch.float32, device=dev)
        out_index = torch.empty((n,), dtype=torch.int32, device=dev) if want_index else None
        rec = torch.zeros((C.sizeof(_lib.LasFrameC),), dtype=torch.uint8, device=dev)
        ws = _workspace(L.pch_ground_filter_las_ws_bytes(n), dev)
        _lib.check(L.pch_ground_filter_las_i32(_ptr(XYZ), n, C.cast(sc_c, C.c_void_p), float(pct), float(offset),
                                               float(fallback_offset), int(min_keep), _ptr(out_points),
                                               _ptr(out_index), _ptr(rec), _ptr(ws), ws.numel(), _stream()))
        f = _lib.LasFrameC.from_buffer_copy(rec.cpu().numpy().tobytes())     # one D2H copy, synchronises the stream
    nf = _lib.check_count(f.count, "ground_filter_las")
    cint = np.array(list(f.centroid), dtype=np.int64)
    out = _ground_result(out_points, out_index, nf, (0.0, 0.0, 0.0), f.base, f.threshold, f.used_fallback != 0,
                         f.count_at_offset, list(f.aabb))
    out.update(centroid=cint.astype(np.float64) * sc + of, centroid_int=cint, frame="las")
    return out


# ------------------------------------------------------------- stage B, opt-in: one RANSAC ground plane
PLANE_MAX_HYPOTHESES = 4096
PLANE_COUNT_TILE = 1024        # rows per workgroup pass of the inlier count (pl_count_k): the sizes tests straddle
_PLANE_KEEP = {"above": 0, "off_plane": 1}


def _check_hypotheses(H):
    if not 1 <= H <= PLANE_MAX_HYPOTHESES:
        raise ValueError(f"between 1 and {PLANE_MAX_HYPOTHESES} hypotheses, got {H}")


def _cos2(max_slope_deg):
    """the slope gate of a fit as the library takes it"""
    import math
    return math.cos(math.radians(float(max_slope_deg))) ** 2


def plane_hypothesis_rows(n, H=256, seed=0):
    """The row triples of H plane hypotheses over a cloud of n rows: host int64 [H,3], drawn with replacement (a
    triple with a repeat is simply an invalid hypothesis).  The first H of a longer draw with the same seed."""
    import numpy as np
    n, H = int(n), int(H)
    if n < 1:
        raise ValueError("plane_hypothesis_rows needs a cloud with at least one row")
    _check_hypotheses(H)
    return np.random.Generator(np.random.PCG64(int(seed))).integers(0, n, size=(H, 3), dtype=np.int64)


def _centroid_dev(centroid, dev):
    """float32 [3] on the device: a device tensor as it is, host values rounded to float32 and uploaded"""
    import numpy as np
    if isinstance(centroid, torch.Tensor):
        return centroid.to(device=dev, dtype=torch.float32).reshape(3).contiguous()
    return torch.from_numpy(np.array(centroid, dtype=np.float32).reshape(3)).to(dev)


def _plane_rows_dev(rows, n, dev):
    """int64 [H,3] hypothesis table on the device, checked on the host when it comes from there"""
    import numpy as np
    if isinstance(rows, torch.Tensor) and rows.is_cuda:
        rows = _need_cuda(rows, torch.int64, "rows").reshape(-1, 3)
    else:
        host = np.ascontiguousarray(np.asarray(rows, dtype=np.int64)).reshape(-1, 3)
        if n and host.size and (host.min() < 0 or host.max() >= n):
            raise ValueError("rows: every entry must lie in [0, n)")
        rows = torch.from_numpy(host).to(dev)
    _check_hypotheses(rows.shape[0])
    return rows


def _plane_fit_launch(raw, cen_dev, rows_dev, residual_threshold, max_slope_deg, best_ptr):
    """pch_plane_fit_f32, enqueued: (planes float64 [H,4], counts int64 [H]) device tensors, the best record at
    best_ptr (device)"""
    L = _lib.lib()
    n, H, dev = raw.shape[0], rows_dev.shape[0], raw.device
    planes = torch.empty((H, 4), dtype=torch.float64, device=dev)
    counts = torch.empty((H,), dtype=torch.int64, device=dev)
    ws = _workspace(L.pch_plane_fit_ws_bytes(n, H), dev)
    _lib.check(L.pch_plane_fit_f32(_ptr(raw), n, _ptr(cen_dev), _ptr(rows_dev), H, float(residual_threshold),
                                   _cos2(max_slope_deg), _ptr(planes), _ptr(counts), best_ptr, _ptr(ws), ws.numel(),
                                   _stream()))
    return planes, counts


def _plane_best(words):
    """PchPlaneBest from its 40 bytes (numpy uint8)"""
    return _lib.PlaneBestC.from_buffer_copy(words.tobytes())


def _plane_record_dev(plane, dev):
    """a PchPlaneBest on the device from (a, b, c), a plane_fit result or None (no plane: best = -1)"""
    import numpy as np
    if isinstance(plane, dict):
        plane = plane["plane"]
    rec = _lib.PlaneBestC(0.0, 0.0, 0.0, 0, -1, 0)
    if plane is not None:
        a, b, c = (float(v) for v in plane)
        rec = _lib.PlaneBestC(a, b, c, 0, 0, 1)
    return torch.from_numpy(np.frombuffer(bytes(rec), dtype=np.uint8).copy()).to(dev)


def plane_fit(raw, centroid, rows, residual_threshold=0.1, max_slope_deg=45.0):
    """RANSAC ground plane z = a x + b y + c of fl32(raw - centroid) over GIVEN hypotheses (test/main_ground.py:21-28;
    the rule is stated in include/pch_hip.h).  raw float32 [n,3] (device), centroid float32 [3] (host values or a
    device tensor), rows int64 [H,3] (plane_hypothesis_rows).  Returns dict(planes float64 [H,4] = a, b, c, valid and
    counts int64 [H] as host arrays, best (-1: no valid hypothesis), plane float64 [3] | None, inliers, nvalid).
    Synchronises once."""
    import numpy as np
    raw = _need_cuda(raw, torch.float32, "raw").reshape(-1, 3)
    dev = raw.device
    with torch.cuda.device(dev):
        rows_dev = _plane_rows_dev(rows, raw.shape[0], dev)
        H = rows_dev.shape[0]
        best = torch.empty((40,), dtype=torch.uint8, device=dev)
        planes, counts = _plane_fit_launch(raw, _centroid_dev(centroid, dev), rows_dev, residual_threshold,
                                           max_slope_deg, _ptr(best))
        host = torch.cat([planes.view(torch.uint8).reshape(-1), counts.view(torch.uint8), best]).cpu().numpy()
    rec = _plane_best(host[40 * H:])
    return dict(planes=host[:32 * H].view(np.float64).reshape(H, 4).copy(),
                counts=host[32 * H:40 * H].view(np.int64).copy(), best=int(rec.best),
                plane=None if rec.best < 0 else np.array([rec.a, rec.b, rec.c], dtype=np.float64),
                inliers=int(rec.count), nvalid=int(rec.nvalid))


def _filter_plane_launch(raw, cen_dev, best_ptr, keep, value, out_points, out_index, cnt_ptr, aabb_ptr):
    L = _lib.lib()
    n = raw.shape[0]
    ws = _workspace(L.pch_filter_plane_ws_bytes(n), raw.device)
    _lib.check(L.pch_filter_plane_f32(_ptr(raw), n, _ptr(cen_dev), best_ptr, _PLANE_KEEP[keep], float(value),
                                      _ptr(out_points), _ptr(out_index), cnt_ptr, aabb_ptr, _ptr(ws), ws.numel(),
                                      _stream()))


def _plane_keep_value(keep, offset, residual_threshold):
    if keep not in _PLANE_KEEP:
        raise ValueError(f"keep must be 'above' or 'off_plane', got {keep!r}")
    return offset if keep == "above" else residual_threshold


def filter_plane(raw, centroid, plane_or_fit, keep="above", offset=3.0, residual_threshold=0.1, want_index=True):
    """points = fl32(raw - centroid), kept by their residual r = z - ((a x + b y) + c) to a GIVEN plane, order
    preserving (test/main_ground.py:28-30): keep="above" keeps r > offset, keep="off_plane" keeps
    !(|r| <= residual_threshold), remove_ground_ransac's own non-ground set.  plane_or_fit: (a, b, c), or what
    plane_fit returned (a fit without a valid hypothesis keeps nothing).  Returns the dict of filter_gt.
    Synchronises."""
    value = _plane_keep_value(keep, offset, residual_threshold)
    raw = _need_cuda(raw, torch.float32, "raw").reshape(-1, 3)
    dev = raw.device
    with torch.cuda.device(dev):
        best = _plane_record_dev(plane_or_fit, dev)
        out_points, out_index, cnt, aabb = _filter_outputs(raw, want_index)
        _filter_plane_launch(raw, _centroid_dev(centroid, dev), _ptr(best), keep, value, out_points, out_index,
                             _ptr(cnt), _ptr(aabb))
        return _filter_result("filter_plane", out_points, out_index, cnt, aabb)


def ground_filter_plane(raw, hypotheses=256, seed=0, residual_threshold=0.1, max_slope_deg=45.0, offset=3.0,
                        fallback_offset=1.0, min_keep=1000, keep="above", want_index=True, rows=None):
    """Stage B with the plane rule, for sloped terrain: centroid (mean_seq_f32), plane_fit over ``rows`` (default:
    plane_hypothesis_rows(n, hypotheses, seed)), filter_plane, and in "above" mode the reference's fallback - fewer
    than min_keep rows above ``offset``: the rows above ``fallback_offset`` instead.  Returns the dict of
    ground_filter - base = float32(c), the plane's height under the centroid; threshold = the offset used - plus
    plane (float64 [3]), inliers, nvalid, best.  ValueError when no hypothesis is valid.  Fit and filter chain on the
    device; one host read, a second after a fallback."""
    import numpy as np
    value = _plane_keep_value(keep, offset, residual_threshold)
    raw = _need_cuda(raw, torch.float32, "raw").reshape(-1, 3)
    n, dev = raw.shape[0], raw.device
    if n == 0:
        raise ValueError("no valid ground plane: the cloud is empty")
    with torch.cuda.device(dev):
        rows_dev = _plane_rows_dev(plane_hypothesis_rows(n, hypotheses, seed) if rows is None else rows, n, dev)

        def check(rec, _):
            if rec.best < 0:
                raise ValueError(f"no valid ground plane among {rows_dev.shape[0]} hypotheses (degenerate triples, or "
                                 f"none within {max_slope_deg} degrees of level)")

        def fits(cen, record_ptr):
            _plane_fit_launch(raw, cen, rows_dev, residual_threshold, max_slope_deg, record_ptr)
            return (lambda *a: _filter_plane_launch(raw, cen, record_ptr, keep, *a)), [], check

        out, rec, _ = _plane_stage_b(raw, "ground_filter_plane", keep, value, fallback_offset, min_keep, want_index,
                                     fits)
    out.update(plane=np.array([rec.a, rec.b, rec.c], dtype=np.float64), inliers=int(rec.count),
               nvalid=int(rec.nvalid), best=int(rec.best))
    return out


def _plane_stage_b(raw, what, keep, value, fallback_offset, min_keep, want_index, fits):
    """What ground_filter_plane and ground_filter_plane_tiles share: one block for the host - [0:40] the record of the
    global fit, [48:56] count, [64:88] aabb, [96:108] centroid - the centroid launch, then ``fits(cen, record_ptr)``,
    which enqueues the rule's fits and returns (launch, extra, check): launch(v, out_points, out_index, cnt_ptr,
    aabb_ptr) enqueues the filter at the value v, ``extra`` are uint8 device tensors that ride along with the block's
    host read, check(rec, extra_host) raises when there is no plane at all.  Sweep, read once, check, and in "above"
    mode the fallback offset with a second read.  Returns (the dict of ground_filter, rec, what check returned)."""
    import numpy as np
    L = _lib.lib()
    n, dev = raw.shape[0], raw.device
    scal = torch.zeros((112,), dtype=torch.uint8, device=dev)
    base = scal.data_ptr()
    cen = scal[96:108].view(torch.float32)
    ws = _workspace(L.pch_mean_seq_f32_ws_bytes(n), dev)
    _lib.check(L.pch_mean_seq_f32(_ptr(raw), n, _ptr(cen), _ptr(ws), ws.numel(), _stream()))
    launch, extra, check = fits(cen, base)
    out_points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    out_index = torch.empty((n,), dtype=torch.int32, device=dev) if want_index else None

    def sweep(v):
        launch(v, out_points, out_index, base + 48, base + 64)
        host = (torch.cat([scal] + extra) if extra else scal).cpu().numpy()
        return host, _lib.check_count(host[48:56].view("<i8")[0], what)

    host, nf = sweep(value)
    rec = _plane_best(host[:40])
    info = check(rec, host[112:])
    first, used_fallback = nf, False
    if keep == "above" and nf < int(min_keep):
        used_fallback, value = True, fallback_offset
        host, nf = sweep(value)
    out = _ground_result(out_points, out_index, nf, host[96:108].view(np.float32),
                         np.float32(rec.c) if rec.best >= 0 else np.float32(np.nan), value, used_fallback, first,
                         host[64:88].view(np.float32))
    return out, rec, info


# ------------------------------------------------------------- stage B, opt-in: one RANSAC plane per xy tile
PLANE_MAX_TILES = 65536
PLANE_MAX_TILE_TABLE = 1 << 22          # tiles x hypotheses
_BEST_FIELDS = [("a", "<f8"), ("b", "<f8"), ("c", "<f8"), ("count", "<i8"), ("best", "<i4"), ("nvalid", "<i4")]


def plane_tile_grid(raw, centroid, tile_size):
    """The xy grid of the per-tile plane rule over the finite x and y of fl32(raw - centroid): dict(x0, y0, tile, nx,
    ny) with x0 = (double)fl32(min_x - cx), nx = floor((max - x0) / tile) + 1, likewise y (PchPlaneGrid,
    include/pch_hip.h).  The bounds come from a torch reduction; one small host read.  ValueError beyond 65 536
    tiles, naming the smallest tile_size that fits."""
    import math
    import numpy as np
    raw = _need_cuda(raw, torch.float32, "raw").reshape(-1, 3)
    tile = float(tile_size)
    if not (tile > 0.0 and math.isfinite(tile)):
        raise ValueError(f"tile_size must be positive and finite, got {tile_size!r}")
    cen = _centroid_dev(centroid, raw.device)
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=raw.device)
    fin = torch.isfinite(raw[:, :2])
    lo = torch.where(fin, raw[:, :2], inf).amin(dim=0) if raw.shape[0] else inf.expand(2)
    hi = torch.where(fin, raw[:, :2], -inf).amax(dim=0) if raw.shape[0] else (-inf).expand(2)
    host = torch.cat([lo, hi, cen]).cpu().numpy()
    return _plane_grid_of(host[0:2], host[2:4], host[4:6], tile)


def _plane_grid_of(lo, hi, cen, tile):
    """the grid from the float32 bounds of the finite raw x, y (inf / -inf without any) and the float32 centroid"""
    import math
    import numpy as np
    out, ext = dict(tile=float(tile)), [0.0, 0.0]
    for k, name in enumerate(("x", "y")):
        if not lo[k] <= hi[k]:                          # no finite coordinate: one tile at the origin
            out[name + "0"], out["n" + name] = 0.0, 1
            continue
        with np.errstate(over="ignore"):
            a, b = float(np.float32(lo[k]) - np.float32(cen[k])), float(np.float32(hi[k]) - np.float32(cen[k]))
        if not (math.isfinite(a) and math.isfinite(b)):
            raise ValueError("the centred bounds of the cloud are not finite")
        out[name + "0"], out["n" + name], ext[k] = a, int(math.floor((b - a) / tile)) + 1, b - a
    if out["nx"] * out["ny"] > PLANE_MAX_TILES:
        fits = lambda s: (math.floor(ext[0] / s) + 1) * (math.floor(ext[1] / s) + 1) <= PLANE_MAX_TILES
        lo_s, hi_s = tile, max(ext) + 1.0                              # hi_s: one tile, fits
        for _ in range(100):
            mid = 0.5 * (lo_s + hi_s)
            lo_s, hi_s = (lo_s, mid) if fits(mid) else (mid, hi_s)
        raise ValueError(f"tile_size {tile:g} gives {out['nx']} x {out['ny']} tiles, more than {PLANE_MAX_TILES}; "
                         f"the smallest tile_size that fits is {hi_s:.6g}")
    return out


def plane_tile_draws(H=64, seed=0):
    """The draw table of H hypotheses, shared by all tiles: host int64 [H,3] in [0, 2^62); the triple of (tile t,
    hypothesis h) is list_t[draws[h][k] mod n_t].  The first H of a longer table with the same seed."""
    import numpy as np
    H = int(H)
    _check_hypotheses(H)
    return np.random.Generator(np.random.PCG64(int(seed))).integers(0, 2 ** 62, size=(H, 3), dtype=np.int64)


def _plane_grid_c(grid):
    g = _lib.PlaneGridC(float(grid["x0"]), float(grid["y0"]), float(grid["tile"]), int(grid["nx"]), int(grid["ny"]))
    ntiles = g.nx * g.ny
    if g.nx < 1 or g.ny < 1 or ntiles > PLANE_MAX_TILES:
        raise ValueError(f"the grid must have between 1 and {PLANE_MAX_TILES} tiles, got {g.nx} x {g.ny}")
    return g, ntiles


def _plane_draws_dev(draws, ntiles, dev):
    import numpy as np
    if isinstance(draws, torch.Tensor) and draws.is_cuda:
        draws = _need_cuda(draws, torch.int64, "draws").reshape(-1, 3)
    else:
        host = np.ascontiguousarray(np.asarray(draws, dtype=np.int64)).reshape(-1, 3)
        if host.size and host.min() < 0:
            raise ValueError("draws: every entry must be >= 0")
        draws = torch.from_numpy(host).to(dev)
    H = draws.shape[0]
    _check_hypotheses(H)
    if ntiles * H > PLANE_MAX_TILE_TABLE:
        raise ValueError(f"{ntiles} tiles x {H} hypotheses exceed {PLANE_MAX_TILE_TABLE} table entries")
    return draws


def _plane_tiles_fit_launch(raw, cen_dev, grid_c, ntiles, draws_dev, min_tile_rows, residual_threshold, max_slope_deg,
                            best, tile_rows, planes=None, counts=None):
    """pch_plane_tiles_fit_f32, enqueued; best: uint8 [ntiles * 40], tile_rows: int64 [ntiles] (device)"""
    import ctypes as C
    L = _lib.lib()
    n, H = raw.shape[0], draws_dev.shape[0]
    ws = _workspace(L.pch_plane_tiles_fit_ws_bytes(n, ntiles, H), raw.device)
    _lib.check(L.pch_plane_tiles_fit_f32(_ptr(raw), n, _ptr(cen_dev), C.cast(C.pointer(grid_c), C.c_void_p), _ptr(draws_dev),
                                         H, int(min_tile_rows), float(residual_threshold), _cos2(max_slope_deg),
                                         _ptr(best), _ptr(tile_rows), _ptr(planes), _ptr(counts), _ptr(ws), ws.numel(),
                                         _stream()))


def _plane_tiles_table(best_bytes, rows):
    """the per-tile host table from the record bytes (numpy uint8 [ntiles * 40]) and the row counts"""
    import numpy as np
    rec = best_bytes.view(np.dtype(_BEST_FIELDS))
    return dict(best=rec["best"].copy(), planes=np.stack([rec["a"], rec["b"], rec["c"]], axis=1),
                inliers=rec["count"].copy(), rows=rows.copy(), nvalid=rec["nvalid"].copy())


def plane_tiles_fit(raw, centroid, grid, draws, min_tile_rows=64, residual_threshold=0.1, max_slope_deg=45.0,
                    want_tables=False):
    """One RANSAC plane per tile of ``grid`` (plane_tile_grid, or any dict(x0, y0, tile, nx, ny)) over the draw table
    ``draws`` (plane_tile_draws); the rule is stated in include/pch_hip.h.  Returns host arrays over the tiles
    t = fy * nx + fx: best int32 (-1: no plane), planes float64 [ntiles,3] (zeros without one), inliers int64, rows
    int64 (the tile's population), nvalid int32, plus grid; with ``want_tables`` also planes_table float64
    [ntiles,H,4] and counts_table int64 [ntiles,H].  Synchronises once."""
    import numpy as np
    if int(min_tile_rows) < 1:
        raise ValueError("min_tile_rows must be at least 1")
    raw = _need_cuda(raw, torch.float32, "raw").reshape(-1, 3)
    dev = raw.device
    grid_c, ntiles = _plane_grid_c(grid)
    with torch.cuda.device(dev):
        draws_dev = _plane_draws_dev(draws, ntiles, dev)
        H = draws_dev.shape[0]
        best = torch.empty((ntiles * 40,), dtype=torch.uint8, device=dev)
        rows = torch.empty((ntiles,), dtype=torch.int64, device=dev)
        planes = torch.empty((ntiles, H, 4), dtype=torch.float64, device=dev) if want_tables else None
        counts = torch.empty((ntiles, H), dtype=torch.int64, device=dev) if want_tables else None
        _plane_tiles_fit_launch(raw, _centroid_dev(centroid, dev), grid_c, ntiles, draws_dev, min_tile_rows,
                                residual_threshold, max_slope_deg, best, rows, planes, counts)
        parts = [best, rows.view(torch.uint8)]
        if want_tables:
            parts += [planes.view(torch.uint8).reshape(-1), counts.view(torch.uint8).reshape(-1)]
        host = torch.cat(parts).cpu().numpy()
    out = _plane_tiles_table(host[:40 * ntiles], host[40 * ntiles:48 * ntiles].view(np.int64))
    out["grid"] = dict(x0=grid_c.x0, y0=grid_c.y0, tile=grid_c.tile, nx=grid_c.nx, ny=grid_c.ny)
    if want_tables:
        at = 48 * ntiles
        out["planes_table"] = host[at:at + 32 * ntiles * H].view(np.float64).reshape(ntiles, H, 4).copy()
        out["counts_table"] = host[at + 32 * ntiles * H:].view(np.int64).reshape(ntiles, H).copy()
    return out


def _filter_plane_tiles_launch(raw, cen_dev, grid_c, ntiles, best_ptr, fallback_ptr, keep, value, out_points,
                               out_index, cnt_ptr, aabb_ptr):
    import ctypes as C
    L = _lib.lib()
    n = raw.shape[0]
    ws = _workspace(L.pch_filter_plane_tiles_ws_bytes(n, ntiles), raw.device)
    _lib.check(L.pch_filter_plane_tiles_f32(_ptr(raw), n, _ptr(cen_dev), C.cast(C.pointer(grid_c), C.c_void_p), best_ptr,
                                            fallback_ptr, _PLANE_KEEP[keep], float(value), _ptr(out_points),
                                            _ptr(out_index), cnt_ptr, aabb_ptr, _ptr(ws), ws.numel(), _stream()))


def filter_plane_tiles(raw, centroid, grid, fit_or_table, fallback=None, keep="above", offset=3.0,
                       residual_threshold=0.1, want_index=True):
    """points = fl32(raw - centroid), every row kept by its residual to the plane of ITS tile, in file order:
    fit_or_table is what plane_tiles_fit returned (or any dict with best [ntiles] and planes [ntiles,3]); a row whose
    tile has no plane, or that lies outside the grid, uses ``fallback`` - (a, b, c), a plane_fit result, or None - and
    a row with no plane at all is dropped.  keep / offset / residual_threshold as in filter_plane.  Returns the dict
    of filter_gt.  Synchronises."""
    import numpy as np
    value = _plane_keep_value(keep, offset, residual_threshold)
    raw = _need_cuda(raw, torch.float32, "raw").reshape(-1, 3)
    dev = raw.device
    grid_c, ntiles = _plane_grid_c(grid)
    rec = np.zeros((ntiles,), dtype=np.dtype(_BEST_FIELDS))
    tb = np.asarray(fit_or_table["best"]).reshape(-1)
    tp = np.asarray(fit_or_table["planes"], dtype=np.float64).reshape(-1, 3)
    if tb.shape[0] != ntiles or tp.shape[0] != ntiles:
        raise ValueError(f"the table must have one entry per tile ({ntiles}), got {tb.shape[0]}")
    rec["a"], rec["b"], rec["c"], rec["best"] = tp[:, 0], tp[:, 1], tp[:, 2], tb
    with torch.cuda.device(dev):
        best = torch.from_numpy(rec.view(np.uint8)).to(dev)
        fb = None if fallback is None else _plane_record_dev(fallback, dev)
        out_points, out_index, cnt, aabb = _filter_outputs(raw, want_index)
        _filter_plane_tiles_launch(raw, _centroid_dev(centroid, dev), grid_c, ntiles, _ptr(best), _ptr(fb), keep, value,
                                   out_points, out_index, _ptr(cnt), _ptr(aabb))
        return _filter_result("filter_plane_tiles", out_points, out_index, cnt, aabb)


def ground_filter_plane_tiles(raw, tile_size=20.0, hypotheses=64, seed=0, min_tile_rows=64, fallback_hypotheses=64,
                              residual_threshold=0.1, max_slope_deg=45.0, offset=3.0, fallback_offset=1.0,
                              min_keep=1000, keep="above", want_index=True):
    """Stage B with one plane per xy tile, for rolling terrain (test/main_ground.py:77-115; tile_size 20 is the
    reference's own call, :142): centroid (mean_seq_f32), the grid (plane_tile_grid), a global plane_fit over
    plane_hypothesis_rows(n, fallback_hypotheses, seed) as the fallback, plane_tiles_fit over plane_tile_draws(
    hypotheses, seed), filter_plane_tiles, and in "above" mode the reference's fallback offset as in
    ground_filter_plane.  Returns the dict of ground_filter plus tiles (grid and the per-tile table of
    plane_tiles_fit) and fallback_plane (float64 [3] | None); base = float32(c) of the fallback plane, NaN without
    one.  ValueError when neither a tile nor the fallback has a plane.  The grid is a host structure, so the centroid
    and the bounds are read once (a few words); fits and filter then chain on the device with one host read, a
    second after a fallback offset."""
    import numpy as np
    value = _plane_keep_value(keep, offset, residual_threshold)
    raw = _need_cuda(raw, torch.float32, "raw").reshape(-1, 3)
    n, dev = raw.shape[0], raw.device
    if n == 0:
        raise ValueError("no valid ground plane: the cloud is empty")
    if int(min_tile_rows) < 1:
        raise ValueError("min_tile_rows must be at least 1")
    with torch.cuda.device(dev):
        def fits(cen, record_ptr):
            grid = plane_tile_grid(raw, cen, tile_size)
            grid_c, ntiles = _plane_grid_c(grid)
            draws_dev = _plane_draws_dev(plane_tile_draws(hypotheses, seed), ntiles, dev)
            rows_dev = _plane_rows_dev(plane_hypothesis_rows(n, fallback_hypotheses, seed), n, dev)
            best = torch.empty((ntiles * 40,), dtype=torch.uint8, device=dev)
            tile_rows = torch.empty((ntiles,), dtype=torch.int64, device=dev)
            _plane_fit_launch(raw, cen, rows_dev, residual_threshold, max_slope_deg, record_ptr)
            _plane_tiles_fit_launch(raw, cen, grid_c, ntiles, draws_dev, min_tile_rows, residual_threshold,
                                    max_slope_deg, best, tile_rows)

            def check(rec, extra_host):
                tiles = _plane_tiles_table(extra_host[:40 * ntiles], extra_host[40 * ntiles:].view(np.int64))
                tiles["grid"] = grid
                if rec.best < 0 and not (tiles["best"] >= 0).any():
                    raise ValueError(f"no valid ground plane in any of {ntiles} tiles nor among {rows_dev.shape[0]} global"
                                     f" hypotheses (degenerate triples, or none within {max_slope_deg} degrees of level)")
                return tiles

            return (lambda *a: _filter_plane_tiles_launch(raw, cen, grid_c, ntiles, _ptr(best), record_ptr, keep, *a),
                    [best, tile_rows.view(torch.uint8)], check)

        out, rec, tiles = _plane_stage_b(raw, "ground_filter_plane_tiles", keep, value, fallback_offset, min_keep,
                                         want_index, fits)
    out.update(tiles=tiles, fallback_plane=None if rec.best < 0 else np.array([rec.a, rec.b, rec.c], dtype=np.float64))
    return out


# ---------------------------------------------------------------------------- stage C
def _dbscan_call(xyz, ws, eps, min_samples, chunk_size, aabb, want_core):
    """pch_dbscan_f32 on float32 [n,3] of the current device, in the workspace tensor ws: (labels, core | None, k)"""
    import ctypes as C
    n, dev = xyz.shape[0], xyz.device
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    core = torch.empty((n,), dtype=torch.uint8, device=dev) if want_core else None
    ncl = torch.zeros((1,), dtype=torch.int32, device=dev)
    box = None if aabb is None else (C.c_float * 6)(*[float(v) for v in aabb])
    _lib.check(_lib.lib().pch_dbscan_f32(_ptr(xyz), n, float(eps), int(min_samples), int(chunk_size),
                                         None if box is None else C.cast(box, C.c_void_p), _ptr(labels),
                                         _ptr(core), _ptr(ncl), _ptr(ws), ws.numel(), _stream()))
    return labels, core, _lib.check_count(ncl.item(), "dbscan")


def dbscan(xyz, eps=8.0, min_samples=80, chunk_size=50000, aabb=None, want_core=False):
    """Chunked exact DBSCAN on float32 [n,3].  Returns (labels int32 [n], core uint8 [n] | None,
    nclusters int).  Synchronises."""
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    with torch.cuda.device(xyz.device):
        ws = _workspace(_lib.lib().pch_dbscan_ws_bytes(xyz.shape[0]), xyz.device)
        return _dbscan_call(xyz, ws, eps, min_samples, chunk_size, aabb, want_core)


class DbscanFit:
    """One exact DBSCAN whose grid stays alive: labels, core flags and cluster count of ``ops.dbscan`` plus a
    workspace that belongs to this fit alone, so that ``first_core_rows`` and ``relabel`` may follow after any
    number of other ops (the shared per-thread scratch buffer of ``_workspace`` is never used here).  The library
    remembers one fit per thread: a second fit on the same thread retires the first, and a retired fit's
    continuation calls raise (PCH_ERR_ARG) instead of reading another run's grid."""

    def __init__(self, xyz, eps=8.0, min_samples=80, chunk_size=0, aabb=None):
        xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
        self.n, self.device, self.eps = xyz.shape[0], xyz.device, float(eps)
        self.chunk_size = int(chunk_size) if 0 < int(chunk_size) < self.n else 0      # 0: one fit over all rows
        with torch.cuda.device(self.device):
            nb = int(_lib.lib().pch_dbscan_ws_bytes(self.n)) + 256
            ws = self.workspace = torch.empty(nb, dtype=torch.uint8, device=self.device)
            self.labels, self.core, self.nclusters = _dbscan_call(xyz, ws, eps, min_samples, chunk_size, aabb, True)

    def first_core_rows(self):
        """Smallest core row of every cluster (int32 [nclusters], ascending with the cluster id)."""
        L = _lib.lib()
        out = torch.empty((self.nclusters,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.pch_dbscan_first_core_rows_i32(self.n, _ptr(out), _ptr(self.workspace),
                                                        self.workspace.numel(), _stream()))
        return out

    def pair_stats(self):
        """Tallies of the radius-count kernel of THIS fit, if it ran with ops.set_pair_counting(True): dict(pair_tests,
        lane_slots, cells_tested, tiles_staged) (pch_dbscan_pair_stats).  Synchronises."""
        import ctypes as C
        L = _lib.lib()
        out = (C.c_uint64 * 4)()
        with torch.cuda.device(self.device):
            _lib.check(L.pch_dbscan_pair_stats(self.n, C.cast(out, C.c_void_p), _ptr(self.workspace),
                                               self.workspace.numel(), _stream()))
        return dict(pair_tests=int(out[0]), lane_slots=int(out[1]), cells_tested=int(out[2]), tiles_staged=int(out[3]))

    def strip_pairs(self, x_lo, x_hi, cap=4096):
        """(int32 [cap,2] device buffer of (local row, cluster id) pairs, int32 [1] device count): one pair per grid
        cell that holds a core point with x_lo <= x < x_hi (pch_dbscan_strip_pairs_i32).  Asynchronous: the count
        is read by whoever needs it (it may exceed cap - then call again with a larger cap).  Before relabel."""
        import numpy as np
        L = _lib.lib()
        pairs = torch.empty((int(cap), 2), dtype=torch.int32, device=self.device)
        count = torch.empty((1,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.pch_dbscan_strip_pairs_i32(self.n, float(np.float32(x_lo)), float(np.float32(x_hi)), int(cap),
                                                    _ptr(pairs), _ptr(count), _ptr(self.workspace),
                                                    self.workspace.numel(), _stream()))
        return pairs, count

    def relabel(self, cluster_map):
        """Core points take cluster_map[old id], border points are decided again as the smallest new id among
        their core neighbours.  ``labels`` is updated in place and returned."""
        L = _lib.lib()
        cmap = _need_cuda(cluster_map, torch.int32, "cluster_map")
        with torch.cuda.device(self.device):
            _lib.check(L.pch_dbscan_relabel_i32(_ptr(cmap), cmap.numel(), self.n, _ptr(self.labels),
                                                _ptr(self.workspace), self.workspace.numel(), _stream()))
        return self.labels

    def assign(self, query, sub=None, chunk=None):
        """Labels (int32 [nq], device) of float32 [nq,3] points that were not part of the fit: the smallest cluster
        id among the fit's core points within eps of ``fl32(query - sub)``, else -1 - the rule the fit applies to its
        own non-core rows (pch_dbscan_assign_f32).  ``sub``: three floats subtracted in float32, e.g. the centroid
        the fitted rows were centred with.  ``chunk``: int32 [nq] device tensor naming the chunk whose fit each query
        is held against; required when the fit has several chunks (``chunk_size``).  Reads the fit only: call it as
        often as needed, before or after ``relabel`` (then it reports the new ids).  Asynchronous."""
        import ctypes as C
        import numpy as np
        query = _need_cuda(query, torch.float32, "query").reshape(-1, 3)
        if chunk is not None:
            chunk = _need_cuda(chunk, torch.int32, "chunk").reshape(-1)
            if chunk.numel() != query.shape[0]:
                raise ValueError("chunk must name one chunk per query row")
        nq = query.shape[0]
        with torch.cuda.device(self.device):
            if self.nclusters == 0:                   # nothing to join, and an all-noise fit may have left no grid
                return torch.full((nq,), -1, dtype=torch.int32, device=self.device)
            out = torch.empty((nq,), dtype=torch.int32, device=self.device)
            if nq == 0:
                return out
            L = _lib.lib()
            s3 = None if sub is None else (C.c_float * 3)(*[float(np.float32(v)) for v in sub])
            qws = torch.empty(int(L.pch_dbscan_assign_ws_bytes(nq)) + 256, dtype=torch.uint8, device=self.device)
            _lib.check(L.pch_dbscan_assign_f32(_ptr(query), nq, None if s3 is None else C.cast(s3, C.c_void_p),
                                               _ptr(chunk), self.n, _ptr(out), _ptr(qws), qws.numel(),
                                               _ptr(self.workspace), self.workspace.numel(), _stream()))
        return out

    def kdist(self, query, k, sub=None, chunk=None, want_count=False):
        """Squared distance (float64 [nq], device) from every float32 [nq,3] point to its ``k``-th nearest row of the
        fit, core or not, exactly: the k-th smallest ``d2 <= eps*eps`` under the library's float64 predicate, ``+inf``
        where fewer than ``k`` rows lie within the fit's eps (pch_dbscan_kdist_f32).  The answer is truncated at the
        fit's eps: fit at the largest eps of interest with any min_samples, one fit then serves every ``k``.  ``sub``
        and ``chunk`` as for ``assign``; ``chunk="own"`` says that the query is the fitted array itself (row i belongs
        to chunk i // chunk_size; the row itself is then its own first neighbour at 0.0).  ``want_count``: also the
        int32 [nq] number of rows within eps - on the fit's own rows ``core == (count >= min_samples)``.  Reads the
        fit only and does not depend on labels.  Asynchronous."""
        import ctypes as C
        import numpy as np
        if int(k) < 1:
            raise ValueError("k must be at least 1")
        own = isinstance(chunk, str)
        if own and chunk != "own":
            raise ValueError('chunk must be an int32 tensor, None or "own"')
        query = _need_cuda(query, torch.float32, "query").reshape(-1, 3)
        nq = query.shape[0]
        if own:
            if nq != self.n:
                raise ValueError('chunk="own" needs the fitted array itself: one query row per fitted row')
            chunk = None
        elif chunk is not None:
            chunk = _need_cuda(chunk, torch.int32, "chunk").reshape(-1)
            if chunk.numel() != nq:
                raise ValueError("chunk must name one chunk per query row")
        with torch.cuda.device(self.device):
            if own and self.chunk_size:
                chunk = (torch.arange(nq, dtype=torch.int64, device=self.device) // self.chunk_size).to(torch.int32)
            d2 = torch.empty((nq,), dtype=torch.float64, device=self.device)
            count = torch.empty((nq,), dtype=torch.int32, device=self.device) if want_count else None
            if nq:
                L = _lib.lib()
                s3 = None if sub is None else (C.c_float * 3)(*[float(np.float32(v)) for v in sub])
                qws = torch.empty(int(L.pch_dbscan_kdist_ws_bytes(nq)) + 256, dtype=torch.uint8, device=self.device)
                _lib.check(L.pch_dbscan_kdist_f32(_ptr(query), nq, None if s3 is None else C.cast(s3, C.c_void_p),
                                                  _ptr(chunk), int(k), self.n, _ptr(d2), _ptr(count), _ptr(qws),
                                                  qws.numel(), _ptr(self.workspace), self.workspace.numel(),
                                                  _stream()))
        return (d2, count) if want_count else d2

    def knn(self, query, k, sub=None, chunk=None, want_count=False):
        """(rows int32 [nq,k], d2 float64 [nq,k]), device: for every float32 [nq,3] point its ``k`` nearest rows of the
        fit, core or not, among those within the fit's eps under the library's float64 predicate, in ``(d2, row)``
        order - ``row`` the global file-order row of the fitted array, so ties go to the smaller row
        (pch_dbscan_knn_f32).  Slots beyond the rows in reach hold ``-1`` and ``+inf``.  ``1 <= k <= ops.KNN_MAX_K``
        (ValueError before any device call).  The answer is truncated at the fit's eps: fit at the radius of interest.
        ``sub``, ``chunk`` and ``chunk="own"`` as for ``kdist`` (on the fit's own rows slot 0 is the row itself at 0.0,
        unless a duplicate with a smaller row comes first).  ``want_count``: also the int32 [nq] number of rows within
        eps.  Reads the fit only and does not depend on labels.  Asynchronous."""
        import ctypes as C
        import numpy as np
        k = check_knn_k(k)
        own = isinstance(chunk, str)
        if own and chunk != "own":
            raise ValueError('chunk must be an int32 tensor, None or "own"')
        query = _need_cuda(query, torch.float32, "query").reshape(-1, 3)
        nq = query.shape[0]
        if own:
            if nq != self.n:
                raise ValueError('chunk="own" needs the fitted array itself: one query row per fitted row')
            chunk = None
        elif chunk is not None:
            chunk = _need_cuda(chunk, torch.int32, "chunk").reshape(-1)
            if chunk.numel() != nq:
                raise ValueError("chunk must name one chunk per query row")
        with torch.cuda.device(self.device):
            if own and self.chunk_size:
                chunk = (torch.arange(nq, dtype=torch.int64, device=self.device) // self.chunk_size).to(torch.int32)
            rows = torch.empty((nq, k), dtype=torch.int32, device=self.device)
            d2 = torch.empty((nq, k), dtype=torch.float64, device=self.device)
            count = torch.empty((nq,), dtype=torch.int32, device=self.device) if want_count else None
            if nq:
                L = _lib.lib()
                s3 = None if sub is None else (C.c_float * 3)(*[float(np.float32(v)) for v in sub])
                qws = torch.empty(int(L.pch_dbscan_knn_ws_bytes(nq)) + 256, dtype=torch.uint8, device=self.device)
                _lib.check(L.pch_dbscan_knn_f32(_ptr(query), nq, None if s3 is None else C.cast(s3, C.c_void_p),
                                                _ptr(chunk), k, self.n, _ptr(rows), _ptr(d2), _ptr(count), _ptr(qws),
                                                qws.numel(), _ptr(self.workspace), self.workspace.numel(), _stream()))
        return (rows, d2, count) if want_count else (rows, d2)

    def shape(self, query, radius, sub=None, chunk=None):
        """(count int32 [nq], moments float64 [nq,9]), device: for every float32 [nq,3] point the number of rows of the
        fit, core or not, within ``radius`` under the library's float64 predicate, and the sums ``(Σdx, Σdy, Σdz, Σdx²,
        Σdy², Σdz², Σdx·dy, Σdx·dz, Σdy·dz)`` of their float64 differences ``row - query`` (pch_dbscan_shape_f32) -
        moments about the query, so a covariance formed from them loses nothing at the scale of projected
        coordinates; ``ops.shape_features`` turns them into eigenvalue features.  ``radius`` must be finite, > 0 and
        <= the fit's eps (ValueError before any device call): fit at the radius of interest.  ``sub``, ``chunk`` and
        ``chunk="own"`` as for ``kdist``.  Reads the fit only and does not depend on labels.  Asynchronous."""
        import ctypes as C
        import numpy as np
        check_shape_radius(radius, self.eps)
        own = isinstance(chunk, str)
        if own and chunk != "own":
            raise ValueError('chunk must be an int32 tensor, None or "own"')
        query = _need_cuda(query, torch.float32, "query").reshape(-1, 3)
        nq = query.shape[0]
        if own:
            if nq != self.n:
                raise ValueError('chunk="own" needs the fitted array itself: one query row per fitted row')
            chunk = None
        elif chunk is not None:
            chunk = _need_cuda(chunk, torch.int32, "chunk").reshape(-1)
            if chunk.numel() != nq:
                raise ValueError("chunk must name one chunk per query row")
        with torch.cuda.device(self.device):
            if own and self.chunk_size:
                chunk = (torch.arange(nq, dtype=torch.int64, device=self.device) // self.chunk_size).to(torch.int32)
            count = torch.empty((nq,), dtype=torch.int32, device=self.device)
            moments = torch.empty((nq, 9), dtype=torch.float64, device=self.device)
            if nq:
                L = _lib.lib()
                s3 = None if sub is None else (C.c_float * 3)(*[float(np.float32(v)) for v in sub])
                qws = torch.empty(int(L.pch_dbscan_shape_ws_bytes(nq)) + 256, dtype=torch.uint8, device=self.device)
                _lib.check(L.pch_dbscan_shape_f32(_ptr(query), nq, None if s3 is None else C.cast(s3, C.c_void_p),
                                                  _ptr(chunk), float(radius), self.n, _ptr(count), _ptr(moments),
                                                  _ptr(qws), qws.numel(), _ptr(self.workspace),
                                                  self.workspace.numel(), _stream()))
        return count, moments


KNN_MAX_K = 256                                  # PCH_KNN_MAX_K of include/pch_hip.h


def check_knn_k(k):
    """``k`` as an int; ValueError unless ``1 <= k <= KNN_MAX_K``.  Touches no device."""
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= KNN_MAX_K:
        raise ValueError(f"k must be an integer in 1..{KNN_MAX_K}, got {k!r}")
    return int(k)


def knn_mean_distance(d2, count, k):
    """float64 [nq]: the mean distance ``sum_j sqrt(d2[:, j]) / k`` over the first ``k`` slots of ``DbscanFit.knn``'s
    answer where ``count >= k``, ``+inf`` elsewhere (fewer than ``k`` rows in reach).  Plain torch arithmetic on the
    tensors' device; the ``+inf`` slots of short answers do not enter the sum."""
    k = check_knn_k(k)
    if not (isinstance(d2, torch.Tensor) and d2.dtype == torch.float64 and d2.dim() == 2):
        raise TypeError("d2 must be a float64 [nq, k] tensor")
    if not (isinstance(count, torch.Tensor) and count.dtype == torch.int32 and count.dim() == 1):
        raise TypeError("count must be an int32 [nq] tensor")
    if d2.shape[1] < k or count.shape[0] != d2.shape[0]:
        raise ValueError(f"d2 must hold at least k = {k} slots per row and one row per count, got {tuple(d2.shape)} "
                         f"for {count.shape[0]} counts")
    full = count >= k
    near = torch.where(full[:, None], d2[:, :k], torch.zeros((), dtype=torch.float64, device=d2.device))
    mean = torch.sqrt(near).sum(dim=1) / float(k)
    return torch.where(full, mean, torch.full((), float("inf"), dtype=torch.float64, device=d2.device))


def check_shape_radius(radius, eps):
    """ValueError unless ``radius`` is finite, > 0 and <= ``eps`` (the grid of a fit reaches its eps and no further).
    Touches no device."""
    import math
    r = float(radius)
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError(f"radius must be finite and > 0, got {radius!r}")
    if r > float(eps):
        raise ValueError(f"radius {r} exceeds the fit's eps {float(eps)}: fit at the largest radius of interest")
    return r


def shape_features(count, moments):
    """Eigenvalue features of the neighbourhoods ``DbscanFit.shape`` summed up: dict of float64 [nq] device tensors
    ``l1 >= l2 >= l3`` (eigenvalues of the covariance ``M2/n - mu mu^T``, cyclic Jacobi in float64,
    pch_shape_features_f64), ``verticality`` (|z| of the unit eigenvector of l1) and the ratios ``linearity =
    (l1-l2)/l1``, ``planarity = (l2-l3)/l1``, ``scattering = l3/l1``, which are 0 where ``l1 <= 0`` (an empty
    neighbourhood, or a single row).  Asynchronous."""
    count = _need_cuda(count, torch.int32, "count").reshape(-1)
    moments = _need_cuda(moments, torch.float64, "moments").reshape(-1, 9)
    nq = count.numel()
    if moments.shape[0] != nq:
        raise ValueError("moments must hold nine sums per count")
    with torch.cuda.device(count.device):
        out4 = torch.empty((nq, 4), dtype=torch.float64, device=count.device)
        _lib.check(_lib.lib().pch_shape_features_f64(_ptr(count), _ptr(moments), nq, _ptr(out4), _stream()))
    l1, l2, l3, v = out4.unbind(1)
    ok = l1 > 0
    den = torch.where(ok, l1, torch.ones_like(l1))
    zero = torch.zeros_like(l1)
    return dict(l1=l1, l2=l2, l3=l3, verticality=v, linearity=torch.where(ok, (l1 - l2) / den, zero),
                planarity=torch.where(ok, (l2 - l3) / den, zero), scattering=torch.where(ok, l3 / den, zero))


def set_mean_slices(k):
    """Slices of the centroid's summary pass for the calls this thread makes from now on: 0 = automatic (by size),
    1..8 = forced (clamped to the number of 65 536-row groups).  Same result whatever it is."""
    _lib.lib().pch_mean_set_slices(int(k))


def set_pair_counting(enable):
    """Counting variant of the radius-count kernel for the fits this thread makes from now on (measurement only)."""
    _lib.lib().pch_dbscan_set_pair_counting(1 if enable else 0)


def set_dbscan_sort_mode(mode):
    """Cell sort of ops.dbscan: "auto" (by chunk count), "chunk" (one workgroup per chunk) or "global"
    (one radix sort).  Same results either way; tests compare them."""
    _lib.lib().pch_dbscan_set_sort_mode({"auto": 0, "chunk": 1, "global": 2}[mode])


def first_nonfinite_row(xyz):
    """Index of the first row of float32 [n,3] holding NaN/inf, -1 if none (what makes sklearn's
    DBSCAN.fit reject a chunk).  Synchronises."""
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    out = torch.empty((1,), dtype=torch.int64, device=xyz.device)
    with torch.cuda.device(xyz.device):
        _lib.check(L.pch_first_nonfinite_row_f32(_ptr(xyz), xyz.shape[0], _ptr(out), _stream()))
    return int(out.item())


# ---------------------------------------------------------------------- stages B + C + D0
_nf_hint = {}          # device index -> fraction of points the previous call kept (sizes the next workspace)
_tower_clusters_route = 0


def last_tower_clusters_route():
    """Route word of this process's last ``tower_clusters`` call (PchTowerClusters.reserved): 1 = the head of stage C
    was planned on the device and ran before the host read the kept count, 0 = the host planned it."""
    return _tower_clusters_route


def tower_clusters(raw, eps=8.0, min_samples=80, chunk_size=50000, pct=25.0, offset=3.0,
                   fallback_offset=1.0, min_keep=1000, want_index=False, segment=True, k_cap=65536):
    """ground_filter + dbscan + segment_by_label behind one library call
    (pch_tower_clusters_f32): the host language is not visited between the stages.
    Returns (ground dict as ops.ground_filter, labels int32 [n_f], nclusters,
    perm | None, offsets | None, stats | None)."""
    import ctypes as C
    L = _lib.lib()
    raw = _need_cuda(raw, torch.float32, "raw").reshape(-1, 3)
    n = raw.shape[0]
    dev = raw.device
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    hint = _nf_hint.get(key)
    # output / workspace capacity for the kept points: the previous call's kept fraction with headroom, a
    # quarter of the input on the first call; a call that keeps more is repeated once, sized for n
    guess = n // 4 if hint is None else int(hint * n * 1.25) + 1024     # hint: kept fraction of the last tile
    caps = [min(n, max(guess, 1 << 16)), n]
    with torch.cuda.device(dev):
        out_points = torch.empty((n, 3), dtype=torch.float32, device=dev)
        out_index = torch.empty((n,), dtype=torch.int32, device=dev) if want_index else None
        info = _lib.TowerClustersInfo()
        for nf_cap in caps:
            labels = torch.empty((nf_cap,), dtype=torch.int32, device=dev)
            perm = torch.empty((nf_cap,), dtype=torch.int32, device=dev) if segment else None
            offsets = torch.empty((k_cap + 1,), dtype=torch.int64, device=dev) if segment else None   # [0..k] are written
            stats = torch.empty((k_cap, 8), dtype=torch.float32, device=dev) if segment else None
            ws = _workspace(L.pch_tower_clusters_ws_bytes(n, nf_cap, k_cap), dev)
            rc = L.pch_tower_clusters_f32(_ptr(raw), n, float(pct), float(offset), float(fallback_offset),
                                          int(min_keep), float(eps), int(min_samples), int(chunk_size),
                                          _ptr(out_points), _ptr(out_index), _ptr(labels), _ptr(perm),
                                          _ptr(offsets), _ptr(stats), nf_cap, k_cap, C.addressof(info),
                                          _ptr(ws), ws.numel(), _stream())
            if rc == -2 and info.count > nf_cap and nf_cap < n:
                continue                                   # kept more than the hint allowed for: once more, sized n
            break
        nf, k = int(info.count), int(info.nclusters)
        global _tower_clusters_route
        _tower_clusters_route = int(info.reserved)
        if rc == -4 and segment and k > k_cap:             # more clusters than k_cap: group separately
            perm, offsets, stats = segment_by_label(labels[:nf], out_points[:nf], k)
            rc = 0
        _lib.check(rc)
    _nf_hint[key] = nf / max(n, 1)
    ground = _ground_result(out_points, out_index, nf, info.centroid, info.base, info.threshold, info.used_fallback,
                            info.count_at_offset, info.aabb)
    if not segment:
        return ground, labels[:nf], k, None, None, None
    return ground, labels[:nf], k, perm[:nf], offsets[:k + 1], stats[:k]


def strip_lattice_reps(xyz, rows, labels, core, strips, eps, cap=4096):
    """One (global row, local cluster) pair per lattice cell of every strip (x_from, x_to) of ``strips`` (at most two):
    the smallest row among the cell's core points with x in the strip (pch_strip_lattice_reps_f32; the lattice is
    anchored at the frame's origin, so neighbouring tiles name the same rows).  xyz float32 [n,3], rows int64 [n]
    ascending, labels int32 [n], core bool / uint8 [n] - device tensors.  Returns a list of int64 [m,2] tensors (row,
    label), sorted by row, one per strip.  Synchronises (reads the counts)."""
    import ctypes as C
    import numpy as np
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    rows = _need_cuda(rows, torch.int64, "rows")
    labels = _need_cuda(labels, torch.int32, "labels")
    core = core.contiguous()
    if not core.is_cuda or core.dtype not in (torch.bool, torch.uint8):
        raise TypeError("core must be a bool / uint8 CUDA/HIP tensor (no CPU fallback in the product path)")
    core = core.view(torch.uint8)
    n, dev = xyz.shape[0], xyz.device
    if len(strips) > 2:
        raise ValueError("at most two strips per call")
    if not (rows.numel() == labels.numel() == core.numel() == n):
        raise ValueError("rows / labels / core must have one entry per point")
    flat = (C.c_float * (2 * max(len(strips), 1)))()
    for k, (a, b) in enumerate(strips):
        flat[2 * k], flat[2 * k + 1] = float(np.float32(a)), float(np.float32(b))
    cap = int(cap)
    with torch.cuda.device(dev):
        while True:
            out_rows = torch.empty((2, max(cap, 1)), dtype=torch.int64, device=dev)
            out_lab = torch.empty((2, max(cap, 1)), dtype=torch.int32, device=dev)
            cnt = torch.empty((4,), dtype=torch.int32, device=dev)
            ws = _workspace(L.pch_strip_lattice_reps_ws_bytes(cap), dev)
            _lib.check(L.pch_strip_lattice_reps_f32(_ptr(xyz), _ptr(rows), _ptr(labels), _ptr(core), n, len(strips),
                                                    C.cast(flat, C.c_void_p), float(eps), cap, _ptr(out_rows),
                                                    _ptr(out_lab), _ptr(cnt), _ptr(ws), ws.numel(), _stream()))
            c = cnt.cpu().tolist()
            if c[2] & 1:
                raise ValueError("strip_lattice_reps: coordinates beyond 2^20 lattice cells from the origin")
            need = max(c[0], c[1])
            if need <= cap and not (c[2] & 2):
                break
            cap = max(2 * cap, need)                       # a strip with more cells than the buffer: once more
    out = []
    for k in range(len(strips)):
        r, lab = out_rows[k, :c[k]], out_lab[k, :c[k]].to(torch.int64)
        order = torch.argsort(r)
        out.append(torch.stack([r[order], lab[order]], dim=1))
    return out


# ---------------------------------------------------------------------------- stage D0
def segment_by_label(labels, xyz, nclusters):
    """Returns (perm int32 [n], offsets int64 [K+1], stats f32 [K,8] (min xyz, max xyz, 0, 0))."""
    L = _lib.lib()
    labels = _need_cuda(labels, torch.int32, "labels")
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    n = labels.shape[0]
    dev = labels.device
    K = int(nclusters)
    with torch.cuda.device(dev):
        perm = torch.empty((n,), dtype=torch.int32, device=dev)
        offsets = torch.zeros((K + 1,), dtype=torch.int64, device=dev)
        stats = torch.zeros((max(K, 1), 8), dtype=torch.float32, device=dev)
        nb = L.pch_segment_by_label_ws_bytes(n, K)
        ws = _workspace(nb, dev)
        _lib.check(L.pch_segment_by_label(_ptr(labels), _ptr(xyz), n, K, _ptr(perm), _ptr(offsets),
                                          _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    return perm, offsets, stats[:K]


# ------------------------------------------------------------- self-tests of the shared scan and sort (tests only)
def selftest_scan_u32(inp, out, form, out_total=None):
    """pch_selftest_scan_u32 on the buffers as given (no copy is made: the entry judges their addresses).  inp / out:
    int32 [n] holding the uint32 bit patterns, out may be inp; out_total: int32 [1] or None."""
    L = _lib.lib()
    n = inp.shape[0]
    with torch.cuda.device(inp.device):
        ws = _workspace(L.pch_selftest_scan_u32_ws_bytes(n, int(form)), inp.device)
        _lib.check(L.pch_selftest_scan_u32(_ptr(inp), _ptr(out), n, int(form), _ptr(out_total), _ptr(ws), ws.numel(),
                                           _stream()))


def selftest_radix_sort_pairs(keys, vals, nbits, out_keys, out_vals):
    """pch_selftest_radix_sort_pairs on the buffers as given.  keys / out_keys: int64 [n] holding the uint64 bit
    patterns; vals / out_vals: int32 [n] holding uint32."""
    L = _lib.lib()
    n = keys.shape[0]
    with torch.cuda.device(keys.device):
        ws = _workspace(L.pch_selftest_radix_sort_ws_bytes(n), keys.device)
        _lib.check(L.pch_selftest_radix_sort_pairs(_ptr(keys), _ptr(vals), n, int(nbits), _ptr(out_keys),
                                                   _ptr(out_vals), _ptr(ws), ws.numel(), _stream()))


# ------------------------------------------------------------- between C and D0, opt-in: merge of cluster pieces
def cluster_centers(xyz, perm, offsets, nclusters):
    """(centers float32 [K,3], sizes int64 [K]), both on the device: per cluster of the grouped rows (perm / offsets of
    ``segment_by_label``) numpy's ``np.mean(P[labels == k], axis=0)`` bit for bit - a sequential float32 sum in row
    order, one float32 division (pch_cluster_centers_f32).  A cluster without rows has centre NaN.  One wave per
    cluster: the time is linear in the largest cluster.  Asynchronous."""
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    perm = _need_cuda(perm, torch.int32, "perm")
    offsets = _need_cuda(offsets, torch.int64, "offsets")
    K = int(nclusters)
    if K < 0 or offsets.numel() != K + 1:
        raise ValueError("offsets must hold nclusters + 1 entries")
    dev = offsets.device
    with torch.cuda.device(dev):
        centers = torch.empty((K, 3), dtype=torch.float32, device=dev)
        sizes = torch.empty((K,), dtype=torch.int64, device=dev)
        _lib.check(L.pch_cluster_centers_f32(_ptr(xyz), _ptr(perm), _ptr(offsets), K, _ptr(centers), _ptr(sizes),
                                             _stream()))
    return centers, sizes


def merge_clusters(xyz, labels, perm, offsets, nclusters, merge_threshold=6.0):
    """Merges the clusters whose centres lie within ``merge_threshold`` of each other, directly or through a chain of
    others - the pieces a chunk boundary of ``dbscan`` cut a tower into (the reference's own remedy, test/tttt.py:93-175;
    the rule is in include/pch_hip.h).  labels / perm / offsets: a fit and its ``segment_by_label`` grouping.

    Returns dict: labels (a new int32 tensor, the input is left untouched), nclusters (after the merge), perm / offsets /
    stats (``segment_by_label`` of the new labels), map int32 [K] (old id -> new id), centers float32 [K,3] (of the OLD
    clusters), nclusters_before.  One host read (the new cluster count)."""
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    labels = _need_cuda(labels, torch.int32, "labels")
    K = int(nclusters)
    centers, _ = cluster_centers(xyz, perm, offsets, K)
    dev = labels.device
    n = labels.shape[0]
    with torch.cuda.device(dev):
        merged = labels.clone()
        cmap = torch.empty((K,), dtype=torch.int32, device=dev)
        cnt = torch.empty((1,), dtype=torch.int32, device=dev)
        ws = _workspace(L.pch_cluster_merge_ws_bytes(K), dev)
        _lib.check(L.pch_cluster_merge_f32(_ptr(centers), K, float(merge_threshold), _ptr(merged), n, _ptr(cmap),
                                           _ptr(cnt), _ptr(ws), ws.numel(), _stream()))
        k2 = int(cnt.item())
    perm2, offsets2, stats2 = segment_by_label(merged, xyz, k2)
    return dict(labels=merged, nclusters=k2, perm=perm2, offsets=offsets2, stats=stats2, map=cmap, centers=centers,
                nclusters_before=K)


# ------------------------------------------------------------- conductor spans, opt-in
def _grouping(xyz, perm, offsets, nclusters):
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    perm = _need_cuda(perm, torch.int32, "perm").reshape(-1)
    offsets = _need_cuda(offsets, torch.int64, "offsets").reshape(-1)
    K = int(nclusters)
    if K < 0 or offsets.numel() != K + 1:
        raise ValueError("offsets must hold nclusters + 1 entries")
    return xyz, perm, offsets, K


def cluster_moments(xyz, perm, offsets, nclusters):
    """(count int64 [K], origin float32 [K,3], moments float64 [K,9]), device: per cluster of the grouped rows (perm /
    offsets of ``segment_by_label``) its size, its first row ``o`` and the float64 sums ``(Σdx, Σdy, Σdz, Σdx², Σdy²,
    Σdz², Σdx·dy, Σdx·dz, Σdy·dz)`` of the exact differences ``row - o`` (pch_cluster_moments_f32; the rule is in
    include/pch_hip.h).  perm is swept in fixed blocks whatever the cluster sizes, so the time is linear in the number
    of grouped rows; the same input gives the same bits on every run.  An empty cluster gives count 0 and zeros.
    Asynchronous."""
    L = _lib.lib()
    xyz, perm, offsets, K = _grouping(xyz, perm, offsets, nclusters)
    dev = offsets.device
    n = perm.numel()
    with torch.cuda.device(dev):
        count = torch.empty((K,), dtype=torch.int64, device=dev)
        origin = torch.empty((K, 3), dtype=torch.float32, device=dev)
        moments = torch.empty((K, 9), dtype=torch.float64, device=dev)
        ws = _workspace(L.pch_cluster_moments_ws_bytes(n, K), dev)
        _lib.check(L.pch_cluster_moments_f32(_ptr(xyz), _ptr(perm), _ptr(offsets), n, K, _ptr(count), _ptr(origin),
                                             _ptr(moments), _ptr(ws), ws.numel(), _stream()))
    return count, origin, moments


def span_frames(count, origin, moments):
    """float64 [K,6] device: per cluster ``(cx, cy, cz, ux, uy, 1/h)`` - the centre ``origin + mean``, the unit
    direction of the larger eigenvalue of the horizontal covariance (``ux > 0``, or ``ux == 0`` and ``uy > 0``) and the
    reciprocal of ``h = sqrt(3 λ)``, half the length of rows spread evenly along a line (``h = 1`` where that is 0).
    Step 2 of include/pch_hip.h's rule: float64 torch arithmetic on K records, no kernel.  Asynchronous."""
    count = _need_cuda(count, torch.int64, "count").reshape(-1)
    origin = _need_cuda(origin, torch.float32, "origin").reshape(-1, 3)
    M = _need_cuda(moments, torch.float64, "moments").reshape(-1, 9)
    if origin.shape[0] != count.numel() or M.shape[0] != count.numel():
        raise ValueError("count, origin and moments must describe the same clusters")
    return _span_frames_of(count, origin, M)


def _span_frames_of(count, origin, M):
    """span_frames' arithmetic, on tensors of any device"""
    n = torch.clamp(count, min=1).to(torch.float64)
    mu = M[:, 0:3] / n[:, None]
    cxx = M[:, 3] / n - mu[:, 0] * mu[:, 0]
    cyy = M[:, 4] / n - mu[:, 1] * mu[:, 1]
    cxy = M[:, 6] / n - mu[:, 0] * mu[:, 1]
    theta = 0.5 * torch.atan2(2.0 * cxy, cxx - cyy)
    ux, uy = torch.cos(theta), torch.sin(theta)
    flip = (ux < 0) | ((ux == 0) & (uy < 0))
    ux, uy = torch.where(flip, -ux, ux), torch.where(flip, -uy, uy)
    lam = 0.5 * (cxx + cyy) + torch.hypot(0.5 * (cxx - cyy), cxy)
    h = torch.sqrt(3.0 * torch.clamp(lam, min=0.0))
    h = torch.where(h == 0, torch.ones_like(h), h)
    h = torch.where(torch.isnan(lam), lam, h)
    c = origin.to(torch.float64) + mu
    return torch.stack([c[:, 0], c[:, 1], c[:, 2], ux, uy, 1.0 / h], dim=1).contiguous()


def cluster_profile(xyz, perm, offsets, nclusters, frames):
    """(sums float64 [K,10], ext float64 [K,4]), device: per cluster, in the frame ``span_frames`` gave it, the sums
    ``(Σs, Σs², Σs³, Σs⁴, Σdz, Σs·dz, Σs²·dz, Σdz², Σt, Σt²)`` of the scaled along-track coordinate ``s``, the height
    ``dz`` above the centre and the across-track offset ``t``, and ``(min s, max s, min dz, max dz)``, which are exact
    (pch_cluster_profile_f32; the rule is in include/pch_hip.h).  The same sweep as ``cluster_moments``.  An empty
    cluster gives zeros and ``(+inf, -inf, +inf, -inf)``.  Asynchronous."""
    L = _lib.lib()
    xyz, perm, offsets, K = _grouping(xyz, perm, offsets, nclusters)
    frames = _need_cuda(frames, torch.float64, "frames").reshape(-1, 6)
    if frames.shape[0] != K:
        raise ValueError("frames must hold six values per cluster")
    dev = offsets.device
    n = perm.numel()
    with torch.cuda.device(dev):
        sums = torch.empty((K, 10), dtype=torch.float64, device=dev)
        ext = torch.empty((K, 4), dtype=torch.float64, device=dev)
        ws = _workspace(L.pch_cluster_profile_ws_bytes(n, K), dev)
        _lib.check(L.pch_cluster_profile_f32(_ptr(xyz), _ptr(perm), _ptr(offsets), n, K, _ptr(frames), _ptr(sums),
                                             _ptr(ext), _ptr(ws), ws.numel(), _stream()))
    return sums, ext


SPAN_TABLE_KEYS = ("count", "centre", "direction", "azimuth_deg", "length", "a", "b", "c", "sag", "z_low", "rms_z",
                   "rms_t", "cond")


def _sym3_extreme_eigenvalues(a11, a12, a13, a22, a23, a33):
    """(largest, smallest) eigenvalue of symmetric 3x3 matrices given by their entries (the trigonometric closed form)"""
    import math
    q = (a11 + a22 + a33) / 3.0
    p1 = a12 * a12 + a13 * a13 + a23 * a23
    p2 = (a11 - q) ** 2 + (a22 - q) ** 2 + (a33 - q) ** 2 + 2.0 * p1
    p = torch.sqrt(p2 / 6.0)
    ps = torch.where(p > 0, p, torch.ones_like(p))
    b11, b22, b33, b12, b13, b23 = (a11 - q) / ps, (a22 - q) / ps, (a33 - q) / ps, a12 / ps, a13 / ps, a23 / ps
    det = b11 * (b22 * b33 - b23 * b23) - b12 * (b12 * b33 - b23 * b13) + b13 * (b12 * b23 - b22 * b13)
    phi = torch.acos(torch.clamp(0.5 * det, -1.0, 1.0)) / 3.0
    hi = q + 2.0 * p * torch.cos(phi)
    lo = q + 2.0 * p * torch.cos(phi + 2.0 * math.pi / 3.0)
    return hi, lo


def span_fit(count, frames, sums, ext):
    """The span table: a dict of device tensors over the K clusters, from ``cluster_profile``'s sums - the least-squares
    parabola ``dz ≈ a + b·s + c·s²`` through the normal equations (step 4 of include/pch_hip.h's rule; float64 torch
    arithmetic on K records, no kernel):

    ``count`` int64; ``centre`` [K,3] and ``direction`` [K,2] (the frame's); ``azimuth_deg`` = atan2(uy, ux) in
    degrees, from +x towards +y, in (-90, 90]; ``length`` = (max s - min s)·h in metres (0 for an empty cluster);
    ``a`` (metres), ``b`` (per metre), ``c`` (per metre²): the curve over the along-track distance from the centre in
    metres, heights above ``centre[2]``; ``sag`` = |c|·(length/2)²; ``z_low``: the curve's lowest height inside the
    piece, absolute; ``rms_z`` and ``rms_t``: the residual of the curve and the across-track spread, metres; ``cond``:
    the 2-norm condition number of the normal matrix (about 14 for rows spread evenly; +inf for a singular one).  Pieces of fewer than three
    rows and pieces whose normal matrix is singular (determinant or smallest eigenvalue not > 0) have NaN in a, b, c, sag, z_low, rms_z."""
    count = _need_cuda(count, torch.int64, "count").reshape(-1)
    F = _need_cuda(frames, torch.float64, "frames").reshape(-1, 6)
    S = _need_cuda(sums, torch.float64, "sums").reshape(-1, 10)
    E = _need_cuda(ext, torch.float64, "ext").reshape(-1, 4)
    K = count.numel()
    if F.shape[0] != K or S.shape[0] != K or E.shape[0] != K:
        raise ValueError("count, frames, sums and ext must describe the same clusters")
    return _span_fit_of(count, F, S, E)


def _span_fit_of(count, F, S, E):
    """span_fit's arithmetic, on tensors of any device"""
    nan = torch.full((), float("nan"), dtype=torch.float64, device=count.device)
    n = count.to(torch.float64)
    n1 = torch.clamp(count, min=1).to(torch.float64)
    S1, S2, S3, S4 = S[:, 0], S[:, 1], S[:, 2], S[:, 3]
    r0, r1, r2, szz, st, stt = S[:, 4], S[:, 5], S[:, 6], S[:, 7], S[:, 8], S[:, 9]
    # G = [[n, S1, S2], [S1, S2, S3], [S2, S3, S4]]: cofactors, determinant along the first row
    c00 = S2 * S4 - S3 * S3
    c01 = S2 * S3 - S1 * S4
    c02 = S1 * S3 - S2 * S2
    c11 = n * S4 - S2 * S2
    c12 = S1 * S2 - n * S3
    c22 = n * S2 - S1 * S1
    det = (n * c00 + S1 * c01) + S2 * c02
    hi, lo = _sym3_extreme_eigenvalues(n, S1, S2, S2, S3, S4)
    pd = (det > 0) & (lo > 0)                                  # the normal matrix is positive definite
    ok = (count >= 3) & pd
    d = torch.where(ok, det, torch.ones_like(det))
    a = torch.where(ok, ((c00 * r0 + c01 * r1) + c02 * r2) / d, nan)
    b = torch.where(ok, ((c01 * r0 + c11 * r1) + c12 * r2) / d, nan)
    c = torch.where(ok, ((c02 * r0 + c12 * r1) + c22 * r2) / d, nan)
    cond = torch.where(pd, hi / torch.where(pd, lo, torch.ones_like(lo)), torch.full_like(hi, float("inf")))
    h = 1.0 / F[:, 5]
    smin, smax = E[:, 0], E[:, 1]
    has = count > 0
    zero = torch.zeros_like(n)
    width = torch.where(has, smax - smin, zero)
    # the lowest point of the curve inside [smin, smax]: an end, or the vertex when it is a minimum and lies inside
    def curve(s):
        return a + s * (b + c * s)
    sv = -b / (2.0 * torch.where(c > 0, c, torch.ones_like(c)))
    inside = (c > 0) & (sv >= smin) & (sv <= smax)
    ends = torch.minimum(curve(smin), curve(smax))
    low = torch.where(inside, torch.minimum(ends, curve(torch.where(inside, sv, zero))), ends)
    res = szz - ((a * r0 + b * r1) + c * r2)
    mt = st / n1
    return dict(count=count, centre=F[:, 0:3].contiguous(), direction=F[:, 3:5].contiguous(),
                azimuth_deg=torch.rad2deg(torch.atan2(F[:, 4], F[:, 3])), length=width * h,
                a=a, b=b / h, c=c / (h * h), sag=torch.abs(c) * (0.5 * width) ** 2,
                z_low=torch.where(ok & has, low + F[:, 2], nan),
                rms_z=torch.sqrt(torch.clamp(res, min=0.0) / n1),
                rms_t=torch.sqrt(torch.clamp(stt / n1 - mt * mt, min=0.0)), cond=cond)


# ------------------------------------------------------------- conductor clearance, opt-in
CLEARANCE_TILE = 1024          # rows per workgroup of the clearance sweep (cl_sweep_k): the sizes tests straddle
CLEARANCE_MAX_SPANS = 4096
CLEARANCE_MAX_SEGMENTS = 128


def span_curves(table, frames, ext):
    """float64 [K,10] device: per piece ``(cx, cy, cz, ux, uy, a, b, c, m0, m1)`` - the frame's centre and direction
    (``span_frames``), the table's curve ``a, b, c`` (``span_fit``; metres along the track) and the piece's along-track
    interval ``m0 = ext[:,0]·h``, ``m1 = ext[:,1]·h`` in metres from its centre, ``h = 1.0 / frames[:,5]``
    (``cluster_profile``'s ext).  include/pch_hip.h's rule: float64 torch arithmetic on K records, no kernel.
    Asynchronous."""
    F = _need_cuda(frames, torch.float64, "frames").reshape(-1, 6)
    E = _need_cuda(ext, torch.float64, "ext").reshape(-1, 4)
    abc = [_need_cuda(table[key], torch.float64, key).reshape(-1) for key in ("a", "b", "c")]
    if E.shape[0] != F.shape[0] or any(v.numel() != F.shape[0] for v in abc):
        raise ValueError("table, frames and ext must describe the same pieces")
    return _span_curves_of(abc[0], abc[1], abc[2], F, E)


def _span_curves_of(a, b, c, F, E):
    """span_curves' arithmetic, on tensors of any device"""
    h = 1.0 / F[:, 5]
    return torch.stack([F[:, 0], F[:, 1], F[:, 2], F[:, 3], F[:, 4], a, b, c, E[:, 0] * h, E[:, 1] * h],
                       dim=1).contiguous()


def check_segments(segments):
    """the segment count of a polyline as an int; ValueError unless 1 <= segments <= 128"""
    if isinstance(segments, bool) or int(segments) != segments or not 1 <= int(segments) <= CLEARANCE_MAX_SEGMENTS:
        raise ValueError(f"segments must be an integer in 1..{CLEARANCE_MAX_SEGMENTS}, got {segments!r}")
    return int(segments)


def span_segments(curves, segments=32):
    """(segs float64 [K,S,5], chord_error float64 [K]), device: the polyline of S segments that stands for each curve of
    ``span_curves`` - per segment ``(m_j, z_j, Δm_j, Δz_j, inv_j)``: its first vertex (metres along the track, height
    above the centre), the step to the next vertex and ``1 / (Δm² + Δz²)`` (0 where that is not > 0) - and the bound
    ``|c|·((m1 − m0)/S)²/4`` on the polyline's vertical distance from the parabola: the polyline lies above a hanging
    wire, so clearances to objects below are over-estimated by at most that.  include/pch_hip.h's rule: float64 torch
    arithmetic on K·S records, no kernel.  Asynchronous."""
    S = check_segments(segments)
    curves = _need_cuda(curves, torch.float64, "curves").reshape(-1, 10)
    return _span_segments_of(curves, S)


def _span_segments_of(curves, S):
    """span_segments' arithmetic, on tensors of any device"""
    c = curves[:, 7:8]
    m, z, step = _span_vertices_of(curves, S)
    dm = m[:, 1:] - m[:, :-1]
    dz = z[:, 1:] - z[:, :-1]
    len2 = (dm * dm) + (dz * dz)
    pos = len2 > 0
    inv = torch.where(pos, torch.ones_like(len2) / torch.where(pos, len2, torch.ones_like(len2)),
                      torch.zeros_like(len2))
    segs = torch.stack([m[:, :-1], z[:, :-1], dm, dz, inv], dim=2).contiguous()
    chord = ((torch.abs(c) * (step * step)) / 4.0).reshape(-1)
    return segs, chord


def _span_vertices_of(curves, S):
    """(m, z float64 [K,S+1], step [K,1]): the vertices of the S-segment polyline of each curve, m_S = m1 - the first
    lines of span_segments' arithmetic, shared with span_ground_profile"""
    a, b, c, m0, m1 = (curves[:, i:i + 1] for i in range(5, 10))
    step = (m1 - m0) / float(S)
    j = torch.arange(S, dtype=torch.float64, device=curves.device)[None, :]
    m = torch.cat([m0 + j * step, m1], dim=1)                                # [K,S+1]: m_S = m1
    z = a + m * (b + c * m)
    return m, z, step


def clearance(xyz, curves, segs, radius, limit, skip=None, want_stats=False):
    """The distance of every row of float32 [n,3] to the span polylines (pch_clearance_f32; the rule is in
    include/pch_hip.h): a dict of device tensors - ``dist2`` float64 [n], the squared distance to the nearest span
    within ``radius`` (+inf if none), ``span`` int32 [n], that span (-1 if none; the lowest index on a tie), and over the
    K spans ``count`` int64 (the rows attributed to it - every row to its nearest span only), ``violations`` int64 (those
    with ``dist2 <= limit²``), ``min_dist2`` float64 (+inf without a row) and ``min_row`` int64 (the lowest row that
    attains it, or -1).  ``curves`` float64 [K,5] or [K,10] (``span_curves``; the first five columns are used), ``segs``
    float64 [K,S,5] (``span_segments``), ``skip`` an optional uint8 or bool [n]: rows with a non-zero entry get +inf and
    -1, as rows with a non-finite coordinate do.  A span with a non-finite value takes no part.  ``want_stats`` adds
    ``loops`` int64 [2]: the (row, span) segment loops run and the (tile, span) pairs walked.  ValueError: radius or
    limit not finite, limit <= 0 or > radius, more than 4096 spans, S outside 1..128.  The same input gives the same
    bits on every run.  Asynchronous."""
    import math
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    curves = _need_cuda(curves, torch.float64, "curves")
    segs = _need_cuda(segs, torch.float64, "segs")
    if curves.dim() != 2 or curves.shape[1] not in (5, 10):
        raise ValueError("curves must be [K,5] or [K,10]")
    K = curves.shape[0]
    if segs.dim() != 3 or segs.shape[0] != K or segs.shape[2] != 5:
        raise ValueError("segs must be [K,S,5] for the K spans of curves")
    S = check_segments(segs.shape[1])
    if K > CLEARANCE_MAX_SPANS:
        raise ValueError(f"clearance takes at most {CLEARANCE_MAX_SPANS} spans per call, got {K}")
    radius, limit = float(radius), float(limit)
    if not (math.isfinite(radius) and math.isfinite(limit) and 0.0 < limit <= radius):
        raise ValueError(f"radius and limit must be finite with 0 < limit <= radius, got {radius!r}, {limit!r}")
    n, dev = xyz.shape[0], xyz.device
    if n >= 1 << 32:
        raise ValueError("clearance takes fewer than 2^32 rows per call")
    if skip is not None:
        if isinstance(skip, torch.Tensor) and skip.dtype == torch.bool:
            skip = skip.view(torch.uint8)
        skip = _need_cuda(skip, torch.uint8, "skip").reshape(-1)
        if skip.numel() != n:
            raise ValueError("skip must hold one entry per row")
    curves5 = curves[:, :5].contiguous()
    with torch.cuda.device(dev):
        dist2 = torch.empty((n,), dtype=torch.float64, device=dev)
        span = torch.empty((n,), dtype=torch.int32, device=dev)
        count = torch.empty((K,), dtype=torch.int64, device=dev)
        violations = torch.empty((K,), dtype=torch.int64, device=dev)
        min_dist2 = torch.empty((K,), dtype=torch.float64, device=dev)
        min_row = torch.empty((K,), dtype=torch.int64, device=dev)
        loops = torch.empty((2,), dtype=torch.int64, device=dev) if want_stats else None
        ws = _workspace(L.pch_clearance_ws_bytes(n, K, S), dev)
        _lib.check(L.pch_clearance_f32(_ptr(xyz), _ptr(skip), n, _ptr(curves5), _ptr(segs), K, S, radius, limit,
                                       _ptr(dist2), _ptr(span), _ptr(count), _ptr(violations), _ptr(min_dist2),
                                       _ptr(min_row), _ptr(loops), _ptr(ws), ws.numel(), _stream()))
    out = dict(dist2=dist2, span=span, count=count, violations=violations, min_dist2=min_dist2, min_row=min_row)
    if want_stats:
        out["loops"] = loops
    return out


# ------------------------------------------------------------- wind swing clearance, opt-in
def swing_angle(angle_deg, K):
    """(sT, cT) float64 numpy [K]: numpy's sine and cosine of the largest swing angle in degrees, a scalar or one value
    per span; ValueError unless every angle is finite with 0 <= angle < 90"""
    import numpy as np
    a = np.asarray(angle_deg.detach().cpu() if isinstance(angle_deg, torch.Tensor) else angle_deg, dtype=np.float64)
    if a.ndim == 0:
        a = np.full((K,), float(a), dtype=np.float64)
    a = a.reshape(-1)
    if a.shape[0] != K:
        raise ValueError(f"angle must be a scalar or hold one value per span ({K}), got {a.shape[0]}")
    if not (np.isfinite(a) & (a >= 0.0) & (a < 90.0)).all():
        raise ValueError("the swing angle must be finite with 0 <= angle < 90 degrees")
    rad = np.radians(a)
    return np.sin(rad), np.cos(rad)


def swing_heads(curves, angle_deg):
    """float64 [K,11] device: per span of ``span_curves``' [K,10] the head record of the swing rule ``(cx, cy, cz, ux, uy,
    mA, mB, zA, kap, sT, cT)`` - the frame, the polyline's ends ``mA = m0``, ``mB = m1``, the height ``zA`` of its first
    vertex, the chord's slope ``kap = (z_S − z_0) / (m_S − m_0)`` and numpy's sine and cosine of ``angle_deg`` (degrees;
    a scalar or [K]; ``0 <= angle < 90``).  The chord runs through the ends of the curve, which are the end vertices of
    every polyline of ``span_segments``, so the record does not depend on S.  include/pch_hip.h's rule: float64 torch
    arithmetic on K records, no kernel.  Insulator strings that swing with the wire are not modelled.  Asynchronous."""
    curves = _need_cuda(curves, torch.float64, "curves").reshape(-1, 10)
    sT, cT = swing_angle(angle_deg, curves.shape[0])
    return _swing_heads_of(curves, torch.from_numpy(sT).to(curves.device), torch.from_numpy(cT).to(curves.device))


def _swing_heads_of(curves, sT, cT):
    """swing_heads' arithmetic, on tensors of any device"""
    a, b, c, m0, m1 = (curves[:, i] for i in range(5, 10))
    z0 = a + m0 * (b + c * m0)
    z1 = a + m1 * (b + c * m1)
    kap = (z1 - z0) / (m1 - m0)
    return torch.stack([curves[:, 0], curves[:, 1], curves[:, 2], curves[:, 3], curves[:, 4], m0, m1, z0, kap,
                        sT.reshape(-1), cT.reshape(-1)], dim=1).contiguous()


def swing_segments(curves, segments=32):
    """float64 [K,S,6] device: the segment records of the swing rule for each curve of ``span_curves`` - per segment
    ``(m_j, z_j, f_j, Δm_j, Δz_j, Δf_j)``: ``span_segments``' vertex, how far it hangs below the chord through the
    polyline's two ends (``f_j = zc_j − z_j``, ``zc_j = z_0 + (m_j − m_0)·kap``) and the steps to the next vertex.
    include/pch_hip.h's rule: float64 torch arithmetic on K·S records, no kernel.  Asynchronous."""
    S = check_segments(segments)
    curves = _need_cuda(curves, torch.float64, "curves").reshape(-1, 10)
    return _swing_segments_of(curves, S)


def _swing_segments_of(curves, S):
    """swing_segments' arithmetic, on tensors of any device"""
    m, z, _ = _span_vertices_of(curves, S)
    kap = (z[:, S:] - z[:, :1]) / (m[:, S:] - m[:, :1])
    zc = z[:, :1] + ((m - m[:, :1]) * kap)
    f = zc - z
    return torch.stack([m[:, :-1], z[:, :-1], f[:, :-1], m[:, 1:] - m[:, :-1], z[:, 1:] - z[:, :-1],
                        f[:, 1:] - f[:, :-1]], dim=2).contiguous()


def swing_clearance(xyz, heads, segs, radius, limit, skip=None, want_stats=False):
    """The distance of every row of float32 [n,3] to the span polylines as the wind can swing them
    (pch_swing_clearance_f32; the rule is in include/pch_hip.h): a dict of device tensors - ``dist2`` float64 [n], the
    squared distance to the nearest swung span within ``radius`` (+inf if none), ``span`` int32 [n], that span (-1 if
    none; the lowest index on a tie), ``sin`` float64 [n], the sine of the angle at which that span is nearest (its sign
    tells the side; NaN if none) and over the K spans ``count``, ``violations``, ``min_dist2`` and ``min_row`` as
    ``clearance`` returns them.  ``heads`` float64 [K,11] (``swing_heads``), ``segs`` float64 [K,S,6]
    (``swing_segments``), ``skip`` as ``clearance`` takes it.  A span with a non-finite value, without length
    (``mB <= mA``) or whose (sT, cT) is not the sine and cosine of an angle in [0°, 90°) takes no part.  ``want_stats``
    adds ``loops`` int64 [2].  ValueError as ``clearance``.  The same input gives the same bits on every run.
    Asynchronous."""
    import math
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    heads = _need_cuda(heads, torch.float64, "heads")
    segs = _need_cuda(segs, torch.float64, "segs")
    if heads.dim() != 2 or heads.shape[1] != 11:
        raise ValueError("heads must be [K,11]")
    K = heads.shape[0]
    if segs.dim() != 3 or segs.shape[0] != K or segs.shape[2] != 6:
        raise ValueError("segs must be [K,S,6] for the K spans of heads")
    S = check_segments(segs.shape[1])
    if K > CLEARANCE_MAX_SPANS:
        raise ValueError(f"swing_clearance takes at most {CLEARANCE_MAX_SPANS} spans per call, got {K}")
    radius, limit = float(radius), float(limit)
    if not (math.isfinite(radius) and math.isfinite(limit) and 0.0 < limit <= radius):
        raise ValueError(f"radius and limit must be finite with 0 < limit <= radius, got {radius!r}, {limit!r}")
    n, dev = xyz.shape[0], xyz.device
    if n >= 1 << 32:
        raise ValueError("swing_clearance takes fewer than 2^32 rows per call")
    if skip is not None:
        if isinstance(skip, torch.Tensor) and skip.dtype == torch.bool:
            skip = skip.view(torch.uint8)
        skip = _need_cuda(skip, torch.uint8, "skip").reshape(-1)
        if skip.numel() != n:
            raise ValueError("skip must hold one entry per row")
    with torch.cuda.device(dev):
        dist2 = torch.empty((n,), dtype=torch.float64, device=dev)
        span = torch.empty((n,), dtype=torch.int32, device=dev)
        sin = torch.empty((n,), dtype=torch.float64, device=dev)
        count = torch.empty((K,), dtype=torch.int64, device=dev)
        violations = torch.empty((K,), dtype=torch.int64, device=dev)
        min_dist2 = torch.empty((K,), dtype=torch.float64, device=dev)
        min_row = torch.empty((K,), dtype=torch.int64, device=dev)
        loops = torch.empty((2,), dtype=torch.int64, device=dev) if want_stats else None
        ws = _workspace(L.pch_swing_clearance_ws_bytes(n, K, S), dev)
        _lib.check(L.pch_swing_clearance_f32(_ptr(xyz), _ptr(skip), n, _ptr(heads), _ptr(segs), K, S, radius, limit,
                                             _ptr(dist2), _ptr(span), _ptr(sin), _ptr(count), _ptr(violations),
                                             _ptr(min_dist2), _ptr(min_row), _ptr(loops), _ptr(ws), ws.numel(),
                                             _stream()))
    out = dict(dist2=dist2, span=span, sin=sin, count=count, violations=violations, min_dist2=min_dist2,
               min_row=min_row)
    if want_stats:
        out["loops"] = loops
    return out


# ------------------------------------------------------------- span sections, opt-in
SECTION_MAX_STATIONS = 128


def check_stations(stations):
    """the station count of a section as an int; ValueError unless 1 <= stations <= 128"""
    if isinstance(stations, bool) or int(stations) != stations or not 1 <= int(stations) <= SECTION_MAX_STATIONS:
        raise ValueError(f"stations must be an integer in 1..{SECTION_MAX_STATIONS}, got {stations!r}")
    return int(stations)


def span_section(xyz, curves, stations, half_width, depth, limit, skip=None, want_stats=False):
    """The longitudinal section of every span (pch_span_section_f32; the rule is in include/pch_hip.h): the rows of
    float32 [n,3] that lie within ``half_width`` (horizontal) of a span's track and at most ``depth`` below its sag
    curve, binned into ``stations`` equal stations B along the span.  A dict of device tensors - over the [K,B] cells
    ``count`` int64 (every row under the span counts, also one that lies under other spans as well), ``violations``
    int64 (those at most ``limit`` below the wire), ``min_v`` float32 (the smallest vertical distance, +inf for an
    empty cell) and ``min_row`` int64 (the lowest row that attains it, or -1); per row ``v`` float32 [n] (the smallest
    vertical distance over the spans the row lies under, +inf if none), ``span`` int32 [n] (the lowest span that attains
    it, -1 if none) and ``station`` int32 [n] (its station there, -1 if none).  ``curves`` float64 [K,10]
    (``span_curves``): the wire height is the parabola itself.  ``skip`` an optional uint8 or bool [n]: rows with a
    non-zero entry take part nowhere, as rows with a non-finite coordinate.  A span with a non-finite value or with
    ``m1 <= m0`` takes no part.  ``want_stats`` adds ``stats`` int64 [3]: the (row, span) pairs that took part, the
    (tile, span) pairs walked and the cell flushes.  ValueError: half_width, depth or limit not finite, half_width <= 0,
    limit <= 0 or > depth, more than 4096 spans, stations outside 1..128.  The same input gives the same bits on every
    run.  Asynchronous."""
    import math
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    curves = _need_cuda(curves, torch.float64, "curves")
    if curves.dim() != 2 or curves.shape[1] != 10:
        raise ValueError("curves must be [K,10]")
    K = curves.shape[0]
    B = check_stations(stations)
    if K > CLEARANCE_MAX_SPANS:
        raise ValueError(f"span_section takes at most {CLEARANCE_MAX_SPANS} spans per call, got {K}")
    half_width, depth, limit = float(half_width), float(depth), float(limit)
    if not (math.isfinite(half_width) and math.isfinite(depth) and math.isfinite(limit) and half_width > 0.0
            and 0.0 < limit <= depth):
        raise ValueError("half_width, depth and limit must be finite with half_width > 0 and 0 < limit <= depth, got "
                         f"{half_width!r}, {depth!r}, {limit!r}")
    n, dev = xyz.shape[0], xyz.device
    if n >= 1 << 32:
        raise ValueError("span_section takes fewer than 2^32 rows per call")
    if skip is not None:
        if isinstance(skip, torch.Tensor) and skip.dtype == torch.bool:
            skip = skip.view(torch.uint8)
        skip = _need_cuda(skip, torch.uint8, "skip").reshape(-1)
        if skip.numel() != n:
            raise ValueError("skip must hold one entry per row")
    with torch.cuda.device(dev):
        v = torch.empty((n,), dtype=torch.float32, device=dev)
        span = torch.empty((n,), dtype=torch.int32, device=dev)
        station = torch.empty((n,), dtype=torch.int32, device=dev)
        count = torch.empty((K, B), dtype=torch.int64, device=dev)
        violations = torch.empty((K, B), dtype=torch.int64, device=dev)
        min_v = torch.empty((K, B), dtype=torch.float32, device=dev)
        min_row = torch.empty((K, B), dtype=torch.int64, device=dev)
        stats = torch.empty((3,), dtype=torch.int64, device=dev) if want_stats else None
        ws = _workspace(L.pch_span_section_ws_bytes(n, K, B), dev)
        _lib.check(L.pch_span_section_f32(_ptr(xyz), _ptr(skip), n, _ptr(curves), K, B, half_width, depth, limit,
                                          _ptr(v), _ptr(span), _ptr(station), _ptr(count), _ptr(violations),
                                          _ptr(min_v), _ptr(min_row), _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    out = dict(count=count, violations=violations, min_v=min_v, min_row=min_row, v=v, span=span, station=station)
    if want_stats:
        out["stats"] = stats
    return out


# ------------------------------------------------------------- terrain grid, opt-in
TERRAIN_TILE = 1024            # rows per workgroup of the lowest-return sweep (tl_low_k): the sizes tests straddle
TERRAIN_MAX_CELLS = 1 << 24
TERRAIN_MAX_WINDOW = 64        # cells
TERRAIN_MAX_GAP = 256          # cells


def _sub3(sub):
    """three floats for a sub3_host argument (a ctypes array, which the caller keeps alive over the call), or None"""
    import ctypes as C
    import numpy as np
    if sub is None:
        return None
    v = np.asarray(sub.detach().cpu() if isinstance(sub, torch.Tensor) else sub, dtype=np.float32).reshape(-1)
    if v.size != 3:
        raise ValueError("sub must hold three values")
    return (C.c_float * 3)(*[float(x) for x in v])


def _sub3_ptr(s3):
    import ctypes as C
    return None if s3 is None else C.cast(s3, C.c_void_p)


def terrain_grid(points, cell, sub=None):
    """The xy grid of a terrain model over the rows of float32 [n,3] that are finite in all three coordinates:
    dict(x0, y0, cell, nx, ny) with x0 = (double)fl32(min_x - sub_x), nx = floor((max - x0) / cell) + 1, likewise y
    (PchTerrainGrid, include/pch_hip.h; derived as ``plane_tile_grid`` derives its grid).  The bounds come from a torch
    reduction; one small host read.  ValueError beyond 2^24 cells, naming the smallest cell size that fits."""
    import math
    import numpy as np
    points = _need_cuda(points, torch.float32, "points").reshape(-1, 3)
    cell = float(cell)
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError(f"cell must be positive and finite, got {cell!r}")
    s3 = _sub3(sub)
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=points.device)
    fin = torch.isfinite(points).all(dim=1, keepdim=True)
    lo = torch.where(fin, points[:, :2], inf).amin(dim=0) if points.shape[0] else inf.expand(2)
    hi = torch.where(fin, points[:, :2], -inf).amax(dim=0) if points.shape[0] else (-inf).expand(2)
    host = torch.cat([lo, hi]).cpu().numpy()
    return _terrain_grid_of(host[0:2], host[2:4], np.zeros(2, np.float32) if s3 is None else np.float32(s3[:2]), cell)


def _terrain_grid_of(lo, hi, sub, cell):
    """the grid from the float32 bounds of the finite rows' x, y (inf / -inf without any) and the float32 offset"""
    import math
    import numpy as np
    out, ext = dict(cell=float(cell)), [0.0, 0.0]
    for k, name in enumerate(("x", "y")):
        if not lo[k] <= hi[k]:                          # no finite row: one cell at the origin
            out[name + "0"], out["n" + name] = 0.0, 1
            continue
        with np.errstate(over="ignore"):
            a, b = float(np.float32(lo[k]) - np.float32(sub[k])), float(np.float32(hi[k]) - np.float32(sub[k]))
        if not (math.isfinite(a) and math.isfinite(b)):
            raise ValueError("the bounds of the cloud in the row frame are not finite")
        out[name + "0"], out["n" + name], ext[k] = a, int(math.floor((b - a) / cell)) + 1, b - a
    if out["nx"] * out["ny"] > TERRAIN_MAX_CELLS:
        fits = lambda s: (math.floor(ext[0] / s) + 1) * (math.floor(ext[1] / s) + 1) <= TERRAIN_MAX_CELLS
        lo_s, hi_s = cell, max(ext) + 1.0                              # hi_s: one cell, fits
        for _ in range(100):
            mid = 0.5 * (lo_s + hi_s)
            lo_s, hi_s = (lo_s, mid) if fits(mid) else (mid, hi_s)
        digit = 10.0 ** (math.floor(math.log10(hi_s)) - 5)               # six digits, rounded up: the figure shown fits
        raise ValueError(f"cell {cell:g} gives {out['nx']} x {out['ny']} cells, more than 2^24 = {TERRAIN_MAX_CELLS}; "
                         f"the smallest cell that fits is {math.ceil(hi_s / digit) * digit:.6g}")
    return out


def _terrain_grid_c(grid):
    import math
    g = _lib.TerrainGridC(float(grid["x0"]), float(grid["y0"]), float(grid["cell"]), int(grid["nx"]), int(grid["ny"]))
    if not (g.cell > 0.0 and math.isfinite(g.cell)) or g.nx < 1 or g.ny < 1 or g.nx * g.ny > TERRAIN_MAX_CELLS:
        raise ValueError(f"the grid needs a positive finite cell and between 1 and 2^24 cells, got cell {g.cell!r}, "
                         f"{g.nx} x {g.ny}")
    return g


def _grid_ptr(grid_c):
    import ctypes as C
    return C.cast(C.pointer(grid_c), C.c_void_p)


def _terrain_cells(t, dtype, name, g):
    t = _need_cuda(t, dtype, name).reshape(-1)
    if t.numel() != g.nx * g.ny:
        raise ValueError(f"{name} must hold one value per cell of the {g.nx} x {g.ny} grid")
    return t


def terrain_low(points, grid, sub=None, skip=None, want_stats=False):
    """The lowest return per cell (pch_terrain_low_f32; the rule is in include/pch_hip.h): dict of device tensors -
    ``low`` float32 [ny,nx], the smallest z of ``fl32(points - sub)`` over the rows that take part in the cell (inside
    the grid, finite z, not skipped; -0.0 below +0.0), NaN for a cell without one, and ``count`` int32 [ny,nx].
    ``points`` float32 [n,3]; ``grid`` a dict as ``terrain_grid`` returns it; ``sub`` three floats subtracted in float32
    (None: nothing); ``skip`` an optional uint8 or bool [n].  ``want_stats`` adds ``stats`` int64 [2]: the rows that
    took part and the (tile, cell) flushes.  The same input gives the same bits on every run.  Asynchronous."""
    L = _lib.lib()
    points = _need_cuda(points, torch.float32, "points").reshape(-1, 3)
    g = _terrain_grid_c(grid)
    n, dev, ncells = points.shape[0], points.device, g.nx * g.ny
    if n >= 1 << 31:
        raise ValueError("terrain_low takes fewer than 2^31 rows per call")
    if skip is not None:
        if isinstance(skip, torch.Tensor) and skip.dtype == torch.bool:
            skip = skip.view(torch.uint8)
        skip = _need_cuda(skip, torch.uint8, "skip").reshape(-1)
        if skip.numel() != n:
            raise ValueError("skip must hold one entry per row")
    s3 = _sub3(sub)
    with torch.cuda.device(dev):
        low = torch.empty((g.ny, g.nx), dtype=torch.float32, device=dev)
        count = torch.empty((g.ny, g.nx), dtype=torch.int32, device=dev)
        stats = torch.empty((2,), dtype=torch.int64, device=dev) if want_stats else None
        ws = _workspace(L.pch_terrain_low_ws_bytes(n, ncells), dev)
        _lib.check(L.pch_terrain_low_f32(_ptr(points), _ptr(skip), n, _sub3_ptr(s3), _grid_ptr(g), _ptr(low),
                                         _ptr(count), _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    out = dict(low=low, count=count)
    if want_stats:
        out["stats"] = stats
    return out


def terrain_ground(low, grid, window_cells, dh, max_gap, want_open=False):
    """Ground cells and fill (pch_terrain_ground_f32): dict of device tensors - ``ground`` float32 [ny,nx] (``low`` in a
    ground cell, the inverse-distance mean of the first ground cells within ``max_gap`` cells in -x, +x, -y, +y
    elsewhere, NaN without one) and ``state`` uint8 [ny,nx] (bit 0 ground, bit 1 filled, bit 2 the cell had rows).  A
    cell is ground iff ``low - open <= dh`` with ``open`` the opening of ``low`` by a square window of radius
    ``window_cells``; ``want_open`` adds ``open``.  ValueError: window_cells outside 0..64, max_gap outside 0..256, dh
    negative or not finite.  Asynchronous."""
    import math
    L = _lib.lib()
    g = _terrain_grid_c(grid)
    low = _terrain_cells(low, torch.float32, "low", g)
    for name, v, top in (("window_cells", window_cells, TERRAIN_MAX_WINDOW), ("max_gap", max_gap, TERRAIN_MAX_GAP)):
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= top:
            raise ValueError(f"{name} must be an integer in 0..{top}, got {v!r}")
    dh = float(dh)
    if not (math.isfinite(dh) and dh >= 0.0):
        raise ValueError(f"dh must be finite and >= 0, got {dh!r}")
    dev, ncells = low.device, g.nx * g.ny
    with torch.cuda.device(dev):
        ground = torch.empty((g.ny, g.nx), dtype=torch.float32, device=dev)
        state = torch.empty((g.ny, g.nx), dtype=torch.uint8, device=dev)
        opened = torch.empty((g.ny, g.nx), dtype=torch.float32, device=dev) if want_open else None
        ws = _workspace(L.pch_terrain_ground_ws_bytes(ncells), dev)
        _lib.check(L.pch_terrain_ground_f32(_ptr(low), _grid_ptr(g), int(window_cells), dh, int(max_gap), _ptr(opened),
                                            _ptr(ground), _ptr(state), _ptr(ws), ws.numel(), _stream()))
    out = dict(ground=ground, state=state)
    if want_open:
        out["open"] = opened
    return out


def terrain_height(points, grid, ground, sub=None, want_ground=False):
    """float32 [n], device: the height of every row of ``fl32(points - sub)`` above the ground under it, the bilinear
    value between the four cell centres around it (its own cell's where one of them has no ground); NaN outside the
    grid, over a cell without ground and for a row that is not finite (pch_terrain_height_f32).  ``want_ground``:
    (height, ground under the row), both float32 [n].  Asynchronous."""
    L = _lib.lib()
    points = _need_cuda(points, torch.float32, "points").reshape(-1, 3)
    g = _terrain_grid_c(grid)
    ground = _terrain_cells(ground, torch.float32, "ground", g)
    n, dev = points.shape[0], points.device
    if n >= 1 << 31:
        raise ValueError("terrain_height takes fewer than 2^31 rows per call")
    s3 = _sub3(sub)
    with torch.cuda.device(dev):
        height = torch.empty((n,), dtype=torch.float32, device=dev)
        under = torch.empty((n,), dtype=torch.float32, device=dev) if want_ground else None
        _lib.check(L.pch_terrain_height_f32(_ptr(points), n, _sub3_ptr(s3), _grid_ptr(g), _ptr(ground), _ptr(height),
                                            _ptr(under), _stream()))
    return (height, under) if want_ground else height


def terrain_sample(xy, grid, ground):
    """float64 [m], device: the ground under the float64 positions [m,2], in doubles, by the rule of ``terrain_height``
    (pch_terrain_sample_f64; no subtraction).  Asynchronous."""
    L = _lib.lib()
    xy = _need_cuda(xy, torch.float64, "xy").reshape(-1, 2)
    g = _terrain_grid_c(grid)
    ground = _terrain_cells(ground, torch.float32, "ground", g)
    m, dev = xy.shape[0], xy.device
    if m >= 1 << 31:
        raise ValueError("terrain_sample takes fewer than 2^31 positions per call")
    with torch.cuda.device(dev):
        out = torch.empty((m,), dtype=torch.float64, device=dev)
        _lib.check(L.pch_terrain_sample_f64(_ptr(xy), m, _grid_ptr(g), _ptr(ground), _ptr(out), _stream()))
    return out


def span_ground_profile(curves, segments, grid, ground, limit):
    """How high each curve of ``span_curves`` hangs above the ground (include/pch_hip.h's rule): the vertices of its
    polyline of ``segments`` segments - ``span_segments``' own - are placed in the frame of the grid, the ground under
    them comes from one ``terrain_sample`` call, the rest is float64 torch arithmetic on K·(S+1) records.  Dict of
    device tensors: ``clearance`` and ``ground`` float64 [K,S+1] (NaN where there is no ground), ``covered`` int64 [K],
    ``min_clearance`` float64 [K] (+inf without a covered vertex), ``min_vertex`` int64 [K] (the lowest vertex that
    attains it, -1 without), ``min_at`` float64 [K,3] = (x, y, ground) at that vertex (NaN without) and ``violation``
    bool [K]: ``min_clearance <= limit``.  The polyline lies above the curve by at most ``span_segments``'
    chord_error, so a clearance is over-estimated by at most that.  Asynchronous."""
    S = check_segments(segments)
    curves = _need_cuda(curves, torch.float64, "curves").reshape(-1, 10)
    m, z, _ = _span_vertices_of(curves, S)
    X, Y, W = _span_vertex_positions_of(curves, m, z)
    g = terrain_sample(torch.stack([X, Y], dim=2).reshape(-1, 2), grid, ground).reshape(-1, S + 1)
    return _span_ground_minima_of(X, Y, W, g, float(limit))


def _span_vertex_positions_of(curves, m, z):
    """(X, Y, W float64 [K,S+1]): the polyline's vertices in the frame of the curves' centres, on tensors of any
    device"""
    cx, cy, cz, ux, uy = (curves[:, i:i + 1] for i in range(5))
    return cx + (m * ux), cy + (m * uy), cz + z


def _span_ground_minima_of(X, Y, W, g, limit):
    """span_ground_profile's arithmetic behind the sample, on tensors of any device"""
    K, V = g.shape
    has = ~torch.isnan(g)
    clr = W - g
    inf = torch.full_like(clr, float("inf"))
    key = torch.where(has, clr, inf)
    minc = key.amin(dim=1)
    j = torch.arange(V, dtype=torch.int64, device=g.device)[None, :].expand(K, V)
    first = torch.where(has & (key == minc[:, None]), j, torch.full_like(j, V)).amin(dim=1)
    found = first < V
    at = first.clamp(max=V - 1)[:, None]
    nan = torch.full((K, 3), float("nan"), dtype=torch.float64, device=g.device)
    xyz = torch.cat([X.gather(1, at), Y.gather(1, at), g.gather(1, at)], dim=1)
    return dict(clearance=clr, ground=g, covered=has.sum(dim=1), min_clearance=minc,
                min_vertex=torch.where(found, first, torch.full_like(first, -1)),
                min_at=torch.where(found[:, None], xyz, nan), violation=minc <= limit)


# ------------------------------------------------------------- tree fall, opt-in
TREEFALL_TILE = 1024           # rows per workgroup of the tree-fall sweep (tf_sweep_k): the sizes tests straddle
TREEFALL_CLEAR, TREEFALL_NEAR, TREEFALL_STRIKE = 0, 1, 2       # PCH_TREEFALL_* of include/pch_hip.h
TREEFALL_OUTPUTS = ("dist2", "span", "height", "hazard", "count", "strikes", "min_dist2", "min_row", "max_height",
                    "max_row")


def check_treefall_rule(h_min, h_max, grow, limit):
    """(h_min, h_max, grow, limit) as floats; ValueError unless all are finite with 0 <= h_min <= h_max, grow >= 0 and
    limit >= 0"""
    import math
    h_min, h_max, grow, limit = float(h_min), float(h_max), float(grow), float(limit)
    if not (all(math.isfinite(v) for v in (h_min, h_max, grow, limit)) and 0.0 <= h_min <= h_max and grow >= 0.0
            and limit >= 0.0):
        raise ValueError("h_min, h_max, grow and limit must be finite with 0 <= h_min <= h_max, grow >= 0 and "
                         f"limit >= 0, got {h_min!r}, {h_max!r}, {grow!r}, {limit!r}")
    return h_min, h_max, grow, limit


def treefall(points, curves, segs, grid, ground, h_min, h_max, grow, limit, sub=None, skip=None, want_stats=False):
    """Which rows reach a conductor if they fall towards the line (pch_treefall_f32; the rule is in include/pch_hip.h):
    for every row of ``fl32(points - sub)`` (float32 [n,3]) its height ``H`` above the ground grid, and for the rows with
    ``h_min <= H <= h_max`` the squared distance from the ground foot ``(x, y, ground)`` to the nearest span polyline
    within the row's own ``R = (H + grow) + limit``.  A dict of device tensors - ``dist2`` float64 [n] (+inf if none),
    ``span`` int32 [n] (-1 if none; the lowest index on a tie), ``height`` float32 [n] (``terrain_height``'s, bit for
    bit), ``hazard`` uint8 [n] (0: clear, 1: within ``limit`` of a conductor after falling, 2: strikes) and over the K
    spans ``count`` and ``strikes`` int64, ``min_dist2`` float64 (+inf without a row), ``min_row`` int64 (-1 without),
    ``max_height`` float32 (NaN without) and ``max_row`` int64 (-1 without) - every row attributed to its nearest span
    only.  ``curves`` float64 [K,5] or [K,10] and ``segs`` float64 [K,S,5] as ``clearance`` takes them; ``grid`` and
    ``ground`` as ``terrain_height`` takes them; ``skip`` an optional uint8 or bool [n].  ``want_stats`` adds ``stats``
    int64 [4]: the rows that took part, the rows without ground under them, the (row, span) segment loops run and the
    (tile, span) pairs walked.  ValueError: a bound that is not finite or negative, h_min > h_max, more than 4096
    spans, S outside 1..128.  The same input gives the same bits on every run.  Asynchronous."""
    L = _lib.lib()
    points = _need_cuda(points, torch.float32, "points").reshape(-1, 3)
    curves = _need_cuda(curves, torch.float64, "curves")
    segs = _need_cuda(segs, torch.float64, "segs")
    if curves.dim() != 2 or curves.shape[1] not in (5, 10):
        raise ValueError("curves must be [K,5] or [K,10]")
    K = curves.shape[0]
    if segs.dim() != 3 or segs.shape[0] != K or segs.shape[2] != 5:
        raise ValueError("segs must be [K,S,5] for the K spans of curves")
    S = check_segments(segs.shape[1])
    if K > CLEARANCE_MAX_SPANS:
        raise ValueError(f"treefall takes at most {CLEARANCE_MAX_SPANS} spans per call, got {K}")
    h_min, h_max, grow, limit = check_treefall_rule(h_min, h_max, grow, limit)
    g = _terrain_grid_c(grid)
    ground = _terrain_cells(ground, torch.float32, "ground", g)
    n, dev = points.shape[0], points.device
    if n >= 1 << 31:
        raise ValueError("treefall takes fewer than 2^31 rows per call")
    if skip is not None:
        if isinstance(skip, torch.Tensor) and skip.dtype == torch.bool:
            skip = skip.view(torch.uint8)
        skip = _need_cuda(skip, torch.uint8, "skip").reshape(-1)
        if skip.numel() != n:
            raise ValueError("skip must hold one entry per row")
    s3 = _sub3(sub)
    curves5 = curves[:, :5].contiguous()
    with torch.cuda.device(dev):
        dist2 = torch.empty((n,), dtype=torch.float64, device=dev)
        span = torch.empty((n,), dtype=torch.int32, device=dev)
        height = torch.empty((n,), dtype=torch.float32, device=dev)
        hazard = torch.empty((n,), dtype=torch.uint8, device=dev)
        count = torch.empty((K,), dtype=torch.int64, device=dev)
        strikes = torch.empty((K,), dtype=torch.int64, device=dev)
        min_dist2 = torch.empty((K,), dtype=torch.float64, device=dev)
        min_row = torch.empty((K,), dtype=torch.int64, device=dev)
        max_height = torch.empty((K,), dtype=torch.float32, device=dev)
        max_row = torch.empty((K,), dtype=torch.int64, device=dev)
        stats = torch.empty((4,), dtype=torch.int64, device=dev) if want_stats else None
        ws = _workspace(L.pch_treefall_ws_bytes(n, K, S), dev)
        _lib.check(L.pch_treefall_f32(_ptr(points), _ptr(skip), n, _sub3_ptr(s3), _grid_ptr(g), _ptr(ground),
                                      _ptr(curves5), _ptr(segs), K, S, h_min, h_max, grow, limit, _ptr(dist2),
                                      _ptr(span), _ptr(height), _ptr(hazard), _ptr(count), _ptr(strikes),
                                      _ptr(min_dist2), _ptr(min_row), _ptr(max_height), _ptr(max_row), _ptr(stats),
                                      _ptr(ws), ws.numel(), _stream()))
    out = dict(dist2=dist2, span=span, height=height, hazard=hazard, count=count, strikes=strikes, min_dist2=min_dist2,
               min_row=min_row, max_height=max_height, max_row=max_row)
    if want_stats:
        out["stats"] = stats
    return out


# ------------------------------------------------------------- canopy grid and tree crowns, opt-in
CANOPY_TILE = 1024             # rows per workgroup of the canopy sweeps (cn_top_k, cn_rows_k): the sizes tests straddle
CANOPY_MAX_SMOOTH = 8          # PCH_CANOPY_MAX_SMOOTH, cells
CANOPY_MAX_WINDOW = 32         # PCH_CANOPY_MAX_WINDOW, cells
CANOPY_MAX_CROWN = 256         # PCH_CANOPY_MAX_CROWN, cells
CANOPY_TABLE_KEYS = ("top_cell", "cells", "rows", "max_height", "max_row")


def check_canopy_rule(h_min=0.0, h_max=0.0, smooth=0, r0=0.0, r1=0.0, top_min=0.0, crown_frac=0.0, crown_cells=1):
    """(h_min, h_max, smooth, r0, r1, top_min, crown_frac, crown_cells) as floats and ints; ValueError unless
    0 <= h_min <= h_max, r0 >= 0, r1 >= 0 and top_min >= 0, all finite, smooth is an integer in 0..8, crown_frac lies in
    [0, 1] and crown_cells is an integer in 1..256"""
    import math
    h_min, h_max, r0, r1, top_min, crown_frac = (float(v) for v in (h_min, h_max, r0, r1, top_min, crown_frac))
    if not (all(math.isfinite(v) for v in (h_min, h_max, r0, r1, top_min)) and 0.0 <= h_min <= h_max and r0 >= 0.0
            and r1 >= 0.0 and top_min >= 0.0):
        raise ValueError("h_min, h_max, r0, r1 and top_min must be finite with 0 <= h_min <= h_max, r0 >= 0, r1 >= 0 and "
                         f"top_min >= 0, got {h_min!r}, {h_max!r}, {r0!r}, {r1!r}, {top_min!r}")
    if not 0.0 <= crown_frac <= 1.0:
        raise ValueError(f"crown_frac must lie in [0, 1], got {crown_frac!r}")
    for name, v, lo, top in (("smooth", smooth, 0, CANOPY_MAX_SMOOTH), ("crown_cells", crown_cells, 1, CANOPY_MAX_CROWN)):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= top:
            raise ValueError(f"{name} must be an integer in {lo}..{top}, got {v!r}")
    return h_min, h_max, int(smooth), r0, r1, top_min, crown_frac, int(crown_cells)


def canopy_grid(grid, cell):
    """The canopy grid of ``cell`` metres over the extent of a terrain grid (a dict as ``terrain_grid`` returns it), in
    the same frame and from the same origin: per axis ``n = floor((b - a) / cell) + 1`` with ``a`` the origin and
    ``b = a + n_terrain * cell_terrain`` the far edge - ``_terrain_grid_of``'s arithmetic on the extent.  ValueError
    beyond 2^24 cells."""
    import math
    cell = float(cell)
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError(f"cell must be positive and finite, got {cell!r}")
    out = dict(cell=cell)
    for name in ("x", "y"):
        a = float(grid[name + "0"])
        b = a + int(grid["n" + name]) * float(grid["cell"])
        out[name + "0"], out["n" + name] = a, int(math.floor((b - a) / cell)) + 1
    if out["nx"] * out["ny"] > TERRAIN_MAX_CELLS:
        raise ValueError(f"cell {cell:g} gives a canopy grid of {out['nx']} x {out['ny']} cells, more than 2^24 = "
                         f"{TERRAIN_MAX_CELLS}")
    return out


def _canopy_rows_args(points, grid, ground, canopy_grid, skip, who):
    points = _need_cuda(points, torch.float32, "points").reshape(-1, 3)
    g, cg = _terrain_grid_c(grid), _terrain_grid_c(canopy_grid)
    ground = _terrain_cells(ground, torch.float32, "ground", g)
    n = points.shape[0]
    if n >= 1 << 31:
        raise ValueError(f"{who} takes fewer than 2^31 rows per call")
    if skip is not None:
        if isinstance(skip, torch.Tensor) and skip.dtype == torch.bool:
            skip = skip.view(torch.uint8)
        skip = _need_cuda(skip, torch.uint8, "skip").reshape(-1)
        if skip.numel() != n:
            raise ValueError("skip must hold one entry per row")
    return points, g, cg, ground, skip, n


def canopy_top(points, grid, ground, canopy_grid, h_min, h_max, sub=None, skip=None, want_height=False,
               want_stats=False):
    """The canopy height model (pch_canopy_top_f32; the rule is in include/pch_hip.h): dict of device tensors over the
    cells of ``canopy_grid`` - ``top`` float32 [ny,nx], the largest height ``H = z - ground`` above the terrain model
    (``grid``, ``ground`` as ``terrain_height`` takes them) over the rows of ``fl32(points - sub)`` that take part
    (not skipped, finite, inside the canopy grid, over ground, ``h_min <= H <= h_max``), NaN for a cell without one;
    ``top_row`` int32 [ny,nx], the lowest row that attains it (-1 without) and ``count`` int32 [ny,nx].  ``want_height``
    adds ``height`` float32 [n], ``terrain_height``'s bit for bit; ``want_stats`` adds ``stats`` int64 [2]: the rows
    that took part and the (tile, cell) flushes.  The same input gives the same bits on every run.  Asynchronous."""
    L = _lib.lib()
    points, g, cg, ground, skip, n = _canopy_rows_args(points, grid, ground, canopy_grid, skip, "canopy_top")
    h_min, h_max = check_canopy_rule(h_min=h_min, h_max=h_max)[:2]
    dev, ncells = points.device, cg.nx * cg.ny
    s3 = _sub3(sub)
    with torch.cuda.device(dev):
        top = torch.empty((cg.ny, cg.nx), dtype=torch.float32, device=dev)
        top_row = torch.empty((cg.ny, cg.nx), dtype=torch.int32, device=dev)
        count = torch.empty((cg.ny, cg.nx), dtype=torch.int32, device=dev)
        height = torch.empty((n,), dtype=torch.float32, device=dev) if want_height else None
        stats = torch.empty((2,), dtype=torch.int64, device=dev) if want_stats else None
        ws = _workspace(L.pch_canopy_top_ws_bytes(n, ncells), dev)
        _lib.check(L.pch_canopy_top_f32(_ptr(points), _ptr(skip), n, _sub3_ptr(s3), _grid_ptr(g), _ptr(ground),
                                        _grid_ptr(cg), h_min, h_max, _ptr(top), _ptr(top_row), _ptr(count),
                                        _ptr(height), _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    out = dict(top=top, top_row=top_row, count=count)
    if want_height:
        out["height"] = height
    if want_stats:
        out["stats"] = stats
    return out


def canopy_trees(top, top_row, count, canopy_grid, smooth, r0, r1, top_min, crown_frac, crown_cells, tree_cap=None,
                 want_smooth=False):
    """Tree tops and crowns on a canopy height model (pch_canopy_trees_f32; the rule is in include/pch_hip.h): ``top``
    smoothed over a square window of radius ``smooth`` cells; a cell is a top iff its smoothed height is at least
    ``top_min`` and no cell within ``r0 + r1 * height`` (in cells, 1..32) beats it; every cell climbs to its greatest
    neighbour until a top is reached and belongs to that top's crown if it stands at least ``crown_frac`` of the top's
    height and lies within ``crown_cells`` cells of it.  Dict of device tensors - ``tree`` int32 [ny,nx] (-1: no tree),
    ``ntrees`` (int) and over the T trees, numbered by ascending cell of the top, ``top_cell`` int32, ``cells`` int32,
    ``rows`` int64, ``max_height`` float32 and ``max_row`` int32; ``want_smooth`` adds ``smooth`` float32 [ny,nx].
    ``tree_cap`` (default ``min(cells, 2^20)``) bounds the tables; ValueError naming the cap if there are more trees.
    Reads the number of trees once."""
    L = _lib.lib()
    cg = _terrain_grid_c(canopy_grid)
    top = _terrain_cells(top, torch.float32, "top", cg)
    top_row = _terrain_cells(top_row, torch.int32, "top_row", cg)
    count = _terrain_cells(count, torch.int32, "count", cg)
    _, _, smooth, r0, r1, top_min, crown_frac, crown_cells = check_canopy_rule(
        smooth=smooth, r0=r0, r1=r1, top_min=top_min, crown_frac=crown_frac, crown_cells=crown_cells)
    dev, ncells = top.device, cg.nx * cg.ny
    cap = min(ncells, 1 << 20) if tree_cap is None else tree_cap
    if isinstance(cap, bool) or int(cap) != cap or not 1 <= int(cap) <= TERRAIN_MAX_CELLS:
        raise ValueError(f"tree_cap must be an integer in 1..2^24, got {tree_cap!r}")
    cap = int(cap)
    with torch.cuda.device(dev):
        sm = torch.empty((cg.ny, cg.nx), dtype=torch.float32, device=dev) if want_smooth else None
        tree = torch.empty((cg.ny, cg.nx), dtype=torch.int32, device=dev)
        ntrees = torch.empty((1,), dtype=torch.int32, device=dev)
        top_cell = torch.empty((cap,), dtype=torch.int32, device=dev)
        cells = torch.empty((cap,), dtype=torch.int32, device=dev)
        rows = torch.empty((cap,), dtype=torch.int64, device=dev)
        max_height = torch.empty((cap,), dtype=torch.float32, device=dev)
        max_row = torch.empty((cap,), dtype=torch.int32, device=dev)
        ws = _workspace(L.pch_canopy_trees_ws_bytes(ncells, cap), dev)
        _lib.check(L.pch_canopy_trees_f32(_ptr(top), _ptr(top_row), _ptr(count), _grid_ptr(cg), smooth, r0, r1, top_min,
                                          crown_frac, crown_cells, cap, _ptr(sm), _ptr(tree), _ptr(ntrees),
                                          _ptr(top_cell), _ptr(cells), _ptr(rows), _ptr(max_height), _ptr(max_row),
                                          _ptr(ws), ws.numel(), _stream()))
        T = int(ntrees.item())
    if T > cap:
        raise ValueError(f"{T} trees, more than tree_cap = {cap}: the tables are truncated; pass a larger tree_cap")
    out = dict(tree=tree, ntrees=T, top_cell=top_cell[:T], cells=cells[:T], rows=rows[:T], max_height=max_height[:T],
               max_row=max_row[:T])
    if want_smooth:
        out["smooth"] = sm
    return out


def canopy_rows(points, grid, ground, canopy_grid, h_min, h_max, tree, sub=None, skip=None):
    """int32 [n], device: for every row of ``fl32(points - sub)`` that takes part by ``canopy_top``'s rule - the same
    arguments - the entry of ``tree`` (int32 over ``canopy_grid``, ``canopy_trees``') for its cell, -1 for every other
    row (pch_canopy_rows_f32).  Asynchronous."""
    L = _lib.lib()
    points, g, cg, ground, skip, n = _canopy_rows_args(points, grid, ground, canopy_grid, skip, "canopy_rows")
    h_min, h_max = check_canopy_rule(h_min=h_min, h_max=h_max)[:2]
    tree = _terrain_cells(tree, torch.int32, "tree", cg)
    dev = points.device
    s3 = _sub3(sub)
    with torch.cuda.device(dev):
        out = torch.empty((n,), dtype=torch.int32, device=dev)
        _lib.check(L.pch_canopy_rows_f32(_ptr(points), _ptr(skip), n, _sub3_ptr(s3), _grid_ptr(g), _ptr(ground),
                                         _grid_ptr(cg), h_min, h_max, _ptr(tree), _ptr(out), _stream()))
    return out


# ------------------------------------------------------------- tower profile, opt-in
SLICES_BLOCK = 512            # entries of perm per wave of the slice sweep (sl_sweep_k): the sizes tests straddle
SLICES_MAX = 256               # PCH_SLICES_MAX: slices per table row
SLICES_MAX_TABLES = 4096       # PCH_SLICES_MAX_TABLES
SLICES_MAX_ENTRIES = 1 << 20   # PCH_SLICES_MAX_ENTRIES: table rows x slices


def cluster_slices(xyz, perm, offsets, nclusters, frames5, slot, ntables, dz, nslices):
    """The slice table of the grouped rows (pch_cluster_slices_f32; the rule is in include/pch_hip.h): dict of device
    tensors - ``count`` int32 [T,B], ``ext`` float64 [T,B,4] = (min s, max s, min t, max t) and ``outside`` int64 [T,2]
    (the rows below slice 0 and at or above slice B).  Cluster k of the grouping (perm / offsets of
    ``segment_by_label``) is looked at in its frame ``frames5[k] = (cx, cy, z0, ux, uy)`` (float64 [K,5]): ``s`` along
    ``u``, ``t`` across it, slice ``floor((z - z0) / dz)``; it writes to table row ``slot[k]`` (int32 [K]; -1 or out of
    range: the cluster takes no part, as with a frame that is not finite; clusters that share a row are combined).  A
    slice without a row holds ``(+inf, -inf, +inf, -inf)`` and count 0.  perm is swept in fixed blocks whatever the
    cluster sizes; counts, minima and maxima only, so the same input gives the same bits on every run.  ValueError:
    ntables outside 1..4096, nslices outside 1..256, more than 2^20 entries, dz not finite or not > 0, 2^31 or more
    grouped rows.  Asynchronous."""
    import math
    L = _lib.lib()
    xyz, perm, offsets, K = _grouping(xyz, perm, offsets, nclusters)
    frames5 = _need_cuda(frames5, torch.float64, "frames5").reshape(-1, 5)
    slot = _need_cuda(slot, torch.int32, "slot").reshape(-1)
    if frames5.shape[0] != K or slot.numel() != K:
        raise ValueError("frames5 must hold five values and slot one entry per cluster")
    for name, v, top in (("ntables", ntables, SLICES_MAX_TABLES), ("nslices", nslices, SLICES_MAX)):
        if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= top:
            raise ValueError(f"{name} must be an integer in 1..{top}, got {v!r}")
    T, B = int(ntables), int(nslices)
    if T * B > SLICES_MAX_ENTRIES:
        raise ValueError(f"ntables * nslices must not exceed 2^20 = {SLICES_MAX_ENTRIES}, got {T} * {B}")
    dz = float(dz)
    if not (math.isfinite(dz) and dz > 0.0):
        raise ValueError(f"dz must be finite and > 0, got {dz!r}")
    dev, n = offsets.device, perm.numel()
    if n >= 1 << 31:
        raise ValueError("cluster_slices takes fewer than 2^31 grouped rows per call")
    with torch.cuda.device(dev):
        count = torch.empty((T, B), dtype=torch.int32, device=dev)
        ext = torch.empty((T, B, 4), dtype=torch.float64, device=dev)
        outside = torch.empty((T, 2), dtype=torch.int64, device=dev)
        ws = _workspace(L.pch_cluster_slices_ws_bytes(n, K, T, B), dev)
        _lib.check(L.pch_cluster_slices_f32(_ptr(xyz), _ptr(perm), _ptr(offsets), n, K, _ptr(frames5), _ptr(slot), T, dz,
                                            B, _ptr(count), _ptr(ext), _ptr(outside), _ptr(ws), ws.numel(), _stream()))
    return dict(count=count, ext=ext, outside=outside)


TOWER_LEVEL_KEYS = ("n_levels", "z_low", "z_high", "width", "rows", "top")


def tower_levels(count, ext, z0, dz, ground=None, min_rows=3, arm_window=3.0, arm_excess=4.0, max_levels=8):
    """Cross-arm levels of ``cluster_slices``' tables (include/pch_hip.h's rule; float64 torch arithmetic on [T,B]
    records, no kernel).  With ``G = ceil(arm_window / dz)``: a slice is occupied when it holds at least ``min_rows``
    rows; its width ``w`` is the larger of its two extents; ``body`` is the smallest width among the occupied slices
    at most G slices away; it is an arm slice when ``w - body >= arm_excess``.  A level is a maximal run of arm slices.

    Returns dict of device tensors: ``n_levels`` int64 [T] (at most ``max_levels``, the lowest are kept); ``z_low``,
    ``z_high``, ``width``, ``rows`` float64 [T, max_levels], NaN-padded - the lower edge ``z0 + b_lo·dz`` and the upper
    edge ``z0 + (b_hi + 1)·dz`` of the run, its largest width and its row count; ``top`` float64 [T] = ``z0 + (b_top +
    1)·dz`` for the highest occupied slice, NaN without one.  ``z0``: float64 [T] or a number.  With ``ground`` (float64
    [T]) also ``tower_height = top - ground`` and ``nominal_height`` = ``z_low`` of the lowest level ``- ground``, NaN
    without a level.  An arm thicker than ``2G + 1`` slices is not found: a slice in its middle sees only arm slices
    within G, so its ``body`` is the arm's own width (an arm of up to ``2G`` slices is found whole; from ``2G + 1`` on
    its middle is missing and it shows as two thin levels at its edges).  Asynchronous."""
    count = _need_cuda(count, torch.int32, "count")
    if count.dim() != 2:
        raise ValueError("count must be [T,B]")
    T, B = count.shape
    ext = _need_cuda(ext, torch.float64, "ext").reshape(-1, 4)
    if ext.shape[0] != T * B:
        raise ValueError("ext must hold four values per entry of count")
    z0 = _levels_column(z0, T, count.device, "z0")
    if ground is not None:
        ground = _levels_column(ground, T, count.device, "ground")
    return _tower_levels_of(count, ext.reshape(T, B, 4), z0, dz, ground, min_rows, arm_window, arm_excess, max_levels)


def _levels_column(v, T, dev, name):
    if isinstance(v, torch.Tensor):
        v = _need_cuda(v, torch.float64, name).reshape(-1)
        if v.numel() != T:
            raise ValueError(f"{name} must hold one value per table row")
        return v
    return torch.full((T,), float(v), dtype=torch.float64, device=dev)


def _tower_levels_of(count, ext, z0, dz, ground=None, min_rows=3, arm_window=3.0, arm_excess=4.0, max_levels=8):
    """tower_levels' arithmetic, on tensors of any device"""
    import math
    dz, arm_window, arm_excess = float(dz), float(arm_window), float(arm_excess)
    if not (math.isfinite(dz) and dz > 0.0):
        raise ValueError(f"dz must be finite and > 0, got {dz!r}")
    if not (math.isfinite(arm_window) and arm_window >= 0.0) or math.isnan(arm_excess):
        raise ValueError(f"arm_window must be finite and >= 0 and arm_excess a number, got {arm_window!r}, {arm_excess!r}")
    if isinstance(max_levels, bool) or int(max_levels) != max_levels or int(max_levels) < 1:
        raise ValueError(f"max_levels must be an integer >= 1, got {max_levels!r}")
    L, G = int(max_levels), int(math.ceil(arm_window / dz))
    T, B = count.shape
    dev = count.device
    f64 = dict(dtype=torch.float64, device=dev)
    z0 = z0.to(torch.float64).reshape(T)
    nan = torch.full((), float("nan"), **f64)
    inf = torch.full((), float("inf"), **f64)
    occ = count >= int(min_rows)
    wide = torch.maximum(ext[:, :, 1] - ext[:, :, 0], ext[:, :, 3] - ext[:, :, 2])
    w = torch.where(occ, wide, nan)
    # body: the sliding minimum of the occupied widths over |b' - b| <= G, one shifted copy per offset
    held = torch.where(occ, wide, inf)
    reach = min(G, max(B - 1, 0))
    padded = torch.nn.functional.pad(held, (reach, reach), value=float("inf"))
    body = held
    for d in range(2 * reach + 1):
        body = torch.minimum(body, padded[:, d:d + B])
    arm = occ & ((w - body) >= arm_excess)
    before = torch.nn.functional.pad(arm[:, :-1], (1, 0), value=False)
    start = arm & ~before
    level = torch.cumsum(start.to(torch.int64), dim=1) - 1                  # the run an arm slice belongs to
    found = start.sum(dim=1)
    kept = arm & (level < L)
    at = torch.where(kept, level, torch.full_like(level, L))                # what is not kept goes to a spare column
    b = torch.arange(B, **f64)[None, :].expand(T, B).contiguous()
    b_lo = torch.full((T, L + 1), float("inf"), **f64).scatter_reduce(1, at, b, "amin", include_self=True)[:, :L]
    b_hi = torch.full((T, L + 1), float("-inf"), **f64).scatter_reduce(1, at, b, "amax", include_self=True)[:, :L]
    width = torch.full((T, L + 1), float("-inf"), **f64).scatter_reduce(
        1, at, torch.where(kept, wide, -inf), "amax", include_self=True)[:, :L]
    rows = torch.zeros((T, L + 1), **f64).scatter_add(1, at, count.to(torch.float64))[:, :L]
    has = torch.arange(L, dtype=torch.int64, device=dev)[None, :] < found[:, None]
    zero = torch.zeros((), **f64)
    out = dict(n_levels=torch.clamp(found, max=L),
               z_low=torch.where(has, z0[:, None] + torch.where(has, b_lo, zero) * dz, nan),
               z_high=torch.where(has, z0[:, None] + (torch.where(has, b_hi, zero) + 1.0) * dz, nan),
               width=torch.where(has, width, nan), rows=torch.where(has, rows, nan))
    b_top = torch.where(occ, b, -inf).amax(dim=1) if B else torch.full((T,), float("-inf"), **f64)
    any_occ = occ.any(dim=1)
    out["top"] = torch.where(any_occ, z0 + (torch.where(any_occ, b_top, zero) + 1.0) * dz, nan)
    if ground is not None:
        ground = ground.to(torch.float64).reshape(T)
        out["tower_height"] = out["top"] - ground
        out["nominal_height"] = out["z_low"][:, 0] - ground
    return out


# ---------------------------------------------------------------------------- stage D1, fast mode
def obb_shell(xyz, perm, offsets, nclusters):
    """uint8 [offsets[K]] in grouped order: 1 for the points of every cluster that can be vertices of its
    convex hull (a superset of them), 0 for points strictly inside it (pch_obb_shell_f32)."""
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    perm = _need_cuda(perm, torch.int32, "perm")
    offsets = _need_cuda(offsets, torch.int64, "offsets")
    K = int(nclusters)
    if offsets.numel() != K + 1:
        raise ValueError("offsets must hold nclusters + 1 entries")
    dev = xyz.device
    with torch.cuda.device(dev):
        ng = int(offsets[K].item()) if K else 0
        keep = torch.empty((ng,), dtype=torch.uint8, device=dev)
        if ng:
            ws = _workspace(L.pch_obb_shell_ws_bytes(K), dev)
            _lib.check(L.pch_obb_shell_f32(_ptr(xyz), _ptr(perm), _ptr(offsets), K, ng, _ptr(keep), _ptr(ws),
                                           ws.numel(), _stream()))
    return keep


# ---------------------------------------------------------------------------- stage D1, upright mode (opt-in)
UPRIGHT_T = 4096
UPRIGHT_RECORD = [("status", "<i4"), ("j", "<i4"), ("j0", "<i4"), ("reserved", "<i4"), ("n", "<i8"),
                  ("umin", "<f8"), ("umax", "<f8"), ("vmin", "<f8"), ("vmax", "<f8"), ("zmin", "<f8"), ("zmax", "<f8")]
_upright_tables = {}
_upright_lock = threading.Lock()


def upright_angle_table_host():
    """float64 [4096,2]: (cos, sin) of j * (pi/2) / 4096, by numpy - the table of the rule in include/pch_hip.h"""
    import numpy as np
    theta = np.arange(UPRIGHT_T, dtype=np.float64) * (np.pi / 2) / UPRIGHT_T
    return np.stack([np.cos(theta), np.sin(theta)], axis=1)


def upright_angle_table(device):
    """The angle table of the upright boxes as a float64 [4096,2] tensor on ``device``: built with numpy once per
    device and kept (the kernels evaluate no sine or cosine of their own)."""
    device = torch.device(device)
    key = device.index if device.index is not None else torch.cuda.current_device()
    with _upright_lock:
        table = _upright_tables.get(key)
        if table is None:
            table = _upright_tables[key] = torch.from_numpy(upright_angle_table_host()).to(torch.device("cuda", key))
    return table


def upright_boxes(xyz, perm, offsets, nclusters, to_host=False):
    """Per cluster of the grouped rows (perm / offsets of ``segment_by_label``) the upright box of the rule in
    include/pch_hip.h: z as one axis, the smallest footprint rectangle among 4096 table angles as the other two
    (pch_upright_boxes_f32).  Returns the PchUprightBox records as a uint8 [K,72] device tensor (asynchronous), or with
    ``to_host`` after one copy as a structured numpy array of dtype ``UPRIGHT_RECORD``."""
    import numpy as np
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float32, "xyz").reshape(-1, 3)
    perm = _need_cuda(perm, torch.int32, "perm")
    offsets = _need_cuda(offsets, torch.int64, "offsets")
    K = int(nclusters)
    if K < 0 or offsets.numel() != K + 1:
        raise ValueError("offsets must hold nclusters + 1 entries")
    dev = offsets.device
    with torch.cuda.device(dev):
        records = torch.empty((K, 72), dtype=torch.uint8, device=dev)
        if K:
            table = upright_angle_table(dev)
            cap = perm.numel()
            ws = _workspace(L.pch_upright_boxes_ws_bytes(K, cap), dev)
            _lib.check(L.pch_upright_boxes_f32(_ptr(xyz), _ptr(perm), _ptr(offsets), K, cap, _ptr(table),
                                               _ptr(records), _ptr(ws), ws.numel(), _stream()))
    if not to_host:
        return records
    return records.cpu().numpy().reshape(-1).view(np.dtype(UPRIGHT_RECORD))


def obb_min_boxes(verts, vert_offsets, tris, tri_offsets, sorted_extents=False, nthreads=0):
    """Host arrays in, host arrays out: (to_origin [H,4,4], extents [H,3], status [H]) of H convex hulls
    (pch_obb_min_boxes_f64)."""
    import numpy as np
    L = _lib.lib()
    verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    vo = np.ascontiguousarray(vert_offsets, dtype=np.int64)
    to = np.ascontiguousarray(tri_offsets, dtype=np.int64)
    H = len(vo) - 1
    if len(to) != H + 1 or (H >= 0 and (vo[-1] != len(verts) or to[-1] != len(tris))):
        raise ValueError("offset tables do not match the vertex / triangle arrays")
    T = np.zeros((max(H, 0), 4, 4), dtype=np.float64)
    E = np.zeros((max(H, 0), 3), dtype=np.float64)
    S = np.zeros((max(H, 0),), dtype=np.int32)
    if H > 0:
        _lib.check(L.pch_obb_min_boxes_f64(verts.ctypes.data, vo.ctypes.data, tris.ctypes.data, to.ctypes.data, H,
                                           int(bool(sorted_extents)), int(nthreads), T.ctypes.data, E.ctypes.data,
                                           S.ctypes.data))
    return T, E, S


def obb_search(verts, vert_offsets, angles, angle_offsets, nthreads=0):
    """Host arrays: (best int32 [H], volumes float64 [sum nc]) - index of the candidate direction of smallest
    box volume per hull, and the volume of every candidate (pch_obb_search_f64)."""
    import numpy as np
    L = _lib.lib()
    verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
    angles = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1, 2)
    vo = np.ascontiguousarray(vert_offsets, dtype=np.int64)
    ao = np.ascontiguousarray(angle_offsets, dtype=np.int64)
    H = len(vo) - 1
    if len(ao) != H + 1 or vo[-1] != len(verts) or ao[-1] != len(angles):
        raise ValueError("offset tables do not match the vertex / angle arrays")
    best = np.full((max(H, 0),), -1, dtype=np.int32)
    vol = np.zeros((len(angles),), dtype=np.float64)
    if H > 0:
        _lib.check(L.pch_obb_search_f64(verts.ctypes.data, vo.ctypes.data, angles.ctypes.data, ao.ctypes.data, H,
                                        int(nthreads), best.ctypes.data, vol.ctypes.data))
    return best, vol


# ---------------------------------------------------------------------------- viewer helpers
def crop_aabb(xyz, lo, hi, want_index=False):
    """points[(p >= lo).all(1) & (p <= hi).all(1)] for float64 [n,3], order preserving (test/kuangxuan.py:69-79).
    Returns points [m,3] (and source rows int64 [m]).  Synchronises (reads m)."""
    import ctypes as C
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float64, "xyz").reshape(-1, 3)
    n = xyz.shape[0]
    dev = xyz.device
    mn, mx = _double3(lo), _double3(hi)
    with torch.cuda.device(dev):
        out = torch.empty((n, 3), dtype=torch.float64, device=dev)
        idx = torch.empty((n,), dtype=torch.int64, device=dev) if want_index else None
        cnt = torch.zeros((1,), dtype=torch.int64, device=dev)
        ws = _workspace(L.pch_crop_aabb_ws_bytes(n), dev)
        _lib.check(L.pch_crop_aabb_f64(_ptr(xyz), n, C.cast(mn, C.c_void_p), C.cast(mx, C.c_void_p), _ptr(out),
                                       _ptr(idx), _ptr(cnt), _ptr(ws), ws.numel(), _stream()))
        m = _lib.check_count(cnt.item(), "crop_aabb")
    return (out[:m], idx[:m]) if want_index else out[:m]


def decimate(xyz, k, seed=0, want_index=False):
    """k distinct rows of float64 [n,3] (seeded; pyGUI_towers_test.py:174-177, ui/vtk_widget.py:115-118)."""
    L = _lib.lib()
    xyz = _need_cuda(xyz, torch.float64, "xyz").reshape(-1, 3)
    n, k = xyz.shape[0], int(k)
    if k > n:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    dev = xyz.device
    with torch.cuda.device(dev):
        out = torch.empty((k, 3), dtype=torch.float64, device=dev)
        idx = torch.empty((k,), dtype=torch.int64, device=dev) if want_index else None
        _lib.check(L.pch_decimate_f64(_ptr(xyz), n, k, int(seed) & (2**64 - 1), _ptr(out), _ptr(idx), _stream()))
    return (out, idx) if want_index else out


MAX_CROP_BOXES = 4096


def crop_box_table(boxes):
    """The PchCropBox table of ``boxes`` as a numpy structured array (host): a list of ("aabb", lo, hi) and
    ("obb", center, rotation, extent) - rotation 3x3 with the box axes in its COLUMNS, extent the FULL side lengths,
    as in a tower dict - or an array this function returned.  Pure host code.  ValueError: more than 4096 boxes, an
    unknown kind, a field of the wrong shape."""
    import numpy as np
    dt = np.dtype(_lib.CropBoxC)
    if isinstance(boxes, np.ndarray) and boxes.dtype.fields is not None:
        if boxes.dtype != dt or boxes.ndim != 1:
            raise ValueError("a prepared box table must be a one-dimensional array of PchCropBox records")
        tab = np.ascontiguousarray(boxes)
    else:
        boxes = list(boxes)
        tab = np.zeros((len(boxes),), dtype=dt)
        for t, box in enumerate(boxes):
            kind = box[0] if len(box) else None
            try:
                if kind == "aabb" and len(box) == 3:
                    tab[t]["lo"] = np.asarray(box[1], dtype=np.float64).reshape(3)
                    tab[t]["hi"] = np.asarray(box[2], dtype=np.float64).reshape(3)
                elif kind == "obb" and len(box) == 4:
                    tab[t]["kind"] = 1
                    tab[t]["center"] = np.asarray(box[1], dtype=np.float64).reshape(3)
                    tab[t]["axes"] = np.asarray(box[2], dtype=np.float64).reshape(9)
                    tab[t]["half"] = np.asarray(box[3], dtype=np.float64).reshape(3) * 0.5
                else:
                    raise ValueError(f"box {t}: unknown kind {kind!r} (\"aabb\", lo, hi / \"obb\", center, rotation, "
                                     "extent)")
            except (TypeError, ValueError) as e:
                raise ValueError(f"box {t}: {e}") from None
    if len(tab) > MAX_CROP_BOXES:
        raise ValueError(f"crop_boxes takes at most {MAX_CROP_BOXES} boxes per call, got {len(tab)}")
    if len(tab) and not np.isin(tab["kind"], (0, 1)).all():
        raise ValueError("box table: unknown kind (0 = axis-aligned, 1 = oriented)")
    return tab


def crop_box_bounds(boxes):
    """float64 [T,6] (lo xyz, hi xyz), host: the axis-aligned bounds the sweep of crop_boxes uses to skip a box for a
    tile of rows (pch_crop_box_bounds_f64).  Pure host code."""
    import numpy as np
    tab = crop_box_table(boxes)
    out = np.zeros((len(tab), 6), dtype=np.float64)
    if len(tab):
        _lib.check(_lib.lib().pch_crop_box_bounds_f64(tab.ctypes.data, len(tab), out.ctypes.data))
    return out


def crop_boxes(xyz, boxes, want_index=False, cap=None):
    """The points of float64 [n,3] inside each of up to 4096 boxes, in one sweep of the cloud (pch_crop_boxes_f64):
    (points [M,3] float64, offsets int64 [T+1]) and, with want_index, the source rows int64 [M] - device tensors; box t
    owns points[offsets[t]:offsets[t+1]], rows ascending as in points[mask], a row inside several boxes once in each.
    boxes: see crop_box_table.  cap: capacity for the hits (default max(n // 8, 65536)); if there are more, the call
    is repeated once with the reported number.  Synchronises (reads the count)."""
    L = _lib.lib()
    tab = crop_box_table(boxes)
    if isinstance(xyz, torch.Tensor) and xyz.dtype != torch.float64:
        raise ValueError(f"xyz must be torch.float64, got {xyz.dtype}")
    xyz = _need_cuda(xyz, torch.float64, "xyz").reshape(-1, 3)
    n, T, dev = xyz.shape[0], len(tab), xyz.device
    cap = max(n // 8, 1 << 16) if cap is None else int(cap)
    if cap < 0:
        raise ValueError("cap must not be negative")
    with torch.cuda.device(dev):
        offsets = torch.empty((T + 1,), dtype=torch.int64, device=dev)
        cnt = torch.empty((1,), dtype=torch.int64, device=dev)
        for attempt in range(2):
            if cap >= 1 << 31:
                raise _lib.PchError(-4, "crop_boxes: 2^31 or more hits")
            out = torch.empty((cap, 3), dtype=torch.float64, device=dev)
            idx = torch.empty((cap,), dtype=torch.int64, device=dev) if want_index else None
            ws = _workspace(L.pch_crop_boxes_ws_bytes(n, T, cap), dev)
            _lib.check(L.pch_crop_boxes_f64(_ptr(xyz), n, tab.ctypes.data, T, cap, _ptr(out), _ptr(idx),
                                            _ptr(offsets), _ptr(cnt), _ptr(ws), ws.numel(), _stream()))
            m = _lib.check_count(cnt.item(), "crop_boxes")
            if m <= cap:
                break
            del out, idx
            cap = m                                        # more hits than the buffer holds: once more, with room
        else:
            raise RuntimeError("crop_boxes: the hit count grew between two calls on the same cloud")
    return (out[:m], offsets, idx[:m]) if want_index else (out[:m], offsets)
