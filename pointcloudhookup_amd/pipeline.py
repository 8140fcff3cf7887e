"""Device orchestration of the hot path (stages B, C, D0) and the host tail (D1-D3).

``cluster_points`` is the unit the benchmark times: float32 [N,3] resident in HBM in,
per-point cluster labels + per-cluster row groups out, all computed by libpch_hip.so.
``tower_table`` turns those clusters into the reference's list of tower dicts
(utils/tower_extraction.py:125-218).
"""
from __future__ import annotations

import numpy as np
import torch

from . import obb as _obb
from . import ops

REF_CHUNK = 50000          # utils/tower_extraction.py:96


def cluster_points(raw, eps=8.0, min_points=80, chunk_size=REF_CHUNK, pct=25.0, offset=3.0,
                   fallback_offset=1.0, min_keep=1000, want_index=False, segment=True, ground="percentile",
                   plane=None, merge_threshold=None, drop_linear=None, drop_sparse=None):
    """Stages B + C + D0 on a float32 [N,3] device tensor.

    Returns dict: ground (ops.ground_filter result), labels int32 [N_f] (device), nclusters,
    perm / offsets / stats (ops.segment_by_label) when ``segment``.

    ``ground`` selects the ground rule of stage B: "percentile" (the reference's, the default: one fused library
    call) or "plane" (opt-in, for sloped terrain: ops.ground_filter_plane, then ops.dbscan and ops.segment_by_label;
    ``plane`` is a dict of keyword arguments for it - hypotheses, seed, residual_threshold, max_slope_deg, keep, ...
    - whose offset / fallback_offset / min_keep / want_index default to this call's) or "plane_tiles" (opt-in, for
    rolling terrain: the same plane per xy tile, ops.ground_filter_plane_tiles; ``plane`` then carries its keyword
    arguments - tile_size, hypotheses, seed, min_tile_rows, fallback_hypotheses, ...).

    ``merge_threshold`` (opt-in, metres; None = off, the reference's behaviour): after the grouping, clusters whose
    centres lie within it of each other become one (ops.merge_clusters - the pieces a chunk boundary cut a tower into;
    the reference's test/tttt.py uses 6.0).  labels / nclusters / perm / offsets / stats are then the merged ones and
    ``merge`` holds map, centers and nclusters_before; with ``segment=False`` the grouping is made internally and only
    the labels are returned.

    ``drop_linear`` (opt-in; None = off, today's path and result): a dict of keyword arguments for ``drop_linear_rows``
    (radius, linearity, verticality, min_rows; ``{}`` takes its defaults).  The kept rows whose neighbourhood is a
    nearly horizontal line - conductors - are removed between stage B and stage C, so that they do not join the towers
    of a line into one cluster; use it with ``chunk_size=0``, ``merge_threshold`` or any mode in which file-order
    chunks no longer cut the line.  The percentile rule then goes the unfused way (ops.ground_filter, the drop,
    ops.dbscan, ops.segment_by_label) as the plane rules do; ``ground`` holds the rows that are left (labels index
    them) and the result gains ``drop_linear = dict(n_dropped, dropped)``, ``dropped`` a bool mask over stage B's rows.

    ``drop_sparse`` (opt-in; None = off, today's path and result): a dict of keyword arguments for ``drop_sparse_rows``
    (k, radius, std_ratio; ``{}`` takes its defaults).  The kept rows with fewer than k rows within the radius and those
    whose mean distance to their k nearest rows is an outlier - stray returns, which otherwise become border points of
    a tower and widen its box - are removed between stage B and stage C, the unfused way as for ``drop_linear``.  When
    both drops are given the sparse rows go first and ``drop_linear`` sees what is left: ``drop_sparse = dict(n_dropped,
    dropped, threshold)`` then has its mask over stage B's rows, ``drop_linear`` its mask over the rows left after it.
    """
    out = _cluster_points(raw, eps, min_points, chunk_size, pct, offset, fallback_offset, min_keep, want_index,
                          segment or merge_threshold is not None, ground, plane, drop_linear, drop_sparse)
    return out if merge_threshold is None else _merged(out, merge_threshold, segment)


def _merged(out, merge_threshold, segment):
    """the opt-in merge behind the grouping, for cluster_points and cluster_points_las"""
    m = ops.merge_clusters(out["ground"]["points"], out["labels"], out["perm"], out["offsets"], out["nclusters"],
                           merge_threshold)
    out.update(labels=m["labels"], nclusters=m["nclusters"],
               merge=dict(map=m["map"], centers=m["centers"], nclusters_before=m["nclusters_before"]))
    if segment:
        out.update(perm=m["perm"], offsets=m["offsets"], stats=m["stats"])
    else:
        for key in ("perm", "offsets", "stats"):
            del out[key]
    return out


def drop_linear_rows(gf, radius=2.0, linearity=0.9, verticality=0.5, min_rows=10):
    """Opt-in wire removal between stage B and stage C: drops the kept rows whose neighbourhood is a nearly horizontal
    line - conductors, which otherwise join the towers of a line into one cluster that ``_accept`` rejects for its
    width.  ``gf`` is a stage-B result (ops.ground_filter and its kin).  One global ``ops.DbscanFit(points, eps=radius,
    min_samples=1, chunk_size=0)`` - the rule is geometric, so file-order chunks play no part, and fitting at the
    radius keeps the neighbour block as small as the rule allows -, ``fit.shape`` on its own rows, ``ops.shape_features``,
    and the mask ``linearity >= L and verticality <= V and count >= min_rows`` (count includes the row itself).

    Returns a copy of ``gf`` whose ``points``, ``index`` (if present), ``count`` and ``aabb`` are those of the rows NOT
    dropped, in file order, plus ``dropped`` (bool [old count], device) and ``n_dropped``.  Stage B kept no row, or the
    fit left no grid to ask (coordinates so spread that it took the compressed-coordinate path, rows that are not
    finite): raises with the cause - nothing is dropped silently.  Synchronises."""
    return _kept_rows(gf, _linear_mask(gf["points"], radius, linearity, verticality, min_rows, "drop_linear_rows"))


def _linear_mask(points, radius=2.0, linearity=0.9, verticality=0.5, min_rows=10, who="drop_linear_rows"):
    """bool [n], device: the rows of ``points`` whose ``radius`` neighbourhood is a nearly horizontal line - the mask of
    ``drop_linear_rows`` and of ``conductor_spans``; ``who`` names the caller in the errors"""
    ops.check_shape_radius(radius, radius)
    n = int(points.shape[0])
    if n == 0:
        raise ValueError(f"{who}: stage B kept no rows, so there is no neighbourhood to look at")
    fit = ops.DbscanFit(points, eps=float(radius), min_samples=1, chunk_size=0)
    try:
        count, moments = fit.shape(points, float(radius), chunk="own")
    except RuntimeError as e:
        raise RuntimeError(f"{who}: the fit of {n} rows at eps = {float(radius)} left no grid to ask "
                           f"(compressed coordinates or rows that are not finite), so no row was examined: {e}") from e
    f = ops.shape_features(count, moments)
    mask = (f["linearity"] >= float(linearity)) & (f["verticality"] <= float(verticality)) & (count >= int(min_rows))
    del fit
    return mask


def conductor_spans(points, rule=None, eps=1.0, min_rows=5, towers=None, cut_radius=9.0, min_length=20.0,
                    max_rms_z=0.25, max_rms_t=0.25):
    """Conductors as a span table: the rows that ``drop_linear_rows`` would drop, grouped into wire
    pieces, each with a fitted sag curve.  ``points``: float32 [n,3] on the device (stage B's rows); ``rule``: a dict
    of ``drop_linear_rows``' keyword arguments (None or ``{}``: its defaults).

    ``towers`` (optional, [T,2] or [T,3] centres in the frame of ``points``): wire rows with ``dx*dx + dy*dy <=
    cut_radius**2`` (float64) to any tower are taken out, which cuts continuous conductors at the towers.  The rows
    left are fitted once (``ops.dbscan(wire_rows, eps, min_rows, chunk_size=0)``), grouped (``ops.segment_by_label``)
    and reduced (``ops.cluster_moments``, ``ops.span_frames``, ``ops.cluster_profile``, ``ops.span_fit``).  A piece is
    accepted iff ``length >= min_length``, ``rms_z <= max_rms_z`` and ``rms_t <= max_rms_t``.

    Returns dict: ``wire`` (bool [n], device: the rows that were grouped), ``labels`` (int32 over the wire rows, in
    file order), ``nclusters``, ``perm`` / ``offsets`` (the grouping, indices into the wire rows), ``table`` (the
    ``ops.span_fit`` dict over the K pieces), ``accepted`` (bool [K]) and ``frames`` / ``ext`` (``ops.span_frames``'
    and ``ops.cluster_profile``'s tensors, which ``conductor_clearance`` turns into curves).  No wire rows: an empty
    table, nothing is raised.  No rows at all, or a fit without a grid: raises as ``drop_linear_rows`` does.  Synchronises."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32:
        raise TypeError("points must be a float32 CUDA/HIP tensor (no CPU fallback in the product path)")
    points = points.reshape(-1, 3).contiguous()
    dev = points.device
    wire = _linear_mask(points, who="conductor_spans", **(rule or {}))
    near = _near_towers(points, towers, cut_radius)
    if near is not None:
        wire = wire & ~near
    rows = points[wire]
    if int(rows.shape[0]):
        labels, _, k = ops.dbscan(rows, float(eps), int(min_rows), 0)
    else:
        labels, k = torch.empty((0,), dtype=torch.int32, device=dev), 0
    perm, offsets, _ = ops.segment_by_label(labels, rows, k)
    count, origin, moments = ops.cluster_moments(rows, perm, offsets, k)
    frames = ops.span_frames(count, origin, moments)
    sums, ext = ops.cluster_profile(rows, perm, offsets, k, frames)
    table = ops.span_fit(count, frames, sums, ext)
    accepted = ((table["length"] >= float(min_length)) & (table["rms_z"] <= float(max_rms_z))
                & (table["rms_t"] <= float(max_rms_t)))
    return dict(wire=wire, labels=labels, nclusters=k, perm=perm, offsets=offsets, table=table, accepted=accepted,
                frames=frames, ext=ext)


def _near_towers(points, towers, cut_radius):
    """bool [n], device: the rows of ``points`` with ``dx*dx + dy*dy <= cut_radius**2`` (float64) to any tower centre -
    the cut of ``conductor_spans`` and of ``conductor_clearance``; None without towers"""
    if towers is None:
        return None
    tw = np.asarray(towers.cpu() if isinstance(towers, torch.Tensor) else towers, dtype=np.float64)
    if tw.size and (tw.ndim != 2 or tw.shape[1] not in (2, 3)):
        raise ValueError("towers must be [T,2] or [T,3] centres")
    if not tw.size:
        return None
    tw = torch.as_tensor(tw[:, :2].copy(), device=points.device)
    xy = points[:, :2].to(torch.float64)
    dx = xy[:, None, 0] - tw[None, :, 0]
    dy = xy[:, None, 1] - tw[None, :, 1]
    return ((dx * dx + dy * dy) <= float(cut_radius) * float(cut_radius)).any(dim=1)


CLEARANCE_TABLE_KEYS = ("count", "violations", "min_distance", "min_row", "min_point", "chord_error")


def conductor_clearance(points, spans, radius=10.0, limit=6.0, segments=32, towers=None, cut_radius=9.0):
    """How close anything that is not the line comes to it: the distance of every row of ``points``
    (float32 [n,3] on the device) to the sag curves of the accepted pieces of ``spans``, the dict ``conductor_spans``
    returned for the same ``points``.  Each accepted piece becomes a polyline of ``segments`` segments
    (``ops.span_curves``, ``ops.span_segments``); the rows that are the conductors (``spans["wire"]``) and, with
    ``towers``, the rows within ``cut_radius`` (horizontal, float64) of a tower - ``conductor_spans``' own predicate -
    are skipped; ``ops.clearance`` does the rest.  Every row is attributed to its nearest piece only.

    Returns dict: ``dist2`` (float64 [n]: the squared distance to the nearest accepted piece within ``radius``, +inf if
    none or skipped), ``span`` (int32 [n]: that piece's id in the span table, -1 if none), ``violating`` (bool [n]:
    ``dist2 <= limit²``) and ``table``, a dict over the K pieces of the span table: ``count`` and ``violations``
    (int64), ``min_distance`` (metres; +inf without a row), ``min_row`` (the lowest row at that distance, -1 without),
    ``min_point`` ([K,3] float32: that row's coordinates, NaN without) and ``chord_error`` (metres: by how much at most
    the polyline over-estimates a clearance below the wire; NaN for a piece that was not accepted).  No accepted piece:
    every row +inf / -1 and a table without rows attributed; nothing is raised.  Synchronises."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32:
        raise TypeError("points must be a float32 CUDA/HIP tensor (no CPU fallback in the product path)")
    points = points.reshape(-1, 3).contiguous()
    n, dev = int(points.shape[0]), points.device
    wire = spans["wire"]
    if wire.numel() != n:
        raise ValueError("spans must be conductor_spans' result for the same points")
    segments = ops.check_segments(segments)
    K = int(spans["nclusters"])
    idx = torch.nonzero(spans["accepted"]).reshape(-1)                        # accepted pieces, ascending
    curves = ops.span_curves(spans["table"], spans["frames"], spans["ext"])[idx].contiguous()
    segs, chord = ops.span_segments(curves, segments)
    near = _near_towers(points, towers, cut_radius)
    skip = wire if near is None else (wire | near)
    res = ops.clearance(points, curves, segs, radius, limit, skip=skip)
    span = res["span"]                                                        # (all -1 without an accepted piece)
    if idx.numel():
        span = torch.where(span >= 0, idx.to(torch.int32)[span.clamp(min=0).long()], torch.full_like(span, -1))
    nan64 = float("nan")
    count = torch.zeros((K,), dtype=torch.int64, device=dev)
    violations = torch.zeros((K,), dtype=torch.int64, device=dev)
    min_distance = torch.full((K,), float("inf"), dtype=torch.float64, device=dev)
    min_row = torch.full((K,), -1, dtype=torch.int64, device=dev)
    chord_error = torch.full((K,), nan64, dtype=torch.float64, device=dev)
    count[idx], violations[idx] = res["count"], res["violations"]
    min_distance[idx], min_row[idx], chord_error[idx] = torch.sqrt(res["min_dist2"]), res["min_row"], chord
    min_point = torch.full((K, 3), nan64, dtype=torch.float32, device=dev)
    has = min_row >= 0
    if n:
        min_point[has] = points[min_row[has]]
    table = dict(count=count, violations=violations, min_distance=min_distance, min_row=min_row, min_point=min_point,
                 chord_error=chord_error)
    return dict(dist2=res["dist2"], span=span, violating=res["dist2"] <= float(limit) * float(limit), table=table)


WIND_TABLE_KEYS = CLEARANCE_TABLE_KEYS + ("min_angle",)


def wind_clearance(points, spans, angle, radius=10.0, limit=6.0, segments=32, towers=None, cut_radius=9.0):
    """How close anything that is not the line comes to it under the largest wind deviation: the
    distance of every row of ``points`` (float32 [n,3] on the device) to the sag curves of the accepted pieces of
    ``spans`` (``conductor_spans``' dict for the same ``points``), each swung sideways about the chord between its
    ends by up to ``angle`` degrees (a scalar, ``0 <= angle < 90``) towards the row.  The pieces, their polylines of
    ``segments`` segments and the skipped rows are ``conductor_clearance``'s; ``ops.swing_heads``,
    ``ops.swing_segments`` and ``ops.swing_clearance`` do the rest.  Every row is attributed to its nearest piece only.
    Insulator strings that swing with the wire are not modelled.

    Returns dict: ``distance`` (float64 [n], metres: to the nearest swung piece within ``radius``, +inf if none or
    skipped), ``span`` (int32 [n]: that piece's id in the span table, -1 if none), ``angle`` (float64 [n], degrees: the
    swing at which that piece is nearest, ``arcsin`` of the call's sine taken on the host, its sign the side; NaN if
    none), ``violating`` (bool [n]: ``dist2 <= limit²``) and ``table``, a dict over the K pieces of the span table with
    ``conductor_clearance``'s keys and ``min_angle`` (degrees: the angle of ``min_row``, NaN without).  No accepted piece:
    every row +inf / -1 / NaN and a table without rows attributed; nothing is raised.  Synchronises."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32:
        raise TypeError("points must be a float32 CUDA/HIP tensor (no CPU fallback in the product path)")
    points = points.reshape(-1, 3).contiguous()
    n, dev = int(points.shape[0]), points.device
    wire = spans["wire"]
    if wire.numel() != n:
        raise ValueError("spans must be conductor_spans' result for the same points")
    segments = ops.check_segments(segments)
    if np.ndim(angle) != 0:
        raise ValueError("angle must be a scalar in degrees")
    K = int(spans["nclusters"])
    idx = torch.nonzero(spans["accepted"]).reshape(-1)                        # accepted pieces, ascending
    curves = ops.span_curves(spans["table"], spans["frames"], spans["ext"])[idx].contiguous()
    heads = ops.swing_heads(curves, float(angle))
    segs = ops.swing_segments(curves, segments)
    _, chord = ops.span_segments(curves, segments)
    near = _near_towers(points, towers, cut_radius)
    skip = wire if near is None else (wire | near)
    res = ops.swing_clearance(points, heads, segs, radius, limit, skip=skip)
    span = res["span"]                                                        # (all -1 without an accepted piece)
    if idx.numel():
        span = torch.where(span >= 0, idx.to(torch.int32)[span.clamp(min=0).long()], torch.full_like(span, -1))
    deg = torch.from_numpy(np.degrees(np.arcsin(res["sin"].cpu().numpy()))).to(dev)
    nan64 = float("nan")
    count = torch.zeros((K,), dtype=torch.int64, device=dev)
    violations = torch.zeros((K,), dtype=torch.int64, device=dev)
    min_distance = torch.full((K,), float("inf"), dtype=torch.float64, device=dev)
    min_row = torch.full((K,), -1, dtype=torch.int64, device=dev)
    chord_error = torch.full((K,), nan64, dtype=torch.float64, device=dev)
    count[idx], violations[idx] = res["count"], res["violations"]
    min_distance[idx], min_row[idx], chord_error[idx] = torch.sqrt(res["min_dist2"]), res["min_row"], chord
    min_point = torch.full((K, 3), nan64, dtype=torch.float32, device=dev)
    min_angle = torch.full((K,), nan64, dtype=torch.float64, device=dev)
    has = min_row >= 0
    if n:
        min_point[has] = points[min_row[has]]
        min_angle[has] = deg[min_row[has]]
    table = dict(count=count, violations=violations, min_distance=min_distance, min_row=min_row, min_point=min_point,
                 chord_error=chord_error, min_angle=min_angle)
    return dict(distance=torch.sqrt(res["dist2"]), span=span, angle=deg,
                violating=res["dist2"] <= float(limit) * float(limit), table=table)


SECTION_KEYS = ("m", "xy", "wire_z", "count", "violations", "min_vertical", "min_row", "top", "ground")
SECTION_TABLE_KEYS = ("count", "violations", "min_vertical", "min_station", "min_row", "min_point")


def span_sections(points, spans, terrain=None, stations=64, half_width=15.0, depth=80.0, limit=7.0, towers=None,
                  cut_radius=9.0):
    """The longitudinal section of every accepted piece of ``spans``: station by station along the wire,
    the rows of ``points`` (float32 [n,3] on the device) that lie within ``half_width`` metres (horizontal) of its track
    and at most ``depth`` metres below its sag curve - how many, how many at most ``limit`` metres below it (the
    vertical distance), the smallest vertical distance and its row.  ``spans`` is ``conductor_spans``' dict for the same
    ``points``; the accepted pieces, their curves (``ops.span_curves``) and the skipped rows - the conductors and, with
    ``towers``, the rows within ``cut_radius`` of a tower - are exactly ``conductor_clearance``'s; ``ops.span_section``
    does the rest.  A row counts under every piece it lies under, not only the nearest.  The wire height is the
    parabola's.

    Returns dict: ``pieces`` (int64 [P]: the accepted pieces' ids, ascending); over the [P,B] cells, B = ``stations``:
    ``m`` (float64: the station's centre, metres from the piece's centre along the track), ``xy`` ([P,B,2] float64:
    that centre in the frame of ``points``), ``wire_z`` (float64: the wire's height there), ``count`` and ``violations``
    (int64), ``min_vertical`` (float32, metres; +inf for an empty cell), ``min_row`` (int64; -1), ``top`` ([P,B,3]
    float32: the coordinates of ``min_row``, NaN where there is none) and ``ground`` (float64: ``ops.terrain_sample`` of
    ``terrain`` - ``terrain_model``'s dict in the same frame - under the station centres; NaN without ``terrain`` or
    where the model has no value); per row ``v`` (float32 [n]: the smallest vertical distance over the pieces the row
    lies under, +inf if none or skipped), ``span`` (int32 [n]: that piece's id in the span table, -1 if none) and
    ``station`` (int32 [n]; -1); and ``table``, a dict over the K pieces of the span table: ``count`` and
    ``violations`` (int64, summed over the stations), ``min_vertical`` (float32; +inf without a row), ``min_station``
    (the lowest station that attains it, -1 without), ``min_row`` (that station's row, -1 without) and ``min_point``
    ([K,3] float32, NaN without).  No accepted piece: P = 0 and a table without rows; nothing is raised.
    Asynchronous."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32:
        raise TypeError("points must be a float32 CUDA/HIP tensor (no CPU fallback in the product path)")
    points = points.reshape(-1, 3).contiguous()
    n, dev = int(points.shape[0]), points.device
    wire = spans["wire"]
    if wire.numel() != n:
        raise ValueError("spans must be conductor_spans' result for the same points")
    B = ops.check_stations(stations)
    K = int(spans["nclusters"])
    idx = torch.nonzero(spans["accepted"]).reshape(-1)                        # accepted pieces, ascending
    P = int(idx.numel())
    curves = ops.span_curves(spans["table"], spans["frames"], spans["ext"])[idx].contiguous()
    near = _near_towers(points, towers, cut_radius)
    skip = wire if near is None else (wire | near)
    res = ops.span_section(points, curves, B, half_width, depth, limit, skip=skip)
    span = res["span"]                                                        # (all -1 without an accepted piece)
    if P:
        span = torch.where(span >= 0, idx.to(torch.int32)[span.clamp(min=0).long()], torch.full_like(span, -1))
    cx, cy, cz, ux, uy, a, b, c, m0, m1 = (curves[:, i:i + 1] for i in range(10))
    step = (m1 - m0) / float(B)
    m = m0 + ((torch.arange(B, dtype=torch.float64, device=dev)[None, :] + 0.5) * step)
    xy = torch.stack([cx + (m * ux), cy + (m * uy)], dim=2)
    wire_z = cz + (a + (m * (b + (c * m))))
    nan = float("nan")
    if terrain is not None and P:
        ground = ops.terrain_sample(xy.reshape(-1, 2).contiguous(), terrain["grid"], terrain["ground"]).reshape(P, B)
    else:
        ground = torch.full((P, B), nan, dtype=torch.float64, device=dev)
    min_row = res["min_row"]
    top = torch.full((P, B, 3), nan, dtype=torch.float32, device=dev)
    has = min_row >= 0
    if n and P:
        top[has] = points[min_row[has]]
    count = torch.zeros((K,), dtype=torch.int64, device=dev)
    violations = torch.zeros((K,), dtype=torch.int64, device=dev)
    min_vertical = torch.full((K,), float("inf"), dtype=torch.float32, device=dev)
    min_station = torch.full((K,), -1, dtype=torch.int64, device=dev)
    tab_row = torch.full((K,), -1, dtype=torch.int64, device=dev)
    min_point = torch.full((K, 3), nan, dtype=torch.float32, device=dev)
    if P:
        low = res["min_v"].min(dim=1).values
        first = (res["min_v"] == low[:, None]).to(torch.int64).argmax(dim=1)
        some = torch.isfinite(low)
        count[idx], violations[idx], min_vertical[idx] = res["count"].sum(dim=1), res["violations"].sum(dim=1), low
        min_station[idx] = torch.where(some, first, torch.full_like(first, -1))
        tab_row[idx] = torch.where(some, min_row.gather(1, first[:, None]).reshape(-1), torch.full_like(first, -1))
        got = tab_row >= 0
        if n:
            min_point[got] = points[tab_row[got]]
    table = dict(count=count, violations=violations, min_vertical=min_vertical, min_station=min_station,
                 min_row=tab_row, min_point=min_point)
    return dict(pieces=idx, m=m, xy=xy, wire_z=wire_z, count=res["count"], violations=res["violations"],
                min_vertical=res["min_v"], min_row=min_row, top=top, ground=ground, v=res["v"], span=span,
                station=res["station"], table=table)


def terrain_cells(cell, window, max_gap):
    """(R, G): the opening's window radius and the fill's gap in cells for ``window`` and ``max_gap`` in metres -
    ``R = ceil(window / (2·cell))``, ``G = ceil(max_gap / cell)``; ValueError beyond the library's limits"""
    import math
    cell, window, max_gap = float(cell), float(window), float(max_gap)
    if not (math.isfinite(cell) and cell > 0.0):
        raise ValueError(f"cell must be finite and > 0, got {cell!r}")
    if not (math.isfinite(window) and window >= 0.0 and math.isfinite(max_gap) and max_gap >= 0.0):
        raise ValueError(f"window and max_gap must be finite and >= 0, got {window!r}, {max_gap!r}")
    R, G = math.ceil(window / (2.0 * cell)), math.ceil(max_gap / cell)
    if R > ops.TERRAIN_MAX_WINDOW:
        raise ValueError(f"window {window:g} m at cell {cell:g} m is a radius of {R} cells; the limit is "
                         f"{ops.TERRAIN_MAX_WINDOW} cells ({2 * ops.TERRAIN_MAX_WINDOW * cell:g} m)")
    if G > ops.TERRAIN_MAX_GAP:
        raise ValueError(f"max_gap {max_gap:g} m at cell {cell:g} m is {G} cells; the limit is "
                         f"{ops.TERRAIN_MAX_GAP} cells ({ops.TERRAIN_MAX_GAP * cell:g} m)")
    return int(R), int(G)


def terrain_model(raw, sub=None, cell=1.0, window=12.0, dh=0.5, max_gap=16.0, skip=None):
    """A ground model that can be sampled: over the rows of ``raw`` (float32 [n,3] on the device, ground
    included; ``sub``: three floats subtracted in float32, e.g. stage B's centroid) a grid of ``cell`` metres with the
    lowest return per cell (``ops.terrain_grid``, ``ops.terrain_low``); the cells whose lowest return stays within
    ``dh`` of its opening by a window of ``window`` metres are ground - roofs, crowns and anything else narrower than
    the window are not -, the others get the inverse-distance mean of the nearest ground cells within ``max_gap`` metres
    along x and y (``ops.terrain_ground``).

    Returns dict: ``grid`` (x0, y0, cell, nx, ny), ``low`` float32 and ``count`` int32 [ny,nx], ``ground`` float32
    [ny,nx] (NaN without a value), ``state`` uint8 [ny,nx] (bit 0 ground, bit 1 filled, bit 2 the cell had rows),
    ``n_ground``, ``n_filled`` and ``n_unfilled`` (cells).  ValueError: a window or a gap beyond the library's limits
    (64 and 256 cells), a grid beyond 2^24 cells.  Synchronises."""
    if not isinstance(raw, torch.Tensor) or not raw.is_cuda or raw.dtype != torch.float32:
        raise TypeError("raw must be a float32 CUDA/HIP tensor (no CPU fallback in the product path)")
    R, G = terrain_cells(cell, window, max_gap)
    raw = raw.reshape(-1, 3).contiguous()
    grid = ops.terrain_grid(raw, cell, sub=sub)
    low = ops.terrain_low(raw, grid, sub=sub, skip=skip)
    res = ops.terrain_ground(low["low"], grid, R, dh, G)
    state = res["state"]
    tally = torch.stack([(state & 1).ne(0).sum(), (state & 2).ne(0).sum(), (state & 3).eq(0).sum()]).cpu()
    return dict(grid=grid, low=low["low"], count=low["count"], ground=res["ground"], state=state,
                n_ground=int(tally[0]), n_filled=int(tally[1]), n_unfilled=int(tally[2]))


def height_above_ground(points, terrain, sub=None):
    """float32 [n], device: the height of every row of ``fl32(points - sub)`` above the ground of ``terrain``
    (``terrain_model``'s dict), NaN where the model has no value (``ops.terrain_height``).  Asynchronous."""
    return ops.terrain_height(points, terrain["grid"], terrain["ground"], sub=sub)


GROUND_CLEARANCE_TABLE_KEYS = ("min_clearance", "min_vertex", "min_at", "covered", "violation", "chord_error")


def span_ground_clearance(spans, terrain, segments=32, limit=7.0):
    """How high the accepted pieces of ``spans`` (``conductor_spans``' dict) hang above the ground of ``terrain``
    (``terrain_model``'s dict, in the same frame) and where they are lowest: each accepted piece becomes
    ``conductor_clearance``'s polyline of ``segments`` segments, whose vertices are held against the ground under them
    (``ops.span_ground_profile``).

    Returns dict: ``pieces`` (int64: the accepted pieces' ids, ascending), ``clearance`` and ``ground`` (float64
    [len(pieces), segments + 1]) and ``table``, a dict over the K pieces of the span table, keyed like
    ``CLEARANCE_TABLE_KEYS``: ``min_clearance`` (metres; +inf without a vertex over ground or for a piece that was not
    accepted), ``min_vertex`` (-1 without), ``min_at`` ([K,3] float64: x, y and the ground's z there, NaN without),
    ``covered`` (int64: the vertices over ground), ``violation`` (bool: ``min_clearance <= limit``) and ``chord_error``
    (metres: by how much at most the polyline over-estimates a clearance; NaN for a piece that was not accepted).  No
    accepted piece: an empty ``pieces`` and a table without a clearance; nothing is raised.  Asynchronous."""
    segments = ops.check_segments(segments)
    K = int(spans["nclusters"])
    idx = torch.nonzero(spans["accepted"]).reshape(-1)                        # accepted pieces, ascending
    dev = spans["accepted"].device
    curves = ops.span_curves(spans["table"], spans["frames"], spans["ext"])[idx].contiguous()
    _, chord = ops.span_segments(curves, segments)
    res = ops.span_ground_profile(curves, segments, terrain["grid"], terrain["ground"], limit)
    nan64 = float("nan")
    table = dict(min_clearance=torch.full((K,), float("inf"), dtype=torch.float64, device=dev),
                 min_vertex=torch.full((K,), -1, dtype=torch.int64, device=dev),
                 min_at=torch.full((K, 3), nan64, dtype=torch.float64, device=dev),
                 covered=torch.zeros((K,), dtype=torch.int64, device=dev),
                 violation=torch.zeros((K,), dtype=torch.bool, device=dev),
                 chord_error=torch.full((K,), nan64, dtype=torch.float64, device=dev))
    for key in ("min_clearance", "min_vertex", "min_at", "covered", "violation"):
        table[key][idx] = res[key]
    table["chord_error"][idx] = chord
    return dict(pieces=idx, clearance=res["clearance"], ground=res["ground"], table=table)


TREEFALL_TABLE_KEYS = ("count", "strikes", "min_distance", "min_row", "max_height", "max_row", "chord_error")
TREEFALL_TREE_KEYS = ("row", "x", "y", "ground", "height", "span", "distance", "margin", "hazard")


def danger_trees(points, spans, terrain, sub=None, h_min=2.0, h_max=45.0, grow=0.0, limit=3.0, segments=32, towers=None,
                 cut_radius=9.0, cell=2.0):
    """Which vegetation, standing where it stands, reaches a conductor if it falls towards the line:
    for every row of ``points`` (float32 [n,3] on the device) its height ``H`` above the ground of ``terrain``
    (``terrain_model``'s dict) and, for the rows with ``h_min <= H <= h_max``, the distance from the ground foot under
    the row to the sag curves of the accepted pieces of ``spans`` (``conductor_spans``' dict for the same ``points``),
    held against ``H + grow`` - ``grow`` being the growth allowed for until the next inspection.  ``points``, ``spans``
    and ``terrain`` are in one frame, as in ``conductor_clearance`` and ``span_ground_clearance``; with ``sub`` the rows
    are ``fl32(points - sub)``, as in ``height_above_ground``, and ``towers`` are in that frame too.  Each accepted piece
    becomes ``conductor_clearance``'s polyline of ``segments`` segments; the rows that are the conductors and, with
    ``towers``, the rows within ``cut_radius`` of a tower are skipped with ``conductor_clearance``'s own predicate;
    ``ops.treefall`` does the rest.  Every row is attributed to its nearest piece only.

    Returns dict: ``dist2`` (float64 [n]: the squared distance from the row's foot to the nearest accepted piece within
    ``(H + grow) + limit``, +inf if none), ``span`` (int32 [n]: that piece's id in the span table, -1 if none),
    ``height`` (float32 [n]: ``height_above_ground``'s), ``hazard`` (uint8 [n]: 0 clear, 1 within ``limit`` of a
    conductor after falling, 2 strikes), ``table``, a dict over the K pieces of the span table (TREEFALL_TABLE_KEYS):
    ``count`` and ``strikes`` (int64), ``min_distance`` (metres; +inf without a row), ``min_row`` (-1 without),
    ``max_height`` (float32, NaN without), ``max_row`` (-1 without) and ``chord_error`` (metres: the polyline lies above
    a hanging wire, so distances from below are over-estimated by at most that; NaN for a piece that was not accepted) -
    and ``trees``, a list of dicts (TREEFALL_TREE_KEYS): the hazard rows (class >= 1) are binned into xy cells of
    ``cell`` metres (``floor(x / cell)``, ``floor(y / cell)`` in the rows' frame) and per occupied cell the tallest
    hazard row is reported, ties to the lowest row index, ordered by (span, row): ``row``, ``x``, ``y``, ``ground``,
    ``height``, ``span``, ``distance``, ``margin = distance - (height + grow)`` and ``hazard``.  No accepted piece:
    every row +inf / -1 / 0, an empty ``trees``; nothing is raised.  Synchronises."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32:
        raise TypeError("points must be a float32 CUDA/HIP tensor (no CPU fallback in the product path)")
    points = points.reshape(-1, 3).contiguous()
    n, dev = int(points.shape[0]), points.device
    wire = spans["wire"]
    if wire.numel() != n:
        raise ValueError("spans must be conductor_spans' result for the same points")
    segments = ops.check_segments(segments)
    h_min, h_max, grow, limit = ops.check_treefall_rule(h_min, h_max, grow, limit)
    cell = float(cell)
    if not (np.isfinite(cell) and cell > 0.0):
        raise ValueError(f"cell must be finite and > 0, got {cell!r}")
    K = int(spans["nclusters"])
    idx = torch.nonzero(spans["accepted"]).reshape(-1)                        # accepted pieces, ascending
    curves = ops.span_curves(spans["table"], spans["frames"], spans["ext"])[idx].contiguous()
    segs, chord = ops.span_segments(curves, segments)
    s3 = ops._sub3(sub)
    framed = points if s3 is None else points - torch.tensor(list(s3), dtype=torch.float32, device=dev)
    near = _near_towers(framed, towers, cut_radius)
    skip = wire if near is None else (wire | near)
    res = ops.treefall(points, curves, segs, terrain["grid"], terrain["ground"], h_min, h_max, grow, limit, sub=sub,
                       skip=skip)
    span = res["span"]                                                        # (all -1 without an accepted piece)
    if idx.numel():
        span = torch.where(span >= 0, idx.to(torch.int32)[span.clamp(min=0).long()], torch.full_like(span, -1))
    nan64 = float("nan")
    table = dict(count=torch.zeros((K,), dtype=torch.int64, device=dev),
                 strikes=torch.zeros((K,), dtype=torch.int64, device=dev),
                 min_distance=torch.full((K,), float("inf"), dtype=torch.float64, device=dev),
                 min_row=torch.full((K,), -1, dtype=torch.int64, device=dev),
                 max_height=torch.full((K,), nan64, dtype=torch.float32, device=dev),
                 max_row=torch.full((K,), -1, dtype=torch.int64, device=dev),
                 chord_error=torch.full((K,), nan64, dtype=torch.float64, device=dev))
    for key in ("count", "strikes", "min_row", "max_height", "max_row"):
        table[key][idx] = res[key]
    table["min_distance"][idx], table["chord_error"][idx] = torch.sqrt(res["min_dist2"]), chord
    # the hazard rows are few: compacted on the device, the records made on the host
    rows = torch.nonzero(res["hazard"] >= ops.TREEFALL_NEAR).reshape(-1)
    at = framed[rows]
    under = ops.terrain_sample(at[:, :2].to(torch.float64), terrain["grid"], terrain["ground"])
    trees = _tree_records(rows.cpu().numpy(), at.cpu().numpy(), under.cpu().numpy(), res["height"][rows].cpu().numpy(),
                          span[rows].cpu().numpy(), res["dist2"][rows].cpu().numpy(), res["hazard"][rows].cpu().numpy(),
                          cell, grow)
    return dict(dist2=res["dist2"], span=span, height=res["height"], hazard=res["hazard"], table=table, trees=trees)


def _tree_records(rows, xyz, under, height, span, dist2, hazard, cell, grow):
    """danger_trees' records from the compacted hazard rows (numpy, ascending row index; ``under``: the ground under
    each): per occupied xy cell the tallest row, ties to the lowest row index; ordered by (span, row)."""
    if not len(rows):
        return []
    fx = np.floor(xyz[:, 0].astype(np.float64) / cell).astype(np.int64)
    fy = np.floor(xyz[:, 1].astype(np.float64) / cell).astype(np.int64)
    # by (cell, tallest first, lowest row first): the first of every cell's run is its record
    order = np.lexsort((rows, -height.astype(np.float64), fy, fx))
    first = np.ones(len(order), dtype=bool)
    first[1:] = (fx[order][1:] != fx[order][:-1]) | (fy[order][1:] != fy[order][:-1])
    pick = order[first]
    pick = pick[np.lexsort((rows[pick], span[pick]))]
    distance = np.sqrt(dist2[pick])
    h = height[pick].astype(np.float64)
    ground = under[pick]
    margin = distance - (h + float(grow))
    return [dict(row=int(rows[p]), x=float(xyz[p, 0]), y=float(xyz[p, 1]), ground=float(ground[j]), height=float(h[j]),
                 span=int(span[p]), distance=float(distance[j]), margin=float(margin[j]), hazard=int(hazard[p]))
            for j, p in enumerate(pick)]


CANOPY_TREE_KEYS = ops.CANOPY_TABLE_KEYS + ("x", "y", "z", "ground", "crown_area")
BY_TREE_KEYS = ("tree", "row", "x", "y", "ground", "height", "rows", "strikes", "hazard", "min_row", "distance", "margin",
                "span")


def canopy_cells(cell, crown_radius):
    """the crown radius in cells for ``crown_radius`` metres, ``ceil(crown_radius / cell)`` as ``terrain_cells`` converts
    its gap, at least 1; ValueError beyond the library's limit"""
    import math
    cell, crown_radius = float(cell), float(crown_radius)
    if not (math.isfinite(cell) and cell > 0.0):
        raise ValueError(f"cell must be finite and > 0, got {cell!r}")
    if not (math.isfinite(crown_radius) and crown_radius >= 0.0):
        raise ValueError(f"crown_radius must be finite and >= 0, got {crown_radius!r}")
    Rc = max(1, math.ceil(crown_radius / cell))
    if Rc > ops.CANOPY_MAX_CROWN:
        raise ValueError(f"crown_radius {crown_radius:g} m at cell {cell:g} m is {Rc} cells; the limit is "
                         f"{ops.CANOPY_MAX_CROWN} cells ({ops.CANOPY_MAX_CROWN * cell:g} m)")
    return int(Rc)


def tree_segments(points, terrain, sub=None, skip=None, cell=0.5, h_min=2.0, h_max=45.0, smooth=1, r0=1.0, r1=0.05,
                  top_min=5.0, crown_frac=0.5, crown_radius=8.0):
    """The vegetation of ``points`` (float32 [n,3] on the device) as trees: a canopy grid of ``cell``
    metres over the extent of ``terrain`` (``terrain_model``'s dict, in the same frame; with ``sub`` the rows are
    ``fl32(points - sub)``) holds the tallest return between ``h_min`` and ``h_max`` above the ground per cell
    (``ops.canopy_top``); smoothed over ``smooth`` cells, a cell of at least ``top_min`` that no cell within
    ``r0 + r1 * height`` metres beats is a tree top, every cell climbs to its top and belongs to its crown if it stands at
    least ``crown_frac`` of the top's height within ``crown_radius`` metres of it (``ops.canopy_trees``), and every row
    gets the tree of its cell (``ops.canopy_rows``).  ``skip`` (uint8 or bool [n]): rows that are no vegetation - the
    conductors, the rows near towers.

    Returns dict: ``grid`` and ``canopy_grid``, ``top``, ``count``, ``smooth`` and ``tree`` over the canopy cells,
    ``row_tree`` (int32 [n], -1 for a row of no tree), ``height`` (float32 [n], ``height_above_ground``'s), ``ntrees``
    and ``trees``, a dict of tensors over the T trees (CANOPY_TREE_KEYS): ``top_cell``, ``cells``, ``rows``,
    ``max_height`` and ``max_row`` of the tree table, ``x``, ``y``, ``z`` of row ``max_row`` in the rows' frame
    (float64), the ``ground`` under it (``ops.terrain_sample``) and ``crown_area = cells * cell^2``; ``points``, ``sub``,
    ``ground`` and the rule are kept for ``danger_trees_by_tree``.  ValueError: a crown radius beyond 256 cells, a canopy grid beyond
    2^24 cells, more than 2^20 trees.  Synchronises."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32:
        raise TypeError("points must be a float32 CUDA/HIP tensor (no CPU fallback in the product path)")
    points = points.reshape(-1, 3).contiguous()
    dev = points.device
    Rc = canopy_cells(cell, crown_radius)
    grid, ground = terrain["grid"], terrain["ground"]
    cg = ops.canopy_grid(grid, cell)
    t = ops.canopy_top(points, grid, ground, cg, h_min, h_max, sub=sub, skip=skip, want_height=True)
    seg = ops.canopy_trees(t["top"], t["top_row"], t["count"], cg, smooth, r0, r1, top_min, crown_frac, Rc,
                           want_smooth=True)
    row_tree = ops.canopy_rows(points, grid, ground, cg, h_min, h_max, seg["tree"], sub=sub, skip=skip)
    s3 = ops._sub3(sub)
    at = points[seg["max_row"].long()]
    if s3 is not None:
        at = at - torch.tensor(list(s3), dtype=torch.float32, device=dev)
    at = at.to(torch.float64)
    trees = {key: seg[key] for key in ops.CANOPY_TABLE_KEYS}
    trees.update(x=at[:, 0], y=at[:, 1], z=at[:, 2], ground=ops.terrain_sample(at[:, :2].contiguous(), grid, ground),
                 crown_area=seg["cells"].to(torch.float64) * (float(cell) * float(cell)))
    return dict(grid=grid, ground=ground, canopy_grid=cg, top=t["top"], count=t["count"], smooth=seg["smooth"], tree=seg["tree"],
                row_tree=row_tree, height=t["height"], ntrees=seg["ntrees"], trees=trees, points=points, sub=sub,
                rule=dict(cell=float(cell), h_min=float(h_min), h_max=float(h_max), crown_cells=Rc))


def danger_trees_by_tree(danger, segments, grow=0.0, cell=2.0):
    """``danger_trees``' hazard rows per tree: ``danger`` is its result and ``segments`` ``tree_segments``' result for the
    same points (and the same ``sub``).  One record (a dict, BY_TREE_KEYS) per tree that owns a hazard row: ``tree``,
    the position of its tallest return (``row``, ``x``, ``y``, the ``ground`` under it and ``height``), the number of
    its hazard ``rows`` and ``strikes``, the worst class ``hazard``, and of the hazard row with the smallest
    ``margin = distance - (height + grow)`` - ties to the lowest row - ``min_row``, ``distance``, ``margin`` and ``span``.
    Hazard rows of no tree are reported as records of their own with ``tree = -1``, binned into xy cells of ``cell``
    metres exactly as ``danger_trees`` bins its ``trees`` (``rows`` and ``strikes`` counting the bin's rows): no hazard
    row is lost.  Ordered by (span, tree, row).  The hazard rows are compacted on the device, the records made on the
    host; ``danger`` itself is not changed.  Synchronises."""
    row_tree, points = segments["row_tree"], segments["points"]
    if danger["hazard"].numel() != row_tree.numel():
        raise ValueError("danger and segments must be results for the same points")
    rows = torch.nonzero(danger["hazard"] >= ops.TREEFALL_NEAR).reshape(-1)
    at = points[rows]
    s3 = ops._sub3(segments["sub"])
    if s3 is not None:
        at = at - torch.tensor(list(s3), dtype=torch.float32, device=points.device)
    under = ops.terrain_sample(at[:, :2].to(torch.float64), segments["grid"], segments["ground"])
    trees = {key: v.cpu().numpy() for key, v in segments["trees"].items()}
    host = lambda v: v[rows].cpu().numpy()
    return _by_tree_records(rows.cpu().numpy(), at.cpu().numpy(), under.cpu().numpy(), host(danger["height"]),
                            host(danger["span"]), host(danger["dist2"]), host(danger["hazard"]), host(row_tree), trees,
                            float(cell), float(grow))


def _by_tree_records(rows, xyz, under, height, span, dist2, hazard, row_tree, trees, cell, grow):
    """danger_trees_by_tree's records from the compacted hazard rows (numpy, ascending row index; ``under``: the ground
    under each; ``trees``: tree_segments' table as numpy)"""
    out = []
    if not len(rows):
        return out
    distance = np.sqrt(dist2)
    margin = distance - (height.astype(np.float64) + float(grow))
    for t in np.unique(row_tree[row_tree >= 0]):
        mine = np.flatnonzero(row_tree == t)
        p = mine[np.lexsort((rows[mine], margin[mine]))[0]]                  # the smallest margin, ties to the lowest row
        out.append(dict(tree=int(t), row=int(trees["max_row"][t]), x=float(trees["x"][t]), y=float(trees["y"][t]),
                        ground=float(trees["ground"][t]), height=float(trees["max_height"][t]), rows=int(len(mine)),
                        strikes=int((hazard[mine] == ops.TREEFALL_STRIKE).sum()), hazard=int(hazard[mine].max()),
                        min_row=int(rows[p]), distance=float(distance[p]), margin=float(margin[p]), span=int(span[p])))
    free = np.flatnonzero(row_tree < 0)
    if len(free):
        fx = np.floor(xyz[free, 0].astype(np.float64) / cell).astype(np.int64)
        fy = np.floor(xyz[free, 1].astype(np.float64) / cell).astype(np.int64)
        for rec in _tree_records(rows[free], xyz[free], under[free], height[free], span[free], dist2[free], hazard[free],
                                 cell, grow):
            j = int(np.flatnonzero(rows[free] == rec["row"])[0])
            same = (fx == fx[j]) & (fy == fy[j])
            out.append(dict(rec, tree=-1, rows=int(same.sum()),
                            strikes=int((hazard[free][same] == ops.TREEFALL_STRIKE).sum()),
                            hazard=int(hazard[free][same].max()), min_row=rec["row"]))
    out.sort(key=lambda r: (r["span"], r["tree"], r["row"]))
    return [{key: r[key] for key in BY_TREE_KEYS} for r in out]


TOWER_PROFILE_TABLE_KEYS = ("ground", "ground_from", "top", "tower_height", "nominal_height", "n_levels", "z_low",
                            "z_high", "width", "rows", "lowest_wire")
TOWER_PROFILE_MAX_LEVELS = 8


def tower_profile(clusters, which=None, terrain=None, spans=None, dz=0.5, height=64.0, min_rows=3, arm_window=3.0,
                  arm_excess=4.0, reach=12.0):
    """Where the towers have their cross-arms and how high they stand.  ``clusters``: ``cluster_points``'
    dict (``ground["points"]``, ``perm``, ``offsets``, ``stats``, ``nclusters``); ``which``: the cluster ids to profile,
    ascending (None: all of them; more than 4096 is a ValueError).  Every cluster gets a horizontal frame over the whole
    grouping (``ops.cluster_moments``, ``ops.span_frames``: the centre, and the principal horizontal direction, which
    for a tower with arms is the arm axis); the rows of the chosen ones are binned into ``B = ceil(height / dz)`` slices
    of ``dz`` metres from ``z0`` upwards (``ops.cluster_slices``; ``B > 256`` is a ValueError) and the cross-arm levels
    are read off the slice table (``ops.tower_levels`` with ``min_rows``, ``arm_window``, ``arm_excess``).

    ``terrain`` (``terrain_model``'s dict, in the frame of the points): ``z0`` and the ground are the model's value under
    the tower's axis (``ops.terrain_sample``) and ``ground_from`` is "terrain"; where the model has none there, or
    without ``terrain``, both are the cluster's lowest z (``stats``) and ``ground_from`` is "cluster" - a stage-B cluster
    has lost its feet, so heights are then measured from where the cluster begins.  ``spans`` (``conductor_spans``' dict,
    same frame): ``lowest_wire`` is the smallest height above the ground, over the two ends of the accepted pieces that
    lie within ``reach`` metres horizontally of the tower's axis, of the piece's sag curve there; NaN without such an
    end or without ``spans``.

    Returns dict: ``which`` (int64 [T], device), ``frames5`` (float64 [T,5] = cx, cy, z0, ux, uy), ``count`` (int32
    [T,B]), ``ext`` (float64 [T,B,4]), ``outside`` (int64 [T,2]) and ``table``, keyed like ``TOWER_PROFILE_TABLE_KEYS``:
    ``ground``, ``top``, ``tower_height``, ``nominal_height`` (the lower edge of the lowest level above the ground),
    ``lowest_wire`` float64 [T]; ``n_levels`` int64 [T]; ``z_low``, ``z_high``, ``width``, ``rows`` float64 [T, 8],
    NaN-padded; ``ground_from`` a list of T strings.  No cluster selected: empty tables, nothing is raised.
    Synchronises."""
    import math
    dz, height, reach = float(dz), float(height), float(reach)
    if not (math.isfinite(dz) and dz > 0.0 and math.isfinite(height) and height > 0.0):
        raise ValueError(f"dz and height must be finite and > 0, got {dz!r}, {height!r}")
    if not (math.isfinite(reach) and reach >= 0.0):
        raise ValueError(f"reach must be finite and >= 0, got {reach!r}")
    B = int(math.ceil(height / dz))
    if B > ops.SLICES_MAX:
        raise ValueError(f"height {height:g} m at dz {dz:g} m is {B} slices; the limit is {ops.SLICES_MAX} slices "
                         f"({ops.SLICES_MAX * dz:g} m)")
    points = clusters["ground"]["points"]
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32:
        raise TypeError("the clustered points must be a float32 CUDA/HIP tensor (no CPU fallback in the product path)")
    points = points.reshape(-1, 3).contiguous()
    dev = points.device
    K = int(clusters["nclusters"]) if "perm" in clusters else 0
    ids = np.arange(K, dtype=np.int64) if which is None else np.asarray(
        which.cpu() if isinstance(which, torch.Tensor) else which, dtype=np.int64).reshape(-1)
    if len(ids) > ops.SLICES_MAX_TABLES:
        raise ValueError(f"tower_profile takes at most {ops.SLICES_MAX_TABLES} clusters per call, got {len(ids)}")
    if len(ids) and (ids[0] < 0 or ids[-1] >= K or (np.diff(ids) <= 0).any()):
        raise ValueError("which must hold cluster ids in 0..nclusters-1, ascending")
    T, L = len(ids), TOWER_PROFILE_MAX_LEVELS
    which_t = torch.as_tensor(ids, device=dev)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    if T == 0:
        table = dict(ground=nan(0), ground_from=[], top=nan(0), tower_height=nan(0), nominal_height=nan(0),
                     n_levels=torch.zeros((0,), dtype=torch.int64, device=dev), z_low=nan(0, L), z_high=nan(0, L),
                     width=nan(0, L), rows=nan(0, L), lowest_wire=nan(0))
        return dict(which=which_t, frames5=nan(0, 5), count=torch.zeros((0, B), dtype=torch.int32, device=dev),
                    ext=nan(0, B, 4), outside=torch.zeros((0, 2), dtype=torch.int64, device=dev), table=table)
    perm, offsets = clusters["perm"], clusters["offsets"]
    count, origin, moments = ops.cluster_moments(points, perm, offsets, K)
    frames = ops.span_frames(count, origin, moments)
    lowest = clusters["stats"][:K, 2].to(torch.float64)
    if terrain is not None:
        under = ops.terrain_sample(frames[:, 0:2].contiguous(), terrain["grid"], terrain["ground"])
        modelled = ~torch.isnan(under)
        z0 = torch.where(modelled, under, lowest)
    else:
        modelled = torch.zeros((K,), dtype=torch.bool, device=dev)
        z0 = lowest
    frames5 = torch.stack([frames[:, 0], frames[:, 1], z0, frames[:, 3], frames[:, 4]], dim=1).contiguous()
    slot = torch.full((K,), -1, dtype=torch.int32, device=dev)
    slot[which_t] = torch.arange(T, dtype=torch.int32, device=dev)
    res = ops.cluster_slices(points, perm, offsets, K, frames5, slot, T, dz, B)
    ground = z0[which_t].contiguous()
    table = ops.tower_levels(res["count"], res["ext"], ground, dz, ground=ground, min_rows=min_rows,
                             arm_window=arm_window, arm_excess=arm_excess, max_levels=L)
    table["ground"] = ground
    table["ground_from"] = ["terrain" if m else "cluster" for m in modelled[which_t].cpu().tolist()]
    table["lowest_wire"] = _lowest_wire(spans, frames5[which_t], ground, reach) if spans is not None else nan(T)
    return dict(which=which_t, frames5=frames5[which_t].contiguous(), count=res["count"], ext=res["ext"],
                outside=res["outside"], table={key: table[key] for key in TOWER_PROFILE_TABLE_KEYS})


def _lowest_wire(spans, frames5, ground, reach):
    """float64 [T]: per tower axis the smallest height above ``ground`` of an accepted piece's sag curve at one of its
    two ends (``m0``, ``m1`` of ``ops.span_curves``: ``cz + a + m(b + c·m)``) within ``reach`` metres horizontally; NaN
    without such an end.  Torch arithmetic on pieces x towers records."""
    idx = torch.nonzero(spans["accepted"]).reshape(-1)
    curves = ops.span_curves(spans["table"], spans["frames"], spans["ext"])[idx]
    cx, cy, cz, ux, uy, a, b, c = (curves[:, i:i + 1] for i in range(8))
    m = curves[:, 8:10]                                                       # [P,2]: the two ends
    X, Y, W = cx + (m * ux), cy + (m * uy), cz + (a + m * (b + c * m))
    dx = X[:, :, None] - frames5[None, None, :, 0]                            # [P,2,T]
    dy = Y[:, :, None] - frames5[None, None, :, 1]
    near = ((dx * dx) + (dy * dy)) <= reach * reach
    inf = torch.full((), float("inf"), dtype=torch.float64, device=ground.device)
    held = torch.where(near & ~torch.isnan(W)[:, :, None], W[:, :, None].expand_as(dx), inf)
    low = held.reshape(-1, ground.numel()).amin(dim=0) if idx.numel() else inf.expand(ground.numel())
    return torch.where(torch.isinf(low), torch.full_like(ground, float("nan")), low - ground)


def _kept_rows(gf, dropped):
    """the copy of the stage-B result ``gf`` without the rows of the bool mask ``dropped``, as the opt-in drops return
    it: points, index (if present), count and aabb of the rows left, in file order, plus dropped and n_dropped"""
    points = gf["points"]
    n = int(points.shape[0])
    keep = ~dropped
    kept = points[keep]                                        # masked select: file order
    m = int(kept.shape[0])
    out = dict(gf)
    out.update(points=kept, count=m, dropped=dropped, n_dropped=n - m,
               index=None if gf.get("index") is None else gf["index"][keep])
    if m:
        out["aabb"] = torch.cat([kept.min(0).values, kept.max(0).values]).cpu().numpy()
    return out


def drop_sparse_rows(gf, k=8, radius=2.0, std_ratio=2.0):
    """Opt-in removal of stray returns between stage B and stage C, the twin of ``drop_linear_rows``: drops the kept
    rows that are isolated or sparse.  ``gf`` is a stage-B result.  One global ``ops.DbscanFit(points, eps=radius,
    min_samples=1, chunk_size=0)``, ``fit.knn`` on its own rows (the row itself is counted among its neighbours), and
    ``m = ops.knn_mean_distance``: the mean distance to the ``k`` nearest rows, ``+inf`` where fewer than ``k`` rows lie
    within ``radius``.  Over the rows with ``count >= k``: ``mu = mean(m)``, ``sd`` the sample standard deviation (n - 1)
    and ``thr = mu + std_ratio * sd``.  A row is dropped iff ``count < k`` (isolated) or ``m > thr`` (sparse); with fewer
    than two rows of ``count >= k`` only the isolated rows are dropped and ``thr`` is ``+inf``.

    Returns the copy of ``gf`` that ``drop_linear_rows`` returns (``points``, ``index``, ``count``, ``aabb``,
    ``dropped``, ``n_dropped``) plus ``threshold`` (a float).  Stage B kept no row, or the fit left no grid to ask:
    raises with the cause - nothing is dropped silently.  Synchronises."""
    k = ops.check_knn_k(k)
    ops.check_shape_radius(radius, radius)
    if std_ratio != std_ratio:
        raise ValueError("std_ratio must be a number, got NaN")
    points = gf["points"]
    n = int(points.shape[0])
    if n == 0:
        raise ValueError("drop_sparse_rows: stage B kept no rows, so there is no neighbourhood to look at")
    fit = ops.DbscanFit(points, eps=float(radius), min_samples=1, chunk_size=0)
    try:
        _, d2, count = fit.knn(points, k, chunk="own", want_count=True)
    except RuntimeError as e:
        raise RuntimeError(f"drop_sparse_rows: the fit of {n} rows at eps = {float(radius)} left no grid to ask "
                           f"(compressed coordinates or rows that are not finite), so no row was examined: {e}") from e
    m = ops.knn_mean_distance(d2, count, k)
    del fit
    full = count >= k
    dense = m[full]
    threshold = float("inf")
    nd = int(dense.shape[0])
    if nd >= 2:                                                # two passes, sums of non-negative terms
        mu = dense.sum() / nd
        sd = torch.sqrt(((dense - mu) ** 2).sum() / (nd - 1))
        threshold = float(mu + float(std_ratio) * sd)
    out = _kept_rows(gf, ~full | (m > threshold))
    out["threshold"] = threshold
    return out


def _drop_then_dbscan(gf, drop_linear, eps, min_points, chunk_size, segment, drop_sparse=None):
    """stage C and D0 on a stage-B result the unfused way, the opt-in drops in between: sparse rows first"""
    sparse = None
    if drop_sparse is not None:
        if gf["count"]:
            gf = drop_sparse_rows(gf, **drop_sparse)
            sparse = dict(n_dropped=gf["n_dropped"], dropped=gf["dropped"], threshold=gf["threshold"])
        else:
            sparse = dict(n_dropped=0, dropped=torch.zeros((0,), dtype=torch.bool, device=gf["points"].device),
                          threshold=float("inf"))
    info = None
    if drop_linear is not None:
        if gf["count"]:
            gf = drop_linear_rows(gf, **drop_linear)
            info = dict(n_dropped=gf["n_dropped"], dropped=gf["dropped"])
        else:
            info = dict(n_dropped=0, dropped=torch.zeros((0,), dtype=torch.bool, device=gf["points"].device))
    points = gf["points"]
    if gf["count"]:
        labels, _, k = ops.dbscan(points, eps, min_points, chunk_size, aabb=gf["aabb"])
    else:
        labels, k = torch.empty((0,), dtype=torch.int32, device=points.device), 0
    out = dict(ground=gf, labels=labels, nclusters=k)
    if sparse is not None:
        out["drop_sparse"] = sparse
    if info is not None:
        out["drop_linear"] = info
    if segment:
        perm, offsets, stats = ops.segment_by_label(labels, points, k)
        out.update(perm=perm, offsets=offsets, stats=stats)
    return out


def _cluster_points(raw, eps, min_points, chunk_size, pct, offset, fallback_offset, min_keep, want_index, segment,
                    ground, plane, drop_linear=None, drop_sparse=None):
    if ground in ("plane", "plane_tiles"):
        kw = dict(offset=offset, fallback_offset=fallback_offset, min_keep=min_keep, want_index=want_index)
        kw.update(plane or {})
        gf = (ops.ground_filter_plane if ground == "plane" else ops.ground_filter_plane_tiles)(raw, **kw)
        return _drop_then_dbscan(gf, drop_linear, eps, min_points, chunk_size, segment, drop_sparse)
    if ground != "percentile":
        raise ValueError(f"ground must be 'percentile', 'plane' or 'plane_tiles', got {ground!r}")
    if drop_linear is not None or drop_sparse is not None:
        gf = ops.ground_filter(raw, pct, offset, fallback_offset, min_keep, want_index=want_index)
        return _drop_then_dbscan(gf, drop_linear, eps, min_points, chunk_size, segment, drop_sparse)
    gf, labels, k, perm, offsets, stats = ops.tower_clusters(
        raw, eps, min_points, chunk_size, pct, offset, fallback_offset, min_keep,
        want_index=want_index, segment=segment)
    out = dict(ground=gf, labels=labels, nclusters=k)
    if segment:
        out.update(perm=perm, offsets=offsets, stats=stats)
    return out


FRAMES = ("reference", "las")
_PLANE_GROUNDS = ("plane", "plane_tiles")


def check_frame(frame, ground="percentile"):
    """ValueError for an unknown frame, and for the "las" frame with a plane ground rule: those rules compute their own
    float32 centroid in the reference's frame.  Touches no device."""
    if frame not in FRAMES:
        raise ValueError(f"frame must be 'reference' or 'las', got {frame!r}")
    if frame == "las" and ground in _PLANE_GROUNDS:
        raise ValueError(f"frame 'las' is defined for the percentile ground rule only, not for ground={ground!r}: "
                         "the plane rules centre the cloud themselves, in the reference's float32 frame")
    return frame


def cluster_points_las(XYZ, scales, offsets, eps=8.0, min_points=80, chunk_size=REF_CHUNK, pct=25.0, offset=3.0,
                       fallback_offset=1.0, min_keep=1000, want_index=False, segment=True, merge_threshold=None,
                       ground="percentile", drop_linear=None, drop_sparse=None):
    """Stages B + C + D0 in the LAS-integer frame (opt-in) on the int32 [N,3] LAS records of a device tensor:
    ops.ground_filter_las, then ops.dbscan with its box, ops.segment_by_label and the optional merge.  Returns the dict
    of ``cluster_points`` - ``tower_table`` and ``tower_table_async`` take it unchanged; ground["centroid"] is the
    float64 world centroid.  ``ground`` exists to say no: a plane rule raises ValueError before any device call.
    ``drop_linear``, ``drop_sparse``: as for ``cluster_points`` (None = off)."""
    check_frame("las", ground)
    if ground != "percentile":
        raise ValueError(f"ground must be 'percentile' in the 'las' frame, got {ground!r}")
    gf = ops.ground_filter_las(XYZ, scales, offsets, pct, offset, fallback_offset, min_keep, want_index=want_index)
    out = _drop_then_dbscan(gf, drop_linear, eps, min_points, chunk_size, segment or merge_threshold is not None,
                            drop_sparse)
    return out if merge_threshold is None else _merged(out, merge_threshold, segment)


def label_full_cloud(sampled_raw, full_raw, eps=8.0, min_points=80, chunk_size=0, pct=25.0, offset=3.0,
                     fallback_offset=1.0, min_keep=1000, segment=False):
    """Which rows of ``full_raw`` belong to which tower of ``sampled_raw``: stage B (``ops.ground_filter``) on the
    sampled cloud, one ``ops.DbscanFit`` on the rows it kept, then ``fit.assign(full_raw, sub=centroid)`` - every row
    of the full cloud takes the smallest cluster id among the fit's core points within eps, else -1.

    Both clouds are float32 [N,3] device tensors in the same (uncentred) frame.  ``full_raw`` may be the cloud before
    it was thinned, a second flight line, or ``sampled_raw`` itself.  Rows BELOW the height threshold may be labelled,
    and that is intended: a tower's feet lie within eps of its core points although the filter removed them.

    ``chunk_size`` > 0 fits the kept rows in file-order chunks as the reference does (one fit per chunk); a row of
    the full cloud can then be held against a chunk only through its own place in that file order, so this needs
    ``full_raw is sampled_raw`` (a kept row meets the chunk it was fitted in, a dropped row the chunk of the next kept
    row) and raises ValueError otherwise.

    Returns dict: ground (ops.ground_filter result), labels int32 [N_f] of the kept rows, nclusters, cloud_labels int32
    [N_full]; with ``segment`` also perm / offsets of ``ops.segment_by_label`` over cloud_labels."""
    if int(chunk_size) > 0 and full_raw is not sampled_raw:
        raise ValueError("chunk_size > 0 fits the kept rows chunk by chunk in file order; rows of another cloud have no "
                         "place in that order - pass full_raw is sampled_raw, or chunk_size=0 for one global fit")
    gf = ops.ground_filter(sampled_raw, pct, offset, fallback_offset, min_keep, want_index=True)
    fit = ops.DbscanFit(gf["points"], eps, min_points, int(chunk_size), aabb=gf["aabb"] if gf["count"] else None)
    chunk = None
    if fit.chunk_size:
        n = full_raw.reshape(-1, 3).shape[0]
        kept = torch.zeros((n,), dtype=torch.int64, device=full_raw.device)
        kept[gf["index"].long()] = 1
        before = torch.cumsum(kept, 0) - kept                  # kept rows in front of every row
        last = (fit.n + fit.chunk_size - 1) // fit.chunk_size - 1
        chunk = torch.clamp(before // fit.chunk_size, max=last).to(torch.int32)
    cloud_labels = fit.assign(full_raw, sub=gf["centroid"], chunk=chunk)
    out = dict(ground=gf, labels=fit.labels, nclusters=fit.nclusters, cloud_labels=cloud_labels)
    if segment:
        perm, offsets, _ = ops.segment_by_label(cloud_labels, full_raw, fit.nclusters)
        out.update(perm=perm, offsets=offsets)
    return out


def kdistance_knee(y):
    """The value of an ascending array furthest below the chord from its first to its last element: with
    ``x_i = i/(m-1)`` and ``yn_i = (y_i - y_0)/(y_{m-1} - y_0)`` it is ``y[argmax(x - yn)]`` (first index on ties).
    Fewer than 3 values: None; a constant array: that constant.  A hint where the k-distance plot bends, not a rule:
    look at the quantiles and at ``core_share`` before setting eps by it."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    m = len(y)
    if m < 3:
        return None
    if y[-1] == y[0]:
        return float(y[0])
    x = np.arange(m, dtype=np.float64) / (m - 1)
    yn = (y - y[0]) / (y[-1] - y[0])
    return float(y[int(np.argmax(x - yn))])


def kdistance_profile(points, k=80, eps_max=16.0, chunk_size=REF_CHUNK, sample=200_000, seed=0,
                      quantiles=(5, 25, 50, 75, 90, 95, 99), aabb=None):
    """The k-distance plot of stage C's input, the instrument DBSCAN's authors give for choosing eps: for a seeded
    sample of the rows, the exact distance to the k-th nearest row of the same file-order chunk (the row itself is
    the first), sorted.  ``points``: the kept, centred float32 [N,3] rows of stage B on the device
    (``cluster_points(...)["ground"]["points"]``).

    One ``ops.DbscanFit(points, eps_max, k, chunk_size)``, ``min(sample, n)`` distinct rows drawn with
    ``numpy.random.default_rng(seed)`` and sorted ascending, ``fit.kdist`` on them with their chunks; the square root
    and the sort run on the host.  Distances beyond ``eps_max`` are not measured (``truncated`` counts them): raise
    ``eps_max`` if too many are.  A row is core at ``(eps, k)`` exactly when its k-distance is <= eps, so the plot
    read at eps gives the share of core rows (``core_share``).

    Returns dict: k, eps_max, n, rows int64 [m]; kdist float64 metres, ascending, finite answers only; truncated
    (answers that were +inf); count int32 [m] rows within eps_max of every sampled row; quantiles {q: np.percentile
    of kdist} or None where there is no finite answer; knee (``kdistance_knee(kdist)``)."""
    points = points.reshape(-1, 3)
    n = points.shape[0]
    fit = ops.DbscanFit(points, float(eps_max), int(k), int(chunk_size), aabb=aabb)
    rows = np.sort(np.random.default_rng(seed).choice(n, min(int(sample), n), replace=False)).astype(np.int64)
    idx = torch.from_numpy(rows).to(points.device)
    chunk = (idx // fit.chunk_size).to(torch.int32) if fit.chunk_size else None
    d2, count = fit.kdist(points[idx], int(k), chunk=chunk, want_count=True)
    d2 = d2.cpu().numpy()
    finite = np.isfinite(d2)
    kdist = np.sort(np.sqrt(d2[finite]))
    return dict(k=int(k), eps_max=float(eps_max), n=int(n), rows=rows, kdist=kdist,
                truncated=int(len(d2) - finite.sum()), count=count.cpu().numpy(),
                quantiles={q: float(np.percentile(kdist, q)) for q in quantiles} if len(kdist) else None,
                knee=kdistance_knee(kdist))


def core_share(profile, eps):
    """Share of a profile's sampled rows that are core at ``(eps, profile["k"])``: the rows whose k-distance is <= eps.
    ``eps`` beyond the profile's ``eps_max`` was not measured: ValueError."""
    if float(eps) > profile["eps_max"]:
        raise ValueError(f"eps {eps} lies beyond the profile's eps_max {profile['eps_max']}: profile again at a larger "
                         f"eps_max")
    if len(profile["rows"]) == 0:
        return 0.0
    return float(np.searchsorted(profile["kdist"], float(eps), side="right")) / len(profile["rows"])


def north_angle_deg(rotation):
    """utils/tower_extraction.py:165-177."""
    hx, hy = float(rotation[0, 0]), float(rotation[1, 0])
    nrm = float(np.linalg.norm(np.array([hx, hy, 0.0])))
    if nrm > 1e-6:
        hx, hy = hx / nrm, hy / nrm
    else:
        hx, hy = 1.0, 0.0
    a = np.degrees(np.arctan2(hy, hx))
    if a < 0:
        a += 360
    return (90 - a) % 360


def _accept(boxes, centroid, aspect_ratio_threshold, min_height, max_width, min_width, duplicate_threshold):
    """The reference's loop body (utils/tower_extraction.py:131-215) over the boxes of all clusters in label order:
    what it logs and what it accepts, as a list of ("log", text) / ("tower", dict) events."""
    events, centers = [], []
    for label, (box, err) in enumerate(boxes):
        try:
            if err is not None:
                raise err
            extents, transform = box
            height = extents[2]
            width = max(extents[0], extents[1])
            aspect_ratio = height / width
            if not (height > min_height and min_width < width < max_width
                    and aspect_ratio > aspect_ratio_threshold):
                continue
            obb_center = transform[:3, 3] + centroid
            dup = None
            for c in centers:
                d = np.linalg.norm(obb_center - c)
                if d < duplicate_threshold:
                    dup = d
                    break
            if dup is not None:
                events.append(("log", f"⚠️ 跳过重复杆塔{label} (中心距: {dup:.1f}m)"))
                continue
            rot = transform[:3, :3]
            tower = dict(label=label, center=obb_center, rotation=rot, extent=extents,
                         height=height, width=width, aspect_ratio=aspect_ratio,
                         north_angle=north_angle_deg(rot), points=None)
            centers.append(obb_center)
            events.append(("tower", tower))
        except Exception as e:                                  # utils/tower_extraction.py:213-215
            events.append(("log", f"⚠️ 簇{label} 处理失败: {str(e)}"))
            continue
    return events


def upright_boxes_from_records(records):
    """The boxes ``_accept`` takes, from the PchUprightBox records of ``ops.upright_boxes(..., to_host=True)`` in label
    order, in pure numpy float64: ((extents, transform), None) per cluster, or (None, ValueError) for a status-1 record
    (no row, or a coordinate that is not finite).  extents = [rect_long, rect_short, height] as a float64 array (a zero
    width then gives inf and a warning in the accept rule, not an exception); the rotation's columns are the long
    rectangle axis, the short one and (0, 0, 1); transform = [R | centre] (include/pch_hip.h)."""
    cs = ops.upright_angle_table_host()
    boxes = []
    for rec in records:
        if int(rec["status"]) != 0:
            boxes.append((None, ValueError("no upright box: the cluster has no rows or a coordinate that is not finite")))
            continue
        c, s = cs[int(rec["j"])]
        umin, umax, vmin, vmax = (np.float64(rec[f]) for f in ("umin", "umax", "vmin", "vmax"))
        zmin, zmax = np.float64(rec["zmin"]), np.float64(rec["zmax"])
        du, dv, dz = umax - umin, vmax - vmin, zmax - zmin
        mu, mv, mz = 0.5 * (umin + umax), 0.5 * (vmin + vmax), 0.5 * (zmin + zmax)
        transform = np.eye(4)
        transform[:3, 3] = (mu * c - mv * s, mu * s + mv * c, mz)
        if dv > du:
            transform[:3, 0], transform[:3, 1] = (-s, c, 0.0), (-c, -s, 0.0)
            extents = np.array([dv, du, dz], dtype=np.float64)
        else:
            transform[:3, 0], transform[:3, 1] = (c, s, 0.0), (-s, c, 0.0)
            extents = np.array([du, dv, dz], dtype=np.float64)
        boxes.append(((extents, transform), None))
    return boxes


class TowerTableJob:
    """Stage D1-D3 of one tile in flight (``tower_table_async``): the clustered points are on their way to (or in)
    a shared host buffer, the boxes are being computed by the worker pool.  ``result()`` waits and returns the tower
    list; ``timings`` (after result()) holds the wall-clock split in ms."""

    def __init__(self):
        import threading
        self._done = threading.Event()
        self._towers = None
        self._error = None
        self.timings = {}

    def result(self, timeout=None):
        if not self._done.wait(timeout):
            raise TimeoutError("tower table still in flight")
        if self._error is not None:
            raise self._error
        return self._towers


_SIDE = {}            # device index -> the stream the hand-off of the clustered points runs on


def _exact_start(clusters, extent_order, timings):
    """Device side of the exact mode: the clustered rows gathered into cluster order and copied into a shared,
    registered host buffer on a side stream; returns (buffer, offsets, event after the copy, host view)."""
    import time
    t0 = time.perf_counter()
    gf = clusters["ground"]
    k = int(clusters["nclusters"])
    perm, pts = clusters["perm"], gf["points"]
    offsets = clusters["offsets"].cpu().numpy()
    if offsets[0] < 0:
        from . import _lib
        _lib.check_count(int(offsets[0]), "segment_by_label")
    m = int(offsets[k])
    dev = pts.device
    pl = _obb.pool()
    buf = pl.buffer(12 * max(m, 1), pin=True)
    side = _SIDE.get(dev.index)
    if side is None:
        side = _SIDE[dev.index] = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        # one gather + one D2H copy for all clustered points (noise rows stay on the device)
        gathered = pts.index_select(0, perm[:m].long())
        host = buf.tensor(torch.float32, 3 * m).view(m, 3)
        host.copy_(gathered, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(side)
    timings["enqueue_gather_d2h_ms"] = 1e3 * (time.perf_counter() - t0)
    # the side stream reads `pts` / `perm` and writes `gathered`: whoever waits for `ev` keeps them alive until then
    # (the caching allocator knows them as the main stream's blocks)
    return pl, buf, offsets, ev, [gathered, pts, perm]


def _exact_finish(pl, buf, offsets, ev, k, centroid, extent_order, params, timings):
    import time
    t0 = time.perf_counter()
    ev.synchronize()
    t1 = time.perf_counter()
    job = _obb.boxes_job(buf, offsets[:k + 1], np.float32, extent_order)
    boxes = _obb.job_results(job)
    t2 = time.perf_counter()
    events = _accept(boxes, centroid, *params)
    m = int(offsets[k])
    host = buf.array[:12 * m].view(np.float32).reshape(m, 3)
    for kind, t in events:
        if kind == "tower":                                     # a copy: the buffer goes back to the pool
            t["points"] = host[offsets[t["label"]]:offsets[t["label"] + 1]].copy()
    del host
    pl.release(buf)
    t3 = time.perf_counter()
    nw = max(pl.size(), 1)
    timings.update({"wait_gather_d2h_ms": 1e3 * (t1 - t0), "boxes_wall_ms": 1e3 * (t2 - t1),
                    "boxes_worker_wall_ms": 1e3 * job.worker_s, "boxes_worker_cpu_ms": 1e3 * job.worker_cpu_s,
                    "workers": nw,
                    "worker_utilisation": round(job.worker_s / max((t2 - t1) * nw, 1e-9), 3),
                    "accept_and_copy_ms": 1e3 * (t3 - t2), "clustered_points": m,
                    "bytes_to_host": 12 * m, "buffer_pinned": bool(buf.pinned)})
    return events


def tower_table_async(clusters, aspect_ratio_threshold=0.8, min_height=15.0, max_width=50.0, min_width=8,
                      duplicate_threshold=30.0, extent_order="unsorted"):
    """``tower_table`` (exact mode) without waiting for it: the hand-off of the clustered points is queued on a side
    stream, a host thread waits for it, lets the worker pool box the clusters and applies the reference's accept /
    de-dup rule.  The caller goes on - typically with ``cluster_points`` of the next tile - and collects the towers
    with ``.result()``.  ``log`` / ``on_accept`` are not taken: replay them from the returned list."""
    import threading
    job = TowerTableJob()
    k = int(clusters["nclusters"])
    if k == 0:
        job._towers = []
        job._done.set()
        return job
    centroid = clusters["ground"]["centroid"]
    params = (aspect_ratio_threshold, min_height, max_width, min_width, duplicate_threshold)
    pl, buf, offsets, ev, keep = _exact_start(clusters, extent_order, job.timings)

    def run():
        try:
            events = _exact_finish(pl, buf, offsets, ev, k, centroid, extent_order, params, job.timings)
            job._towers = [t for kind, t in events if kind == "tower"]
            job.events = events
        except BaseException as e:                              # handed to result()
            job._error = e
        finally:
            del keep[:]
            job._done.set()

    threading.Thread(target=run, name="pch-tower-table", daemon=True).start()
    return job


def tower_table(clusters, aspect_ratio_threshold=0.8, min_height=15.0, max_width=50.0, min_width=8,
                duplicate_threshold=30.0, extent_order="unsorted", log=None, on_accept=None, obb_mode="exact",
                timings=None, prepare=None):
    """Stage D1-D3 for every cluster, in ascending label order (the iteration order of the
    reference's ``set(all_labels) - {-1}``).  Returns list of dicts with the reference's keys
    (center, rotation, extent, height, width, north_angle, points) plus 'label' and
    'aspect_ratio'.  ``log`` receives the duplicate / failure messages, ``on_accept(tower)`` is
    called for every accepted tower in order (the drop-in writes the tower LAS there).
    ``obb_mode``: "exact" (qhull on every full cluster, in the worker pool of obb.py: the clustered points go
    to a shared, registered host buffer in one copy and the workers map it) or "fast" (obb.boxes_fast: device
    pre-filter + native candidate search; only the accepted towers' points are copied to the host) or "upright"
    (opt-in: ops.upright_boxes - z as one axis, the smallest footprint rectangle among 4096 table angles as the other
    two, the rule of include/pch_hip.h, all on the device; ``extent_order`` does not apply: the extents are always
    [rect_long, rect_short, height]; only the accepted towers' points are copied to the host, no worker is started).
    ``timings``: optional dict that receives the wall-clock split of the exact mode in ms.
    ``prepare(accepted)``: called once with all accepted towers (points filled in) before the replay starts - the
    drop-in starts writing the per-tower files there."""
    if obb_mode not in ("exact", "fast", "upright"):
        raise ValueError("obb_mode must be 'exact', 'fast' or 'upright'")
    gf = clusters["ground"]
    k = int(clusters["nclusters"])
    towers = []
    if k == 0:
        return towers
    centroid = gf["centroid"]                                   # float32[3]
    params = (aspect_ratio_threshold, min_height, max_width, min_width, duplicate_threshold)
    tm = timings if timings is not None else {}
    if obb_mode == "exact":
        pl, buf, offsets, ev, keep = _exact_start(clusters, extent_order, tm)
        events = _exact_finish(pl, buf, offsets, ev, k, centroid, extent_order, params, tm)
        del keep
    else:
        offsets = clusters["offsets"].cpu().numpy()
        perm, pts = clusters["perm"], gf["points"]
        if obb_mode == "fast":
            boxes = _obb.boxes_fast(pts, perm, clusters["offsets"], k, extent_order)
        else:
            if offsets[0] < 0:
                from . import _lib
                _lib.check_count(int(offsets[0]), "segment_by_label")
            # two launches per level on the device, then K records of 72 bytes to the host: no hull, no worker pool
            boxes = upright_boxes_from_records(ops.upright_boxes(pts, perm, clusters["offsets"], k, to_host=True))
        events = _accept(boxes, centroid, *params)
        accepted = [ev[1] for ev in events if ev[0] == "tower"]
        if accepted:
            spans = [(int(offsets[t["label"]]), int(offsets[t["label"] + 1])) for t in accepted]
            pos = torch.cat([torch.arange(a, b, device=perm.device) for a, b in spans])
            host_pts = pts.index_select(0, perm.index_select(0, pos).long()).cpu().numpy()
            at = 0
            for t, (a, b) in zip(accepted, spans):
                t["points"] = host_pts[at:at + (b - a)]
                at += b - a
    if prepare:
        prepare([item for kind, item in events if kind == "tower"])
    for kind, item in events:
        if kind == "log":
            if log:
                log(item)
            continue
        towers.append(item)
        if on_accept:
            on_accept(item)
    return towers
