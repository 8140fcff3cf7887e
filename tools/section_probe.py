"""What the span section query costs (ops.span_section: pch_span_section_f32).  The cloud, the curves and the skip mask
are tools/swing_probe.py's, i.e. tools/clearance_probe.py's: the corridor with three conductors strung between its
towers and --veg-rows vegetation rows under and beside the line.

Before any time is reported the answer is checked against the torch statement of the rule - a dense rows x spans
broadcast in float64 on 12 288 rows (random ones and ones that lie under a span), the same operations in the same order,
so the bits of v, span and station must agree - and the cells against a scatter of every row's pairs over the whole
cloud, span by span.  Then one JSON line: the call's time (device events around the call, one warm-up, then --runs
runs: all of them and their median), the kernels' own times from the library's event profile, the three stats - the (row,
span) pairs that took part, the (tile, span) pairs walked, the cell flushes -, the bytes per second over the 12 B/row
read and the 12 B/row written, and beside it ops.clearance with --segments segments on the same rows and curves, measured
the same way in the same run.  No time is a pass / fail condition.
python tools/section_probe.py [--points N] [--veg-rows M] [--stations 64] [--half-width 15] [--depth 80] [--limit 7]
                              [--segments 32] [--runs 7]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clearance_probe import cloud, line_curves  # noqa: E402
from swing_probe import timed  # noqa: E402
from pointcloudhookup_amd import ops  # noqa: E402

KERNELS = ["section_bounds", "section_sweep", "section_decode"]
REST_KERNELS = ["clearance_bounds", "clearance_sweep", "clearance_finish"]


def pairs(xyz, skip, curve, B, half, depth):
    """(part bool [n], v float64 [n], j int64 [n]) of the rows against one span by the rule of include/pch_hip.h"""
    cx, cy, cz, ux, uy, a, b, c, m0, m1 = (curve[i] for i in range(10))
    step = (m1 - m0) / float(B)
    p = xyz.double()
    dx, dy, w = p[:, 0] - cx, p[:, 1] - cy, p[:, 2] - cz
    m = (dx * ux) + (dy * uy)
    t = (dy * ux) - (dx * uy)
    zw = a + (m * (b + (c * m)))
    v = zw - w
    part = ((m >= m0) & (m <= m1) & (t >= -half) & (t <= half) & (v >= 0.0) & (v <= depth) & (skip == 0)
            & torch.isfinite(xyz).all(dim=1) & torch.isfinite(curve).all() & (m1 > m0))
    j = torch.floor(torch.where(part, m - m0, torch.zeros_like(m)) / step).clamp(max=B - 1).long()
    return part, v, j


def check(xyz, skip, curves, out, B, half, depth, limit):
    n, dev, K = xyz.shape[0], xyz.device, curves.shape[0]
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    under = torch.nonzero(out["span"] >= 0).reshape(-1)
    pick = [torch.randint(0, n, (4096,), generator=g, device=dev)]
    if under.numel():
        pick.append(under[torch.randint(0, under.numel(), (8192,), generator=g, device=dev)])
    rows = torch.cat(pick)
    best = torch.full((rows.numel(),), float("inf"), dtype=torch.float32, device=dev)
    who = torch.full((rows.numel(),), -1, dtype=torch.int32, device=dev)
    at = torch.full((rows.numel(),), -1, dtype=torch.int32, device=dev)
    for k in range(K):
        part, v, j = pairs(xyz[rows], skip[rows], curves[k], B, half, depth)
        vf = v.float().abs()
        take = part & (vf < best)
        best, who, at = torch.where(take, vf, best), torch.where(take, k, who), torch.where(take, j.int(), at)
    assert torch.equal(who, out["span"][rows]) and torch.equal(at, out["station"][rows]), "span / station differ"
    assert torch.equal(best.view(torch.int32), out["v"][rows].view(torch.int32)), "v differs from the torch statement"
    big = torch.iinfo(torch.int64).max
    for k in range(K):
        part, v, j = pairs(xyz, skip, curves[k], B, half, depth)
        hit = torch.nonzero(part).reshape(-1)
        vf = v[hit].float().abs()
        count = torch.bincount(j[hit], minlength=B)
        viol = torch.bincount(j[hit][v[hit] <= limit], minlength=B)
        assert torch.equal(count, out["count"][k]) and torch.equal(viol, out["violations"][k]), f"counts of span {k}"
        low = torch.full((B,), float("inf"), dtype=torch.float32, device=dev)
        low.scatter_reduce_(0, j[hit], vf, reduce="amin")
        assert torch.equal(low, out["min_v"][k]), f"minima of span {k}"
        first = torch.full((B,), big, dtype=torch.int64, device=dev)
        attains = vf == low[j[hit]]
        first.scatter_reduce_(0, j[hit][attains], hit[attains], reduce="amin")
        assert torch.equal(torch.where(first == big, -1, first), out["min_row"][k]), f"rows of span {k}"
    return int(rows.numel()), int(under.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--veg-rows", type=int, default=2_000_000)
    ap.add_argument("--stations", type=int, default=64)
    ap.add_argument("--half-width", type=float, default=15.0)
    ap.add_argument("--depth", type=float, default=80.0)
    ap.add_argument("--limit", type=float, default=7.0)
    ap.add_argument("--segments", type=int, default=32)
    ap.add_argument("--radius", type=float, default=10.0)
    ap.add_argument("--clearance-limit", type=float, default=6.0)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    curves = line_curves(args.points, dev)
    segs5, chord = ops.span_segments(curves, args.segments)
    xyz, skip = cloud(args.points, args.veg_rows, dev)
    n, K, B = int(xyz.shape[0]), int(curves.shape[0]), args.stations
    call = lambda: ops.span_section(xyz, curves, B, args.half_width, args.depth, args.limit, skip=skip,  # noqa: E731
                                    want_stats=True)
    rest = lambda: ops.clearance(xyz, curves, segs5, args.radius, args.clearance_limit, skip=skip,  # noqa: E731
                                 want_stats=True)
    out = call()
    checked, under = check(xyz, skip, curves, out, B, args.half_width, args.depth, args.limit)
    ms, kern, out = timed(call, args.runs, KERNELS)
    rest_ms, rest_kern, calm = timed(rest, args.runs, REST_KERNELS)
    stats, rest_loops = out["stats"].tolist(), calm["loops"].tolist()
    tiles = -(-n // ops.CLEARANCE_TILE)
    med = statistics.median(ms)
    print(json.dumps({
        "rows": n, "corridor_points": args.points, "vegetation_rows": args.veg_rows, "spans": K, "stations": B,
        "half_width": args.half_width, "depth": args.depth, "limit": args.limit,
        "rows_checked_against_torch": checked, "rows_under_a_span": under, "rows_skipped": int(skip.sum().item()),
        "cells_with_rows": int((out["count"] > 0).sum().item()), "cells": K * B,
        "largest_cell": int(out["count"].max().item()) if K else 0,
        "violations": int(out["violations"].sum().item()),
        "cells_in_violation": int((out["violations"] > 0).sum().item()),
        "min_vertical_m": float(out["min_v"].min().item()) if K else float("inf"),
        "chord_error_max_m": float(chord.max().item()) if K else 0.0,
        "section_ms": {"median": med, "runs": [round(t, 4) for t in ms]},
        "bytes_per_s": 24.0 * n / (med * 1e-3),
        "kernel_ms": kern,
        "row_span_pairs_taking_part": stats[0], "row_span_pairs": n * K, "tile_span_pairs_walked": stats[1],
        "tile_span_pairs": tiles * K, "cell_flushes": stats[2],
        "clearance": {"segments": args.segments, "radius": args.radius, "limit": args.clearance_limit,
                      "ms": {"median": statistics.median(rest_ms), "runs": [round(t, 4) for t in rest_ms]},
                      "kernel_ms": rest_kern, "segment_loops_run": rest_loops[0],
                      "tile_span_pairs_walked": rest_loops[1]}}), flush=True)


if __name__ == "__main__":
    main()
