"""What the wind swing query costs (ops.swing_clearance: pch_swing_clearance_f32).  The cloud, the curves, the skip
mask, the radius and S are tools/clearance_probe.py's: the corridor with three conductors strung between its towers and
--veg-rows vegetation rows under and beside the line.  The largest swing angle is --angle degrees (45).

Before any time is reported the answer is checked on 12 288 rows (random ones, ones within the radius and ones the wire
meets at a swing of more than 0.1 in sine) against the torch statement of the rule - a dense rows x spans x segments
broadcast in float64, the same operations in the same order, so the bits of dist2, span and sin must agree - and the
table against the rows' own answers.  Then one JSON line: the call's time (device events around the call, one warm-up,
then --runs runs: all of them and their median), the kernels' own times from the library's event profile, the (row,
span) segment loops actually run and the (tile, span) pairs walked, and as the yardstick for what the 3-D loop and the
division per segment cost ops.clearance at the same radius on the same cloud, measured the same way.  No time is a pass
/ fail condition.
python tools/swing_probe.py [--points N] [--veg-rows M] [--segments 32] [--angle 45] [--runs 7]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clearance_probe import cloud, line_curves  # noqa: E402
from eps_probe import event_ms  # noqa: E402
from pointcloudhookup_amd import ops  # noqa: E402

KERNELS = ["swing_bounds", "swing_sweep", "clearance_finish"]
REST_KERNELS = ["clearance_bounds", "clearance_sweep", "clearance_finish"]


def torch_statement(xyz, skip, heads, segs, radius, chunk):
    """(dist2 float64 [n], span int32 [n], sin float64 [n]) by the rule of include/pch_hip.h as a dense broadcast,
    ``chunk`` rows at a time: every row against every span and segment, nothing culled"""
    K = heads.shape[0]
    r2 = float(radius) * float(radius)
    cx, cy, cz, ux, uy, mA, mB, zA, kap, sT, cT = (heads[:, i][None, :] for i in range(11))
    mj, zj, fj, dm, dz, df = (segs[:, :, i][None] for i in range(6))
    turn = ((sT * sT) + (cT * cT)) - 1.0
    part = (torch.isfinite(heads).all(1) & torch.isfinite(segs).all(2).all(1) & (mB > mA)[0] & (sT >= 0)[0] & (sT <= 1)[0]
            & (cT > 0)[0] & (cT <= 1)[0] & (turn.abs() <= 1e-6)[0])
    inf = torch.full((), float("inf"), dtype=torch.float64, device=xyz.device)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=xyz.device)
    ks = torch.arange(K, device=xyz.device)[None, :]
    best_all, who_all, sin_all = [], [], []
    for c0 in range(0, xyz.shape[0], chunk):
        p = xyz[c0:c0 + chunk].double()
        dx, dy, w = p[:, 0:1] - cx, p[:, 1:2] - cy, p[:, 2:3] - cz
        m = (dx * ux) + (dy * uy)
        t = (dy * ux) - (dx * uy)
        mh = torch.where(m < mA, mA.expand_as(m), m)
        mh = torch.where(mh > mB, mB.expand_as(m), mh)
        bb = (zA + ((mh - mA) * kap)) - w
        inside = (bb > 0) & ((t.abs() * cT) <= (bb * sT))
        rho = torch.sqrt((t * t) + (bb * bb))
        s = torch.where(inside, t / rho, torch.where(t >= 0, sT.expand_as(t), (-sT).expand_as(t)))
        e = 1.0 - torch.where(inside, bb / rho, cT.expand_as(t))
        s3, e3 = s[:, :, None], e[:, :, None]
        ey, ez = df * s3, dz + (df * e3)
        rm, rt, rw = m[:, :, None] - mj, t[:, :, None] - (fj * s3), w[:, :, None] - (zj + (fj * e3))
        len2 = ((dm * dm) + (ey * ey)) + (ez * ez)
        pos = len2 > 0
        q = torch.where(pos, (((rm * dm) + (rt * ey)) + (rw * ez)) / torch.where(pos, len2, torch.ones_like(len2)),
                        torch.zeros_like(len2))
        q = torch.where(q < 0, torch.zeros_like(q), q)
        q = torch.where(q > 1, torch.ones_like(q), q)
        vm, vt, vw = rm - (q * dm), rt - (q * ey), rw - (q * ez)
        d = ((vm * vm) + (vt * vt)) + (vw * vw)
        g = torch.where(torch.isnan(d), inf, d).min(dim=2).values                  # `if d < g` never takes a NaN
        alive = (skip[c0:c0 + chunk] == 0)[:, None]
        cand = torch.where(part[None, :] & alive & (g <= r2), g, inf)
        best = cand.min(dim=1).values
        who = torch.where(cand == best[:, None], ks, K).min(dim=1).values          # the lowest index on a tie
        none = torch.isinf(best)
        sin = s.gather(1, who.clamp(max=max(K - 1, 0))[:, None])[:, 0]
        best_all.append(best)
        who_all.append(torch.where(none, -1, who).to(torch.int32))
        sin_all.append(torch.where(none, nan, sin))
    return torch.cat(best_all), torch.cat(who_all), torch.cat(sin_all)


def check(xyz, skip, heads, segs, out, radius, limit, chunk):
    n, dev = xyz.shape[0], xyz.device
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    near = torch.nonzero(out["span"] >= 0).reshape(-1)
    swung = torch.nonzero(out["sin"].abs() > 0.1).reshape(-1)
    pick = [torch.randint(0, n, (4096,), generator=g, device=dev)]
    for some in (near, swung):
        if some.numel():
            pick.append(some[torch.randint(0, some.numel(), (4096,), generator=g, device=dev)])
    rows = torch.cat(pick)
    d2, who, sin = torch_statement(xyz[rows], skip[rows], heads, segs, radius, chunk)
    assert torch.equal(who, out["span"][rows]), "span differs from the torch statement"
    assert torch.equal(d2.view(torch.int64), out["dist2"][rows].view(torch.int64)), "dist2 differs from the torch statement"
    assert torch.equal(torch.isnan(sin), torch.isnan(out["sin"][rows])), "sin: NaN where there is no span"
    hit = who >= 0
    assert torch.equal(sin[hit].view(torch.int64), out["sin"][rows][hit].view(torch.int64)), "sin differs"
    K = heads.shape[0]
    hit = out["span"] >= 0
    count = torch.bincount(out["span"][hit].long(), minlength=K)
    viol = torch.bincount(out["span"][hit & (out["dist2"] <= limit * limit)].long(), minlength=K)
    assert torch.equal(count, out["count"]) and torch.equal(viol, out["violations"]), "the table's counts"
    mind = torch.full((K,), float("inf"), dtype=torch.float64, device=dev)
    mind.scatter_reduce_(0, out["span"][hit].long(), out["dist2"][hit], reduce="amin")
    assert torch.equal(mind, out["min_dist2"]), "the table's minima"
    has = out["min_row"] >= 0
    assert torch.equal(has, count > 0) and torch.equal(out["dist2"][out["min_row"][has]], mind[has]), "min_row"
    return int(rows.numel()), int(near.numel()), int(swung.numel())


def timed(call, runs, kernels):
    """(ms of ``runs`` runs behind one warm-up, {kernel: ms of three profiled runs behind one}, the last result)"""
    ms, out = [], None
    for r in range(runs + 1):
        t, out = event_ms(call)
        if r:
            ms.append(t)
    ops.set_profiling(True, only=kernels)
    kern = {name: [] for name in kernels}
    for _ in range(4):
        call()
        torch.cuda.synchronize()
        for name, t, _l in ops.get_profile():
            if name in kern:
                kern[name].append(round(t, 4))
    ops.set_profiling(False)
    return ms, {name: v[1:] for name, v in kern.items()}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--veg-rows", type=int, default=2_000_000)
    ap.add_argument("--segments", type=int, default=32)
    ap.add_argument("--radius", type=float, default=10.0)
    ap.add_argument("--limit", type=float, default=6.0)
    ap.add_argument("--angle", type=float, default=45.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--torch-chunk", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    curves = line_curves(args.points, dev)
    heads = ops.swing_heads(curves, args.angle)
    segs = ops.swing_segments(curves, args.segments)
    segs5, chord = ops.span_segments(curves, args.segments)
    xyz, skip = cloud(args.points, args.veg_rows, dev)
    n, K = int(xyz.shape[0]), int(curves.shape[0])
    call = lambda: ops.swing_clearance(xyz, heads, segs, args.radius, args.limit, skip=skip, want_stats=True)  # noqa: E731
    rest = lambda: ops.clearance(xyz, curves, segs5, args.radius, args.limit, skip=skip, want_stats=True)  # noqa: E731
    out = call()
    checked, within, swung = check(xyz, skip, heads, segs, out, args.radius, args.limit, args.torch_chunk)
    ms, kern, out = timed(call, args.runs, KERNELS)
    rest_ms, rest_kern, calm = timed(rest, args.runs, REST_KERNELS)
    loops, rest_loops = out["loops"].tolist(), calm["loops"].tolist()
    tiles = -(-n // ops.CLEARANCE_TILE)
    sag = float(segs[:, :, 2].max().item())
    print(json.dumps({
        "rows": n, "corridor_points": args.points, "vegetation_rows": args.veg_rows, "spans": K,
        "segments": args.segments, "radius": args.radius, "limit": args.limit, "angle_deg": args.angle,
        "sag_max_m": sag, "low_point_moves_m": sag * math.sin(math.radians(args.angle)),
        "chord_error_max_m": float(chord.max().item()),
        "rows_checked_against_torch": checked, "rows_within_radius": within, "rows_met_beside": swung,
        "rows_skipped": int(skip.sum().item()),
        "violations": int(out["violations"].sum().item()), "violations_at_rest": int(calm["violations"].sum().item()),
        "rows_within_radius_at_rest": int((calm["span"] >= 0).sum().item()),
        "min_distance_m": float(out["min_dist2"].min().sqrt().item()),
        "swing_ms": {"median": statistics.median(ms), "runs": [round(t, 4) for t in ms]},
        "kernel_ms": kern,
        "segment_loops_run": loops[0], "row_span_pairs": n * K, "tile_span_pairs_walked": loops[1],
        "tile_span_pairs": tiles * K,
        "clearance": {"ms": {"median": statistics.median(rest_ms), "runs": [round(t, 4) for t in rest_ms]},
                      "kernel_ms": rest_kern, "segment_loops_run": rest_loops[0],
                      "tile_span_pairs_walked": rest_loops[1]}}), flush=True)


if __name__ == "__main__":
    main()
