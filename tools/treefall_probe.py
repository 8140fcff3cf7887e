"""What the tree-fall query costs (ops.treefall: pch_treefall_f32).  The cloud is clearance_probe.py's: bench.py's
corridor in its local frame as float32 followed by --veg-rows vegetation rows under and beside the line, in file order,
the skip mask the rows within 9 m of a tower axis.  The ground is pipeline.terrain_model's grid of that cloud.  bench.py's
corridor has no wires, so pipeline.cluster_points and pipeline.conductor_spans would leave no accepted piece to measure
to: the conductors are strung between the corridor's towers as curves, as clearance_probe.py strings them.

Before any time is reported every output is compared bit for bit with the torch statement of the rule on a sample of
rows (random ones and every kind of hazard row) - the bilinear ground and a dense rows x spans x segments broadcast in
float64, the same operations in the same order, so the bits must agree -, ``height`` with ops.terrain_height on all
rows, and the table with the rows' own answers.  Then one JSON line: the call's time (device events around the call,
one warm-up, then --runs runs: all of them and their median), the kernels' own times from the library's event profile,
the compulsory bytes (12 B in and 17 B out per row; the skip byte on top) and the rate at the median, ``stats`` (the
rows that took part, the uncovered rows, the (row, span) segment loops run and the (tile, span) pairs walked), and for
comparison the time of the composed route that exists without this call - ops.terrain_height, a torch build of float32
feet, ops.clearance at radius = Rmax - whose results are not the rule's: it is a time only.  No time is a pass / fail
condition.
python tools/treefall_probe.py [--points N] [--veg-rows M] [--segments 32] [--runs 7]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clearance_probe import cloud, line_curves  # noqa: E402
from eps_probe import event_ms  # noqa: E402
from pointcloudhookup_amd import ops, pipeline  # noqa: E402
from terrain_probe import same_bits  # noqa: E402

KERNELS = ["clearance_bounds", "treefall_sweep", "treefall_finish"]
COMPOSED = ["terrain_height", "clearance_bounds", "clearance_sweep", "clearance_finish"]


def ground_statement(xyz, grid, ground):
    """float64 [m]: g(X, Y) of include/pch_hip.h's terrain rule in torch float64 (NaN for a row that is not finite)"""
    G = ground.double()
    X, Y = xyz[:, 0].double(), xyz[:, 1].double()

    def axis(pos, o, nc):
        u = ((pos - o) / grid["cell"]) - 0.5
        i0 = torch.floor(u).clamp(0, max(nc - 2, 0)).long()
        i1 = torch.clamp(i0 + 1, max=nc - 1)
        a = u - i0.double()
        a = torch.where(a < 0, torch.zeros_like(a), a)
        return i0, i1, torch.where(a > 1, torch.ones_like(a), a)

    qx = torch.floor((X - grid["x0"]) / grid["cell"])
    qy = torch.floor((Y - grid["y0"]) / grid["cell"])
    inside = (qx >= 0) & (qx < grid["nx"]) & (qy >= 0) & (qy < grid["ny"]) & torch.isfinite(xyz).all(dim=1)
    fx, fy = torch.where(inside, qx, 0).long(), torch.where(inside, qy, 0).long()
    i0, i1, a = axis(torch.where(inside, X, grid["x0"]), grid["x0"], grid["nx"])
    j0, j1, b = axis(torch.where(inside, Y, grid["y0"]), grid["y0"], grid["ny"])
    g00, g10, g01, g11 = G[j0, i0], G[j0, i1], G[j1, i0], G[j1, i1]
    bil = (((g00 * (1.0 - a)) + (g10 * a)) * (1.0 - b)) + (((g01 * (1.0 - a)) + (g11 * a)) * b)
    four = ~(torch.isnan(g00) | torch.isnan(g10) | torch.isnan(g01) | torch.isnan(g11))
    return torch.where(inside, torch.where(four, bil, G[fy, fx]), torch.full_like(bil, float("nan")))


def torch_statement(xyz, skip, grid, ground, curves, segs, rule, chunk):
    """(dist2 float64, span int32, height float32, hazard uint8) over the rows of ``xyz`` by the rule of
    include/pch_hip.h as a dense broadcast, ``chunk`` rows at a time: every row against every span and segment, nothing
    culled"""
    h_min, h_max, grow, limit = rule
    K = curves.shape[0]
    cx, cy, cz, ux, uy = (curves[:, i][None, :] for i in range(5))
    mj, zj, dm, dz, inv = (segs[:, :, i][None] for i in range(5))
    takes = torch.isfinite(curves[:, :5]).all(1) & torch.isfinite(segs).all(2).all(1)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=xyz.device)
    ks = torch.arange(K, device=xyz.device)[None, :]
    outs = [[], [], [], []]
    for c0 in range(0, xyz.shape[0], chunk):
        p = xyz[c0:c0 + chunk]
        X, Y, Z = p[:, 0].double(), p[:, 1].double(), p[:, 2].double()
        g = ground_statement(p, grid, ground)
        H = Z - g
        part = (skip[c0:c0 + chunk] == 0) & torch.isfinite(p).all(dim=1) & ~torch.isnan(g) & (h_min <= H) & (H <= h_max)
        reach = H + grow
        s2 = reach * reach
        R = reach + limit
        R2 = R * R
        dx, dy, w = X[:, None] - cx, Y[:, None] - cy, g[:, None] - cz
        m = (dx * ux) + (dy * uy)
        t = (dy * ux) - (dx * uy)
        rm, rw = m[:, :, None] - mj, w[:, :, None] - zj
        q = ((rm * dm) + (rw * dz)) * inv
        q = torch.where(q < 0, torch.zeros_like(q), q)
        q = torch.where(q > 1, torch.ones_like(q), q)
        em, ew = rm - (q * dm), rw - (q * dz)
        d = (em * em) + (ew * ew)
        gmin = torch.where(torch.isnan(d), inf, d).min(dim=2).values               # `if d < gmin` never takes a NaN
        d2 = gmin + (t * t)
        cand = torch.where(takes[None, :] & part[:, None] & (d2 <= R2[:, None]), d2, inf)
        best = cand.min(dim=1).values
        who = torch.where(cand == best[:, None], ks, K).min(dim=1).values          # the lowest index on a tie
        found = ~torch.isinf(best)
        hazard = torch.where(found, torch.where(best <= s2, 2, 1), 0).to(torch.uint8)
        height = torch.where(torch.isnan(g), torch.full_like(H, float("nan")), H).float()
        for acc, v in zip(outs, (best, torch.where(found, who, -1).to(torch.int32), height, hazard)):
            acc.append(v)
    return tuple(torch.cat(v) for v in outs)


def check(xyz, skip, grid, ground, curves, segs, rule, out, chunk):
    n, dev = xyz.shape[0], xyz.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    pick = [torch.randint(0, n, (4096,), generator=gen, device=dev)]
    kinds = {}
    for name, cls in (("near", ops.TREEFALL_NEAR), ("strike", ops.TREEFALL_STRIKE)):
        rows = torch.nonzero(out["hazard"] == cls).reshape(-1)
        kinds[name] = int(rows.numel())
        if rows.numel():
            pick.append(rows[torch.randint(0, rows.numel(), (4096,), generator=gen, device=dev)])
    rows = torch.cat(pick)
    d2, who, height, hazard = torch_statement(xyz[rows], skip[rows], grid, ground, curves, segs, rule, chunk)
    assert torch.equal(who, out["span"][rows]), "span differs from the torch statement"
    assert torch.equal(d2.view(torch.int64), out["dist2"][rows].view(torch.int64)), "dist2 differs from the torch statement"
    assert torch.equal(hazard, out["hazard"][rows]), "the class differs from the torch statement"
    assert same_bits(height, out["height"][rows]), "height differs from the torch statement"
    assert same_bits(out["height"], ops.terrain_height(xyz, grid, ground)), "height differs from ops.terrain_height"
    K = curves.shape[0]
    hit = out["span"] >= 0
    ids = out["span"][hit].long()
    assert torch.equal(torch.bincount(ids, minlength=K), out["count"]), "the table's counts"
    strikes = torch.bincount(out["span"][out["hazard"] == ops.TREEFALL_STRIKE].long(), minlength=K)
    assert torch.equal(strikes, out["strikes"]), "the table's strikes"
    mind = torch.full((K,), float("inf"), dtype=torch.float64, device=dev)
    mind.scatter_reduce_(0, ids, out["dist2"][hit], reduce="amin")
    assert torch.equal(mind, out["min_dist2"]), "the table's minima"
    top = torch.full((K,), float("-inf"), dtype=torch.float32, device=dev)
    top.scatter_reduce_(0, ids, out["height"][hit], reduce="amax")
    has = out["count"] > 0
    assert torch.equal(top[has], out["max_height"][has]) and bool(torch.isnan(out["max_height"][~has]).all()), "maxima"
    assert torch.equal(out["min_row"] >= 0, has) and torch.equal(out["dist2"][out["min_row"][has]], mind[has]), "min_row"
    assert torch.equal(out["max_row"] >= 0, has) and torch.equal(out["height"][out["max_row"][has]], top[has]), "max_row"
    return int(rows.numel()), kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--veg-rows", type=int, default=2_000_000)
    ap.add_argument("--segments", type=int, default=32)
    ap.add_argument("--h-min", type=float, default=2.0)
    ap.add_argument("--h-max", type=float, default=45.0)
    ap.add_argument("--grow", type=float, default=0.0)
    ap.add_argument("--limit", type=float, default=3.0)
    ap.add_argument("--cell", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--torch-chunk", type=int, default=16384)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    curves = line_curves(args.points, dev)
    segs, chord = ops.span_segments(curves, args.segments)
    xyz, skip = cloud(args.points, args.veg_rows, dev)
    n, K = int(xyz.shape[0]), int(curves.shape[0])
    terrain = pipeline.terrain_model(xyz, cell=args.cell)
    grid, ground = terrain["grid"], terrain["ground"]
    rule = (args.h_min, args.h_max, args.grow, args.limit)
    rmax = (args.h_max + args.grow) + args.limit
    call = lambda: ops.treefall(xyz, curves, segs, grid, ground, *rule, skip=skip, want_stats=True)  # noqa: E731
    out = call()
    checked, kinds = check(xyz, skip, grid, ground, curves, segs, rule, out, args.torch_chunk)

    def composed():
        height, under = ops.terrain_height(xyz, grid, ground, want_ground=True)
        feet = torch.stack([xyz[:, 0], xyz[:, 1], under], dim=1)
        return height, ops.clearance(feet, curves, segs, rmax, rmax, skip=skip)

    def timed(fn):
        ms = []
        for r in range(args.runs + 1):                                           # the first run warms up
            t, res = event_ms(fn)
            if r:
                ms.append(t)
            del res
        return statistics.median(ms), [round(t, 4) for t in ms]

    median, runs = timed(call)
    c_median, c_runs = timed(composed)
    kern = {}
    for names, fn in ((KERNELS, call), (COMPOSED, composed)):
        ops.set_profiling(True, only=names)
        acc = {name: [] for name in names}
        for _ in range(4):
            fn()
            torch.cuda.synchronize()
            for name, t, _l in ops.get_profile():
                if name in acc:
                    acc[name].append(round(t, 4))
        ops.set_profiling(False)
        kern["treefall" if fn is call else "composed"] = {name: v[1:] for name, v in acc.items()}
    stats = out["stats"].tolist()
    tiles = -(-n // ops.TREEFALL_TILE)
    nbytes = 29 * n
    print(json.dumps({
        "rows": n, "corridor_points": args.points, "vegetation_rows": args.veg_rows, "spans": K,
        "segments": args.segments, "grid": [grid["nx"], grid["ny"]], "cell_m": args.cell, "h_min": args.h_min,
        "h_max": args.h_max, "grow": args.grow, "limit": args.limit, "rmax": rmax,
        "chord_error_max_m": float(chord.max().item()), "rows_checked_against_torch": checked,
        "rows_skipped": int(skip.sum().item()), "rows_near": kinds["near"], "rows_strike": kinds["strike"],
        "treefall_ms": {"median": median, "runs": runs}, "kernel_ms": kern["treefall"],
        "compulsory_bytes": nbytes, "bytes_per_row": {"in": 12, "out": 17}, "gb_per_s": nbytes / (median * 1e-3) / 1e9,
        "rows_took_part": stats[0], "rows_uncovered": stats[1], "segment_loops_run": stats[2],
        "row_span_pairs": n * K, "tile_span_pairs_walked": stats[3], "tile_span_pairs": tiles * K,
        "composed_route_ms": {"median": c_median, "runs": c_runs, "kernel_ms": kern["composed"],
                              "note": "terrain_height + torch feet + clearance at radius Rmax: a time only"}}),
        flush=True)


if __name__ == "__main__":
    main()
