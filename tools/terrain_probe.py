"""What the terrain grid costs (ops.terrain_low, ops.terrain_ground, ops.terrain_height: pch_terrain_*).  The cloud is
bench.py's corridor in its local frame as float32, in file order (50 m strips, shuffled inside; nine rows in ten are
ground), with a skip mask that skips nothing, so that its byte per row is read.

Before any time is reported the whole ``low`` and ``count`` grids are compared bit for bit with the torch statement of
the rule (the cell of every row in float64, ``scatter_reduce`` with ``amin`` on the keys, ``bincount``) and 8192 rows of
``height`` with the torch statement of the bilinear rule - the same operations in the same order, so the bits must
agree.  Then one JSON line per cell size: each call's time (device events around the call, one warm-up, then --runs
runs: all of them and their median), the kernels' own times from the library's event profile, the bytes a call must
move (13 B per row for the lowest return, 16 B per row for the heights) and the rate at the median, ``out_stats`` (the
rows binned and the (tile, cell) flushes, against the one global atomic pair per row a kernel without the LDS table
would issue), and for scale the torch statement's time on the same rows.  No time is a pass / fail condition.
python tools/terrain_probe.py [--points N] [--cells 1,0.5] [--runs 7]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eps_probe import event_ms  # noqa: E402
from pointcloudhookup_amd import ops, pipeline, synth  # noqa: E402

KERNELS = ["terrain_low", "terrain_decode", "terrain_open", "terrain_accept", "terrain_fill", "terrain_height"]


def cells_statement(xyz, grid):
    """(part bool [n], cell int64 [n]) by the rule: float64 on the float32 rows, no subtraction, nothing skipped"""
    X, Y = xyz[:, 0].double(), xyz[:, 1].double()
    qx = torch.floor((X - grid["x0"]) / grid["cell"])
    qy = torch.floor((Y - grid["y0"]) / grid["cell"])
    part = (qx >= 0) & (qx < grid["nx"]) & (qy >= 0) & (qy < grid["ny"]) & torch.isfinite(xyz[:, 2])
    cell = torch.where(part, qy * grid["nx"] + qx, torch.zeros_like(qx)).long()
    return part, cell


def low_statement(xyz, grid):
    """(low float32 [ny,nx], count int32 [ny,nx]) with scatter_reduce(amin) on the order-preserving keys and bincount"""
    ncells = grid["nx"] * grid["ny"]
    part, cell = cells_statement(xyz, grid)
    bits = xyz[:, 2].contiguous().view(torch.int32).long() & 0xFFFFFFFF
    key = bits ^ torch.where((bits >> 31) != 0, 0xFFFFFFFF, 0x80000000)
    best = torch.full((ncells,), 0xFFFFFFFF, dtype=torch.int64, device=xyz.device)
    best.scatter_reduce_(0, cell[part], key[part], reduce="amin")
    count = torch.bincount(cell[part], minlength=ncells).to(torch.int32)
    back = best ^ torch.where((best >> 31) != 0, 0x80000000, 0xFFFFFFFF)
    low = torch.where(back >= 2 ** 31, back - 2 ** 32, back).to(torch.int32).view(torch.float32)
    low = torch.where(count > 0, low, torch.full_like(low, float("nan")))
    return low.reshape(grid["ny"], grid["nx"]), count.reshape(grid["ny"], grid["nx"])


def height_statement(xyz, grid, ground):
    """float32 [m]: the bilinear rule of include/pch_hip.h in torch float64, the same operations in the same order"""
    G = ground.double()
    X, Y, Z = xyz[:, 0].double(), xyz[:, 1].double(), xyz[:, 2].double()

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
    g = torch.where(inside, torch.where(four, bil, G[fy, fx]), torch.full_like(bil, float("nan")))
    return (Z - g).float()


def same_bits(a, b):
    """bit for bit, one NaN being as good as another"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32)))


def timed(fn, runs):
    ms = []
    for r in range(runs + 1):                                                    # the first run warms up
        t, out = event_ms(fn)
        if r:
            ms.append(t)
    return statistics.median(ms), [round(t, 4) for t in ms], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--cells", type=str, default="1,0.5")
    ap.add_argument("--window", type=float, default=12.0)
    ap.add_argument("--dh", type=float, default=0.5)
    ap.add_argument("--max-gap", type=float, default=16.0)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    xyz = synth.corridor_torch(args.points, device=dev, dtype=torch.float32)
    n = int(xyz.shape[0])
    skip = torch.zeros((n,), dtype=torch.uint8, device=dev)
    for cell in (float(c) for c in args.cells.split(",")):
        grid = ops.terrain_grid(xyz, cell)
        R, G = pipeline.terrain_cells(cell, args.window, args.max_gap)
        low_call = lambda: ops.terrain_low(xyz, grid, skip=skip, want_stats=True)  # noqa: E731
        out = low_call()
        want_low, want_count = low_statement(xyz, grid)
        assert torch.equal(out["count"], want_count), "count differs from the torch statement"
        assert same_bits(out["low"], want_low), "low differs from the torch statement"
        del want_low, want_count
        ground_call = lambda: ops.terrain_ground(out["low"], grid, R, args.dh, G)  # noqa: E731
        res = ground_call()
        height_call = lambda: ops.terrain_height(xyz, grid, res["ground"])  # noqa: E731
        height = height_call()
        g = torch.Generator(device=dev)
        g.manual_seed(11)
        rows = torch.randint(0, n, (8192,), generator=g, device=dev)
        assert same_bits(height[rows], height_statement(xyz[rows], grid, res["ground"])), "height differs"
        low_ms, low_runs, out = timed(low_call, args.runs)
        ground_ms, ground_runs, res = timed(ground_call, args.runs)
        height_ms, height_runs, height = timed(height_call, args.runs)
        ops.set_profiling(True, only=KERNELS)
        kern = {name: [] for name in KERNELS}
        for _ in range(4):
            for call in (low_call, ground_call, height_call):
                call()
            torch.cuda.synchronize()
            for name, t, _l in ops.get_profile():
                if name in kern:
                    kern[name].append(round(t, 4))
        ops.set_profiling(False)
        torch_ms = [event_ms(lambda: low_statement(xyz, grid))[0] for _ in range(2)]   # one warm-up, one run
        stats = out["stats"].tolist()
        state = res["state"]
        print(json.dumps({
            "rows": n, "cell_m": cell, "grid": [grid["nx"], grid["ny"]], "cells": grid["nx"] * grid["ny"],
            "window_cells": R, "max_gap_cells": G, "rows_of_height_checked": int(rows.numel()),
            "cells_ground": int((state & 1).ne(0).sum()), "cells_filled": int((state & 2).ne(0).sum()),
            "cells_without_ground": int((state & 3).eq(0).sum()),
            "low_ms": {"median": low_ms, "runs": low_runs}, "low_bytes": 13 * n,
            "low_gb_per_s": 13 * n / (low_ms * 1e-3) / 1e9,
            "ground_ms": {"median": ground_ms, "runs": ground_runs},
            "height_ms": {"median": height_ms, "runs": height_runs}, "height_bytes": 16 * n,
            "height_gb_per_s": 16 * n / (height_ms * 1e-3) / 1e9,
            "kernel_ms": {name: v[1:] for name, v in kern.items()},
            "rows_binned": stats[0], "tile_cell_flushes": stats[1], "global_atomic_pairs_without_the_table": n,
            "torch_statement_low_ms": round(torch_ms[1], 3)}), flush=True)
        del out, res, height


if __name__ == "__main__":
    main()
