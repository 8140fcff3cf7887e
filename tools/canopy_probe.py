"""What the canopy grid and the tree segmentation cost (ops.canopy_top, ops.canopy_trees, ops.canopy_rows).  The cloud is
treefall_probe.py's: bench.py's corridor in its local frame as float32 followed by --veg-rows vegetation rows under and
beside the line, in file order, the skip mask the rows within 9 m of a tower axis; the ground is
pipeline.terrain_model's grid of that cloud at --cell, the canopy grid lies over its extent at --canopy-cell (widened
by a quarter at a time should it exceed 2^24 cells; the cell used is reported).

Before any time is reported the whole ``top`` and ``count`` grids are compared bit for bit with a torch statement of
step 1 - the bilinear ground in float64, H = (float)(Z - g), a scatter_reduce ``amax`` of the keys (key(H) << 32) | ~row
and a bincount -, ``tree`` with the numpy statement of tests/canopy_cases.py on a window of 512 x 200 cells around the
cell with the most rows, and 8192 rows of ``row_tree`` with the statement.  Then one JSON line: per call the time
(device events around the call, one warm-up, then --runs runs: all of them and their median), the kernels' own times
from the library's event profile, ``stats`` (the rows that took part and the (tile, cell) flushes), the compulsory
bytes of the two row sweeps - 13 B per row in for step 1 (the row and its skip byte), 13 B in and 4 B out for step 9 -
with the rate at the median, and the torch statement's time beside them.  No time is a pass / fail condition.
python tools/canopy_probe.py [--points N] [--veg-rows M] [--runs 7]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import canopy_cases as cn  # noqa: E402
from clearance_probe import cloud  # noqa: E402
from eps_probe import event_ms  # noqa: E402
from pointcloudhookup_amd import ops, pipeline  # noqa: E402
from terrain_probe import same_bits  # noqa: E402
from treefall_probe import ground_statement  # noqa: E402

TOP_KERNELS = ["canopy_top", "canopy_decode"]
TREE_KERNELS = ["canopy_smooth", "canopy_parent", "canopy_root", "canopy_count", "canopy_scan", "canopy_number",
                "canopy_crown", "canopy_table"]
ROW_KERNELS = ["canopy_rows"]


def part_statement(xyz, skip, grid, ground, cg, h_min, h_max):
    """(part bool, cell int64, H float32) over the rows of ``xyz`` by the rule of include/pch_hip.h in torch"""
    X, Y, Z = xyz[:, 0].double(), xyz[:, 1].double(), xyz[:, 2].double()
    g = ground_statement(xyz, grid, ground)
    Hd = Z - g
    qx, qy = torch.floor((X - cg["x0"]) / cg["cell"]), torch.floor((Y - cg["y0"]) / cg["cell"])
    inside = (qx >= 0) & (qx < cg["nx"]) & (qy >= 0) & (qy < cg["ny"])
    part = (skip == 0) & torch.isfinite(xyz).all(dim=1) & inside & ~torch.isnan(g) & (h_min <= Hd) & (Hd <= h_max)
    cell = torch.where(part, qy * cg["nx"] + qx, torch.zeros_like(qx)).long()
    return part, cell, Hd.float()


def top_statement(xyz, skip, grid, ground, cg, h_min, h_max):
    """(top float32, top_row int32, count int32 over the cells): one amax of 64-bit keys and one bincount.  H >= -0.0 for
    a row that takes part, so key(H) - 0x7FFFFFFF fits 31 bits and the packed key orders as a signed integer"""
    ncells = cg["nx"] * cg["ny"]
    part, cell, H = part_statement(xyz, skip, grid, ground, cg, h_min, h_max)
    rows = torch.nonzero(part).reshape(-1)
    bits = H[rows].view(torch.int32).long() & 0xFFFFFFFF
    k32 = torch.where(bits >> 31 != 0, (~bits) & 0xFFFFFFFF, bits | 0x80000000) - 0x7FFFFFFF
    key = (k32 << 32) | ((~rows) & 0xFFFFFFFF)
    best = torch.full((ncells,), -1, dtype=torch.int64, device=xyz.device)
    best.scatter_reduce_(0, cell[rows], key, reduce="amax")
    count = torch.bincount(cell[rows], minlength=ncells).to(torch.int32)
    has = count > 0
    top_row = torch.where(has, (~best) & 0xFFFFFFFF, torch.full_like(best, -1))
    top = torch.where(has, H[top_row.clamp(min=0)], torch.full((ncells,), float("nan"), device=xyz.device))
    return top, top_row.to(torch.int32), count


def timed(fn, runs):
    ms = []
    for r in range(runs + 1):                                                    # the first run warms up
        t, out = event_ms(fn)
        if r:
            ms.append(t)
        del out
    return statistics.median(ms), [round(t, 4) for t in ms]


def kernel_ms(fn, names):
    ops.set_profiling(True, only=names)
    acc = {name: [] for name in names}
    for _ in range(4):
        fn()
        torch.cuda.synchronize()
        run = {}
        for name, t, _l in ops.get_profile():
            if name in acc:
                run[name] = run.get(name, 0.0) + t
        for name, t in run.items():
            acc[name].append(round(t, 4))
    ops.set_profiling(False)
    return {name: v[1:] for name, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--veg-rows", type=int, default=2_000_000)
    ap.add_argument("--cell", type=float, default=1.0)
    ap.add_argument("--canopy-cell", type=float, default=0.5)
    ap.add_argument("--h-min", type=float, default=2.0)
    ap.add_argument("--h-max", type=float, default=45.0)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    xyz, skip = cloud(args.points, args.veg_rows, dev)
    n = int(xyz.shape[0])
    terrain = pipeline.terrain_model(xyz, cell=args.cell)
    grid, ground = terrain["grid"], terrain["ground"]
    cell = args.canopy_cell
    while True:
        try:
            cg = ops.canopy_grid(grid, cell)
            break
        except ValueError:
            cell *= 1.25
    rule = dict(smooth=1, r0=1.0, r1=0.05, top_min=5.0, crown_frac=0.5, crown_cells=pipeline.canopy_cells(cell, 8.0))
    h = (args.h_min, args.h_max)
    top_call = lambda: ops.canopy_top(xyz, grid, ground, cg, *h, skip=skip)  # noqa: E731
    stats_call = lambda: ops.canopy_top(xyz, grid, ground, cg, *h, skip=skip, want_stats=True)  # noqa: E731
    t = stats_call()
    tree_call = lambda: ops.canopy_trees(t["top"], t["top_row"], t["count"], cg, **rule)  # noqa: E731
    seg = tree_call()
    rows_call = lambda: ops.canopy_rows(xyz, grid, ground, cg, *h, seg["tree"], skip=skip)  # noqa: E731
    row_tree = rows_call()
    # ---- checks
    statement = lambda: top_statement(xyz, skip, grid, ground, cg, *h)  # noqa: E731
    want_top, want_row, want_count = statement()
    assert torch.equal(want_count, t["count"].reshape(-1)), "count differs from the torch statement"
    assert same_bits(want_top, t["top"].reshape(-1)), "top differs from the torch statement"
    assert torch.equal(want_row, t["top_row"].reshape(-1)), "top_row differs from the torch statement"
    del want_top, want_row, want_count
    busiest = int(t["count"].reshape(-1).argmax().item())
    y0 = min(max(busiest // cg["nx"] - 100, 0), max(cg["ny"] - 200, 0))
    x0 = min(max(busiest % cg["nx"] - 256, 0), max(cg["nx"] - 512, 0))
    win = {key: t[key][y0:y0 + 200, x0:x0 + 512].contiguous() for key in ("top", "top_row", "count")}
    wg = dict(x0=0.0, y0=0.0, cell=cell, nx=int(win["top"].shape[1]), ny=int(win["top"].shape[0]))
    got = ops.canopy_trees(win["top"], win["top_row"], win["count"], wg, **rule)
    want = cn.segment_reference(win["top"].cpu().numpy(), win["top_row"].cpu().numpy(), win["count"].cpu().numpy(), cell,
                                rule["smooth"], rule["r0"], rule["r1"], rule["top_min"], rule["crown_frac"],
                                rule["crown_cells"])
    assert got["ntrees"] == want["ntrees"] and np.array_equal(got["tree"].cpu().numpy(), want["tree"]), "tree (window)"
    for key in cn.TABLE_KEYS:
        assert cn.same(got[key].cpu().numpy(), want[key]), key
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    owned = torch.nonzero(row_tree >= 0).reshape(-1)
    pick = [torch.randint(0, n, (4096,), generator=gen, device=dev)]
    if owned.numel():
        pick.append(owned[torch.randint(0, owned.numel(), (4096,), generator=gen, device=dev)])
    pick = torch.cat(pick)
    part, pcell, _ = part_statement(xyz[pick], skip[pick], grid, ground, cg, *h)
    want_rows = torch.where(part, seg["tree"].reshape(-1)[pcell], torch.full_like(pcell, -1).int())
    assert torch.equal(want_rows, row_tree[pick]), "row_tree differs from the statement"
    # ---- times
    out = {}
    for name, fn, kernels in (("top", top_call, TOP_KERNELS), ("top_with_stats", stats_call, TOP_KERNELS),
                              ("trees", tree_call, TREE_KERNELS), ("rows", rows_call, ROW_KERNELS)):
        median, runs = timed(fn, args.runs)
        out[name] = dict(median=median, runs=runs, kernel_ms=kernel_ms(fn, kernels))
    s_median, s_runs = timed(statement, args.runs)
    stats = t["stats"].tolist()
    top_bytes, rows_bytes = 13 * n, 17 * n
    print(json.dumps({
        "rows": n, "corridor_points": args.points, "vegetation_rows": args.veg_rows, "grid": [grid["nx"], grid["ny"]],
        "cell_m": args.cell, "canopy_grid": [cg["nx"], cg["ny"]], "canopy_cell_m": cell, "h_min": h[0], "h_max": h[1],
        "rule": rule, "trees": seg["ntrees"], "rows_owned": int(owned.numel()), "rows_skipped": int(skip.sum().item()),
        "window_checked": [wg["nx"], wg["ny"]], "window_trees": want["ntrees"], "rows_checked": int(pick.numel()),
        "rows_took_part": stats[0], "tile_cell_flushes": stats[1], "canopy_top_ms": out["top"],
        "canopy_top_with_stats_ms": out["top_with_stats"],
        "canopy_trees_ms": out["trees"], "canopy_rows_ms": out["rows"],
        "compulsory_bytes": {"top": top_bytes, "rows": rows_bytes},
        "gb_per_s": {"top": top_bytes / (out["top"]["median"] * 1e-3) / 1e9,
                     "rows": rows_bytes / (out["rows"]["median"] * 1e-3) / 1e9},
        "torch_statement_ms": {"median": s_median, "runs": s_runs,
                               "note": "ground, keys, scatter_reduce amax and bincount: step 1 only"}}), flush=True)


if __name__ == "__main__":
    main()
