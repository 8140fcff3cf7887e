"""Time of the per-tile plane ground rule (ops.ground_filter_plane_tiles) beside the one-plane rule
(ops.ground_filter_plane) and the percentile rule (ops.ground_filter) on the same cloud: the synthetic corridor over
rolling terrain - the V-shaped valley of the tests across the 100 m width on a slope along the corridor,
z += 0.3 |y - 50| + 0.1 x - float32, offset frame.  Per size (default 10 M and 100 M rows), with H = 64 on both plane
rules: (a) one call of each rule, host reads included; (b) inside one ops.plane_tiles_fit call, by the library's own event timing, the count kernel
plt_count_k alone and the grouping alone (plt_key_k, the radix sort's launches, plt_starts_k, plt_passes_k).  The tile
size is 20 m, doubled until the grid has at most 65 536 tiles.  Median of 7 runs after a warm-up, a synchronise on both
sides of each timed run.  No time is a pass / fail condition: the script only reports.
python tools/plane_tiles_probe.py [points ...]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudhookup_amd import ops, synth  # noqa: E402

RUNS, H = 7, 64
NOT_GROUPING = ("plt_planes", "plt_count", "plt_best")


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def median_ms(fn):
    timed(fn)                                        # warm-up
    runs = [timed(fn)[0] for _ in range(RUNS)]
    return statistics.median(runs), runs


def fit_kernels_ms(fn):
    """(count ms, grouping ms, {kernel: ms}) of one plane_tiles_fit call: medians over RUNS calls after a warm-up"""
    ops.set_profiling(True)
    count, group, last = [], [], {}
    for _ in range(RUNS + 1):
        fn()
        torch.cuda.synchronize()
        last = {}
        for k, v, c in ops.get_profile():
            last[k] = last.get(k, 0.0) + v
        count.append(last.get("plt_count", 0.0))
        group.append(sum(v for k, v in last.items() if k not in NOT_GROUPING))
    ops.set_profiling(False)
    return statistics.median(count[1:]), statistics.median(group[1:]), last


for n in [int(a) for a in sys.argv[1:]] or [10_000_000, 100_000_000]:
    cloud = synth.corridor_torch(n, seed=synth.SEED0, kind="corridor", offset=False, device="cuda")
    cloud[:, 2] += 0.3 * (cloud[:, 1] - 50.0).abs() + 0.1 * cloud[:, 0]
    raw = (cloud + torch.tensor(synth.GLOBAL_OFFSET, device="cuda")).to(torch.float32).contiguous()
    del cloud
    centroid = ops.mean_seq_f32(raw)
    tile = 20.0
    while True:
        try:
            grid = ops.plane_tile_grid(raw, centroid, tile)
            break
        except ValueError:
            tile *= 2.0
    c, c_runs = median_ms(lambda: ops.ground_filter(raw, want_index=False))
    p, p_runs = median_ms(lambda: ops.ground_filter_plane(raw, hypotheses=H, want_index=False))
    t, t_runs = median_ms(lambda: ops.ground_filter_plane_tiles(raw, tile_size=tile, hypotheses=H, want_index=False))
    kept = [ops.ground_filter(raw, want_index=False)["count"],
            ops.ground_filter_plane(raw, hypotheses=H, want_index=False)["count"]]
    gf = ops.ground_filter_plane_tiles(raw, tile_size=tile, hypotheses=H, want_index=False)
    draws = ops.plane_tile_draws(H, 0)
    cnt, grp, kernels = fit_kernels_ms(lambda: ops.plane_tiles_fit(raw, centroid, grid, draws))
    own, occupied = int((gf["tiles"]["best"] >= 0).sum()), int((gf["tiles"]["rows"] > 0).sum())
    print(f"{n} rows, tile {tile:g} m, grid {grid['nx']} x {grid['ny']}, {own} of {occupied} occupied tiles with a plane")
    print(f"  ground_filter (percentile rule):   {c:.3f} ms, keeps {kept[0]}  {[round(v, 3) for v in c_runs]}")
    print(f"  ground_filter_plane, H = {H}:        {p:.3f} ms, keeps {kept[1]}  {[round(v, 3) for v in p_runs]}")
    print(f"  ground_filter_plane_tiles, H = {H}:  {t:.3f} ms, keeps {gf['count']}  {[round(v, 3) for v in t_runs]}")
    print(f"  inside plane_tiles_fit: plt_count_k {cnt:.3f} ms, grouping {grp:.3f} ms")
    print("  last run per kernel: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(kernels.items())))
    del raw
    torch.cuda.empty_cache()
