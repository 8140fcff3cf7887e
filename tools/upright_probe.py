"""Cost and quality of the opt-in upright boxes (obb_mode="upright") beside the exact mode, on the synthetic corridor
(float32, offset frame): per size (default 10 M and 100 M rows) the clusters of one pipeline.cluster_points call, then
  - pipeline.tower_table in exact mode (the path of the commit before the upright mode: worker pool, qhull) and in
    upright mode on those clusters: median of 7 after a warm-up, a synchronise on both sides of each timed run;
  - ops.upright_boxes alone (four launches, asynchronous), and its two levels apart by the library's kernel timers
    (sweep + combine per level);
  - the labels either mode accepts, the distance between the centres of the towers both accept, and for every tower the
    upright mode accepts the area of its rectangle over the smallest rectangle around its points' 2-D hull (rotating
    calipers over scipy's hull edges, float64 on the host).
No time is a pass / fail condition: the script only reports.
python tools/upright_probe.py [points ...]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudhookup_amd import ops, pipeline, synth  # noqa: E402

RUNS = 7
KERNELS = ("upright_sweep0", "upright_combine0", "upright_sweep1", "upright_combine1")


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def median_ms(fn):
    timed(fn)                                        # warm-up
    runs = [timed(fn)[0] for _ in range(RUNS)]
    return statistics.median(runs), [round(t, 3) for t in runs]


def smallest_rectangle_area(xy):
    """area of the smallest rectangle around the points: one side lies along an edge of their convex hull"""
    from scipy.spatial import ConvexHull
    xy = np.asarray(xy, dtype=np.float64)
    hull = xy[ConvexHull(xy).vertices]
    edges = np.roll(hull, -1, axis=0) - hull
    edges = edges / np.linalg.norm(edges, axis=1)[:, None]
    u = hull @ edges.T
    v = hull @ np.stack([-edges[:, 1], edges[:, 0]], axis=1).T
    return float(((u.max(axis=0) - u.min(axis=0)) * (v.max(axis=0) - v.min(axis=0))).min())


for n in [int(a) for a in sys.argv[1:]] or [10_000_000, 100_000_000]:
    raw = synth.corridor_torch(n, seed=synth.SEED0, kind="corridor", offset=True, device="cuda",
                               dtype=torch.float32).contiguous()
    cl = pipeline.cluster_points(raw)
    K, pts = int(cl["nclusters"]), cl["ground"]["points"]
    clustered = int(cl["offsets"][K].item()) if K else 0
    sizes = (cl["offsets"][1:] - cl["offsets"][:-1]).cpu().numpy()
    print(f"{n} rows: {int(cl['ground']['count'])} kept, K = {K} clusters, {clustered} clustered rows, largest "
          f"cluster {int(sizes.max()) if K else 0} rows")
    exact_ms, exact_runs = median_ms(lambda: pipeline.tower_table(cl))
    up_ms, up_runs = median_ms(lambda: pipeline.tower_table(cl, obb_mode="upright"))
    call_ms, call_runs = median_ms(lambda: ops.upright_boxes(pts, cl["perm"], cl["offsets"], K))
    print(f"  tower_table exact (the path as it was): {exact_ms:.3f} ms  {exact_runs}")
    print(f"  tower_table upright: {up_ms:.3f} ms  {up_runs}")
    print(f"  ops.upright_boxes alone (4 launches): {call_ms:.3f} ms  {call_runs}")
    ops.set_profiling(True, only=KERNELS)
    levels = []
    for _ in range(RUNS):
        ops.upright_boxes(pts, cl["perm"], cl["offsets"], K)
        torch.cuda.synchronize()
        prof = {name: ms for name, ms, _ in ops.get_profile()}
        levels.append([prof.get(name, float("nan")) for name in KERNELS])
    ops.set_profiling(False)
    med = np.median(np.array(levels), axis=0)
    print("  kernels (median of 7, ms): " + ", ".join(f"{name} {ms:.3f}" for name, ms in zip(KERNELS, med))
          + f"; level 0 {med[0] + med[1]:.3f}, level 1 {med[2] + med[3]:.3f}")
    ws = ops._lib.lib().pch_upright_boxes_ws_bytes(K, cl["perm"].numel())
    print(f"  workspace {ws / 2 ** 20:.1f} MiB")

    exact = {t["label"]: t for t in pipeline.tower_table(cl)}
    ordered = {t["label"]: t for t in pipeline.tower_table(cl, extent_order="trimesh_sorted")}
    upright = {t["label"]: t for t in pipeline.tower_table(cl, obb_mode="upright")}
    print(f"  accepted: exact {len(exact)}, exact with trimesh_sorted extents {len(ordered)}, upright {len(upright)}; "
          f"upright only {sorted(set(upright) - set(ordered))}, exact (sorted) only {sorted(set(ordered) - set(upright))}, "
          f"exact (unsorted) only {sorted(set(exact) - set(upright))}")
    both = sorted(set(upright) & set(ordered))
    if both:
        d = np.array([np.linalg.norm(upright[k]["center"] - ordered[k]["center"]) for k in both])
        dh = np.array([upright[k]["height"] - ordered[k]["height"] for k in both])
        print(f"  centres of the {len(both)} towers both accept: median {np.median(d):.3f} m apart, largest {d.max():.3f} m; "
              f"upright height minus the exact box's tall extent: median {np.median(dh):.3f} m, range {dh.min():.3f} .. {dh.max():.3f} m")
    if upright:
        ratio = np.array([t["extent"][0] * t["extent"][1] / smallest_rectangle_area(t["points"][:, :2])
                          for t in upright.values()])
        print(f"  rectangle area over the rotating-calipers optimum, {len(ratio)} towers: median {np.median(ratio):.7f}, "
              f"largest {ratio.max():.7f}")
    del raw, cl, pts, exact, ordered, upright
    torch.cuda.empty_cache()
