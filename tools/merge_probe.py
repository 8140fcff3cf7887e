"""Time of the opt-in cluster merge (ops.merge_clusters) beside the step it follows, on the synthetic corridor (float32,
offset frame): per size (default 10 M and 100 M rows) one pipeline.cluster_points call without the merge (the step as
it was) and one with merge_threshold=6.0, then the two new library calls alone on that step's clusters: (a)
ops.cluster_centers (pch_cluster_centers_f32, one wave per cluster - linear in the largest cluster) and (b)
pch_cluster_merge_f32 (all pairs, union-find, ranking scan, relabel sweep).  Prints K (clusters of the fit), C
(clusters after the merge) and the largest cluster.  Median of 7 runs after a warm-up, a synchronise on both sides of
each timed run.  No time is a pass / fail condition: the script only reports.
python tools/merge_probe.py [points ...]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudhookup_amd import _lib, ops, pipeline, synth  # noqa: E402

RUNS, THRESHOLD = 7, 6.0


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


def merge_call(centers, labels, K):
    """pch_cluster_merge_f32 alone, on a copy of the labels (it relabels in place)"""
    L = _lib.lib()
    lab = labels.clone()
    cmap = torch.empty((max(K, 1),), dtype=torch.int32, device=lab.device)
    cnt = torch.empty((1,), dtype=torch.int32, device=lab.device)
    need = L.pch_cluster_merge_ws_bytes(K)
    ws = torch.empty((need,), dtype=torch.uint8, device=lab.device)

    def run():
        lab.copy_(labels)
        _lib.check(L.pch_cluster_merge_f32(centers.data_ptr(), K, THRESHOLD, lab.data_ptr(), lab.numel(), cmap.data_ptr(),
                                           cnt.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
    return run, lambda: lab.copy_(labels)


for n in [int(a) for a in sys.argv[1:]] or [10_000_000, 100_000_000]:
    raw = synth.corridor_torch(n, seed=synth.SEED0, kind="corridor", offset=True, device="cuda",
                               dtype=torch.float32).contiguous()
    step, step_runs = median_ms(lambda: pipeline.cluster_points(raw))
    both, both_runs = median_ms(lambda: pipeline.cluster_points(raw, merge_threshold=THRESHOLD))
    cl = pipeline.cluster_points(raw)
    merged = pipeline.cluster_points(raw, merge_threshold=THRESHOLD)
    K, C = int(cl["nclusters"]), int(merged["nclusters"])
    pts, nf = cl["ground"]["points"], int(cl["ground"]["count"])
    sizes = ops.cluster_centers(pts, cl["perm"], cl["offsets"], K)[1]
    largest = int(sizes.max().item()) if K else 0
    a, a_runs = median_ms(lambda: ops.cluster_centers(pts, cl["perm"], cl["offsets"], K))
    centers = ops.cluster_centers(pts, cl["perm"], cl["offsets"], K)[0]
    run, copy_only = merge_call(centers, cl["labels"], K)
    b, b_runs = median_ms(run)
    c, _ = median_ms(copy_only)
    print(f"{n} rows: {nf} kept, K = {K} clusters, C = {C} after the merge at {THRESHOLD} m, largest cluster {largest} rows")
    print(f"  cluster_points without the merge (the step as it was): {step:.3f} ms  {step_runs}")
    print(f"  cluster_points with merge_threshold={THRESHOLD}: {both:.3f} ms = +{both - step:.3f} ms  {both_runs}")
    print(f"  (a) ops.cluster_centers alone: {a:.3f} ms = {1e6 * a / max(largest, 1):.2f} ns per row of the largest "
          f"cluster  {a_runs}")
    print(f"  (b) pch_cluster_merge_f32 alone (labels copy of {c:.3f} ms taken off): {b - c:.3f} ms  {b_runs}")
    del raw, cl, merged, pts
    torch.cuda.empty_cache()
