"""Time of stage B from resident int32 LAS records, both ways, on the synthetic corridor at EPSG:4547 magnitudes
(LAS scale 0.001, offsets 437000 / 3139000 / 80):
  (a) the reference frame: ops.las_scale + ops.cast_f32 + ops.ground_filter (a float64 and a float32 copy of the cloud)
  (b) the LAS-integer frame: ops.ground_filter_las on the records themselves
Device events around each call, the two routes alternating, one warm-up each, the median of RUNS runs.  Then, with the
library's own event timing, the kernels of (b) one by one, beside the bytes the algorithm needs of each: 12 B per row
and sweep, plus 12 B per kept row written by the filter sweep.  No time is a pass / fail condition: the script reports.
python tools/frame_probe.py [points ...]     (default 100 M rows)"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudhookup_amd import ops, synth  # noqa: E402

RUNS = 7
SCALES = np.array([0.001, 0.001, 0.001])
OFFSETS = synth.GLOBAL_OFFSET.copy()


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def reference_route(XYZ):
    return ops.ground_filter(ops.cast_f32(ops.las_scale(XYZ, SCALES, OFFSETS)), want_index=False)


def las_route(XYZ):
    return ops.ground_filter_las(XYZ, SCALES, OFFSETS, want_index=False)


for n in [int(a) for a in sys.argv[1:]] or [100_000_000]:
    cloud = synth.corridor_torch(n, seed=synth.SEED0 + 2, kind="corridor", offset=False, device="cuda")
    XYZ = torch.round(cloud / torch.tensor(SCALES, device="cuda")).to(torch.int32).contiguous()
    del cloud
    torch.cuda.empty_cache()
    event_ms(lambda: reference_route(XYZ))                       # warm-up of either route
    event_ms(lambda: las_route(XYZ))
    ref_ms, las_ms = [], []
    for _ in range(RUNS):
        ref_ms.append(event_ms(lambda: reference_route(XYZ))[0])
        t, gf = event_ms(lambda: las_route(XYZ))
        las_ms.append(t)
    a, b = statistics.median(ref_ms), statistics.median(las_ms)
    print(f"{n} rows from resident int32 records, median of {RUNS}")
    print(f"  (a) las_scale + cast_f32 + ground_filter: {a:.3f} ms  {[round(t, 3) for t in ref_ms]}")
    print(f"  (b) ground_filter_las:                    {b:.3f} ms  {[round(t, 3) for t in las_ms]}")
    print(f"  (b) / (a) = {b / a:.3f}; (b) keeps {gf['count']} rows, integer centroid {gf['centroid_int'].tolist()}, "
          f"base {float(gf['base']):.4f}, threshold {float(gf['threshold']):.4f}")
    ops.set_profiling(True)
    per = {}
    for _ in range(RUNS + 1):
        las_route(XYZ)
        torch.cuda.synchronize()
        for name, ms, _launches in ops.get_profile():
            per.setdefault(name, []).append(ms)
    ops.set_profiling(False)
    sweep = 12.0 * n
    need = {"fr_sum": sweep, "fr_hist0": sweep, "fr_hist1": sweep, "fr_hist2": sweep,
            "fr_filter": sweep + 12.0 * gf["count_at_offset"], "fr_filter_fb": sweep + 12.0 * gf["count"]}
    print("  kernels of (b), median ms | bytes the pass needs when it runs | GB/s if it ran")
    for name, ms in per.items():
        m = statistics.median(ms[1:])
        if name in need:
            print(f"    {name:13s} {m:8.3f} ms | {need[name] / 1e6:9.1f} MB | {need[name] / (m * 1e-3) / 1e9:8.1f} GB/s")
        else:
            print(f"    {name:13s} {m:8.3f} ms")
    del XYZ
    torch.cuda.empty_cache()
