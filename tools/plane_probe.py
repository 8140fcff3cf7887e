"""Time of the plane ground rule (ops.ground_filter_plane) beside the percentile rule (ops.ground_filter) on the same
cloud: the synthetic corridor on a 15 % / -5 % slope, float32, offset frame.  Per size (default 10 M and 100 M rows)
and per hypothesis count H = 64 / 256 / 1000: (a) one ground_filter_plane call, (b) the inlier count kernel pl_count_k
alone (the library's own event timing), with its float64 lane-instruction rate by the algorithmic count - 6 per
residual test, valid hypotheses only - against the 39.3 T lane-instr/s float64 vector peak VERDICT.md uses; and once
per size (c) one ground_filter call.  Median of 7 runs after a warm-up, a synchronise on both sides of each timed run.
No time is a pass / fail condition: the script only reports.
python tools/plane_probe.py [points ...]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudhookup_amd import ops, synth  # noqa: E402

F64_PEAK = 39.3e12                                   # float64 vector lane-instructions per second
RUNS, HYPS = 7, (64, 256, 1000)
SLOPE = (0.15, -0.05)


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


def kernel_ms(fn, name):
    ops.set_profiling(True, only=[name])
    ms = []
    for _ in range(RUNS + 1):
        fn()
        torch.cuda.synchronize()
        ms.append(dict((k, v) for k, v, c in ops.get_profile())[name])
    ops.set_profiling(False)
    return statistics.median(ms[1:])


for n in [int(a) for a in sys.argv[1:]] or [10_000_000, 100_000_000]:
    cloud = synth.corridor_torch(n, seed=synth.SEED0, kind="corridor", offset=False, device="cuda")
    cloud[:, 2] += SLOPE[0] * cloud[:, 0] + SLOPE[1] * cloud[:, 1]
    raw = (cloud + torch.tensor(synth.GLOBAL_OFFSET, device="cuda")).to(torch.float32).contiguous()
    del cloud
    c, c_runs = median_ms(lambda: ops.ground_filter(raw, want_index=False))
    kept_pct = ops.ground_filter(raw, want_index=False)["count"]
    print(f"{n} rows, slope {SLOPE}")
    print(f"  (c) ground_filter (percentile rule): {c:.3f} ms, keeps {kept_pct}  {[round(t, 3) for t in c_runs]}")
    for H in HYPS:
        a, a_runs = median_ms(lambda: ops.ground_filter_plane(raw, hypotheses=H, want_index=False))
        gf = ops.ground_filter_plane(raw, hypotheses=H, want_index=False)
        b = kernel_ms(lambda: ops.ground_filter_plane(raw, hypotheses=H, want_index=False), "pl_count")
        rate = 6.0 * n * gf["nvalid"] / (b * 1e-3)
        print(f"  H = {H} ({gf['nvalid']} valid, best holds {gf['inliers']} rows, keeps {gf['count']}):")
        print(f"    (a) ground_filter_plane: {a:.3f} ms = {a / c:.2f} x (c)  {[round(t, 3) for t in a_runs]}")
        print(f"    (b) pl_count_k alone: {b:.3f} ms = {rate / 1e12:.2f} T float64 lane-instr/s = "
              f"{100 * rate / F64_PEAK:.1f} % of {F64_PEAK / 1e12:.1f} T; derived floor {6.0 * n * gf['nvalid'] / F64_PEAK * 1e3:.3f} ms")
    del raw
    torch.cuda.empty_cache()
