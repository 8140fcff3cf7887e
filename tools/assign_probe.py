"""Time of ops.DbscanFit.assign on a corridor: the ground filter and one global fit on the kept rows, then every raw
row assigned with sub=centroid.  Median of 5 runs after a warm-up, a synchronise on both sides of each timed run.
python tools/assign_probe.py [points]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudhookup_amd import ops, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
raw = synth.corridor_torch(n, seed=synth.SEED0, kind="corridor", offset=True, device="cuda", dtype=torch.float32)
gf = ops.ground_filter(raw)
fit = ops.DbscanFit(gf["points"], 8.0, 80, 0, aabb=gf["aabb"])
print(f"{n} rows, {gf['count']} kept, {fit.nclusters} clusters")


def run():
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fit.assign(raw, sub=gf["centroid"])
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


run()                                                # warm-up
times = []
for _ in range(5):
    dt, labels = run()
    times.append(dt)
assert torch.equal(labels[gf["index"].long()], fit.labels), "kept rows do not get their own labels back"
ops.set_profiling(True)
fit.assign(raw, sub=gf["centroid"])
torch.cuda.synchronize()
prof = {k: round(ms, 3) for k, ms, c in ops.get_profile()}
ops.set_profiling(False)
print(f"assign of {n} rows: median {statistics.median(times):.2f} ms (runs {[round(t, 2) for t in times]}), "
      f"{int((labels >= 0).sum())} rows labelled, {int((labels >= 0).sum()) - int((fit.labels >= 0).sum())} of them "
      f"not among the kept rows' own")
print(f"kernels: {prof}")
