"""Time of ops.crop_boxes against the loop of ops.crop_aabb calls it replaces: a float64 corridor with 32 towers, one
kuangxuan box on each, once in generator order (50 m strips: spatially coherent) and once fully shuffled.  Per order:
(a) one crop_boxes call (default cap, and with cap = the hit count, i.e. without the repeat), (b) the loop of 32
crop_aabb calls, (c) the hit sweep alone (the library's own event timing).  Median of 7 runs after a warm-up, a
synchronise on both sides of each timed run.  Also: the hit count, the mean number of boxes a 2048-row tile has to
test, and the sweep's fraction of the HBM peak by algorithmic bytes (24 B/row + 32 B/hit).
python tools/crop_probe.py [points]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudhookup_amd import ops, synth  # noqa: E402
from pointcloudhookup_amd.ui import extract  # noqa: E402

HBM_PEAK = 8.0e12                                    # bytes/s, MI355X data sheet
TOWERS, RUNS, TILE = 32, 7, 2048

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
cloud = synth.corridor_torch(n, seed=synth.SEED0, kind="corridor", offset=True, towers=TOWERS, device="cuda")
step = synth.corridor_length(n) / TOWERS
towers = [dict(center=synth.GLOBAL_OFFSET + [(k + 0.5) * step, synth.W / 2, 22.0], rotation=np.eye(3),
               extent=np.array([6.0, 6.0, 45.0])) for k in range(TOWERS)]
boxes = extract.tower_crop_boxes(towers)
bounds = torch.from_numpy(ops.crop_box_bounds(boxes)).cuda()


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


def active_boxes_per_tile(x):
    """mean number of boxes whose cull bounds meet a tile's bounding box (what the sweep tests per tile)"""
    pad = (-x.shape[0]) % TILE
    t = torch.cat([x, x[-1:].expand(pad, 3)]).reshape(-1, TILE, 3)
    lo, hi = t.amin(1), t.amax(1)
    meets = ((lo[:, None, :] <= bounds[None, :, 3:]) & (hi[:, None, :] >= bounds[None, :, :3])).all(2)
    return float(meets.sum(1).double().mean())


ok = True
for name, x in (("generator order", cloud), ("shuffled", cloud[torch.randperm(n, device="cuda")].contiguous())):
    pts, offs, idx = ops.crop_boxes(x, boxes, want_index=True)
    hits = int(offs[-1])
    loop = [ops.crop_aabb(x, b[1], b[2], want_index=True) for b in boxes]
    assert torch.equal(pts, torch.cat([p for p, _ in loop])) and torch.equal(idx, torch.cat([i for _, i in loop]))
    del loop
    retried = hits > max(n // 8, 1 << 16)
    a, a_runs = median_ms(lambda: ops.crop_boxes(x, boxes))
    a1, a1_runs = median_ms(lambda: ops.crop_boxes(x, boxes, cap=hits))
    b, b_runs = median_ms(lambda: [ops.crop_aabb(x, bx[1], bx[2]) for bx in boxes])
    ops.set_profiling(True, only=["crop_sweep"])
    sweeps = []
    for _ in range(RUNS + 1):
        ops.crop_boxes(x, boxes, cap=hits)
        torch.cuda.synchronize()
        sweeps.append(dict((k, ms) for k, ms, c in ops.get_profile())["crop_sweep"])
    ops.set_profiling(False)
    c = statistics.median(sweeps[1:])
    frac = (24.0 * n + 32.0 * hits) / (c * 1e-3) / HBM_PEAK
    print(f"{name}: {n} rows, {TOWERS} boxes, {hits} hits, {active_boxes_per_tile(x):.2f} boxes per tile")
    print(f"  (a) crop_boxes, default cap{' (repeated once: more hits than n/8)' if retried else ''}: "
          f"{a:.3f} ms  {[round(t, 3) for t in a_runs]}")
    print(f"  (a) crop_boxes, cap = hits: {a1:.3f} ms  {[round(t, 3) for t in a1_runs]}")
    print(f"  (b) {TOWERS} crop_aabb calls: {b:.3f} ms  {[round(t, 3) for t in b_runs]}")
    print(f"  (c) sweep alone: {c:.3f} ms = {100 * frac:.1f} % of {HBM_PEAK / 1e12:.1f} TB/s by algorithmic bytes")
    ok = ok and a < b
print("crop_boxes faster than the loop in both orders:", ok)
sys.exit(0 if ok else 1)
