"""What the slice table of the tower profile costs (ops.cluster_slices: pch_cluster_slices_f32).  The rows are the
clustered rows of bench.py's corridor (``synth.corridor_torch`` through ``pipeline.cluster_points``, the benchmark's
step), every cluster profiled in its own table row (the first 4096 if there are more) at dz = 0.5 m and B = 128 slices
from the cluster's lowest point.

Before any time is reported ``count``, ``ext`` and ``outside`` are compared bit for bit with the torch statement of the
rule: the cluster of every grouped entry from ``offsets``, s, t and the slice in float64 with one torch operation per
operation of the rule (so nothing is contracted), ``bincount`` for the counts and ``scatter_reduce`` with ``amin`` /
``amax`` on the order-preserving keys for the extents.  Then one JSON line: the call's time (device events around the
call, one warm-up, then --runs runs: all of them and their median), the kernels' own times from the library's event
profile, the rows, clusters and occupied slices, and for scale the torch statement's time on the same rows.  No time is
a pass / fail condition.
python tools/tower_profile_probe.py [--points N] [--dz 0.5] [--slices 128] [--runs 7]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eps_probe import event_ms  # noqa: E402
from pointcloudhookup_amd import ops, pipeline, synth  # noqa: E402

KERNELS = ["cluster_slices", "cluster_slices_decode"]
FLIP = 0x7FFFFFFFFFFFFFFF


def keys_of(v):
    """int64 keys that order like the doubles under a SIGNED comparison (the rule's key with its top bit flipped)"""
    bits = v.contiguous().view(torch.int64)
    return torch.where(bits < 0, bits ^ FLIP, bits)


def slices_statement(points, perm, offsets, K, frames5, slot, T, dz, B):
    """(count int32 [T,B], ext float64 [T,B,4], outside int64 [T,2]) in torch"""
    dev = points.device
    n = int(offsets[K].item()) if K else 0
    j = torch.arange(n, dtype=torch.int64, device=dev)
    k = torch.searchsorted(offsets, j, right=True) - 1                         # the cluster of every grouped entry
    p = points[perm[:n].long()].double()
    f = frames5[k]
    tab = slot[k].long()
    part = (tab >= 0) & (tab < T) & torch.isfinite(f).all(dim=1)
    dx, dy, h = p[:, 0] - f[:, 0], p[:, 1] - f[:, 1], p[:, 2] - f[:, 2]
    s = (dx * f[:, 3]) + (dy * f[:, 4])
    t = (dy * f[:, 3]) - (dx * f[:, 4])
    q = torch.floor(h / torch.full_like(h, dz))                                # (a tensor: a true division, no reciprocal)
    outside = torch.zeros((T, 2), dtype=torch.int64, device=dev)
    outside[:, 0] = torch.bincount(tab[part & (q < 0)], minlength=T)
    outside[:, 1] = torch.bincount(tab[part & (q >= B)], minlength=T)
    binned = part & (q >= 0) & (q < B) & torch.isfinite(s) & torch.isfinite(t)
    e = tab[binned] * B + q[binned].long()
    count = torch.bincount(e, minlength=T * B).to(torch.int32)
    ks, kt = keys_of(s[binned]), keys_of(t[binned])
    lo = torch.full((T * B,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
    hi = torch.full((T * B,), torch.iinfo(torch.int64).min, dtype=torch.int64, device=dev)
    planes = [lo.clone().scatter_reduce_(0, e, ks, reduce="amin"), hi.clone().scatter_reduce_(0, e, ks, reduce="amax"),
              lo.clone().scatter_reduce_(0, e, kt, reduce="amin"), hi.clone().scatter_reduce_(0, e, kt, reduce="amax")]
    empty = (float("inf"), float("-inf"), float("inf"), float("-inf"))
    has = count > 0
    ext = torch.stack([torch.where(has, torch.where(v < 0, v ^ FLIP, v).view(torch.float64),
                                   torch.full((T * B,), empty[c], dtype=torch.float64, device=dev))
                       for c, v in enumerate(planes)], dim=1)
    return count.reshape(T, B), ext.reshape(T, B, 4), outside


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
    ap.add_argument("--dz", type=float, default=0.5)
    ap.add_argument("--slices", type=int, default=128)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    raw = synth.corridor_torch(args.points, device=dev, dtype=torch.float32)
    out = pipeline.cluster_points(raw)
    del raw
    points, perm, offsets, K = out["ground"]["points"], out["perm"], out["offsets"], int(out["nclusters"])
    T, B, dz = max(min(K, ops.SLICES_MAX_TABLES), 1), args.slices, args.dz
    count, origin, moments = ops.cluster_moments(points, perm, offsets, K)
    frames = ops.span_frames(count, origin, moments)
    z0 = out["stats"][:K, 2].double()
    frames5 = torch.stack([frames[:, 0], frames[:, 1], z0, frames[:, 3], frames[:, 4]], dim=1).contiguous()
    slot = torch.arange(K, dtype=torch.int32, device=dev)
    slot = torch.where(slot < T, slot, torch.full_like(slot, -1))
    call = lambda: ops.cluster_slices(points, perm, offsets, K, frames5, slot, T, dz, B)  # noqa: E731
    got = call()
    statement = lambda: slices_statement(points, perm, offsets, K, frames5, slot, T, dz, B)  # noqa: E731
    want = statement()
    assert torch.equal(got["count"], want[0]), "count differs from the torch statement"
    assert torch.equal(got["ext"].view(torch.int64), want[1].view(torch.int64)), "ext differs from the torch statement"
    assert torch.equal(got["outside"], want[2]), "outside differs from the torch statement"
    del want
    call_ms, call_runs, got = timed(call, args.runs)
    ops.set_profiling(True, only=KERNELS)
    kern = {name: [] for name in KERNELS}
    for _ in range(args.runs + 1):
        call()
        torch.cuda.synchronize()
        for name, t, _l in ops.get_profile():
            if name in kern:
                kern[name].append(round(t, 4))
    ops.set_profiling(False)
    torch_ms, torch_runs, _ = timed(statement, args.runs)
    grouped = int(offsets[K].item()) if K else 0
    sizes = (offsets[1:] - offsets[:-1])
    levels = ops.tower_levels(got["count"], got["ext"], z0[:T].contiguous(), dz, ground=z0[:T].contiguous())
    print(json.dumps({
        "rows_kept": int(points.shape[0]), "rows_grouped": grouped, "perm_entries": int(perm.numel()), "clusters": K,
        "largest_cluster": int(sizes.max()) if K else 0, "tables": T, "slices": B, "dz_m": dz,
        "rows_binned": int(got["count"].sum()), "rows_outside": got["outside"].sum(dim=0).tolist(),
        "slices_occupied": int((got["count"] > 0).sum()), "clusters_with_a_level": int((levels["n_levels"] > 0).sum()),
        "call_ms": {"median": call_ms, "runs": call_runs},
        "kernel_ms": {name: {"median": statistics.median(v[1:]), "runs": v[1:]} for name, v in kern.items()},
        "bytes": 16 * int(perm.numel()), "gb_per_s": 16 * int(perm.numel()) / (call_ms * 1e-3) / 1e9,
        "torch_statement_ms": {"median": round(torch_ms, 3), "runs": torch_runs}}), flush=True)


if __name__ == "__main__":
    main()
