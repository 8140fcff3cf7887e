"""What the two per-cluster reductions of the conductor spans cost (ops.cluster_moments, ops.cluster_profile).
bench.py's corridor has no wires, so the probe strings synthetic conductors between the corridor's towers
(synth.n_towers(--points) towers at x = (t + 1/2) L/T, y = W/2): per span three conductors at y offsets -6, 0, +6,
--wire-rows rows in all, a parabola with 2 % sag, N(0, 0.02) jitter, shuffled, at the corridor's global offset.  The rows
are grouped twice - one cluster per conductor, and all of them in ONE cluster (the load-balance case) - and for either
grouping one JSON line gives the time of each call (device events around the call, one warm-up, then --runs runs: all of
them and their median), the sweep kernels' own time from the library's event profile, the bytes a sweep must move
(4 B of perm + 12 B of row per grouped row) and the rate at the median, and as a yardstick pch_cluster_centers_f32 (one
wave per cluster) on the same grouping.  The one-cluster answer (count, first moments, extrema of s) is checked against
torch's own sums.  No time is a pass / fail condition.
python tools/span_probe.py [--points N] [--wire-rows M] [--runs 7]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eps_probe import event_ms  # noqa: E402
from pointcloudhookup_amd import ops, synth  # noqa: E402


def conductors(points, wire_rows, dev):
    """(rows float32 [m,3] shuffled, label int32 [m]: 3 * span + conductor)"""
    L = synth.corridor_length(points)
    T = synth.n_towers(points)
    per = max(wire_rows // (3 * (T - 1)), 2)
    g = torch.Generator(device=dev)
    g.manual_seed(synth.SEED0 + 5)
    parts, labels = [], []
    for sp in range(T - 1):
        x0, x1 = (sp + 0.5) * L / T, (sp + 1.5) * L / T
        tau = torch.linspace(0.0, 1.0, per, dtype=torch.float64, device=dev)
        x = x0 + (x1 - x0) * tau
        z = 30.0 - 4.0 * 0.02 * (x1 - x0) * tau * (1.0 - tau)
        for c, dy in enumerate((-6.0, 0.0, 6.0)):
            line = torch.stack([x, torch.full_like(x, synth.W / 2 + dy), z], dim=1)
            parts.append(line + 0.02 * torch.randn(line.shape, generator=g, dtype=torch.float64, device=dev))
            labels.append(torch.full((per,), 3 * sp + c, dtype=torch.int32, device=dev))
    P = torch.cat(parts) + torch.tensor(synth.GLOBAL_OFFSET, dtype=torch.float64, device=dev)
    lab = torch.cat(labels)
    order = torch.randperm(P.shape[0], generator=g, device=dev)
    return P[order].to(torch.float32).contiguous(), lab[order].contiguous(), 3 * (T - 1)


def timed(fn, runs):
    ms = []
    for r in range(runs + 1):                                                    # the first run warms up
        t, out = event_ms(fn)
        if r:
            ms.append(t)
    return {"median": statistics.median(ms), "runs": [round(t, 4) for t in ms]}, out


def kernel_ms(fn, names):
    ops.set_profiling(True, only=names)
    got = {name: [] for name in names}
    for _ in range(4):
        fn()
        torch.cuda.synchronize()
        for name, ms, _l in ops.get_profile():
            if name in got:
                got[name].append(round(ms, 4))
    ops.set_profiling(False)
    return {name: v[1:] for name, v in got.items()}


def measure(rows, labels, K, runs):
    perm, offsets, _ = ops.segment_by_label(labels, rows, K)
    n = int(perm.numel())
    mom, (count, origin, M) = timed(lambda: ops.cluster_moments(rows, perm, offsets, K), runs)
    frames = ops.span_frames(count, origin, M)
    pro, (S, E) = timed(lambda: ops.cluster_profile(rows, perm, offsets, K, frames), runs)
    cen, _ = timed(lambda: ops.cluster_centers(rows, perm, offsets, K), runs)
    table = ops.span_fit(count, frames, S, E)
    if K == 1:                                                                   # the long chain of folds, checked
        d = rows.double() - origin[0].double()
        bound = 2.0 * (n + 1.0) * 2.0 ** -53 * d.abs().sum(0)
        assert int(count[0].item()) == n and bool(((M[0, 0:3] - d.sum(0)).abs() <= bound).all()), "one-cluster moments"
        f = frames[0]
        s_ = ((rows[:, 0].double() - f[0]) * f[3] + (rows[:, 1].double() - f[1]) * f[4]) * f[5]
        assert max(abs(float(E[0, 0] - s_.min())), abs(float(E[0, 1] - s_.max()))) <= 1e-9, "one-cluster extrema"
    kern = kernel_ms(lambda: (ops.cluster_moments(rows, perm, offsets, K),
                              ops.cluster_profile(rows, perm, offsets, K, frames)),
                     ["span_moments", "span_moments_finish", "span_profile", "span_profile_finish"])
    nbytes = 16 * n
    return {"clusters": K, "grouped_rows": n, "largest_cluster": int(count.max().item()),
            "sweep_bytes": nbytes, "cluster_moments_ms": mom, "cluster_profile_ms": pro,
            "moments_gb_per_s": nbytes / (mom["median"] * 1e-3) / 1e9,
            "profile_gb_per_s": nbytes / (pro["median"] * 1e-3) / 1e9, "kernel_ms": kern,
            "cluster_centers_ms": cen, "cond_median": float(table["cond"].median().item()),
            "rms_z_median": float(table["rms_z"].median().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--wire-rows", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows, labels, K = conductors(args.points, args.wire_rows, dev)
    out = {"corridor_points": args.points, "towers": synth.n_towers(args.points),
           "span_m": synth.corridor_length(args.points) / synth.n_towers(args.points),
           "per_conductor": measure(rows, labels, K, args.runs),
           "one_cluster": measure(rows, torch.zeros_like(labels), 1, args.runs)}
    assert math.isfinite(out["per_conductor"]["cond_median"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
