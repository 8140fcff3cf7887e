"""What the neighbourhood shapes of stage C's input cost (ops.DbscanFit.shape), and what the default wire-removal rule
(pipeline.drop_linear_rows) drops.  Input: the synthetic corridor of bench.py (default 100 M rows) or --las PATH, either
through stage B; one global fit of the kept rows at eps = radius, then fit.shape on the fit's own rows.
One JSON line: the time of the fit (one run) and of the shape call (device events around the call, one warm-up, then
--runs runs: all of them and their median), the dq_shape kernel's own time from the library's event profile, the pair
evaluations of one call from a census of the cells (for every row the rows in the 5x5x5 block of cells around it: one
sweep each), pairs per second at the median, the time of ops.shape_features, and the share of rows the rule drops.
No time is a pass / fail condition.
python tools/shape_probe.py [--points N | --las PATH] [--radius 2] [--runs 7]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eps_probe import block_rows, event_ms  # noqa: E402
from pointcloudhookup_amd import las, ops, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--las", default=None)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--linearity", type=float, default=0.9)
    ap.add_argument("--verticality", type=float, default=0.5)
    ap.add_argument("--min-rows", type=int, default=10)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.las:
        hdr, XYZ = las.read_device(args.las, dev)
        raw = ops.cast_f32(ops.las_scale(XYZ, hdr.scales, hdr.offsets))
        del XYZ
    else:
        raw = synth.corridor_torch(args.points, seed=synth.SEED0 + 2, kind="corridor", offset=True, device=dev,
                                   dtype=torch.float32)
    gf = ops.ground_filter(raw, want_index=False)
    points = gf["points"].clone()
    n_raw = raw.shape[0]
    del raw, gf
    torch.cuda.empty_cache()
    n = points.shape[0]
    fit_ms, fit = event_ms(lambda: ops.DbscanFit(points, args.radius, 1, 0))
    shape_ms = []
    for r in range(args.runs + 1):                                               # the first run warms up
        t, (count, moments) = event_ms(lambda: fit.shape(points, args.radius, chunk="own"))
        if r:
            shape_ms.append(t)
    ops.set_profiling(True, only=["dq_shape"])
    kern = []
    for _ in range(3):
        fit.shape(points, args.radius, chunk="own")
        torch.cuda.synchronize()
        kern += [ms for name, ms, _l in ops.get_profile() if name == "dq_shape"]
    ops.set_profiling(False)
    feat_ms, f = event_ms(lambda: ops.shape_features(count, moments))
    dropped = (f["linearity"] >= args.linearity) & (f["verticality"] <= args.verticality) & (count >= args.min_rows)
    share = float(dropped.double().mean().item())
    within = count.double()
    del f, moments, dropped
    torch.cuda.empty_cache()
    cand = block_rows(points, torch.arange(n, device=dev), args.radius, 0)
    pairs = int(cand.sum().item())
    med = statistics.median(shape_ms)
    print(json.dumps({"radius": args.radius, "raw_rows": int(n_raw), "kept_rows": int(n), "fit_ms": round(fit_ms, 3),
                      "shape_ms": {"median": med, "runs": [round(t, 3) for t in shape_ms]},
                      "dq_shape_kernel_ms": [round(t, 3) for t in kern[1:]],
                      "candidates_per_query": {"mean": float(cand.double().mean().item()), "max": int(cand.max().item())},
                      "within_radius_per_query": {"mean": float(within.mean().item()), "max": int(within.max().item())},
                      "pair_evaluations": pairs, "pairs_per_second": pairs / (med * 1e-3),
                      "shape_features_ms": round(feat_ms, 3),
                      "rule": {"linearity": args.linearity, "verticality": args.verticality, "min_rows": args.min_rows},
                      "dropped_share": share}), flush=True)


if __name__ == "__main__":
    main()
