"""What the k nearest rows of stage C's input cost (ops.DbscanFit.knn), and what the default sparse-row rule
(pipeline.drop_sparse_rows) drops.  Input: the synthetic corridor of bench.py (default 100 M rows) through stage B; per
radius (default 2 m and 0.5 m) one global fit of the kept rows at eps = radius, then fit.knn on the fit's own rows at
every k (default 8 and 32).
One JSON line per (radius, k): the time of the fit (one run) and of the knn call (device events around the call, one
warm-up, then --runs runs: all of them and their median), the dq_knn kernel's own time from the library's event profile,
and the pair evaluations of one call in DESIGN.md section 5a's currency, from a census of the cells (T: for every row
the rows in the 5x5x5 block of cells around it) and the counts the call returned: the select sweeps T once where at most
DK_CAP rows are in reach (or fewer than k) and eight times beyond it, the emit sweeps it once more; the four sweeps of
a row select (ties at the cut) cannot be seen from outside and are not counted.  At k = 8 the share of rows the rule
(k, radius, 2.0) drops is reported too.  No time is a pass / fail condition.
python tools/knn_probe.py [--points N] [--radius 2 0.5] [--k 8 32] [--runs 7]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eps_probe import DK_CAP, block_rows, event_ms  # noqa: E402
from pointcloudhookup_amd import ops, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--radius", type=float, nargs="+", default=[2.0, 0.5])
    ap.add_argument("--k", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    raw = synth.corridor_torch(args.points, seed=synth.SEED0 + 2, kind="corridor", offset=True, device=dev,
                               dtype=torch.float32)
    gf = ops.ground_filter(raw, want_index=False)
    points = gf["points"].clone()
    n_raw = raw.shape[0]
    del raw, gf
    torch.cuda.empty_cache()
    n = points.shape[0]
    for radius in args.radius:
        fit_ms, fit = event_ms(lambda: ops.DbscanFit(points, radius, 1, 0))
        cand = block_rows(points, torch.arange(n, device=dev), radius, 0).double()
        for k in args.k:
            knn_ms = []
            for r in range(args.runs + 1):                                       # the first run warms up
                t, (rows, d2, count) = event_ms(lambda: fit.knn(points, k, chunk="own", want_count=True))
                if r:
                    knn_ms.append(t)
            ops.set_profiling(True, only=["dq_knn"])
            kern = []
            for _ in range(3):
                fit.knn(points, k, chunk="own")
                torch.cuda.synchronize()
                kern += [ms for name, ms, _l in ops.get_profile() if name == "dq_knn"]
            ops.set_profiling(False)
            resweep = (count > DK_CAP) & (count >= k)
            pairs = int((cand * torch.where(resweep, 9.0, 2.0)).sum().item())
            med = statistics.median(knn_ms)
            out = {"radius": radius, "k": k, "raw_rows": int(n_raw), "kept_rows": int(n), "fit_ms": round(fit_ms, 3),
                   "knn_ms": {"median": med, "runs": [round(t, 3) for t in knn_ms]},
                   "dq_knn_kernel_ms": [round(t, 3) for t in kern[1:]],
                   "candidates_per_query": {"mean": float(cand.mean().item()), "max": int(cand.max().item())},
                   "within_radius_per_query": {"mean": float(count.double().mean().item()), "max": int(count.max().item())},
                   "full_answers_share": float((count >= k).double().mean().item()),
                   "resweep_share": float(resweep.double().mean().item()),
                   "pair_evaluations": pairs, "pairs_per_second": pairs / (med * 1e-3)}
            if k == 8:
                m = ops.knn_mean_distance(d2, count, k)
                dense = m[count >= k]
                thr = float(dense.mean() + 2.0 * dense.std(unbiased=True)) if dense.numel() >= 2 else float("inf")
                out["rule"] = {"k": k, "radius": radius, "std_ratio": 2.0, "threshold": thr,
                               "dropped_share": float(((count < k) | (m > thr)).double().mean().item())}
            print(json.dumps(out), flush=True)
            del rows, d2, count
        del fit, cand
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
