"""The k-distance profile of stage C's input, for choosing eps / min_points (pipeline.kdistance_profile), and what it
costs.  Input: the synthetic corridor of bench.py (default 100 M rows) or --las PATH (las.read_device), either through
stage B; the profile is taken on the rows stage B keeps, in the reference's file-order chunks.
One JSON line with an entry for every k of --k: quantiles and knee of the k-distance in metres, the share of sampled
rows whose k-distance lies beyond --eps-max (truncated), the share that is core at the reference's eps = 8, the times of the
fit and of the kdist call (device events, one warm-up, then --runs runs: all of them and their median), the dq_kdist
kernel's own time from the library's event profile, and the work it did: candidate pairs per query (rows in the 5x5x5
block of cells around the query) and sweeps per query (1, or 8 where at least k rows lie within eps_max and they do not
fit the wave's buffer of 1024 keys).  --sklearn N: N sampled rows of one chunk against NearestNeighbors(kd_tree) on
the host - values bit for bit, and the host's time for orientation.  No time is a pass / fail condition.
python tools/eps_probe.py [--points N | --las PATH] [--k 20 80 200] [--eps-max 16] [--sample 200000] [--runs 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudhookup_amd import las, ops, pipeline, synth  # noqa: E402

REF_EPS = 8.0
DK_CAP = 1024                                  # keys a wave of dq_kdist_k keeps in LDS (pch_dbscan_query.hip)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def block_rows(points, idx, eps, chunk_size):
    """int64 [len(idx)]: rows of the query's chunk in the 5x5x5 block of stage C's cells around each sampled row -
    the candidates one sweep of dq_kdist_k visits for it"""
    p = points.double()
    inv = 1.0 / (float(eps) / 1.7320508075688772 * (1.0 - 1.0 / 65536.0))
    c = torch.floor((p - p.min(0).values) * inv).long() + 2                     # room for the block below cell 0
    dims = c.max(0).values + 3
    chunk = torch.arange(len(p), device=p.device) // chunk_size if chunk_size else torch.zeros_like(c[:, 0])
    key = ((chunk * dims[2] + c[:, 2]) * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    uniq, cnt = torch.unique(key, return_counts=True)
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=p.device), torch.cumsum(cnt, 0)])
    q = key[idx]
    total = torch.zeros_like(q)
    for dz in range(-2, 3):
        for dy in range(-2, 3):                                                  # a row of five cells: one key range
            base = q + (dz * dims[1] + dy) * dims[0]
            total += csum[torch.searchsorted(uniq, base + 2, right=True)] - csum[torch.searchsorted(uniq, base - 2)]
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--las", default=None)
    ap.add_argument("--k", type=int, nargs="+", default=[20, 80, 200])
    ap.add_argument("--eps-max", type=float, default=16.0)
    ap.add_argument("--sample", type=int, default=200_000)
    ap.add_argument("--chunk", type=int, default=pipeline.REF_CHUNK)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sklearn", type=int, default=0)
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
    profiles = []
    for k in args.k:
        prof = pipeline.kdistance_profile(points, k=k, eps_max=args.eps_max, chunk_size=args.chunk, sample=args.sample,
                                          seed=args.seed)
        rows = torch.from_numpy(prof["rows"]).to(dev)
        q = points[rows]
        fit_ms, kd_ms = [], []
        for r in range(args.runs + 1):                                           # the first run warms up
            t, fit = event_ms(lambda: ops.DbscanFit(points, args.eps_max, k, args.chunk))
            chunk = (rows // fit.chunk_size).to(torch.int32) if fit.chunk_size else None
            t2, _ = event_ms(lambda: fit.kdist(q, k, chunk=chunk))
            if r:
                fit_ms.append(t)
                kd_ms.append(t2)
        ops.set_profiling(True, only=["dq_kdist"])
        kern = []
        for _ in range(3):
            fit.kdist(q, k, chunk=chunk)
            torch.cuda.synchronize()
            kern += [ms for name, ms, _l in ops.get_profile() if name == "dq_kdist"]
        ops.set_profiling(False)
        cand = block_rows(points, rows, args.eps_max, fit.chunk_size).cpu().numpy()
        count = prof["count"].astype(np.int64)
        sweeps = np.where((count >= k) & (count > DK_CAP), 8, 1)
        lds = np.where((count >= k) & (count <= DK_CAP), 7 * count, 0)
        out = {"k": k, "sampled": len(prof["rows"]), "quantiles_m": prof["quantiles"], "knee_m": prof["knee"],
               "truncated_share": prof["truncated"] / max(len(prof["rows"]), 1),
               "core_share_at_eps8": pipeline.core_share(prof, REF_EPS) if args.eps_max >= REF_EPS else None,
               "fit_ms": {"median": statistics.median(fit_ms), "runs": [round(t, 3) for t in fit_ms]},
               "kdist_ms": {"median": statistics.median(kd_ms), "runs": [round(t, 3) for t in kd_ms]},
               "dq_kdist_kernel_ms": [round(t, 3) for t in kern[1:]],
               "candidates_per_query": {"mean": float(cand.mean()), "max": int(cand.max())},
               "within_eps_max_per_query": {"mean": float(count.mean()), "max": int(count.max())},
               "queries_resweeping": float((sweeps == 8).mean()),
               "pair_evaluations": int((cand * sweeps).sum()), "lds_key_reads": int(lds.sum())}
        if args.sklearn:
            from sklearn.neighbors import NearestNeighbors
            c0 = int(prof["rows"][len(prof["rows"]) // 2]) // (fit.chunk_size or n)   # the chunk of the middle row
            lo, hi = c0 * (fit.chunk_size or n), min((c0 + 1) * (fit.chunk_size or n), n)
            sel = np.flatnonzero((prof["rows"] >= lo) & (prof["rows"] < hi))[:args.sklearn]
            X = points[lo:hi].cpu().numpy()
            qs = X[prof["rows"][sel] - lo]
            d2 = fit.kdist(q[torch.from_numpy(sel).to(dev)], k, chunk=None if chunk is None else
                           chunk[torch.from_numpy(sel).to(dev)]).cpu().numpy()
            t0 = time.perf_counter()
            nn = NearestNeighbors(algorithm="kd_tree").fit(X)
            t1 = time.perf_counter()
            dist = nn.kneighbors(qs, n_neighbors=min(k, len(X)))[0][:, -1]
            t2 = time.perf_counter()
            fin = np.isfinite(d2)
            out["sklearn"] = {"rows": len(sel), "chunk_rows": int(hi - lo), "build_s": t1 - t0, "query_s": t2 - t1,
                              "finite": int(fin.sum()), "bit_equal": bool(len(X) >= k and np.array_equal(
                                  np.sqrt(d2[fin]).view(np.uint64), dist[fin].view(np.uint64))),
                              "beyond_eps_max_agree": bool(len(X) >= k and (dist[~fin] >= args.eps_max).all())}
        profiles.append(out)
        del fit
        torch.cuda.empty_cache()
    print(json.dumps({"eps_max": args.eps_max, "raw_rows": int(n_raw), "kept_rows": int(n), "chunk": args.chunk,
                      "profiles": profiles}), flush=True)


if __name__ == "__main__":
    main()
