#!/usr/bin/env python3
"""Benchmark of the hot path: ground filter + tower clustering on a synthetic corridor.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--mode stream|tiled] [--points P] [--kind corridor|uniform]
                  [--dump-outputs DIR] [--full]

--dump-outputs DIR (e.g. bench_outputs/, which git ignores) writes the outputs of the last timed step as .npy files:
the inputs are seeded, so two builds run with the same arguments can be compared output for output.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints its line: the headline value, the
config, and what the timed steps record anyway (per-kernel hipEvent times, rooflines by algorithmic bytes).  --full
adds everything that needs work of its own: the kNN byte models and the pair-counting fit, the counter figures of
profiles/traffic.json, the config-4 side run (`tiled`), the side measurements (other workloads, H2D, tower table,
voxel stage, drop-ins end to end, config 5, two tiles in flight) and the CPU baseline; --no-side, --no-e2e,
--no-tile-stream and --no-cpu-baseline leave parts of that out.  A --mode tiled line is the same with or without --full.

One "step" = one pass of stages B + C + D0 (float32 centroid/centring, percentile height
filter, chunked exact DBSCAN, label grouping) over one resident float32 [P,3] tile per GPU.
Prints ONE JSON line (rank 0).  One rank per GPU: under torch.distributed.run (RANK / WORLD_SIZE in the
environment) this process IS a rank; started plainly with --gpus N > 1 it starts the N ranks itself
(`python -m torch.distributed.run ...` as a child, before anything here touches the GPU) and relays rank 0's line.

--mode stream (default; BASELINE configs[2] per GPU): every rank owns an independent 100 M-point tile, the
  reference's 50 000-row chunked DBSCAN; the only collective is the cluster-table reconciliation
  (tiles.reconcile).  Weak scaling.  With --full the line also carries a `tiled` object: the config-4 path below on
  --tiled-points-per-gpu points per rank (50 M: at 8 GPUs exactly BASELINE configs[3]), so that the scaling runs
  show the real cross-tile path over RCCL.
--mode tiled (BASELINE configs[3]): ONE corridor spread over the ranks as x-tiles + halo; chained float32 centroid,
  percentile threshold across the ranks, per-tile filter, global DBSCAN per tile and the cross-tile label
  reconciliation (tiles.tiled_step).  --points is then the WHOLE cloud (default 400 M); each rank generates only
  its own tile + halo.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
EPS, MIN_POINTS, CHUNK = 8.0, 80, 50000
DUMP_BUDGET_BYTES = 64 << 20   # --dump-outputs: all files together
DUMP_SAMPLE_ROWS = 1 << 20     # per-point outputs with more rows than this are written as a fixed sample of rows
DUMP_SEED = 20261015


def dump_outputs(dirname, whole, per_row, n_rows):
    """--dump-outputs: writes what the timed path handed its caller in the last timed step as DIR/<name>.npy, float32
    arrays as they are and everything else as float64 (exact for the integers here), so that two builds can be
    compared output for output.  `whole` maps names to small arrays (numpy or device tensors) written in full;
    `per_row` maps names to tensors of n_rows rows, written in full up to DUMP_SAMPLE_ROWS rows and otherwise as the
    same DUMP_SAMPLE_ROWS rows of each, drawn with a fixed seed; sample_rows.npy holds the row indices either way.
    Returns a summary for the result line."""
    import torch
    if n_rows <= DUMP_SAMPLE_ROWS:
        rows = np.arange(n_rows, dtype=np.int64)
    else:
        rows = np.sort(np.random.default_rng(DUMP_SEED).choice(n_rows, DUMP_SAMPLE_ROWS, replace=False))
    arrays = {"sample_rows": rows}
    for name, v in whole.items():
        arrays[name] = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    for name, t in per_row.items():
        assert t.shape[0] == n_rows, (name, tuple(t.shape), n_rows)
        arrays[name] = t.index_select(0, torch.from_numpy(rows).to(t.device)).cpu().numpy()
    arrays = {name: a if a.dtype in (np.float32, np.float64) else a.astype(np.float64) for name, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BUDGET_BYTES:
        raise SystemExit(f"bench.py: --dump-outputs would write {total} bytes (limit {DUMP_BUDGET_BYTES})")
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, f"{name}.npy"), a)
    return {"dir": dirname, "files": sorted(f"{name}.npy" for name in arrays), "bytes": int(total),
            "rows": int(n_rows), "rows_written": int(len(rows)), "sample_seed": DUMP_SEED}


def _tile_sum(points, side, chunk, query_mask_fn=None):
    """sum over (masked) query cells c of the points in the <=27 occupied cells around c, cells cubic of
    side `side`, chunks kept apart.  Returns (sum, unique keys, counts, mask)."""
    import torch
    n = points.shape[0]
    lo = points.min(dim=0).values
    ck = torch.arange(n, device=points.device) // chunk
    c = torch.floor((points - lo).double() / side).long()
    dims = c.max(dim=0).values + 3
    key = ((ck * dims[2] + c[:, 2] + 1) * dims[1] + c[:, 1] + 1) * dims[0] + c[:, 0] + 1
    uniq, cnt = torch.unique(key, return_counts=True)
    mask = torch.ones_like(cnt, dtype=torch.bool) if query_mask_fn is None else query_mask_fn(cnt)
    total = torch.zeros((), dtype=torch.int64, device=points.device)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nk = uniq + (dz * dims[1] + dy) * dims[0] + dx
                pos = torch.searchsorted(uniq, nk).clamp(max=uniq.numel() - 1)
                hit = (uniq[pos] == nk) & mask
                total += (cnt[pos] * hit).sum()
    return int(total), uniq, cnt, mask


def knn_tile_bytes(points, eps, chunk, min_samples):
    """Byte models of the radius-count kernel (db_core), both from SURVEY.md 8(d)'s tile formula
    bytes = 12 * sum_c sum_{c' in N27(c), occupied} n_c' + 4 * N_f:

    * all cells   - the formula as written: cubic cells of side eps, every query cell stages its 27 tiles;
    * sparse path - the same formula on the kernel's OWN grid (side eps/sqrt(3): two points of a cell are
                    neighbours by construction), summed over the query cells with fewer than min_samples
                    points only.  A denser cell is core without a single distance test and moves nothing
                    but its output; pricing its neighbour tiles is what pushed the round-1 fraction above 1
                    on tower data.  The 27-block of such cells is what a sparse query cell stages before the
                    early exit (every query at min_samples) normally ends the sweep.
    Returns (bytes all cells, bytes sparse path, occupancy summary)."""
    import torch
    n = points.shape[0]
    if n == 0:
        return 0, 0, {}
    total, uniq, cnt, _ = _tile_sum(points, eps, chunk)
    side = eps / 3 ** 0.5 * (1.0 - 2.0 ** -16)
    total_sparse, funiq, fcnt, fmask = _tile_sum(points, side, chunk, lambda c: c < min_samples)
    # occupancy histogram in power-of-two bins [2^k, 2^(k+1)) and the neighbour sums themselves, so that the
    # byte counts can be recomputed: bytes = 12 * neighbour_points + 4 * points
    bins = torch.floor(torch.log2(cnt.double())).long()
    hist = torch.bincount(bins).tolist()
    occ = dict(cells=int(uniq.numel()), max=int(cnt.max()), mean=float(cnt.double().mean()),
               cell_side=eps, hist_log2=hist, neighbour_points=int(total), points=int(n),
               kernel_cell_side=side, kernel_cells=int(funiq.numel()), kernel_cells_sparse=int(fmask.sum()),
               points_in_sparse_kernel_cells=int(fcnt[fmask].sum()),
               neighbour_points_of_sparse_kernel_cells=int(total_sparse))
    return int(12 * total + 4 * n), int(12 * total_sparse + 4 * n), occ


def algorithmic_bytes(name, N, NF):
    """Compulsory HBM bytes of one launch of kernel `name` ("kernels" table)."""
    table = {
        "mean_summary": 16 * N, "sel_hist0": 4 * N, "sel_hist1": 4 * N, "sel_hist2": 4 * N,
        "sel_next": 4 * N, "gf_compact": 4 * N + 8 * NF + 16 * NF,    # z column, x/y of survivors, rows + index out
        # bracketed select: the column once (sel_bracket), a 1/64 sample written and read; with the bracket in place
        # sel_hist0/1/2 and sel_next read the candidates (~1 % of N) instead of the 4 N priced above
        "sel_bracket": 4 * N, "sel_sample": 8 * (N // 64),
        # chunk sort: rows in (12) three times (box sweep, histogram sweep, pass 0), 16-byte rows through the
        # passes, rows + 8-byte keys out, head flags: 100 B per point at 2 passes (keys relative to the chunk's box)
        "db_chunksort": 100 * NF,
        "db_keys": 24 * NF, "db_gather": 44 * NF, "db_cells": 24 * NF, "db_label": 33 * NF,
        "radix_hist": 8 * NF, "radix_scatter": 24 * NF, "scan_reduce": 4 * NF, "scan_apply": 8 * NF,
        "seg_keys": 16 * NF, "seg_perm": 8 * NF, "seg_stats": 16 * NF, "seg_hist": 4 * NF, "seg_scatter": 8 * NF,
        "db_cellstats": 21 * NF,                                       # rows (16) + cell id (4) + core flag (1)
        # serial certified walk over the level-2 summary rows (3 columns x 400 B per 65 536 points):
        # a dependency chain on 3 wavefronts, bounded by latency, not by HBM or MFMA
        "mean_walk": 3 * 400 * (N // 65536 + 1),
        "mean_level2": 3 * 384 * (N // 1024 + 1),                      # one 384-byte record per column and block
    }
    return table.get(name)


HALO = 2 * EPS + 1.0       # tile overlap: 2*eps (exact core flags eps beyond the edge) + the float32 rounding of
                           # EPSG-scale x coordinates (ulp 0.03 m) between the raw frame that cuts the tiles and
                           # the centred frame that is clustered


def launch_ranks(args, argv):
    """--gpus N > 1 without a launcher: start `torch.distributed.run` as a CHILD process - this process has not
    imported torch, let alone touched the GPU - relay rank 0's JSON line and exit with the child's code."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["PCH_BENCH_PARENT_TORCH"] = str("torch" in sys.modules)     # must be False: the parent stays off the GPU
    if env.get("PCH_BENCH_SINGLE_DEVICE") and not env.get("PCH_BENCH_PROBE_RCCL"):
        env.setdefault("PCH_DIST_BACKEND", "gloo")          # RCCL refuses two ranks on one device (PCH_BENCH_PROBE_RCCL=1:
                                                            # let the probe find that out and fall back - a test of it)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout:
        t = ln.strip()
        if t.startswith("{") and '"metric"' in t:
            line = t
        else:
            sys.stderr.write(ln)
    rc = proc.wait()
    if rc == 0 and line is None:
        sys.stderr.write("bench.py: the ranks exited without a result line\n")
        rc = 1
    if line is not None and rc == 0:
        print(line)
    sys.exit(rc)


def dryrun(args):
    """PCH_BENCH_DRYRUN=1: the launcher path without a GPU (tests/test_host.py): every rank joins a gloo group,
    the ranks count themselves with one all_reduce and rank 0 prints a result line.  PCH_BENCH_DRYRUN=fail:<r> makes
    rank r exit with an error instead - the launcher must then exit non-zero without a line."""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    how = os.environ["PCH_BENCH_DRYRUN"]
    if how.startswith("fail:") and int(how[5:]) == rank:
        raise SystemExit(f"rank {rank}: failing on purpose")
    seen = torch.ones(1, dtype=torch.int64)
    if world > 1:
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        dist.all_reduce(seen)
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": "dryrun", "value": 0.0, "n_gpus": world, "ranks_seen": int(seen.item()),
                          "mode": args.mode, "steps": args.steps, "warmup": args.warmup, "full": args.full,
                          "parent_imported_torch": os.environ.get("PCH_BENCH_PARENT_TORCH")}))


def prepare_tiled(points_total, kind, frame, rank, world, dev, seed):
    """this rank's x-tile + halo of the strip corridor (no collective)"""
    import torch
    from pointcloudhookup_amd import synth
    return synth.corridor_tile_torch(points_total, rank, world, HALO, seed=seed, kind=kind, offset=(frame == "offset"),
                                     device=dev, dtype=torch.float32)


def run_tiled(points_total, kind, frame, rank, world, dev, steps, warmup, seed, verify=False, prepared=None,
              dump_dir=None):
    """BASELINE configs[3] on `world` ranks: every rank generates its own x-tile + halo of ONE strip corridor of
    points_total points and runs tiles.tiled_step on it.  Timed like the main loop (barrier + synchronize on both
    sides, max over ranks).  With dump_dir, rank 0 writes its tile's result of the last timed step there
    (dump_outputs).  Returns the result dict on rank 0, None elsewhere."""
    import torch
    import torch.distributed as dist
    from pointcloudhookup_amd import synth, tiles
    import numpy as np
    t = prepared if prepared is not None else prepare_tiled(points_total, kind, frame, rank, world, dev, seed)
    tile, own = t["points"], t["own_range"]
    rows, total = tiles.global_rows(t["local_row"], t["n_own"])
    assert total == points_total, (total, points_total)
    torch.cuda.synchronize()

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    def step(tm=None):
        return tiles.tiled_step(tile, rows, own, total, t["x_lo"], t["x_hi"], EPS, MIN_POINTS, halo=HALO, timings=tm)

    for _ in range(max(warmup, 1)):
        res = step()
    barrier()
    calls_before = dict(tiles.COLLECTIVES)
    trace = {"trace": []} if os.environ.get("PCH_BENCH_TRACE") else None
    t0 = time.perf_counter()
    for _ in range(steps):
        res = step(trace)
    barrier()
    elapsed = time.perf_counter() - t0
    dumped = None
    if dump_dir and rank == 0:                             # labels are defined on the owned rows only
        dumped = dump_outputs(dump_dir,
                              dict(centroid=np.asarray(res["centroid"], np.float32),
                                   threshold=np.array([res["threshold"]], np.float32),
                                   counts=np.array([res["nclusters"], res["used_fallback"], res["survivors"]],
                                                   np.float64)),
                              dict(points=res["points"], rows=res["rows"], own=res["own"],
                                   labels=torch.where(res["own"], res["labels"], -2)),
                              int(res["points"].shape[0]))
    calls = {k: (v - calls_before.get(k, 0)) / steps for k, v in tiles.COLLECTIVES.items() if v - calls_before.get(k, 0)}
    if trace:                                              # host timestamps of every phase of every timed step, per rank
        prev = t0
        for label, ts in trace["trace"]:
            print(f"[trace rank {rank}] {label:18s} +{1e3 * (ts - prev):10.3f} ms", file=sys.stderr)
            prev = ts
    tm = {}
    for _ in range(2):                                     # phase split on two extra steps (adds syncs: not timed above)
        step(tm)
    barrier()
    # the dominant kernel of this rank's step, hipEvent-timed on two more steps (not timed above)
    from pointcloudhookup_amd import ops as _ops
    _ops.set_profiling(True)
    for _ in range(2):
        res_p = step()
    barrier()
    prof_t = sorted(((nm, ms / max(c, 1), c) for nm, ms, c in _ops.get_profile()), key=lambda r: -r[1] * r[2])
    _ops.set_profiling(False)
    tiled_roof = None
    n_own_rows, nf_tile = int(own[1]) - int(own[0]), int(res_p["points"].shape[0])
    for nm, avg_ms, _launches in prof_t:
        b = algorithmic_bytes(nm, n_own_rows if nm.startswith("mean_") else int(tile.shape[0]), nf_tile)
        if b and avg_ms > 0:
            a = b / (avg_ms * 1e-3) / 1e9
            tiled_roof = dict(kernel=nm, bound="hbm", achieved=round(a, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                              frac=round(a / HBM_PEAK_GBS, 4), traffic=None, avg_ms=round(avg_ms, 4),
                              bytes_per_launch=int(b), rows=n_own_rows if nm.startswith("mean_") else int(tile.shape[0]),
                              note="rank 0's tile; hipEvent time on two extra steps; no counter set for this workload")
            break
    del res_p
    phases = torch.tensor([elapsed, tm["filter_ms"] / 2, tm["fit_ms"] / 2, tm["reconcile_ms"] / 2,
                           float(tile.shape[0])], dtype=torch.float64)
    kept_own = torch.tensor([int(res["own"].sum())], dtype=torch.int64)
    if world > 1:
        on_dev = dist.get_backend() == "nccl"
        phases = phases.to(dev) if on_dev else phases
        kept_own = kept_own.to(dev) if on_dev else kept_own
        dist.all_reduce(phases, op=dist.ReduceOp.MAX)
        dist.all_reduce(kept_own, op=dist.ReduceOp.SUM)
    verified = None
    if verify:
        # the check (not timed): rank 0 ALONE builds the whole cloud, runs the single-GPU path over it (fused filter +
        # one global DBSCAN) and compares centroid and threshold bit for bit and every rank's owned labels
        from pointcloudhookup_amd import ops
        o = res["own"]
        mine = (res["rows"][o].cpu(), res["labels"][o].cpu(), res["centroid"], np.float32(res["threshold"]))
        parts = [mine]
        if world > 1:
            parts = [None] * world if rank == 0 else None
            dist.gather_object(mine, parts, dst=0)
        if rank == 0:
            full = torch.cat([synth.corridor_strip_torch(points_total, s, seed, kind, frame == "offset", dev)
                              .to(torch.float32) for s in range(synth.n_strips(points_total))])
            gf = ops.ground_filter(full, want_index=True)
            want, _, k1 = ops.dbscan(gf["points"], EPS, MIN_POINTS, 0)
            want_full = torch.full((full.shape[0],), -2, dtype=torch.int32, device=dev)
            want_full[gf["index"].long()] = want
            seen = torch.zeros(full.shape[0], dtype=torch.int32, device=dev)
            ok = int(res["nclusters"]) == int(k1)
            for rws, lab, cen, thr in parts:
                ok = ok and np.array_equal(np.asarray(cen, np.float32).view(np.uint32), gf["centroid"].view(np.uint32))
                ok = ok and np.float32(thr).view(np.uint32) == np.float32(gf["threshold"]).view(np.uint32)
                ok = ok and bool(torch.equal(lab.to(dev), want_full[rws.to(dev)]))
                seen[rws.to(dev)] += 1
            kept_mask = want_full > -2
            ok = ok and bool(torch.equal(seen, kept_mask.to(torch.int32)))      # every kept row owned exactly once
            verified = bool(ok)
            del full, gf, want, want_full, seen
    if rank != 0:
        return None
    ph = phases.cpu().tolist()
    return {"verified_against_single_gpu_run": verified,
            "workload": f"{points_total / 1e6:g} M-pt strip corridor ({kind}) cut into {world} x-tile(s) + "
                        f"{HALO:g} m halo, chained float32 centroid + shared percentile + filter + global "
                        f"DBSCAN(eps={EPS:g}, min_samples={MIN_POINTS}) per tile + cross-tile label reconciliation "
                        "(BASELINE configs[3] at 400 M / 8 GPUs)",
            "points_total": int(points_total), "ranks_seen": int(dist.get_world_size()) if world > 1 else 1,
            "backend": tiles.exchange_backend(), "roofline": tiled_roof,
            "kernels_rank0": [dict(name=nm, avg_ms=round(ms, 4), launches=c // 2) for nm, ms, c in prof_t[:8]],
            "collectives_per_step_rank0": calls, "collectives_per_step_rank0_total": round(sum(calls.values()), 2),
            "forced_collectives": bool(os.environ.get("PCH_TILES_FORCE_COLLECTIVES") == "1"),
            "devices": "one GPU shared by all ranks (rehearsal)" if os.environ.get("PCH_BENCH_SINGLE_DEVICE") else "one GPU per rank",
            "steps": steps, "ms_per_step": round(1e3 * ph[0] / steps, 3), "dump_outputs": dumped,
            "Mpts_per_s": round(points_total * steps / ph[0] / 1e6, 1),
            "phase_ms_max_over_ranks": {"centroid_chain+threshold+filter": round(ph[1], 3),
                                        "local_fit": round(ph[2], 3), "reconciliation": round(ph[3], 3)},
            "largest_tile_points": int(ph[4]), "kept_points": int(kept_own.item()),
            "clusters": int(res["nclusters"]), "used_fallback": bool(res["used_fallback"]),
            "centroid": [float(v) for v in res["centroid"]], "threshold": float(res["threshold"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", default="stream", choices=["stream", "tiled"])
    ap.add_argument("--points", type=int, default=None,
                    help="stream: points per GPU (default 100 M); tiled: points of the WHOLE cloud (default 400 M)")
    ap.add_argument("--verify", action="store_true",
                    help="tiled runs: rank 0 rebuilds the whole cloud, runs the single-GPU path and checks centroid, "
                         "threshold and every rank's owned labels against it (not timed)")
    ap.add_argument("--full", action="store_true",
                    help="stream mode: also the kNN byte models, the counter figures, the config-4 side run, the side "
                         "measurements and the CPU baseline (a plain run times the steps and prints the line only)")
    ap.add_argument("--tiled-points-per-gpu", type=int, default=50_000_000,
                    help="size of the config-4 side run of the default mode with --full (x world = its cloud)")
    ap.add_argument("--kind", default="corridor", choices=["corridor", "uniform"])
    ap.add_argument("--frame", default="offset", choices=["offset", "local"],
                    help="offset: EPSG:4547-scale coordinates like the reference's data (default); "
                         "local: corridor starts at the origin")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-tile-stream", action="store_true",
                    help="--full without the two-tiles-in-flight side measurement (profiling runs)")
    ap.add_argument("--no-side", action="store_true",
                    help="--full without any side measurement (voxel stage, other workloads): profiling runs")
    ap.add_argument("--no-e2e", action="store_true",
                    help="--full without the 100 M-point LAS file run through the drop-ins")
    ap.add_argument("--e2e-points", type=int, default=100_000_000)
    ap.add_argument("--las", default=None,
                    help="BASELINE config 5 (--full): a real .las file run end to end through the drop-in modules "
                         "(voxel downsample -> extract_towers); reported as a side value, 'skipped' without a file")
    ap.add_argument("--cpu-budget-s", type=float, default=20.0)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (rank 0) as DIR/<name>.npy, "
                         f"at most {DUMP_BUDGET_BYTES >> 20} MB; per-point outputs above {DUMP_SAMPLE_ROWS} rows as a "
                         "fixed, seeded sample of rows")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.points is None:
        args.points = 100_000_000 if args.mode == "stream" else 400_000_000
    env_world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "RANK" not in os.environ:
        launch_ranks(args, sys.argv[1:])                     # never returns
    if env_world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={env_world}: start it either plainly "
                         f"(it launches its own ranks) or under torch.distributed.run with --nproc-per-node {args.gpus}")
    if os.environ.get("PCH_BENCH_SINGLE_DEVICE") and env_world > 3 and not os.environ.get("PCH_BENCH_ALLOW_STALLS"):
        # a rehearsal mode (ranks sharing one device over gloo).  From four processes on, this platform stalls ALL
        # device work of all of them for seconds at a time (profiles/r03_shared_device_stalls.txt, DESIGN.md
        # section 9): results stay correct, timings are meaningless - refused before any GPU work
        raise SystemExit("bench.py: PCH_BENCH_SINGLE_DEVICE supports at most 3 ranks on the one device "
                         "(PCH_BENCH_ALLOW_STALLS=1 overrides)")

    if os.environ.get("PCH_BENCH_DRYRUN"):
        return dryrun(args)

    import torch
    import torch.distributed as dist
    from pointcloudhookup_amd import ops, pipeline, synth, tiles

    rank, world, local = tiles.init_from_env(timeout_s=600, single_device=bool(os.environ.get("PCH_BENCH_SINGLE_DEVICE")))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    if os.environ.get("PCH_BENCH_SINGLE_DEVICE"):           # rehearsal of the N>1 path on a 1-GPU box
        local = 0
    elif torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py: {world} ranks but {torch.cuda.device_count()} GPU(s) visible "
                         "(PCH_BENCH_SINGLE_DEVICE=1 rehearses up to 3 ranks on one device over gloo)")
    dev = torch.device(f"cuda:{local}")
    torch.cuda.set_device(dev)
    if args.mode == "tiled":                                 # BASELINE configs[3]: the whole line is the tiled run
        seed = synth.SEED0 + 3
        ops.set_profiling(False)
        res = run_tiled(int(args.points), args.kind, args.frame, rank, world, dev, args.steps, args.warmup, seed,
                        verify=args.verify, dump_dir=args.dump_outputs)
        if rank == 0 and res.get("verified_against_single_gpu_run") is False:
            print(json.dumps({"error": "tiled labels differ from the single-GPU run", "tiled": res}), file=sys.stderr)
            if world > 1:
                dist.destroy_process_group()
            raise SystemExit(4)
        if rank == 0:
            out = {"metric": "Mpts/s ground-filter+tower-cluster, 100 M-pt corridor; % HBM roofline on kNN",
                   "value": res["Mpts_per_s"], "unit": "Mpts/s", "n_gpus": world, "steps": args.steps,
                   "warmup": args.warmup, "ms_per_step": res["ms_per_step"], "higher_is_better": True,
                   "scaling": "strong", "vs_baseline": None, "dtype": "f32 (filter) + f64 (distance predicate)",
                   "data": "synthetic",
                   "config": {"workload": res["workload"], "points_total": res["points_total"],
                              "frame": "global-offset (+437000,+3139000,+80)" if args.frame == "offset" else "local",
                              "seed": seed, "parallelism": f"x-tiles x{world}"},
                   "tiled": res, "roofline": res.get("roofline"), "cpu_baseline": None,
                   "dump_outputs": res.get("dump_outputs"),
                   "note": "cpu_baseline is carried by the --full line of the default mode (--mode stream)"}
            print(json.dumps(out))
        if world > 1:
            dist.destroy_process_group()
        return
    N = int(args.points)
    seed = synth.SEED0 + 2 + rank
    raw = synth.corridor_torch(N, seed=seed, kind=args.kind, offset=(args.frame == "offset"), device=dev,
                               dtype=torch.float32)
    torch.cuda.synchronize()

    def step():
        cl = pipeline.cluster_points(raw, EPS, MIN_POINTS, CHUNK)
        if world > 1:
            off, total, table, owner = tiles.reconcile(cl["nclusters"], cl["stats"])
            cl["label_offset"], cl["global_clusters"] = off, total
        return cl

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    # warm-up steps are profiled in full to learn which kernels matter; the timed steps then record
    # hipEvents only around those (two event records per launch are not free on the host)
    ops.set_profiling(True)
    for _ in range(max(args.warmup, 1)):
        cl = step()
    barrier()
    warm = sorted(ops.get_profile(), key=lambda r: -r[1])
    keep = [r[0] for r in warm[:10]]
    for must in ("db_core", "mean_summary", "mean_walk"):
        if must not in keep:
            keep.append(must)
    warm_ms = {r[0]: r[1] / max(args.warmup, 1) for r in warm}
    ops.set_profiling(True, only=keep)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        cl = step()
    barrier()
    elapsed = time.perf_counter() - t0
    prof = ops.get_profile()
    ops.set_profiling(False)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device="cpu" if dist.get_backend() == "gloo" else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    NF = int(cl["ground"]["count"])
    K = int(cl["nclusters"])
    dumped = None
    if args.dump_outputs and rank == 0:
        g = cl["ground"]
        counts = [NF, K, g["count_at_offset"], g["used_fallback"]]
        if world > 1:
            counts += [cl["label_offset"], cl["global_clusters"]]
        dumped = dump_outputs(args.dump_outputs,
                              dict(centroid=g["centroid"], base_threshold=np.array([g["base"], g["threshold"]], np.float32),
                                   aabb=g["aabb"], counts=np.array(counts, np.float64), offsets=cl["offsets"],
                                   stats=cl["stats"]),
                              dict(points=g["points"], labels=cl["labels"], perm=cl["perm"]), NF)

    # ---- config-4 side run (--full, every rank takes part): ONE cloud of world x tiled-points-per-gpu points
    tiled_res = None
    if args.full and not args.no_side and args.tiled_points_per_gpu > 0:
        # Only what can fail BEFORE the first collective is caught per rank (building the tile: memory); whether every
        # rank got that far is agreed over the default group, so either all ranks enter tiled_step or none does.  An
        # error inside the collective phase propagates: the launcher then exits non-zero at once instead of leaving
        # the other ranks in an all_gather until its timeout.
        tile_args = None
        try:
            tile_args = prepare_tiled(int(args.tiled_points_per_gpu) * world, args.kind, args.frame, rank, world, dev,
                                      synth.SEED0 + 3)
            why = ""
        except Exception as e:
            why = f"rank {rank}: {type(e).__name__}: {e}"
        ok = torch.tensor([0 if why else 1], dtype=torch.int64,
                          device=dev if (world > 1 and dist.get_backend() == "nccl") else "cpu")
        if world > 1:
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 1:
            tiled_res = run_tiled(int(args.tiled_points_per_gpu) * world, args.kind, args.frame, rank, world, dev,
                                  max(3, min(args.steps, 10)), 2, synth.SEED0 + 3, verify=args.verify, prepared=tile_args)
        else:
            tiled_res = {"error": why or "another rank could not build its tile"}
        del tile_args

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    ms_per_step = 1e3 * elapsed / args.steps
    value = N * world * args.steps / elapsed / 1e6

    # ---- per-kernel times from the library's own hipEvents (timed region only)
    kernels = sorted(((n, ms / max(c, 1), c, ms / args.steps) for n, ms, c in prof),
                     key=lambda r: -r[3])
    timed = {r[0] for r in kernels}
    gpu_ms = sum(r[3] for r in kernels) + sum(v for k, v in warm_ms.items() if k not in timed)
    # the kNN byte models take two cell sweeps of their own over the kept points: --full only (without them the kNN
    # kernels have no roofline)
    knn_bytes_all, knn_bytes, occ = (knn_tile_bytes(cl["ground"]["points"], EPS, CHUNK, MIN_POINTS) if args.full
                                     else (None, None, None))
    dom = kernels[0]

    def roof(name, avg_ms, per_step=1.0):
        # a kernel that is launched several times per step over consecutive parts of the tile (mean_summary in slices):
        # algorithmic bytes per LAUNCH = the step's bytes / launches per step, against the average launch duration
        if name in ("db_core", "db_union", "db_border"):
            b = knn_bytes
        else:
            b = algorithmic_bytes(name, N, NF)
        if b is None or avg_ms <= 0:
            return None
        b = b / max(per_step, 1.0)
        a = b / (avg_ms * 1e-3) / 1e9
        r = dict(kernel=name, bound="hbm", achieved=round(a, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                 frac=round(a / HBM_PEAK_GBS, 4), traffic=None, avg_ms=round(avg_ms, 4),
                 bytes_per_launch=int(b))
        if per_step > 1.0:
            r["launches_per_step"] = per_step
        return r

    roofline = roof(dom[0], dom[1], dom[2] / args.steps) or dict(kernel=dom[0], bound="hbm", achieved=None,
                                                                 peak=HBM_PEAK_GBS, unit="GB/s", frac=None, traffic=None)
    knn = next((roof(r[0], r[1], r[2] / args.steps) for r in kernels if r[0] == "db_core"), None)
    if knn:
        # The radius kernel is not bound by HBM: its figure of merit is
        # pair tests per second.  The byte MODELS of SURVEY 8(d) stay in the line, after the counter-based figures,
        # labelled as models: they price L2/LDS-resident tile reuse as HBM bytes, which the counters show never moved.
        knn = {"kernel": "db_core", "avg_ms": knn["avg_ms"],
               "bound": "not HBM: vector-ALU issue on sparse data, load latency where few cells reach the test path "
                        "(see valu_issue_frac_measured / wave_wait_frac_measured)",
               "hbm_model": {"note": "SURVEY 8d tile formula, NOT measured traffic: 12*sum of the points of the "
                                     "occupied neighbour cells + 4*N_f; 'sparse_cells' = on the kernel's own grid "
                                     "(side eps/sqrt(3)) over the query cells below min_samples only, 'all_cells' = "
                                     "as written (side eps, every cell)",
                             "bytes_sparse_cells": int(knn_bytes), "frac_sparse_cells": knn["frac"],
                             "bytes_all_cells": int(knn_bytes_all),
                             "frac_all_cells": round(knn_bytes_all / (knn["avg_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}}
        if world == 1 and not args.no_side:
            try:                                         # the same fit once more in the counting variant of the kernel
                ops.set_pair_counting(True)
                fitc = ops.DbscanFit(cl["ground"]["points"], EPS, MIN_POINTS, CHUNK, aabb=cl["ground"]["aabb"])
                st = fitc.pair_stats()
                same = bool(torch.equal(fitc.labels, cl["labels"]))
                del fitc
                t_s = knn["avg_ms"] * 1e-3
                lane_rate = 1024 * 16 * 2.4e9              # SIMDs x lanes per clock x max clock (MI355X_MICROARCH.md)
                knn.update({
                    "pair_tests": st["pair_tests"], "lane_slots_issued": st["lane_slots"],
                    "lane_utilisation": round(st["pair_tests"] / max(st["lane_slots"], 1), 4),
                    "cells_on_the_test_path": st["cells_tested"], "lds_tiles_staged": st["tiles_staged"],
                    "pair_tests_per_s": round(st["pair_tests"] / t_s, 1),
                    "lane_slots_per_s": round(st["lane_slots"] / t_s, 1),
                    "valu_peak_lane_instr_per_s": lane_rate,
                    "valu_instr_per_test_model": 7,
                    "frac_valu_model": round(st["lane_slots"] * 7 / lane_rate / t_s, 4),
                    "counting_variant_labels_identical": same,
                    "pair_tests_note": "counted by the kernel's counting variant (same control flow, "
                                       "pch_dbscan_set_pair_counting) on the timed tile; rates use the plain kernel's "
                                       "hipEvent time; frac_valu_model = issued lane slots x 7 vector instructions per "
                                       "test / (1024 SIMDs x 16 lanes x 2.4 GHz); the measured issue occupancy is "
                                       "`valu_issue_frac_measured` (SQ_INSTS_VALU, profiles/)"})
            except Exception as e:
                knn["pair_tests_error"] = f"{type(e).__name__}: {e}"
            finally:
                ops.set_pair_counting(False)
    if roofline.get("kernel") == "mean_walk":
        roofline["note"] = ("largest kernel by time is the exact-centroid walk: a serial dependency chain on "
                            "3 wavefronts (latency-bound); see streaming_kernel for the largest HBM-bound kernel")
    stream = next((roof(r[0], r[1], r[2] / args.steps) for r in kernels
                   if r[0] not in ("mean_walk", "db_core", "db_union0", "db_union1", "db_border")
                   and algorithmic_bytes(r[0], N, NF)), None)
    tr_path = os.path.join(ROOT, "profiles", "traffic.json")   # PMC passes, see profiles/README.md
    step_traffic = None
    traffic_dropped = None
    if args.full and os.path.exists(tr_path):
        try:
            tr = json.load(open(tr_path)).get("workloads", {}).get(f"{args.kind}/{args.frame}/{N}")
            sys.path.insert(0, os.path.join(ROOT, "profiles"))
            from stamp import csrc_sha
            here_sha = csrc_sha()
            if tr and tr.get("csrc_sha") != here_sha:
                # counters of OTHER kernel sources: never paired with this run's times
                traffic_dropped = (f"profiles/traffic.json[{args.kind}/{args.frame}/{N}] (set {tr.get('source')}) was collected "
                                   f"on kernel sources {tr.get('csrc_sha')}, this run is {here_sha}: every counter-based "
                                   "figure (traffic, frac_traffic, valu_issue_frac_measured, step_traffic) is left out")
                tr = None
            for r in (roofline, knn, stream):     # counters of the SAME workload (kind / frame / points) only
                if r and tr and r["kernel"] in tr.get("kernels", {}):
                    r["traffic"] = tr["kernels"][r["kernel"]]
                    r["traffic_source"] = f"profiles/{tr.get('source')}_pmc_traffic.csv"
                    r["frac_traffic"] = round(r["traffic"] / (r["avg_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                if r and tr and r["kernel"] in tr.get("sq", {}):
                    sqk = tr["sq"][r["kernel"]]
                    r["valu_issue_frac_measured"] = sqk.get("valu_issue_frac")
                    if sqk.get("SQ_WAVE_CYCLES"):
                        r["wave_wait_frac_measured"] = round(sqk.get("SQ_WAIT_ANY", 0) / sqk["SQ_WAVE_CYCLES"], 4)
                    r["sq_source"] = f"profiles/{tr.get('source')}_sq_counters.csv"
            if tr and tr.get("step_bytes"):
                # every kernel of one step, from the counter passes, against what one step must move at least:
                # the tile once (12 B/pt) + the z column written and read (8) + per kept point the row out (12), the
                # sorted copy written and read (32), labels (4) and the grouped index (4)
                compulsory = 20 * N + 52 * NF
                step_traffic = {"bytes_per_step": tr["step_bytes"], "compulsory_bytes_per_step": compulsory,
                                "amplification": round(tr["step_bytes"] / compulsory, 3),
                                "achieved_GBps": round(tr["step_bytes"] / (ms_per_step * 1e-3) / 1e9, 1),
                                "frac_of_hbm_peak": round(tr["step_bytes"] / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                "launches_per_step_profiled": tr.get("launches_per_step"),
                                "source": f"profiles/{tr.get('source')}_pmc_traffic.csv (all pch kernels, "
                                          "2*FETCH_SIZE + WRITE_SIZE)"}
        except Exception:
            pass
    if knn and knn.get("traffic") is not None:
        knn["hbm_counters"] = {"bytes": knn.pop("traffic"), "frac_of_hbm_peak": knn.pop("frac_traffic"),
                               "source": knn.pop("traffic_source")}

    out = {
        "metric": "Mpts/s ground-filter+tower-cluster, 100 M-pt corridor; % HBM roofline on kNN",
        "value": round(value, 2), "unit": "Mpts/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32 (filter) + f64 (distance predicate)",
        "data": "synthetic",
        "config": {"workload": f"{N / 1e6:g} M-pt synthetic {args.kind}, ground filter + chunked "
                               f"DBSCAN(eps={EPS:g}, min_samples={MIN_POINTS}, chunk={CHUNK}) + label "
                               "grouping, 1 tile per GPU (BASELINE configs[2])",
                   "points_per_gpu": N, "frame": "global-offset (+437000,+3139000,+80)" if args.frame == "offset" else "local",
                   "filtered_points": NF, "clusters": K, "seed": seed},
        "roofline": roofline,
        "streaming_kernel": stream,
        "knn_kernel": knn,
        "gpu_kernel_ms_per_step": round(gpu_ms, 3),
        "kernels_note": "hipEvent-timed inside the timed steps: the 10 heaviest kernels of the warm-up step "
                        "(+ db_core / mean_*); gpu_kernel_ms_per_step adds the warm-up times of the rest",
        "kernels": [dict(name=r[0], avg_ms=round(r[1], 4), launches_per_step=r[2] / args.steps,
                         ms_per_step=round(r[3], 4)) for r in kernels[:12]],
        "knn_cell_occupancy": occ,
        "step_traffic": step_traffic,
        "counter_figures_dropped": traffic_dropped,
        "tiled": tiled_res,
        "dump_outputs": dumped,
    }

    # ---- side measurements (--full; none of them in `value`)
    if world == 1 and args.full and not args.no_side:
        def timed_steps(tile, k):
            pipeline.cluster_points(tile, EPS, MIN_POINTS, CHUNK)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                c2 = pipeline.cluster_points(tile, EPS, MIN_POINTS, CHUNK)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / k, c2

        # the other workloads of SURVEY 8d on the same harness: the local (zero-offset) frame and the uniform cloud - and
        # the worst case of the exact centroid, the corridor centred on itself
        others = {}
        for kind, frame in (("corridor", "local" if args.frame == "offset" else "offset"), ("uniform", args.frame),
                            ("corridor", "centred")):
            if kind == args.kind and frame == args.frame:
                continue
            try:
                tile = synth.corridor_torch(N, seed=seed, kind=kind, offset=(frame == "offset"), device=dev,
                                            dtype=torch.float32)
                if frame == "centred":      # a cloud normalised to its own centre: zero-mean columns, the float32
                    tile = tile - tile.double().mean(dim=0).float()   # running sums wander about zero all file long
                dt2, c2 = timed_steps(tile, 3)
                others[f"{kind}/{frame}"] = {"ms_per_step": round(dt2 * 1e3, 3), "Mpts_per_s": round(N / dt2 / 1e6, 1),
                                             "filtered_points": int(c2["ground"]["count"]), "clusters": int(c2["nclusters"])}
                del tile, c2
            except Exception as e:
                others[f"{kind}/{frame}"] = {"error": str(e)}
        out["other_workloads"] = others

        # the same step with the tile handed over as a HOST buffer: pinned host tile -> device -> one step (BASELINE.md
        # section 3, "Mpts/s (GPU incl. H2D)"); never the headline value
        try:
            host_tile = torch.empty((N, 3), dtype=torch.float32, pin_memory=True)
            host_tile.copy_(raw)
            dev_tile = torch.empty_like(raw)
            torch.cuda.synchronize()
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                dev_tile.copy_(host_tile, non_blocking=True)
                c2 = pipeline.cluster_points(dev_tile, EPS, MIN_POINTS, CHUNK)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            dev_tile.copy_(host_tile, non_blocking=True)
            torch.cuda.synchronize()
            t_copy = time.perf_counter() - t0
            out["h2d_inclusive"] = {"ms_per_step": round(1e3 * min(times), 3), "Mpts_per_s": round(N / min(times) / 1e6, 1),
                                    "h2d_ms": round(1e3 * t_copy, 3), "h2d_GBps": round(12 * N / t_copy / 1e9, 1),
                                    "clusters": int(c2["nclusters"]),
                                    "note": "pinned host float32 [N,3] -> device copy -> one step, best of 3; measured, "
                                            "not the reported value (the input of `value` is resident in HBM)"}
            del host_tile, dev_tile, c2
        except Exception as e:
            out["h2d_inclusive"] = {"error": f"{type(e).__name__}: {e}"}

        # stage D1-D3 on the clusters of the timed tile (host: per-cluster oriented boxes; SURVEY 8f "next"):
        # exact mode through the worker pool (one worker per usable core, shared-memory hand-off), with its split
        try:
            from pointcloudhookup_amd import obb as _obbm
            t0 = time.perf_counter()
            towers = pipeline.tower_table(cl)
            first_ms = (time.perf_counter() - t0) * 1e3
            best_ms, split, spaced, packed = None, None, [], []
            quota = _obbm.cpu_quota()
            for i in range(8):                      # five calls a quota period apart, then three back to back
                if i < 5:
                    time.sleep(0.15 if quota is None else 1.5 * quota[1])
                tm = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                towers = pipeline.tower_table(cl, timings=tm)
                ms = (time.perf_counter() - t0) * 1e3
                (spaced if i < 5 else packed).append(round(ms, 1))
                if best_ms is None or ms < best_ms:
                    best_ms, split = ms, tm
            out["tower_table"] = {"ms": round(best_ms, 1), "ms_median_spaced": sorted(spaced)[2],
                                  "ms_runs_spaced": spaced, "ms_runs_back_to_back": packed,
                                  "first_call_ms": round(first_ms, 1),
                                  "clusters": K, "towers": len(towers), "obb_workers": _obbm.pool().size(),
                                  "usable_cpus": _obbm.usable_cpus(), "os_cpu_count": os.cpu_count(),
                                  "cpu_quota": None if quota is None else {"cores": quota[0], "period_s": quota[1]},
                                  "split_ms": {k: (round(v, 2) if isinstance(v, float) else v) for k, v in split.items()},
                                  "note": "host stage D1-D3, exact mode, `ms` = best of 8: the clustered points are gathered "
                                          "on the device and copied once into a shared, HIP-registered memfd buffer; worker "
                                          "processes map it and box their clusters (qhull on the cluster minus the rows "
                                          "inside its initial simplex, candidate directions priced by libpch_obbhost.so, "
                                          "winner in python), tasks and answers are a few dozen bytes.  Under a cgroup CPU "
                                          "quota (`cpu_quota`) the pool holds 2 workers per quota core and spends one "
                                          "period's budget at that parallelism: a call that finds the budget untouched "
                                          "(`ms_runs_spaced`, one period of quiet before each - the drop-in's single call) "
                                          "is faster than calls back to back (`ms_runs_back_to_back`), which run at the "
                                          "quota's pace like `stream_with_tower_table`; the first call also starts the "
                                          "workers (~1 s of scipy imports, which the drop-in hides behind the file read); "
                                          "outside the timed region"}
            # tile stream WITH the tower table: the boxes of tile k are computed by the pool while the device
            # clusters tile k+1 (same resident tile each time; at most three tables in flight)
            try:
                ntiles = 8
                pipeline.cluster_points(raw, EPS, MIN_POINTS, CHUNK)
                torch.cuda.synchronize()
                jobs, done_towers = [], []
                t0 = time.perf_counter()
                for _ in range(ntiles):
                    c2 = pipeline.cluster_points(raw, EPS, MIN_POINTS, CHUNK)
                    jobs.append(pipeline.tower_table_async(c2))
                    del c2
                    while len(jobs) > 2:
                        done_towers.append(len(jobs.pop(0).result()))
                t_dev = time.perf_counter() - t0
                while jobs:
                    done_towers.append(len(jobs.pop(0).result()))
                dts = time.perf_counter() - t0
                out["stream_with_tower_table"] = {
                    "tiles": ntiles, "points_per_tile": N, "ms_per_tile": round(1e3 * dts / ntiles, 2),
                    "Mpts_per_s": round(N * ntiles / dts / 1e6, 1), "towers_per_tile": done_towers,
                    "ms_until_last_tile_clustered": round(1e3 * t_dev, 2),
                    "note": "filter + cluster + grouping on the device AND the tower table (exact mode) per tile; "
                            "the table of tile k runs in the worker pool beside the device work of tile k+1, so the "
                            "rate is the pool's (hull CPU seconds per tile / usable cores)"}
            except Exception as e:
                out["stream_with_tower_table"] = {"error": f"{type(e).__name__}: {e}"}
            # the same table in fast mode (device pre-filter + native candidate search), twice: the first call
            # pays one-off allocations; centre / extent deltas of the towers both modes accept
            try:
                pipeline.tower_table(cl, obb_mode="fast")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fast = pipeline.tower_table(cl, obb_mode="fast")
                ms_fast = (time.perf_counter() - t0) * 1e3
                ex = {t["label"]: t for t in towers}
                both = [(ex[t["label"]], t) for t in fast if t["label"] in ex]
                dc = sorted(float(np.abs(a["center"] - b["center"]).max()) for a, b in both)
                de = sorted(float(np.abs(np.asarray(a["extent"]) - np.asarray(b["extent"])).max()) for a, b in both)
                out["tower_table_fast"] = {
                    "ms": round(ms_fast, 1), "towers": len(fast), "towers_in_both": len(both),
                    "centre_delta_m": {"median": dc[len(dc) // 2] if dc else None, "max": dc[-1] if dc else None,
                                       "above_1e-3": sum(d > 1e-3 for d in dc)},
                    "extent_delta_m": {"median": de[len(de) // 2] if de else None, "max": de[-1] if de else None},
                    "note": "opt-in (PCH_OBB_MODE=fast): pch_obb_shell_f32 + qhull on the kept ~1 % (in the worker "
                            "processes the exact mode started) + pch_obb_min_boxes_f64; exact mode stays the default"}
            except Exception as e:
                out["tower_table_fast"] = {"error": str(e)}
        except Exception as e:
            out["tower_table"] = {"error": str(e)}

        # BASELINE config 2: the voxel stage on 10 M float64 points, and the drop-ins end to end on a LAS file
        # of that cloud (LAS in -> voxel LAS out -> tower dicts out, wall clock incl. file I/O)
        try:
            nv = 10_000_000
            xyz64 = synth.corridor_torch(nv, seed=synth.SEED0 + 1, kind="corridor", offset=True, device=dev)
            ops.voxel_downsample(xyz64, 0.2, 500000)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                vi, vm, vc, vo = ops.voxel_downsample(xyz64, 0.2, 500000)
            torch.cuda.synchronize()
            dtv = (time.perf_counter() - t0) / 3
            out["voxel_stage"] = {"points": nv, "voxel": 0.2, "chunk": 500000, "voxels_out": int(vi.shape[0]),
                                  "ms": round(dtv * 1e3, 3), "Mpts_per_s": round(nv / dtv / 1e6, 1)}
            del vi, vm, vc, vo
            import tempfile
            from pointcloudhookup_amd import las as _las
            from pointcloudhookup_amd.ui import import_PC as _imp
            from pointcloudhookup_amd.utils import tower_extraction as _te
            with tempfile.TemporaryDirectory(prefix="pch_bench_") as td:
                sc, of = np.array([0.001, 0.001, 0.001]), np.array([437000.0, 3139000.0, 0.0])
                src = os.path.join(td, "cloud.las")
                _las.write_device(src, _las.LasHeader(point_format=3, version=(1, 2), scales=sc, offsets=of),
                                  ops.las_unscale(xyz64, sc, of))
                del xyz64
                cwd = os.getcwd()
                os.chdir(td)
                try:
                    t0 = time.perf_counter()
                    _imp.run_voxel_downsampling(src, os.path.join(td, "output", "point_2.las"), 0.2, 500000)
                    t1 = time.perf_counter()
                    tw = _te.extract_towers(os.path.join(td, "output", "point_2.las"), log_callback=lambda m: None)
                    t2 = time.perf_counter()
                finally:
                    os.chdir(cwd)
                out["dropin_end_to_end"] = {"points": nv, "run_voxel_downsampling_s": round(t1 - t0, 3),
                                            "extract_towers_s": round(t2 - t1, 3), "towers": len(tw),
                                            "note": "wall clock, LAS files in and out (config 2 cloud)"}
        except Exception as e:
            out.setdefault("voxel_stage", {"error": str(e)})
            out["dropin_end_to_end"] = {"error": str(e)}

    # ---- the drop-ins end to end at the HEADLINE size and the GUI's own settings (voxel 0.1 m, 500 000-row chunks:
    # pyGUI_towers_test.py:351-358): a 100 M-point format-3 LAS file (3.4 GB, warm page cache) through
    # run_voxel_downsampling, then extract_towers on its output, each with a per-stage wall-clock table
    if world == 1 and args.full and not args.no_side and not args.no_e2e:
        try:
            import shutil
            import tempfile
            from pointcloudhookup_amd import las as _las, stages as _stages
            from pointcloudhookup_amd.ui import import_PC as _imp
            from pointcloudhookup_amd.utils import tower_extraction as _te
            ne = int(args.e2e_points)
            td = tempfile.mkdtemp(prefix="pch_e2e_")
            try:
                if shutil.disk_usage(td).free < 8 * 34 * ne // 4:
                    raise RuntimeError(f"not enough free space under {td}")
                sc, of = np.array([0.001, 0.001, 0.001]), np.array([437000.0, 3139000.0, 0.0])
                src = os.path.join(td, "cloud.las")
                xyz64 = synth.corridor_torch(ne, seed=synth.SEED0 + 5, kind="corridor", offset=True, device=dev)
                ints = ops.las_unscale(xyz64, sc, of)
                del xyz64
                t0 = time.perf_counter()
                _las.write_device(src, _las.LasHeader(point_format=3, version=(1, 2), scales=sc, offsets=of), ints)
                t_write_src = time.perf_counter() - t0
                del ints
                torch.cuda.empty_cache()
                size_in = os.path.getsize(src)
                cwd = os.getcwd()
                os.chdir(td)
                out_las = os.path.join(td, "output", "point_2.las")
                import hashlib

                def file_sha(path):
                    h = hashlib.sha256()
                    with open(path, "rb") as f:
                        for blk in iter(lambda: f.read(1 << 24), b""):
                            h.update(blk)
                    return h.hexdigest()

                def fresh():                                 # truncating 2.9 GB of cached pages is not part of a run
                    if os.path.exists(out_las):
                        os.unlink(out_las)
                    torch.cuda.synchronize()

                try:
                    # warm-up of everything that is paid once per process (worker pool, pinned rings, allocator)
                    _imp.run_voxel_downsampling(src, out_las, 0.1, 500000)
                    _te.extract_towers(out_las, log_callback=lambda m: None)
                    # (a) background writer + records handed over on the device, no stage timers (they drain the device
                    # at every stage edge): run_voxel_downsampling returns once the records exist, extract_towers
                    # takes them from the device and joins the writer before it returns
                    fresh()
                    _imp.ASYNC_WRITE = True
                    ta0 = time.perf_counter()
                    _imp.run_voxel_downsampling(src, out_las, 0.1, 500000)
                    ta1 = time.perf_counter()
                    twa = _te.extract_towers(out_las, log_callback=lambda m: None)
                    ta2 = time.perf_counter()
                    sha_async = file_sha(out_las)
                    _imp.ASYNC_WRITE = False
                    # (b) the default: writer in the foreground, records still handed over on the device
                    fresh()
                    tb0 = time.perf_counter()
                    _imp.run_voxel_downsampling(src, out_las, 0.1, 500000)
                    tb1 = time.perf_counter()
                    twb = _te.extract_towers(out_las, log_callback=lambda m: None)
                    tb2 = time.perf_counter()
                    sha_sync = file_sha(out_las)
                    # (c) as in round 3: no hand-over (the file is read back), stage timers on
                    os.environ["PCH_RESIDENT_HANDOFF"] = "0"
                    _stages.enable(True)
                    fresh()
                    t0 = time.perf_counter()
                    _imp.run_voxel_downsampling(src, out_las, 0.1, 500000)
                    t1 = time.perf_counter()
                    tw = _te.extract_towers(out_las, log_callback=lambda m: None)
                    t2 = time.perf_counter()
                    sha_plain = file_sha(out_las)
                finally:
                    _imp.ASYNC_WRITE = False
                    os.environ.pop("PCH_RESIDENT_HANDOFF", None)
                    _stages.enable(False)
                    os.chdir(cwd)
                size_mid = os.path.getsize(out_las)
                hv = _las.read_header_native(out_las)
                sv = {k: round(v, 4) for k, v in (_stages.last("run_voxel_downsampling") or {}).items()}
                se = {k: round(v, 4) for k, v in (_stages.last("extract_towers") or {}).items()}
                rd = sv.get("read LAS -> device int32 (file, H2D, decode)")
                out["dropin_end_to_end_100m"] = {
                    "points_in": ne, "las_bytes_in": size_in, "voxel": 0.1, "chunk": 500000,
                    "voxels_out": int(hv.point_count), "las_bytes_between": size_mid, "towers": len(tw),
                    "run_voxel_downsampling_s": round(tb1 - tb0, 3), "extract_towers_s": round(tb2 - tb1, 3),
                    "Mpts_per_s_file_to_dicts": round(ne / (ta2 - ta0) / 1e6, 1),
                    "headline_keys_note": "run_voxel_downsampling_s / extract_towers_s: the default configuration "
                                          "(foreground writer, records handed over on the device); "
                                          "Mpts_per_s_file_to_dicts: the opt-in background writer; all three "
                                          "configurations under file_to_dicts; the stage tables below are the round-3 "
                                          "path (file read back) with the device drained at every stage edge",
                    "file_to_dicts": {
                        "background_writer+device_handoff": {
                            "run_voxel_downsampling_s": round(ta1 - ta0, 3), "extract_towers_s": round(ta2 - ta1, 3),
                            "Mpts_per_s": round(ne / (ta2 - ta0) / 1e6, 1), "towers": len(twa),
                            "note": "import_PC.ASYNC_WRITE (PCH_ASYNC_LAS_WRITE=1): opt-in, because an unchanged caller "
                                    "may open the file with its own reader as soon as run_voxel_downsampling returns"},
                        "default: foreground_writer+device_handoff": {
                            "run_voxel_downsampling_s": round(tb1 - tb0, 3), "extract_towers_s": round(tb2 - tb1, 3),
                            "Mpts_per_s": round(ne / (tb2 - tb0) / 1e6, 1), "towers": len(twb)},
                        "round 3 path: file read back (PCH_RESIDENT_HANDOFF=0), stage timers on": {
                            "run_voxel_downsampling_s": round(t1 - t0, 3), "extract_towers_s": round(t2 - t1, 3),
                            "Mpts_per_s": round(ne / (t2 - t0) / 1e6, 1), "towers": len(tw)},
                        "intermediate_file_identical_in_all_three": bool(sha_async == sha_sync == sha_plain),
                        "tower_dicts_identical": bool(
                            len(twa) == len(twb) == len(tw) and all(
                                np.array_equal(a["center"], b["center"]) and np.array_equal(a["center"], c["center"])
                                and np.array_equal(a["extent"], b["extent"]) and np.array_equal(a["extent"], c["extent"])
                                for a, b, c in zip(twa, twb, tw)))},
                    "Mpts_per_s_extract_towers_on_its_input": round(int(hv.point_count) / (tb2 - tb1) / 1e6, 1),
                    "stages_run_voxel_downsampling_s": sv, "stages_extract_towers_s": se,
                    "read_GBps": round(size_in / rd / 1e9, 2) if rd else None,
                    "source_file_write_GBps": round(size_in / t_write_src / 1e9, 2),
                    "las_io_threads": os.environ.get("PCH_LAS_THREADS", "default (8 when >= 16 cores)"),
                    "note": "wall clock with stage timers on (the device is drained at every stage edge); page cache "
                            "warm (the file was just written); LAS reader: pread by several threads -> pinned ring -> "
                            "H2D || decode; writer: records laid out on the device, pwrite by several threads"}
            finally:
                shutil.rmtree(td, ignore_errors=True)
        except Exception as e:
            out["dropin_end_to_end_100m"] = {"error": f"{type(e).__name__}: {e}"}

    # ---- BASELINE config 5: a real .las through the drop-ins (--full)
    if world == 1 and args.full:
        if args.las and os.path.exists(args.las):
            try:
                import tempfile
                from pointcloudhookup_amd.ui import import_PC as _imp
                from pointcloudhookup_amd.utils import tower_extraction as _te
                with tempfile.TemporaryDirectory(prefix="pch_cfg5_") as td:
                    cwd = os.getcwd()
                    os.chdir(td)
                    try:
                        t0 = time.perf_counter()
                        _imp.run_voxel_downsampling(os.path.abspath(args.las) if os.path.isabs(args.las)
                                                    else os.path.join(cwd, args.las),
                                                    os.path.join(td, "output", "point_2.las"), 0.1, 500000)
                        t1 = time.perf_counter()
                        tw = _te.extract_towers(os.path.join(td, "output", "point_2.las"), log_callback=lambda m: None)
                        t2 = time.perf_counter()
                    finally:
                        os.chdir(cwd)
                out["config5_real_las"] = {"file": args.las, "run_voxel_downsampling_s": round(t1 - t0, 3),
                                           "extract_towers_s": round(t2 - t1, 3), "towers": len(tw)}
            except Exception as e:
                out["config5_real_las"] = {"file": args.las, "error": str(e)}
        else:
            out["config5_real_las"] = {"skipped": "no file" if not args.las else f"no file at {args.las}",
                                       "note": "the reference ships no .las sample; pass --las PATH"}

    # ---- tile stream side measurement (--full, not in `value`): two host threads, each with its own HIP
    # stream and workspace, work through tiles at the same time - one tile's latency-bound
    # clustering overlaps the other's issue/bandwidth-bound filter.  Same tile as above.
    if world == 1 and args.full and not args.no_tile_stream:
        try:
            import threading
            per_thread, nthreads = max(2, args.steps), 2
            errs, marks = [], {}
            gate = threading.Barrier(nthreads + 1)

            def worker(i):
                try:
                    st = torch.cuda.Stream(device=dev)
                    with torch.cuda.stream(st):
                        pipeline.cluster_points(raw, EPS, MIN_POINTS, CHUNK)     # warm-up: this thread's workspace
                        st.synchronize()
                        gate.wait()
                        t_go = time.perf_counter() + 0.45e-3 * ms_per_step * i    # staggered start: identical tiles
                        while time.perf_counter() < t_go:                        # would run their phases in lockstep
                            pass
                        for _ in range(per_thread):
                            pipeline.cluster_points(raw, EPS, MIN_POINTS, CHUNK)
                        st.synchronize()
                    gate.wait()
                    ops.release_workspace()
                except Exception as e:                           # pragma: no cover
                    errs.append(str(e))
                    gate.abort()

            ths = [threading.Thread(target=worker, args=(i,)) for i in range(nthreads)]
            for t in ths:
                t.start()
            gate.wait()
            t0 = time.perf_counter()
            gate.wait()
            dts = time.perf_counter() - t0
            for t in ths:
                t.join()
            if errs:
                raise RuntimeError(errs[0])
            out["tile_stream"] = {"threads": nthreads, "tiles": nthreads * per_thread, "points_per_tile": N,
                                  "ms_per_tile": round(1e3 * dts / (nthreads * per_thread), 3),
                                  "Mpts_per_s": round(N * nthreads * per_thread / dts / 1e6, 1),
                                  "note": "two tiles in flight on one GPU; not the headline value"}
        except Exception as e:
            out["tile_stream"] = {"error": str(e)}

    # ---- CPU baseline (--full): the reference's own library calls (numpy + sklearn) on host cores
    if world == 1 and args.full and not args.no_cpu_baseline:
        try:
            from oracle import ground_filter as ogf, dbscan as odb
            host = raw.cpu().numpy()
            t0 = time.perf_counter()
            gf = ogf.ground_filter(host)
            t_filter = time.perf_counter() - t0
            filt = gf["filtered"]
            nch = (len(filt) + CHUNK - 1) // CHUNK
            fit = "sklearn"
            try:
                import sklearn  # noqa: F401
            except Exception:
                fit = "c"
            gpu_labels = cl["labels"].cpu().numpy()
            parity = (len(filt) == NF)
            done, t_cl = 0, 0.0
            stride = max(1, nch // 6)
            for ci in range(0, nch, stride):
                chunk = filt[ci * CHUNK:(ci + 1) * CHUNK]
                t1 = time.perf_counter()
                ref, _ = odb._FITS[fit](chunk, EPS, MIN_POINTS)
                t_cl += time.perf_counter() - t1
                done += 1
                g = gpu_labels[ci * CHUNK:(ci + 1) * CHUNK].astype(np.int64)
                base = g[g >= 0].min() if (g >= 0).any() else 0
                parity = parity and np.array_equal(np.where(g >= 0, g - base, -1), ref)
                if t_filter + t_cl > args.cpu_budget_s and done >= 2:
                    break
            est = t_filter + (t_cl / max(done, 1)) * nch
            out["cpu_baseline"] = {
                "value": round(N / est / 1e6, 4), "unit": "Mpts/s", "cores": os.cpu_count(),
                "kind": "port",
                "sample": f"numpy mean/percentile/mask on all {N} pts ({t_filter:.2f} s) + "
                          f"{'sklearn DBSCAN(ball_tree, n_jobs=-1)' if fit == 'sklearn' else 'oracle C all-pairs DBSCAN'}"
                          f" on {done} of {nch} 50k-chunks ({t_cl:.2f} s), clustering time extrapolated "
                          f"x{nch / max(done, 1):.1f}",
                "parity_on_sample": bool(parity)}
        except Exception as e:                                   # never lose the GPU line
            out["cpu_baseline"] = {"value": None, "unit": "Mpts/s", "cores": os.cpu_count(),
                                   "kind": "port", "sample": f"failed: {e}"}
    print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
