"""The statement of the per-tile plane ground rule (pch_plane_tiles_fit_f32 / pch_filter_plane_tiles_f32,
include/pch_hip.h) and the clouds its tests use (TEST INFRASTRUCTURE, pure numpy; imported by the CPU and the GPU tests,
not a conftest).  The plane of a triple, the residual and the keep rule are plane_cases'; this file adds the grid, the
grouping, the shared draw table and the per-row plane lookup.  Elementwise numpy only, float64 on (double) of the
float32 centred rows, in the association the header writes.
"""
import functools
import math

import numpy as np

import plane_cases as pc
from pointcloudhookup_amd import synth

PASS = pc.COUNT_TILE             # a pass of the count kernel: at most 1024 grouped rows of one tile
MAX_TILES = 65536
MAX_TABLE = 1 << 22


# ------------------------------------------------------------------ the statement
def draws(H, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 2 ** 62, size=(H, 3), dtype=np.int64)


def grid_of(raw, centroid, tile):
    """dict(x0, y0, tile, nx, ny) over the finite x and y: x0 = (double)fl32(min_x - cx), nx = floor((max - x0) / tile)
    + 1 with max = (double)fl32(max_x - cx)"""
    cen = np.asarray(centroid, dtype=np.float32)
    out = dict(tile=float(tile))
    for k, name in enumerate("xy"):
        v = raw[:, k][np.isfinite(raw[:, k])]
        if len(v) == 0:
            out[name + "0"], out["n" + name] = 0.0, 1
            continue
        a, b = float(np.float32(v.min()) - cen[k]), float(np.float32(v.max()) - cen[k])
        out[name + "0"], out["n" + name] = a, int(math.floor((b - a) / float(tile))) + 1
    return out


def tile_of(P, grid):
    """int64 [n]: t = fy nx + fx, -1 for a row outside the grid (NaN and inf fail the comparisons)"""
    D = P.astype(np.float64)
    with np.errstate(all="ignore"):
        fx = np.floor((D[:, 0] - grid["x0"]) / grid["tile"])
        fy = np.floor((D[:, 1] - grid["y0"]) / grid["tile"])
        ok = (fx >= 0) & (fx < grid["nx"]) & (fy >= 0) & (fy < grid["ny"])
    t = np.full((len(P),), -1, dtype=np.int64)
    t[ok] = fy[ok].astype(np.int64) * grid["nx"] + fx[ok].astype(np.int64)
    return t


def fit(P, grid, table, min_tile_rows=64, thr=0.1, max_slope_deg=45.0):
    """dict(best int32 [T], planes float64 [T,3], inliers int64, rows int64, nvalid int32, planes_table [T,H,4],
    counts_table [T,H], grid, tile): steps 1-5"""
    T, H = grid["nx"] * grid["ny"], len(table)
    assert 1 <= T <= MAX_TILES and T * H <= MAX_TABLE and (table >= 0).all()
    tile = tile_of(P, grid)
    order = np.argsort(tile, kind="stable")                  # list_t: ascending row order inside a tile
    rows = np.bincount(tile[tile >= 0], minlength=T).astype(np.int64)
    first = np.searchsorted(tile[order], np.arange(T))
    out = dict(best=np.full((T,), -1, dtype=np.int32), planes=np.zeros((T, 3)), inliers=np.zeros((T,), dtype=np.int64),
               rows=rows, nvalid=np.zeros((T,), dtype=np.int32), planes_table=np.zeros((T, H, 4)),
               counts_table=np.zeros((T, H), dtype=np.int64), grid=dict(grid), tile=tile)
    cos2 = pc.cos2_of(max_slope_deg)
    for t in np.flatnonzero(rows >= max(int(min_tile_rows), 1)):
        members = order[first[t]:first[t] + rows[t]]
        planes = pc.planes_of(P, members[table % rows[t]], cos2)
        Pt = P[members]
        counts = np.zeros((H,), dtype=np.int64)
        for h in np.flatnonzero(planes[:, 3] != 0):
            counts[h] = np.count_nonzero(pc.inliers(Pt, planes[h], thr))
        valid = planes[:, 3] != 0
        out["planes_table"][t], out["counts_table"][t], out["nvalid"][t] = planes, counts, valid.sum()
        if valid.any():
            b = int(np.argmax(np.where(valid, counts, -1)))                 # argmax: the first of a tie
            out["best"][t], out["planes"][t], out["inliers"][t] = b, planes[b, :3], counts[b]
    return out


def row_planes(P, grid, f, fallback):
    """(has bool [n], abc float64 [n,3]): the plane every row uses - its tile's, else the fallback's (None: none)"""
    tile = tile_of(P, grid)
    own = (tile >= 0) & (np.asarray(f["best"])[np.maximum(tile, 0)] >= 0)
    abc = np.zeros((len(P), 3))
    abc[own] = np.asarray(f["planes"], dtype=np.float64)[tile[own]]
    has = own.copy()
    if fallback is not None:
        abc[~own] = np.asarray(fallback, dtype=np.float64)
        has[:] = True
    return has, abc


def keep_mask(P, grid, f, fallback, keep, offset=3.0, thr=0.1):
    """step 6; a row with no plane at all is not kept, in either mode"""
    has, abc = row_planes(P, grid, f, fallback)
    D = P.astype(np.float64)
    with np.errstate(all="ignore"):
        res = D[:, 2] - ((abc[:, 0] * D[:, 0] + abc[:, 1] * D[:, 1]) + abc[:, 2])
        if keep == "above":
            return has & (res > offset)
        assert keep == "off_plane"
        return has & ~(np.abs(res) <= thr)


def ground(raw, tile_size=20.0, hypotheses=64, seed=0, min_tile_rows=64, fallback_hypotheses=64, thr=0.1,
           max_slope_deg=45.0, offset=3.0, fallback_offset=1.0, min_keep=1000, keep="above"):
    """what ops.ground_filter_plane_tiles returns (ValueError without any plane)"""
    centroid = np.mean(raw, axis=0)
    P = pc.centre(raw, centroid)
    grid = grid_of(raw, centroid, tile_size)
    g = pc.fit(P, pc.hypothesis_rows(len(raw), fallback_hypotheses, seed), thr, max_slope_deg)
    f = fit(P, grid, draws(hypotheses, seed), min_tile_rows, thr, max_slope_deg)
    if g["best"] < 0 and not (f["best"] >= 0).any():
        raise ValueError("no valid ground plane")
    out = pc.filtered(P, keep_mask(P, grid, f, g["plane"], keep, offset, thr))
    first, used, value = out["count"], False, offset if keep == "above" else thr
    if keep == "above" and first < min_keep:
        used, value = True, fallback_offset
        out = pc.filtered(P, keep_mask(P, grid, f, g["plane"], keep, fallback_offset, thr))
    out.update(centroid=centroid, base=np.float32(np.nan if g["plane"] is None else g["plane"][2]),
               threshold=np.float32(value), used_fallback=used, count_at_offset=first, tiles=f,
               fallback_plane=g["plane"], P=P)
    return out


# ------------------------------------------------------------------ clouds
VALLEY_N = 200_000
VALLEY_KW = dict(tile_size=10.0, hypotheses=64, seed=0, min_tile_rows=64, fallback_hypotheses=256)
VALLEY_FIGURES = (0, 81_458, 19_690)   # rows off the truth: tiled rule, one plane (256 hypotheses); rows the tiled rule keeps


@functools.lru_cache(maxsize=None)
def valley(n=VALLEY_N):
    """(raw float32 [n,3], truth bool [n]): the synthetic corridor (3 towers) in a V-shaped valley on a slope,
    z += 0.3 |y - 50| + 0.1 x, in the offset frame; truth = generator height above the true ground > 3 m"""
    pts = synth.corridor_numpy(max(n, pc.SPREAD_N), seed=synth.SEED0, kind="corridor", offset=False, towers=3)[:n]
    truth = pts[:, 2] > 3.0
    pts[:, 2] += 0.3 * np.abs(pts[:, 1] - 50.0) + 0.1 * pts[:, 0]
    raw = (pts + synth.GLOBAL_OFFSET).astype(np.float32)
    raw.setflags(write=False)
    return raw, truth


POPULATIONS = (0, 1, 63, 64, 1023, 1024, 1025, 2049, 5000)


@functools.lru_cache(maxsize=None)
def populations_cloud(seed=5):
    """(raw float32 [n,3] for centroid 0, grid): nine 8 m tiles in a row along x holding exactly POPULATIONS rows of
    valley terrain (z = 0.3 |y - 4| + 0.1 x plus 3 cm of noise, every 7th row 5 m up), file order shuffled"""
    rng = np.random.Generator(np.random.PCG64(seed))
    parts = []
    for k, m in enumerate(POPULATIONS):
        x = 8.0 * k + rng.uniform(0.25, 7.75, m)
        y = rng.uniform(0.25, 7.75, m)
        z = 0.3 * np.abs(y - 4.0) + 0.1 * x + rng.normal(0.0, 0.03, m)
        z[::7] += 5.0
        parts.append(np.stack([x, y, z], axis=1))
    raw = np.concatenate(parts)[rng.permutation(sum(POPULATIONS))].astype(np.float32)
    raw.setflags(write=False)
    return raw, dict(x0=0.0, y0=0.0, tile=8.0, nx=len(POPULATIONS), ny=1)
