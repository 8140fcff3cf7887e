"""The statement of the plane ground rule (pch_plane_fit_f32 / pch_filter_plane_f32, include/pch_hip.h) and the clouds
its tests use (TEST INFRASTRUCTURE, pure numpy; imported by the CPU and the GPU tests, not a conftest).

Everything is float64 on (double) of the float32 centred rows, in exactly the association the header writes, with
elementwise numpy only (never ``@``: a BLAS kernel may fuse a product into a sum, and the comparison with the library
is bit for bit).  An invalid hypothesis is four zeros in ``planes`` and 0 in ``counts``.
"""
import math

import numpy as np

from pointcloudhookup_amd import synth

COUNT_TILE = 1024                # rows per workgroup pass of pl_count_k (ops.PLANE_COUNT_TILE)


# ------------------------------------------------------------------ the statement
def cos2_of(max_slope_deg):
    return math.cos(math.radians(float(max_slope_deg))) ** 2


def hypothesis_rows(n, H, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, n, size=(H, 3), dtype=np.int64)


def centre(raw, centroid):
    """P = raw - centroid in float32 (utils/tower_extraction.py:64)"""
    return raw.astype(np.float32) - np.asarray(centroid, dtype=np.float32).reshape(1, 3)


def planes_of(P, rows, cos2):
    """float64 [H,4]: a, b, c, valid"""
    H = len(rows)
    out = np.zeros((H, 4), dtype=np.float64)
    if len(P) == 0:
        return out
    D = P.astype(np.float64)
    with np.errstate(all="ignore"):
        p0, p1, p2 = D[rows[:, 0]], D[rows[:, 1]], D[rows[:, 2]]
        ux, uy, uz = p1[:, 0] - p0[:, 0], p1[:, 1] - p0[:, 1], p1[:, 2] - p0[:, 2]
        vx, vy, vz = p2[:, 0] - p0[:, 0], p2[:, 1] - p0[:, 1], p2[:, 2] - p0[:, 2]
        nx = uy * vz - uz * vy
        ny = uz * vx - ux * vz
        nz = ux * vy - uy * vx
        nn = (nx * nx + ny * ny) + nz * nz
        valid = np.isfinite(nn) & (nz != 0) & (nz * nz >= cos2 * nn)
        a = -nx / nz
        b = -ny / nz
        c = p0[:, 2] - (a * p0[:, 0] + b * p0[:, 1])
        valid &= np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    out[valid, 0], out[valid, 1], out[valid, 2], out[valid, 3] = a[valid], b[valid], c[valid], 1.0
    return out


def residual(P, plane):
    D = P.astype(np.float64)
    with np.errstate(all="ignore"):
        return D[:, 2] - ((plane[0] * D[:, 0] + plane[1] * D[:, 1]) + plane[2])


def inliers(P, plane, thr):
    with np.errstate(invalid="ignore"):
        return np.abs(residual(P, plane)) <= thr                # NaN compares false


def fit(P, rows, thr=0.1, max_slope_deg=45.0):
    """dict(planes, counts, best, plane | None, inliers, nvalid): steps 1-4"""
    planes = planes_of(P, rows, cos2_of(max_slope_deg))
    counts = np.zeros((len(rows),), dtype=np.int64)
    for h in np.flatnonzero(planes[:, 3] != 0):
        counts[h] = np.count_nonzero(inliers(P, planes[h], thr))
    valid = planes[:, 3] != 0
    best = int(np.argmax(np.where(valid, counts, -1))) if valid.any() else -1      # argmax: the first of a tie
    return dict(planes=planes, counts=counts, best=best, plane=None if best < 0 else planes[best, :3].copy(),
                inliers=0 if best < 0 else int(counts[best]), nvalid=int(valid.sum()))


def keep_mask(P, plane, keep, offset=3.0, thr=0.1):
    """step 5; plane None (no valid hypothesis) keeps nothing"""
    if plane is None:
        return np.zeros((len(P),), dtype=bool)
    with np.errstate(invalid="ignore"):
        if keep == "above":
            return residual(P, plane) > offset
        assert keep == "off_plane"
        return ~inliers(P, plane, thr)


def filtered(P, mask):
    """what the filter returns for a mask: dict(points float32, index int32, count, aabb float32 [6])"""
    pts = P[mask]
    fin = pts[np.isfinite(pts).all(axis=1)]
    aabb = np.zeros((6,), dtype=np.float32)
    if len(fin):
        aabb[:3], aabb[3:] = fin.min(axis=0), fin.max(axis=0)
    return dict(points=pts, index=np.flatnonzero(mask).astype(np.int32), count=int(mask.sum()), aabb=aabb)


PATCHY_TILE, PATCHY_SEG = 2048, 512      # rows a workgroup / a wave of the compacting sweeps takes (PF_TILE, CR_TILE)


def patchy_cloud():
    """(raw float32 [n,3], mask bool [n]), n = 5 tiles + 300 rows, for the sweeps that compact a tile of four wave
    segments (ops.crop_aabb, filter_plane, filter_plane_tiles): x, y random, z = 10 in a kept row and 0 otherwise, the
    kept set chosen per segment - tile 0 keeps everything, tile 1 nothing, tile 2 its last row alone, tile 3 every
    7th row of wave 2's segment alone, tile 4 nothing, the partial tile 5 the cloud's last row alone"""
    kinds = ["all"] * 4 + ["none"] * 4 + ["none", "none", "none", "last"] + ["none", "none", "every7", "none"] + \
            ["none"] * 4 + ["last"]
    n = 5 * PATCHY_TILE + 300
    mask = np.zeros((n,), dtype=bool)
    for s, kind in enumerate(kinds):
        seg = mask[PATCHY_SEG * s:PATCHY_SEG * (s + 1)]          # a view; the last one has 300 rows
        if kind == "all":
            seg[:] = True
        elif kind == "last":
            seg[-1] = True
        elif kind == "every7":
            seg[::7] = True
    raw = np.empty((n, 3), dtype=np.float32)
    raw[:, :2] = np.random.Generator(np.random.PCG64(7)).uniform(0.0, 100.0, size=(n, 2))
    raw[:, 2] = np.where(mask, 10.0, 0.0)
    return raw, mask


def ground(raw, rows, thr=0.1, max_slope_deg=45.0, offset=3.0, fallback_offset=1.0, min_keep=1000, keep="above"):
    """steps 1-6 on a float32 cloud: what ops.ground_filter_plane returns (ValueError without a valid plane)"""
    centroid = np.mean(raw, axis=0)
    P = centre(raw, centroid)
    f = fit(P, rows, thr, max_slope_deg)
    if f["best"] < 0:
        raise ValueError("no valid ground plane")
    out = filtered(P, keep_mask(P, f["plane"], keep, offset, thr))
    first, used, value = out["count"], False, offset if keep == "above" else thr
    if keep == "above" and first < min_keep:
        used, value = True, fallback_offset
        out = filtered(P, keep_mask(P, f["plane"], keep, fallback_offset, thr))
    out.update(centroid=centroid, base=np.float32(f["plane"][2]), threshold=np.float32(value), used_fallback=used,
               count_at_offset=first, plane=f["plane"], inliers=f["inliers"], nvalid=f["nvalid"], best=f["best"],
               P=P)
    return out


def percentile_mask(P):
    """the default rule on the same centred rows (utils/tower_extraction.py:82-84)"""
    z = P[:, 2]
    return z > np.percentile(z, 25) + 3.0


# ------------------------------------------------------------------ clouds
SPREAD_N = 50_000                # the smallest corridor generated: 5 m x 100 m, wide enough for level triples


def tilted(n, sx=0.15, sy=-0.05, offset=True, towers=3):
    """(raw float32 [n,3], truth bool [n]): the synthetic corridor on a slope, z += sx x + sy y about the corridor's own
    origin, then the global offset, then the float32 cast; truth = generator height above the true ground > 3 m.
    Below SPREAD_N rows: the first n rows of the SPREAD_N-row corridor (its file order is a shuffle, so they are
    spread over all of it - an n-row corridor would be n / 10 000 m long and all its triples degenerate)."""
    pts = synth.corridor_numpy(max(n, SPREAD_N), seed=synth.SEED0, kind="corridor", offset=False, towers=towers)[:n]
    truth = pts[:, 2] > 3.0
    pts[:, 2] += sx * pts[:, 0] + sy * pts[:, 1]
    if offset:
        pts = pts + synth.GLOBAL_OFFSET
    return pts.astype(np.float32), truth


def special_cloud(n=5000):
    """(raw float32 [n,3] for centroid 0, rows int64 [13,3], expected validity [13]): a small slope with hand-placed
    rows in front, and one triple per special case of the rule"""
    raw, _ = tilted(n, 0.05, 0.02, offset=False)
    e = np.float32(2.0 ** -20)
    head = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0],                    # 0-2 span the plane z = 0
                     [0, 0, 1],                                          # 3: above row 0 (vertical with 0 and 1)
                     [1, 1, 1], [2, 2, 2],                               # 4, 5: collinear with row 0
                     [1, 0, 1 - e], [1, 0, 1 + e],                       # 6 / 7: a 45 degree slope, minus / plus a hair
                     [np.nan, 0, 0], [np.inf, 0, 0], [1, 0, 1]], dtype=np.float32)
    raw[:len(head)] = head
    raw[n - 1] = [3.0, 50.0, 1.5]
    good = [20, 500, 3000]
    rows = np.array([[20, 20, 500],          # 0  a repeated row
                     [0, 4, 5],              # 1  collinear
                     [0, 3, 1],              # 2  vertical: nz == 0
                     [0, 6, 2],              # 3  just inside the slope gate
                     [0, 7, 2],              # 4  just outside
                     [0, 10, 2],             # 5  exactly 45 degrees: outside, cos2(45 deg) rounds above 1/2
                     [8, 1, 2],              # 6  a NaN row
                     [9, 1, 2],              # 7  an inf row
                     [0, 1, n - 1],          # 8  first and last row
                     good, [0, 1, 2], good,  # 9, 11 the same triple twice; 10 the plane z = 0
                     [3000, 20, 500]], dtype=np.int64)
    valid = np.array([0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1], dtype=bool)
    return raw, rows, valid


def boundary_cloud(a=0.0, b=0.0):
    """(raw float32 [m,3] for centroid 0, rows int64 [1,3], residuals float64 [m]): dyadic coordinates around the plane
    z = a x + b y that rows 0-2 define exactly; every row's residual is exact, and the rows sit at 0, +-0.125, 3.0, one
    float32 ulp to either side of each, and NaN.  Use residual_threshold 0.125 and offset 3.0."""
    f = np.float32
    up = lambda v: np.nextafter(f(v), f(np.inf))
    dn = lambda v: np.nextafter(f(v), f(-np.inf))
    xy = [(0.0, 0.0), (0.25, 0.5), (-0.5, 0.25), (0.75, -0.25), (0.0, 1.0)]
    body = []
    for (x, y) in xy:
        # with a, b in {0, 0.5, -0.25} every a x + b y here is a multiple of 2^-4 below 1, so z0 is exact in float32
        # and the row lies exactly on the boundary; its float32 neighbours lie one ulp of the z coordinate off it
        body.append((x, y, f(a * x + b * y)))
        for bound in (0.125, -0.125, 3.0, -3.0):
            z0 = f(a * x + b * y + bound)
            assert float(z0) == a * x + b * y + bound
            body += [(x, y, z0), (x, y, up(z0)), (x, y, dn(z0))]
        body += [(x, y, f(np.nan)), (x, y, f(a * x + b * y + 40.0))]
    body += [(np.nan, 0.0, 0.0), (0.0, np.nan, 0.0)]
    head = [(0.0, 0.0, 0.0), (2.0, 0.0, 2.0 * a), (0.0, 4.0, 4.0 * b)]
    raw = np.array(head + body, dtype=np.float32)
    res = raw[:, 2].astype(np.float64) - (a * raw[:, 0].astype(np.float64) + b * raw[:, 1].astype(np.float64))
    return raw, np.array([[0, 1, 2]], dtype=np.int64), res
