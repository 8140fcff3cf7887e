"""The upright boxes of stage D1 as a statement in plain numpy (no library import), and the seeded builders of their
tests.  The rule (include/pch_hip.h): T = 4096 table angles cs[j] = (cos, sin)(j * (pi/2) / T) in float64; per cluster
  1 status 1 (no box: j = j0 = -1, NaN bounds) without rows or with a coordinate that is not finite, else 0
  2 rectangle at j: x, y as float64 of the float32 coordinates, u = x*c + y*s, v = y*c - x*s (no FMA); umin, umax, vmin,
    vmax over the cluster's rows; area(j) = (umax - umin) * (vmax - vmin) from the bounds of the whole cluster
  3 level 0: j0 = the index among {a * 32 : a = 0..127} of smallest area, ties to the smallest index
  4 level 1: j = the candidate among {(j0 + d) mod T : d = -31..31} of smallest area, ties to the smallest table index
  5 zmin, zmax: the extremes of the float32 z values as float64
Everything is a minimum or a maximum of float64 products, so no order of the rows enters.
"""
import numpy as np

import merge_cases as mc

COARSE, FINE, T = 128, 32, 4096
H = np.pi / 512                                          # half the coarse step: some coarse angle lies within it
RECORD = np.dtype([("status", "<i4"), ("j", "<i4"), ("j0", "<i4"), ("reserved", "<i4"), ("n", "<i8"),
                   ("umin", "<f8"), ("umax", "<f8"), ("vmin", "<f8"), ("vmax", "<f8"), ("zmin", "<f8"), ("zmax", "<f8")])
BOUNDS = ("umin", "umax", "vmin", "vmax", "zmin", "zmax")
FRAMES = mc.FRAMES
_ROWS_AT_ONCE = 8192                                     # the minima of pieces are the minima of the whole


# ---------------------------------------------------------------------------------------------------- the statement
def table():
    """float64 [T,2]: (cos, sin) of j * (pi/2) / T"""
    theta = np.arange(T, dtype=np.float64) * (np.pi / 2) / T
    return np.stack([np.cos(theta), np.sin(theta)], axis=1)


def rect(rows, js, cs=None):
    """float64 [len(js),4]: (umin, umax, vmin, vmax) of the rows' footprint at every table index of ``js``"""
    cs = table() if cs is None else cs
    xy = np.asarray(rows)[:, :2].astype(np.float64)
    c, s = cs[np.asarray(js), 0][None, :], cs[np.asarray(js), 1][None, :]
    out = np.empty((len(js), 4), dtype=np.float64)
    out[:, 0] = out[:, 2] = np.inf
    out[:, 1] = out[:, 3] = -np.inf
    for at in range(0, len(xy), _ROWS_AT_ONCE):
        x, y = xy[at:at + _ROWS_AT_ONCE, 0:1], xy[at:at + _ROWS_AT_ONCE, 1:2]
        u = x * c + y * s                                 # separate ufunc calls: two products, one add, no FMA
        v = y * c - x * s
        out[:, 0] = np.minimum(out[:, 0], u.min(axis=0))
        out[:, 1] = np.maximum(out[:, 1], u.max(axis=0))
        out[:, 2] = np.minimum(out[:, 2], v.min(axis=0))
        out[:, 3] = np.maximum(out[:, 3], v.max(axis=0))
    return out


def areas(bounds):
    return (bounds[:, 1] - bounds[:, 0]) * (bounds[:, 3] - bounds[:, 2])


def _smallest(js, a):
    """position of the smallest area, ties to the smallest table index"""
    js = np.asarray(js)
    tied = np.flatnonzero(a == a.min())
    return int(tied[np.argmin(js[tied])])


def box(rows, cs=None):
    """the record of one cluster (a RECORD scalar) and the level-0 area"""
    cs = table() if cs is None else cs
    rows = np.asarray(rows).reshape(-1, 3)
    rec = np.zeros((), dtype=RECORD)
    rec["n"] = len(rows)
    if len(rows) == 0 or not np.isfinite(rows).all():
        rec["status"], rec["j"], rec["j0"] = 1, -1, -1
        for f in BOUNDS:
            rec[f] = np.nan
        return rec, np.nan
    coarse = np.arange(COARSE) * FINE
    b0 = rect(rows, coarse, cs)
    a0 = areas(b0)
    at0 = _smallest(coarse, a0)
    j0 = int(coarse[at0])
    fine = (j0 + np.arange(-(FINE - 1), FINE)) % T
    b1 = rect(rows, fine, cs)
    at1 = _smallest(fine, areas(b1))
    rec["j0"], rec["j"] = j0, int(fine[at1])
    rec["umin"], rec["umax"], rec["vmin"], rec["vmax"] = b1[at1]
    z = rows[:, 2]
    rec["zmin"], rec["zmax"] = np.float64(z.min()), np.float64(z.max())
    return rec, float(a0[at0])


def expected(P, labels, K):
    """RECORD [K]: the records of the clusters labels == 0 .. K-1 of the float32 rows P"""
    P = np.asarray(P, dtype=np.float32).reshape(-1, 3)
    cs = table()
    out = np.zeros((K,), dtype=RECORD)
    for k in range(K):
        out[k] = box(P[labels == k], cs)[0]
    return out


def area_of(rec):
    return (rec["umax"] - rec["umin"]) * (rec["vmax"] - rec["vmin"])


def tower_from_record(rec, cs=None):
    """(extents float64 [3], transform float64 [4,4]) of a status-0 record, None for status 1"""
    if int(rec["status"]) != 0:
        return None
    cs = table() if cs is None else cs
    c, s = cs[int(rec["j"])]
    du, dv, dz = rec["umax"] - rec["umin"], rec["vmax"] - rec["vmin"], rec["zmax"] - rec["zmin"]
    mu, mv, mz = 0.5 * (rec["umin"] + rec["umax"]), 0.5 * (rec["vmin"] + rec["vmax"]), 0.5 * (rec["zmin"] + rec["zmax"])
    centre = np.array([mu * c - mv * s, mu * s + mv * c, mz], dtype=np.float64)
    if dv > du:
        X, Y, extents = (-s, c, 0.0), (-c, -s, 0.0), [dv, du, dz]
    else:
        X, Y, extents = (c, s, 0.0), (-s, c, 0.0), [du, dv, dz]
    transform = np.zeros((4, 4), dtype=np.float64)
    transform[:3, 0], transform[:3, 1], transform[:3, 2], transform[:3, 3] = X, Y, (0.0, 0.0, 1.0), centre
    transform[3, 3] = 1.0
    return np.array(extents, dtype=np.float64), transform


def bound_factor(r):
    """the derived quality bound: found area <= optimum * this, for a footprint of aspect r"""
    return 1.0 + H * (r + 1.0 / r) + H * H


def assert_records_equal(got, want):
    """integer fields equal, bounds equal by value (-0.0 == +0.0), NaN in the same places"""
    for f in ("status", "j", "j0", "n"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    for f in BOUNDS:
        np.testing.assert_array_equal(np.isnan(got[f]), np.isnan(want[f]), err_msg=f)
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)      # (NaN == NaN for assert_array_equal)


# ------------------------------------------------------------------------------------------------------ the builders
centers_cloud = mc.centers_cloud      # sizes 1, 2, 63, 64, 65, 127, 128, 129, 4097, 50 000, an empty, a NaN, a +inf cluster


def big_cloud():
    """(P float32 [n,3], labels int32 [n], K = 201): cluster 100 has 300 001 rows on a 40 x 12 m footprint turned by
    27.3 degrees, the 200 others 1-3 rows; noise in between, all shuffled in file order"""
    rng = np.random.default_rng(23)
    K, big = 201, 100
    sizes = rng.integers(1, 4, K)
    sizes[big] = 300_001
    lab = np.concatenate([np.repeat(np.arange(K, dtype=np.int32), sizes), np.full((5000,), -1, dtype=np.int32)])
    lab = lab[rng.permutation(len(lab))]
    mid = np.column_stack([rng.uniform(-800, 800, K + 1), rng.uniform(-300, 300, K + 1), rng.uniform(5, 40, K + 1)])
    P = mid[lab] + rng.normal(0, 1, (len(lab), 3))
    t = np.radians(27.3)
    a, b = rng.uniform(-20, 20, sizes[big]), rng.uniform(-6, 6, sizes[big])
    rows = np.flatnonzero(lab == big)
    P[rows, 0] = mid[big, 0] + a * np.cos(t) - b * np.sin(t)
    P[rows, 1] = mid[big, 1] + a * np.sin(t) + b * np.cos(t)
    return P.astype(np.float32), lab, K


EDGE_SIZES = [7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]


def tile_edges_cloud():
    """(P, labels, K): clusters of EDGE_SIZES rows - the edges of the kernels' 256-row tile, of the 8 and 16 rows a round
    of the tile walk takes, and of two and four tiles - each an elongated blob turned by an angle of its own, shuffled
    with noise.  The extreme rows of a cluster lie anywhere in it, so a row left out or read twice past the end shows"""
    rng = np.random.default_rng(29)
    K = len(EDGE_SIZES)
    lab = np.concatenate([np.repeat(np.arange(K, dtype=np.int32), EDGE_SIZES), np.full((777,), -1, dtype=np.int32)])
    lab = lab[rng.permutation(len(lab))]
    mid = np.column_stack([rng.uniform(-500, 500, K + 1), rng.uniform(-500, 500, K + 1), rng.uniform(0, 30, K + 1)])
    turn = np.append(rng.uniform(0, np.pi, K), 0.0)[lab]
    a, b = rng.normal(0, 6.0, len(lab)), rng.normal(0, 1.5, len(lab))
    P = np.column_stack([mid[lab, 0] + a * np.cos(turn) - b * np.sin(turn),
                         mid[lab, 1] + a * np.sin(turn) + b * np.cos(turn), mid[lab, 2] + rng.normal(0, 8.0, len(lab))])
    return P.astype(np.float32), lab, K


ON_COARSE, ON_FINE = 37 * FINE, 37 * FINE + 11
# name -> (angle in radians, table index the optimum lies on or None)
RECT_ANGLES = {
    "on_coarse": (ON_COARSE * (np.pi / 2) / T, ON_COARSE),
    "on_fine": (ON_FINE * (np.pi / 2) / T, ON_FINE),
    "between_33.3": (np.radians(33.3), None),
    "at_45": (np.radians(45.0), T // 2),
    "wrap_89.99": (np.radians(89.99), None),             # level 0 picks index 0, level 1 looks at 4065..4095 too
    "wrap_89.97": (np.radians(89.97), None),             # the winner itself is a wrapped index (4095)
}
RECT_SIDES = (20.0, 8.0)


def _turned(a, b, angle, centre):
    c, s = np.cos(angle), np.sin(angle)
    return np.column_stack([centre[0] + a * c - b * s, centre[1] + a * s + b * c])


def rectangle_rows(name):
    """float64 [204,3], before the rounding to float32: the four corners and 200 interior points of a 20 x 8 rectangle
    around the origin, turned by the case's angle (the on-table cases by the table's own angle)"""
    angle = RECT_ANGLES[name][0]
    rng = np.random.default_rng(31)
    la, lb = RECT_SIDES[0] / 2, RECT_SIDES[1] / 2
    a = np.concatenate([[-la, la, la, -la], rng.uniform(-la, la, 200)])
    b = np.concatenate([[-lb, -lb, lb, lb], rng.uniform(-lb, lb, 200)])
    return np.column_stack([_turned(a, b, angle, (0.0, 0.0)), rng.uniform(2.0, 30.0, len(a))])


def degenerate_rows():
    """name -> float64 rows: the tie and zero-area cases, where the smallest index wins"""
    q = np.array([-3.0, 3.0, 3.0, -3.0]), np.array([-3.0, -3.0, 3.0, 3.0])
    inner = np.random.default_rng(37).uniform(-3, 3, (2, 40))
    return {
        "square": np.column_stack([np.concatenate([q[0], inner[0]]), np.concatenate([q[1], inner[1]]),
                                   np.linspace(0.0, 9.0, 44)]),
        "single_point": np.array([[4.25, -7.5, 3.0]]),
        "two_points": np.array([[1.0, 2.0, 0.0], [6.0, 2.0, 5.0]]),
        "same_point_twice": np.array([[1.5, 2.5, 1.0], [1.5, 2.5, 1.0]]),
        "collinear_y": np.column_stack([np.full(9, 2.0), np.arange(9.0), np.arange(9.0)]),
        "collinear_diagonal": np.column_stack([np.arange(9.0), np.arange(9.0), np.zeros(9)]),
    }


def rectangles():
    """name -> dict(rows float32 [n,3], exact float64 [n,3] (before rounding), index (on-table cases, else None), area and
    aspect of the true rectangle (None for the zero-area cases))"""
    out = {}
    for name, (_, index) in RECT_ANGLES.items():
        exact = rectangle_rows(name)
        out[name] = dict(rows=exact.astype(np.float32), exact=exact, index=index,
                         area=RECT_SIDES[0] * RECT_SIDES[1], aspect=RECT_SIDES[0] / RECT_SIDES[1])
    for name, exact in degenerate_rows().items():
        square = name == "square"
        out[name] = dict(rows=exact.astype(np.float32), exact=exact, index=0 if square else None,
                         area=36.0 if square else None, aspect=1.0 if square else None)
    return out


def rectangles_cloud():
    """(P float32 [n,3], labels int32 [n], K, names): every rectangles() case as one cluster of one cloud, each moved
    to a place of its own (the statement is applied to the moved float32 rows), rows shuffled, noise in between"""
    cases = rectangles()
    names = list(cases)
    rng = np.random.default_rng(41)
    rows, lab = [], []
    for k, name in enumerate(names):
        shift = np.array([64.0 * k, -32.0 * k, 0.0]) if k % 2 else np.zeros(3)     # powers of two: exact in float32
        rows.append((cases[name]["rows"].astype(np.float64) + shift).astype(np.float32))
        lab.append(np.full((len(rows[-1]),), k, dtype=np.int32))
    rows.append(rng.uniform(-50, 50, (300, 3)).astype(np.float32))
    lab.append(np.full((300,), -1, dtype=np.int32))
    P, lab = np.vstack(rows), np.concatenate(lab)
    order = rng.permutation(len(lab))
    return P[order], lab[order], len(names), names
