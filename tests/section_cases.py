"""Span sections: the numpy statement of include/pch_hip.h's rule - per row and span, per cell, per row -, an independent
statement of the same section in space (the distance of a point to the vertical strip through the track, its height
under the parabola), random sagging spans with rows under them, the rule's boundaries on dyadic values, and the scene:
``clearance_cases.tree_scene`` (TEST INFRASTRUCTURE, pure numpy; imported by the CPU and the GPU tests, not a conftest).
The statement loops spans over all rows; nothing here knows about tiles, bounds, waves or culling."""
import numpy as np

import clearance_cases as cc

OUTPUTS = ("count", "violations", "min_v", "min_row", "v", "span", "station")
STATIONS, HALF, DEPTH, LIMIT = 64, 15.0, 80.0, 7.0


# ------------------------------------------------------------------ the rule
def takes_part(curves):
    """bool [K]: all ten values finite and m1 > m0"""
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 10)
    with np.errstate(invalid="ignore"):
        return np.isfinite(curves).all(axis=1) & (curves[:, 9] > curves[:, 8])


def span_pairs(X, curve, B, half, depth):
    """(part bool [n], v float64 [n], j int64 [n]) of float32 rows against one span that takes part: the rule's lines,
    one after the other; j is 0 where the row takes no part"""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    px, py, pz = (X[:, i].astype(np.float64) for i in range(3))
    cx, cy, cz, ux, uy, a, b, c, m0, m1 = (float(v) for v in curve)
    with np.errstate(all="ignore"):
        step = (m1 - m0) / float(B)
        dx, dy, w = px - cx, py - cy, pz - cz
        m = (dx * ux) + (dy * uy)
        t = (dy * ux) - (dx * uy)
        corridor = (m >= m0) & (m <= m1) & (t >= -half) & (t <= half)
        zw = a + (m * (b + (c * m)))
        v = zw - w
        part = corridor & (v >= 0.0) & (v <= depth) & np.isfinite(X).all(axis=1)
        j = np.floor(np.where(part, m - m0, 0.0) / step)
        j = np.where(j > B - 1, B - 1, j).astype(np.int64)
    return part, v, j


def section_reference(X, curves, B, half, depth, limit, skip=None):
    """dict of OUTPUTS: count / violations int64 [K,B], min_v float32 [K,B], min_row int64 [K,B], v float32 [n],
    span / station int32 [n]; spans in ascending k, ``if vf < best``"""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 10)
    K, n = len(curves), len(X)
    alive = np.ones(n, dtype=bool) if skip is None else np.asarray(skip).reshape(-1) == 0
    count = np.zeros((K, B), dtype=np.int64)
    viol = np.zeros((K, B), dtype=np.int64)
    min_v = np.full((K, B), np.inf, dtype=np.float32)
    min_row = np.full((K, B), -1, dtype=np.int64)
    best = np.full(n, np.inf, dtype=np.float32)
    who = np.full(n, -1, dtype=np.int32)
    at = np.full(n, -1, dtype=np.int32)
    use = takes_part(curves)
    for k in range(K):
        if not use[k]:
            continue
        part, v, j = span_pairs(X, curves[k], B, half, depth)
        part &= alive
        vf = np.abs(v.astype(np.float32))
        rows = np.flatnonzero(part)
        for i in rows:                                                         # ascending: the first to attain stays
            c = j[i]
            count[k, c] += 1
            viol[k, c] += int(v[i] <= limit)
            if vf[i] < min_v[k, c]:
                min_v[k, c], min_row[k, c] = vf[i], i
        take = part & (vf < best)
        best = np.where(take, vf, best)
        who = np.where(take, np.int32(k), who)
        at = np.where(take, j.astype(np.int32), at)
    return dict(count=count, violations=viol, min_v=min_v, min_row=min_row, v=best, span=who, station=at)


# ------------------------------------------------------------------ an independent statement, in space
def strip_brute(X, curve, B, half, depth, limit):
    """per row of one span, by vectors in space: ``s`` the station of the row's foot on the track line (metres from
    the centre), ``lateral`` its distance to the vertical plane through the track (np.linalg.norm of the rejection),
    ``v`` the height of the parabola's world point over the foot above the row, ``j`` the station index by proportion,
    ``part`` / ``viol`` the section's two tests and ``margin``, how far the row is from the nearest decision (a side or
    end of the strip, the wire, the depth, the limit, a station boundary), metres"""
    P = np.asarray(X, dtype=np.float32).astype(np.float64)
    cx, cy, cz, ux, uy, a, b, c, m0, m1 = (float(v) for v in curve)
    u = np.array([ux, uy])
    rel = P[:, :2] - np.array([cx, cy])
    s = rel @ u
    lateral = np.linalg.norm(rel - s[:, None] * u[None, :], axis=1)
    wire = cz + a + b * s + c * s * s
    v = wire - P[:, 2]
    frac = (s - m0) / (m1 - m0) * B
    j = np.minimum(np.floor(frac), B - 1).astype(np.int64)
    part = (s >= m0) & (s <= m1) & (lateral <= half) & (v >= 0.0) & (v <= depth)
    edges = np.abs(frac - np.round(frac)) * (m1 - m0) / B
    edges = np.where(np.round(frac) >= B, np.inf, edges)                        # beyond the last boundary: clamped anyway
    margin = np.minimum.reduce([np.abs(s - m0), np.abs(s - m1), np.abs(lateral - half), np.abs(v), np.abs(v - depth),
                                np.abs(v - limit), edges])
    return dict(s=s, lateral=lateral, v=v, j=np.where(part, j, 0), part=part, viol=part & (v <= limit), margin=margin)


# ------------------------------------------------------------------ random sagging spans with rows under them
def random_case(n, K, seed, shift=None, spread=120.0, phases=False):
    """(X float32 [n,3], curves float64 [K,10]): K random sagging, sloped spans in a square of ``spread`` metres
    (``phases``: in groups of three parallel ones 4 m apart) and n rows, four in five of them scattered about a span -
    beyond its ends, beside its corridor, above the wire and up to 30 m below it -, the others anywhere"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-0.5 * np.pi, 0.5 * np.pi, K)
    half = rng.uniform(10.0, 35.0, K)
    C = np.stack([rng.uniform(0.0, spread, K), rng.uniform(0.0, spread, K), rng.uniform(25.0, 40.0, K), np.cos(ang),
                  np.sin(ang), rng.uniform(-0.5, 0.5, K), rng.uniform(-0.1, 0.1, K), rng.uniform(0.0, 0.01, K),
                  -half * rng.uniform(0.8, 1.0, K), half], axis=1).reshape(K, 10)
    if phases:
        for k in range(K):
            if k % 3:
                C[k] = C[k - k % 3]
                C[k, 0] -= (k % 3) * 4.0 * C[k, 4]
                C[k, 1] += (k % 3) * 4.0 * C[k, 3]
    X = np.concatenate([rng.uniform(-20.0, spread + 20.0, (n, 2)), rng.uniform(0.0, 40.0, (n, 1))], axis=1)
    if K:
        k = rng.integers(0, K, n)
        m = rng.uniform(C[k, 8] - 8.0, C[k, 9] + 8.0)
        t = rng.normal(0.0, 8.0, n)
        z = C[k, 2] + C[k, 5] + m * (C[k, 6] + C[k, 7] * m) - rng.uniform(-3.0, 30.0, n)
        near = np.stack([C[k, 0] + m * C[k, 3] - t * C[k, 4], C[k, 1] + m * C[k, 4] + t * C[k, 3], z], axis=1)
        X = np.where((rng.uniform(0.0, 1.0, n) < 0.8)[:, None], near, X)
    if shift is not None:
        X = X + shift
        C[:, 0:3] += shift
    return X.astype(np.float32), C


# ------------------------------------------------------------------ the rule's boundaries on dyadic values
E_STATIONS, E_HALF, E_DEPTH, E_LIMIT = 4, 4.0, 16.0, 4.0


def edge_case():
    """(X float32 [31,3], skip uint8, curves [3,10], want): the wire z = 32 + m*m/64 over m in [-32, 32] along x at
    y = 0 (span 1; span 0 is the same wire with m1 == m0 and takes no part, span 2 the same wire again: every cell of
    it equals span 1's and no row goes to it) with four stations of 16 m, a corridor of +-4 m, depth 16 and limit 4: m,
    t, zw and v are exact.  ``want``: per row (takes part, station, violation) as the rule's text says"""
    f32 = np.float32
    below = lambda v: np.nextafter(f32(v), f32(-np.inf))
    above = lambda v: np.nextafter(f32(v), f32(np.inf))
    wire = cc.curve(a=32.0, c=1.0 / 64.0, m0=-32.0, m1=32.0)
    none = wire.copy()
    none[9] = none[8]
    curves = np.stack([none, wire, wire])
    rows = [([-32.0, 0.0, 40.0], (True, 0, False)),            # 0: m == m0, zw = 48, v = 8
            ([below(-32.0), 0.0, 40.0], (False, -1, False)),   # 1: before the first station
            ([32.0, 0.0, 40.0], (True, 3, False)),             # 2: m == m1: floor gives 4, the last station takes it
            ([above(32.0), 0.0, 40.0], (False, -1, False)),    # 3
            ([16.0, 0.0, 30.0], (True, 3, False)),             # 4: on a station boundary, zw = 36, v = 6: the upper one
            ([below(16.0), 0.0, 30.0], (True, 2, False)),      # 5: one float32 below it
            ([above(16.0), 0.0, 30.0], (True, 3, False)),      # 6
            ([0.0, 0.0, 22.0], (True, 2, False)),              # 7: the boundary at the centre, v = 10
            ([-16.0, 0.0, 30.0], (True, 1, False)),            # 8
            ([below(-16.0), 0.0, 30.0], (True, 0, False)),     # 9
            ([8.0, 4.0, 25.0], (True, 2, False)),              # 10: t == half, zw = 33, v = 8
            ([8.0, above(4.0), 25.0], (False, -1, False)),     # 11
            ([8.0, -4.0, 25.0], (True, 2, False)),             # 12: t == -half
            ([8.0, below(-4.0), 25.0], (False, -1, False)),    # 13
            ([0.0, 1.0, 32.0], (True, 2, True)),               # 14: v == 0: touches the wire
            ([0.0, 1.0, above(32.0)], (False, -1, False)),     # 15: above the wire
            ([0.0, 1.0, below(32.0)], (True, 2, True)),        # 16
            ([0.0, 2.0, 28.0], (True, 2, True)),               # 17: v == limit: a violation
            ([0.0, 2.0, below(28.0)], (True, 2, False)),       # 18: v just above the limit
            ([0.0, 2.0, above(28.0)], (True, 2, True)),        # 19
            ([0.0, 3.0, 16.0], (True, 2, False)),              # 20: v == depth
            ([0.0, 3.0, below(16.0)], (False, -1, False)),     # 21: deeper
            ([0.0, 3.0, above(16.0)], (True, 2, False)),       # 22
            ([3.0, 0.0, 50.0], (False, -1, False)),            # 23: far above the wire
            ([np.inf, 0.0, 30.0], (False, -1, False)), ([0.0, -np.inf, 30.0], (False, -1, False)),     # 24, 25
            ([0.0, 0.0, np.nan], (False, -1, False)), ([0.0, 0.0, -np.inf], (False, -1, False)),       # 26, 27
            ([0.0, 0.0, 30.0], (False, -1, False)),            # 28: skipped
            ([-24.0, -0.0, 40.0], (True, 0, True)),            # 29: zw = 41, v = 1
            ([24.0, 0.5, 40.5], (True, 3, True))]              # 30: v = 0.5
    X = np.array([r[0] for r in rows], dtype=np.float32)
    skip = np.zeros(len(X), dtype=np.uint8)
    skip[28] = 1
    return X, skip, curves, [r[1] for r in rows]


# ------------------------------------------------------------------ the scene
_REF = {}


def reference():
    """``clearance_cases.reference``'s ``spans`` / ``idx`` / ``curves`` / ``skip`` / ``tol`` / ``kind`` and the outputs
    of ``section_reference`` on ``tree_scene`` at STATIONS, HALF, DEPTH and LIMIT, computed once; ``margin`` float64 [n]:
    how far, at the least, a row that is not skipped stands from a decision of any span's section (strip_brute)"""
    if not _REF:
        X, kind = cc.tree_scene()
        r = cc.reference()
        out = section_reference(X, r["curves"], STATIONS, HALF, DEPTH, LIMIT, skip=r["skip"])
        margin = np.minimum.reduce([strip_brute(X, c, STATIONS, HALF, DEPTH, LIMIT)["margin"] for c in r["curves"]])
        _REF.update(out, spans=r["spans"], idx=r["idx"], curves=r["curves"], skip=r["skip"], tol=r["tol"], kind=kind,
                    margin=np.where(r["skip"] == 0, margin, np.inf))
    return _REF
