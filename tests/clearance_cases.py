"""Conductor clearance: the numpy statement of include/pch_hip.h's rule - curves, polyline, per row and span, per span -,
an independent statement of the same distances on world-space vertices, and the scene: ``span_cases.line_scene`` with
three trees under and beside the conductors (TEST INFRASTRUCTURE, pure numpy; imported by the CPU and the GPU tests, not
a conftest).  The statement loops spans and segments over all rows; nothing here knows about tiles, bounds or culling."""
import numpy as np

import shape_cases as sc
import span_cases as sp

RADIUS, LIMIT, SEGMENTS = 10.0, 6.0, 32


# ------------------------------------------------------------------ curves and polyline
def curves_reference(table, frames, ext):
    """float64 [K,10]: (cx, cy, cz, ux, uy, a, b, c, m0, m1)"""
    F = np.asarray(frames, dtype=np.float64).reshape(-1, 6)
    E = np.asarray(ext, dtype=np.float64).reshape(-1, 4)
    h = 1.0 / F[:, 5]
    cols = [F[:, 0], F[:, 1], F[:, 2], F[:, 3], F[:, 4]] + [np.asarray(table[k], dtype=np.float64) for k in "abc"]
    return np.stack(cols + [E[:, 0] * h, E[:, 1] * h], axis=1)


def segments_reference(curves, S):
    """(segs float64 [K,S,5] = (m_j, z_j, dm_j, dz_j, inv_j), chord_error float64 [K]), one loop per span and vertex"""
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 10)
    K = len(curves)
    segs = np.zeros((K, S, 5), dtype=np.float64)
    chord = np.zeros(K, dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(K):
            a, b, c, m0, m1 = curves[k, 5:10]
            step = (m1 - m0) / float(S)
            m = np.array([m0 + float(j) * step for j in range(S)] + [m1])
            z = np.array([a + mj * (b + c * mj) for mj in m])
            for j in range(S):
                dm, dz = m[j + 1] - m[j], z[j + 1] - z[j]
                len2 = (dm * dm) + (dz * dz)
                segs[k, j] = (m[j], z[j], dm, dz, 1.0 / len2 if len2 > 0 else 0.0)
            chord[k] = (abs(c) * (step * step)) / 4.0
    return segs, chord


def curve(cx=0.0, cy=0.0, cz=0.0, ux=1.0, uy=0.0, a=0.0, b=0.0, c=0.0, m0=-8.0, m1=8.0):
    """one row of a curves table"""
    return np.array([cx, cy, cz, ux, uy, a, b, c, m0, m1], dtype=np.float64)


# ------------------------------------------------------------------ per row and span, per span
def span_distances(X, curves, segs):
    """float64 [K,n]: the rule's d2 of every row to every span (NaN / inf as IEEE arithmetic gives them), rows in
    float32 as the kernel reads them; spans that take no part have +inf"""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    curves = np.asarray(curves, dtype=np.float64)
    segs = np.asarray(segs, dtype=np.float64)
    K, S = segs.shape[0], segs.shape[1]
    px, py, pz = (X[:, i].astype(np.float64) for i in range(3))
    out = np.full((K, len(X)), np.inf)
    with np.errstate(all="ignore"):
        for k in range(K):
            if not (np.isfinite(curves[k, :5]).all() and np.isfinite(segs[k]).all()):
                continue
            cx, cy, cz, ux, uy = curves[k, :5]
            dx, dy, w = px - cx, py - cy, pz - cz
            m = (dx * ux) + (dy * uy)
            t = (dy * ux) - (dx * uy)
            g = np.full(len(X), np.inf)
            for j in range(S):
                mj, zj, dm, dz, inv = segs[k, j]
                rm, rw = m - mj, w - zj
                q = ((rm * dm) + (rw * dz)) * inv
                q = np.where(q < 0, 0.0, q)
                q = np.where(q > 1, 1.0, q)
                em, ew = rm - (q * dm), rw - (q * dz)
                d = (em * em) + (ew * ew)
                g = np.where(d < g, d, g)
            out[k] = g + (t * t)
    return out


def clearance_reference(X, curves, segs, radius, limit, skip=None, d2=None):
    """dict: dist2 float64 [n], span int32 [n], count / violations int64 [K], min_dist2 float64 [K], min_row int64 [K];
    ``d2``: a precomputed ``span_distances``"""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    K, n = np.asarray(segs).shape[0], len(X)
    r2, l2 = float(radius) * float(radius), float(limit) * float(limit)
    d2 = span_distances(X, curves, segs) if d2 is None else d2
    alive = np.ones(n, dtype=bool) if skip is None else np.asarray(skip).reshape(-1) == 0
    best = np.full(n, np.inf)
    who = np.full(n, -1, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for k in range(K):
            take = alive & (d2[k] <= r2) & (d2[k] < best)
            best = np.where(take, d2[k], best)
            who = np.where(take, np.int32(k), who)
    count = np.zeros(K, dtype=np.int64)
    viol = np.zeros(K, dtype=np.int64)
    mind = np.full(K, np.inf)
    minrow = np.full(K, -1, dtype=np.int64)
    for k in range(K):
        rows = np.flatnonzero(who == k)
        count[k] = len(rows)
        viol[k] = int((best[rows] <= l2).sum())
        if len(rows):
            mind[k] = best[rows].min()
            minrow[k] = rows[best[rows] == mind[k]][0]
    return dict(dist2=best, span=who, count=count, violations=viol, min_dist2=mind, min_row=minrow)


OUTPUTS = ("dist2", "span", "count", "violations", "min_dist2", "min_row")


# ------------------------------------------------------------------ an independent statement
def polyline_world(curves, S):
    """float64 [K,S+1,3]: the vertices of the S-segment polyline in world coordinates, straight from the curve"""
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 10)
    tau = np.arange(S + 1, dtype=np.float64) / S
    m = curves[:, 8:9] * (1.0 - tau) + curves[:, 9:10] * tau
    z = curves[:, 5:6] + curves[:, 6:7] * m + curves[:, 7:8] * m * m
    return np.stack([curves[:, 0:1] + m * curves[:, 3:4], curves[:, 1:2] + m * curves[:, 4:5], curves[:, 2:3] + z],
                    axis=2)


def polyline_distance(P, V):
    """float64 [n]: the distance of the points P [n,3] to the polyline with vertices V [S+1,3], by np.linalg.norm on
    the vectors in space"""
    P = np.asarray(P, dtype=np.float64)
    out = np.full(len(P), np.inf)
    for j in range(len(V) - 1):
        e = V[j + 1] - V[j]
        ee = float(e @ e)
        q = np.clip(((P - V[j]) @ e) / ee, 0.0, 1.0) if ee > 0 else np.zeros(len(P))
        out = np.minimum(out, np.linalg.norm(P - (V[j] + q[:, None] * e), axis=1))
    return out


# ------------------------------------------------------------------ the scene: the line with three trees
TREES = (("breach", 40.0, 0.0, 17.0), ("near", 115.0, -6.0, 19.5), ("between", 60.0, 2.6, 18.5))
TREE_ROWS = 150
_SCENE = {}
_REF = {}


def tree_scene():
    """(X float32 [12867 + 450, 3], kind int8): ``span_cases.line_scene`` followed by three cones of 150 rows each
    (apex up, 6 m high, 2 m base radius), kind 10, 11, 12: "breach" under the middle conductor of the first span at
    station 40, apex 4.5 m below the wire; "near" under the outer conductor (lateral -6) of the second span at station
    115, apex 7.5 m below it - inside the radius, outside the limit; "between" at lateral 2.6 and station 60, between
    the middle and an outer conductor.  The trees keep 4 m and more from every conductor, twice the wire rule's
    radius, so the wire rows and the span table are ``line_scene``'s."""
    if not _SCENE:
        X, kind = sp.line_scene()
        rng = np.random.default_rng(23)
        parts, kinds = [X], [kind]
        for i, (_, station, lateral, apex) in enumerate(TREES):
            depth = rng.uniform(0.0, 6.0, TREE_ROWS)
            rad = rng.uniform(0.0, 1.0, TREE_ROWS) * depth / 3.0
            ang = rng.uniform(0.0, 2.0 * np.pi, TREE_ROWS)
            xy = sp._line_xy(station + rad * np.cos(ang), lateral + rad * np.sin(ang))
            parts.append(np.concatenate([xy, (apex - depth)[:, None]], axis=1).astype(np.float32))
            kinds.append(np.full(TREE_ROWS, 10 + i, dtype=np.int8))
        X, kind = np.vstack(parts), np.concatenate(kinds)
        for a in (X, kind):
            a.setflags(write=False)
        _SCENE["case"] = (X, kind)
    return _SCENE["case"]


def reference():
    """the scene's reference answers, computed once: ``spans`` (span_cases.conductor_spans_reference with the towers),
    ``idx`` (the accepted pieces), ``curves``, ``segs``, ``chord``, ``skip``, ``d2`` [K,n], ``tol`` and the outputs of
    ``clearance_reference`` at RADIUS, LIMIT, SEGMENTS.  The scene's margins are asserted here, on the host."""
    if not _REF:
        X, kind = tree_scene()
        # the wire rule looks 2 m around a row and no tree row lies that close to a row of the line, so the all-pairs
        # mask of the scene is the line's (shared with the span tests) followed by the trees' own
        n0 = sp.LINE_ROWS
        sp.reference("line_cut")
        gap = min(float(np.sqrt(((X[n0:, None, :].astype(np.float64) - X[None, i:min(i + 2048, n0), :]) ** 2).sum(2).min()))
                  for i in range(0, n0, 2048))
        assert gap > 2.0 * sc.SCENE_RULE["radius"], gap
        wire = np.concatenate([sp._REF["mask_line"][0], sc.drop_mask_reference(X[n0:], **sc.SCENE_RULE)[0]])
        assert not wire[n0:].any()
        spans = sp.conductor_spans_reference(X, towers=sp.line_towers(), mask=(wire, None, None))
        idx = np.flatnonzero(spans["accepted"])
        assert len(idx) == 6
        curves = curves_reference(spans["table"], spans["frames"], spans["ext"])[idx]
        segs, chord = segments_reference(curves, SEGMENTS)
        skip = (spans["wire"] | (spans["tower_d2"] <= 9.0 * 9.0)).astype(np.uint8)
        d2 = span_distances(X, curves, segs)
        out = clearance_reference(X, curves, segs, RADIUS, LIMIT, skip=skip, d2=d2)
        # how far the device's table may move a distance: a, b·m, c·m² and the centre each by a table bound
        Lm = float(np.abs(curves[:, 8:10]).max())
        tol = (1.0 + Lm + Lm * Lm) * float(np.max(sp.table_bounds(spans["table"])[idx]))
        alive = skip == 0
        dist = np.sqrt(d2[:, alive])
        assert tol < 2e-5, tol
        assert np.abs(dist - RADIUS).min() > 10.0 * tol and np.abs(dist - LIMIT).min() > 10.0 * tol
        two = np.sort(dist, axis=0)[:2]
        assert (two[1] - two[0])[two[0] <= RADIUS].min() > 10.0 * tol
        _REF.update(out, spans=spans, idx=idx, curves=curves, segs=segs, chord=chord, skip=skip, d2=d2, tol=tol,
                    kind=kind)
    return _REF
