"""Conductor spans: the numpy statement of steps 1 to 4 of include/pch_hip.h's rule, one loop per cluster, the bound on a
sum taken in another order, ``pipeline.conductor_spans`` restated on top of ``shape_cases.drop_mask_reference`` and
scikit-learn's DBSCAN, and the scene of three towers on a line (TEST INFRASTRUCTURE, pure numpy; imported by the CPU and
the GPU tests, not a conftest).  Nothing here knows about blocks, waves or partials."""
import numpy as np

import shape_cases as sc

U = 2.0 ** -53                                   # unit roundoff of float64
TABLE_KEYS = ("count", "centre", "direction", "azimuth_deg", "length", "a", "b", "c", "sag", "z_low", "rms_z", "rms_t",
              "cond")


# ------------------------------------------------------------------ grouping, as pch_segment_by_label writes it
def group_reference(labels, nclusters):
    """(perm int32 [n], offsets int64 [K+1]): rows ordered by (label, row), noise rows last"""
    labels = np.asarray(labels)
    key = np.where((labels < 0) | (labels >= nclusters), nclusters, labels)
    perm = np.argsort(key, kind="stable").astype(np.int32)
    offsets = np.searchsorted(key[perm], np.arange(nclusters + 1)).astype(np.int64)
    return perm, offsets


# ------------------------------------------------------------------ step 1
def moments_reference(P, perm, offsets):
    """(count int64 [K], origin float32 [K,3], moments float64 [K,9], abs float64 [K,9]: Σ|t| of every sum)"""
    P = np.asarray(P, dtype=np.float32).reshape(-1, 3)
    K = len(offsets) - 1
    count = np.zeros(K, dtype=np.int64)
    origin = np.zeros((K, 3), dtype=np.float32)
    M = np.zeros((K, 9), dtype=np.float64)
    A = np.zeros((K, 9), dtype=np.float64)
    for k in range(K):
        rows = perm[offsets[k]:offsets[k + 1]]
        count[k] = len(rows)
        if not len(rows):
            continue
        origin[k] = P[rows[0]]
        d = P[rows].astype(np.float64) - origin[k].astype(np.float64)
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        for a, t in enumerate((dx, dy, dz, dx * dx, dy * dy, dz * dz, dx * dy, dx * dz, dy * dz)):
            M[k, a] = t.sum()
            A[k, a] = np.abs(t).sum()
    return count, origin, M, A


def sum_bounds(n, abs_sums):
    """how far a sum of n terms may lie from the same sum in another order: each order is within (n+1)·u·Σ|t| of the
    exact sum, two are compared, hence 2(n+1)·u·Σ|t| (shape_cases.moment_bounds' argument with Σ|t| itself in place of
    n·r).  n [K], abs_sums [K,m] -> [K,m]"""
    n = np.asarray(n, dtype=np.float64)
    return 2.0 * (n[:, None] + 1.0) * U * np.asarray(abs_sums, dtype=np.float64)


# ------------------------------------------------------------------ step 2
def frames_reference(count, origin, M):
    """float64 [K,6]: (cx, cy, cz, ux, uy, 1/h)"""
    n = np.maximum(np.asarray(count, dtype=np.float64), 1.0)
    M = np.asarray(M, dtype=np.float64).reshape(-1, 9)
    F = np.zeros((len(M), 6), dtype=np.float64)
    for k in range(len(M)):
        if not np.isfinite(M[k]).all():                                   # non-finite rows: nothing to frame
            F[k] = np.nan
            continue
        mu = M[k, 0:3] / n[k]
        cxx = M[k, 3] / n[k] - mu[0] * mu[0]
        cyy = M[k, 4] / n[k] - mu[1] * mu[1]
        cxy = M[k, 6] / n[k] - mu[0] * mu[1]
        theta = 0.5 * np.arctan2(2.0 * cxy, cxx - cyy)
        ux, uy = np.cos(theta), np.sin(theta)
        if ux < 0 or (ux == 0 and uy < 0):
            ux, uy = -ux, -uy
        lam = 0.5 * (cxx + cyy) + np.hypot(0.5 * (cxx - cyy), cxy)
        h = np.sqrt(3.0 * max(lam, 0.0))
        if h == 0:
            h = 1.0
        F[k] = (origin[k, 0] + mu[0], origin[k, 1] + mu[1], origin[k, 2] + mu[2], ux, uy, 1.0 / h)
    return F


# ------------------------------------------------------------------ step 3
def profile_terms(P, rows, f):
    """the ten terms per row and (s, dz), with the rule's parentheses"""
    p = np.asarray(P, dtype=np.float32)[rows].astype(np.float64)
    dx, dy, dz = p[:, 0] - f[0], p[:, 1] - f[1], p[:, 2] - f[2]
    s = ((dx * f[3]) + (dy * f[4])) * f[5]
    t = (dy * f[3]) - (dx * f[4])
    s2 = s * s
    return (s, s2, s2 * s, s2 * s2, dz, s * dz, s2 * dz, dz * dz, t, t * t), s, dz


def profile_reference(P, perm, offsets, frames):
    """(sums float64 [K,10], ext float64 [K,4], abs float64 [K,10])"""
    K = len(offsets) - 1
    S = np.zeros((K, 10), dtype=np.float64)
    A = np.zeros((K, 10), dtype=np.float64)
    E = np.tile(np.array([np.inf, -np.inf, np.inf, -np.inf]), (K, 1))
    for k in range(K):
        rows = perm[offsets[k]:offsets[k + 1]]
        if not len(rows):
            continue
        terms, s, dz = profile_terms(P, rows, frames[k])
        for a, t in enumerate(terms):
            S[k, a] = t.sum()
            A[k, a] = np.abs(t).sum()
        # a NaN is never smaller or larger than anything: the extrema skip it, as the header says
        E[k] = (np.fmin.reduce(s, initial=np.inf), np.fmax.reduce(s, initial=-np.inf),
                np.fmin.reduce(dz, initial=np.inf), np.fmax.reduce(dz, initial=-np.inf))
    return S, E, A


# ------------------------------------------------------------------ step 4
def normal_matrix(n, S):
    return np.array([[n, S[0], S[1]], [S[0], S[1], S[2]], [S[1], S[2], S[3]]], dtype=np.float64)


def fit_reference(count, frames, sums, ext):
    """the span table as a dict of numpy arrays over the K clusters (ops.span_fit's keys)"""
    K = len(count)
    out = {key: np.full(K, np.nan) for key in TABLE_KEYS}
    out["count"] = np.asarray(count, dtype=np.int64).copy()
    out["centre"] = np.asarray(frames)[:, 0:3].copy()
    out["direction"] = np.asarray(frames)[:, 3:5].copy()
    for k in range(K):
        f, S, E = frames[k], sums[k], ext[k]
        n, n1 = float(count[k]), float(max(count[k], 1))
        h = 1.0 / f[5]
        width = E[1] - E[0] if count[k] > 0 else 0.0
        out["azimuth_deg"][k] = np.degrees(np.arctan2(f[4], f[3]))
        out["length"][k] = width * h
        mt = S[8] / n1
        out["rms_t"][k] = np.sqrt(max(S[9] / n1 - mt * mt, 0.0))
        G = normal_matrix(n, S)
        w = np.linalg.eigvalsh(G)
        regular = np.linalg.det(G) > 0 and w[0] > 0
        out["cond"][k] = w[2] / w[0] if regular else np.inf
        if count[k] < 3 or not regular:
            continue
        r = np.array([S[4], S[5], S[6]])
        a, b, c = np.linalg.solve(G, r)
        out["a"][k], out["b"][k], out["c"][k] = a, b / h, c / (h * h)
        out["sag"][k] = abs(c) * (0.5 * width) ** 2
        cand = [a + E[0] * (b + c * E[0]), a + E[1] * (b + c * E[1])]
        if c > 0 and E[0] <= -b / (2.0 * c) <= E[1]:
            sv = -b / (2.0 * c)
            cand.append(a + sv * (b + c * sv))
        out["z_low"][k] = min(cand) + f[2]
        out["rms_z"][k] = np.sqrt(max(S[7] - (a * r[0] + b * r[1] + c * r[2]), 0.0) / n1)
    return out


def table_bounds(table):
    """[K] how far an entry of the table may lie from the reference's: 64·(n+1)·u·cond·max(1, length) - the moments
    differ by at most 2(n+1)·u relative, the frame and the solve amplify that by cond, 64 is slack for the two chained
    steps"""
    n = np.asarray(table["count"], dtype=np.float64)
    return 64.0 * (n + 1.0) * U * np.asarray(table["cond"]) * np.maximum(1.0, np.asarray(table["length"]))


# ------------------------------------------------------------------ the pipeline call
def conductor_spans_reference(X, rule=None, eps=1.0, min_rows=5, towers=None, cut_radius=9.0, min_length=20.0,
                              max_rms_z=0.25, max_rms_t=0.25, mask=None):
    """pipeline.conductor_spans by the references.  ``mask``: a precomputed sc.drop_mask_reference result (it is
    all-pairs); the dict also carries ``features`` and ``neighbours`` of that mask and ``tower_d2`` [n] (the smallest
    squared horizontal distance to a tower, +inf without towers)"""
    from sklearn.cluster import DBSCAN
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    wire, feats, neigh = mask if mask is not None else sc.drop_mask_reference(X, **dict(sc.SCENE_RULE, **(rule or {})))
    wire = wire.copy()
    d2min = np.full(len(X), np.inf)
    if towers is not None and len(towers):
        tw = np.asarray(towers, dtype=np.float64)[:, :2]
        xy = X[:, :2].astype(np.float64)
        dx = xy[:, None, 0] - tw[None, :, 0]
        dy = xy[:, None, 1] - tw[None, :, 1]
        d2min = (dx * dx + dy * dy).min(1)
        wire &= ~(d2min <= float(cut_radius) * float(cut_radius))
    rows = X[wire]
    if len(rows):
        labels = DBSCAN(eps=eps, min_samples=min_rows, algorithm="ball_tree").fit(rows).labels_.astype(np.int32)
    else:
        labels = np.zeros(0, dtype=np.int32)
    K = int(labels.max()) + 1 if len(labels) else 0
    perm, offsets = group_reference(labels, K)
    count, origin, M, _ = moments_reference(rows, perm, offsets)
    frames = frames_reference(count, origin, M)
    S, E, _ = profile_reference(rows, perm, offsets, frames)
    table = fit_reference(count, frames, S, E)
    with np.errstate(invalid="ignore"):
        accepted = (table["length"] >= min_length) & (table["rms_z"] <= max_rms_z) & (table["rms_t"] <= max_rms_t)
    return dict(wire=wire, labels=labels, nclusters=K, perm=perm, offsets=offsets, table=table, accepted=accepted,
                features=feats, neighbours=neigh, tower_d2=d2min, frames=frames, sums=S, ext=E)


# ------------------------------------------------------------------ the scene: three towers on a line
LINE_ROWS = 12867
LINE_AZIMUTH_DEG = 20.0
LINE_STATIONS = (0.0, 80.0, 150.0)
LINE_BASES = (0.0, 5.0, 12.0)
LINE_SAGS = (2.0, 2.5)
LINE_OFFSETS = (-6.0, 0.0, 6.0)
_LINE = {}
_REF = {}


def _line_xy(station, lateral):
    a = np.radians(LINE_AZIMUTH_DEG)
    return np.stack([station * np.cos(a) - lateral * np.sin(a), station * np.sin(a) + lateral * np.cos(a)], axis=1)


def line_towers():
    """float64 [3,3]: the tower axes' feet in the scene's frame"""
    st = np.array(LINE_STATIONS)
    return np.concatenate([_line_xy(st, np.zeros(3)), np.array(LINE_BASES)[:, None]], axis=1)


def line_scene():
    """(X float32 [12867,3], kind int8 [12867]).  Three of ``shape_cases.scene``'s towers (2000 rows of a tapering
    column, 500 of a cross-arm, the arm across the line) at stations 0, 80 and 150 m of a line at azimuth 20 degrees,
    bases at z = 0, 5 and 12.  Per span three conductors at lateral offsets -6, 0 and +6: one row every 0.1 m of
    station, attached 21 m above each base, a parabola below the chord with mid-span sag 2.0 m (first span) and 2.5 m
    (second), N(0, 0.02) jitter per coordinate.  One Gaussian blob of 800 rows (sigma 1.5 m) beside the first span and
    one 6 m horizontal bar of 61 rows beside the second.  Cast to float32, then permuted.  kind: 0 tower, 1 + 3 span +
    conductor for the six conductors, 7 blob, 8 bar."""
    if not _LINE:
        rng = np.random.default_rng(5)
        parts, kind = [], []
        for st, base in zip(LINE_STATIONS, LINE_BASES):
            z = rng.uniform(0.0, 30.0, 2000)
            hw = 4.0 - 3.0 * z / 30.0
            col = np.concatenate([_line_xy(st + rng.uniform(-1.0, 1.0, 2000) * hw, rng.uniform(-1.0, 1.0, 2000) * hw),
                                  (base + z)[:, None]], axis=1)
            arm = np.concatenate([_line_xy(st + rng.uniform(-1.0, 1.0, 500), rng.uniform(-8.0, 8.0, 500)),
                                  (base + rng.uniform(25.0, 27.0, 500))[:, None]], axis=1)
            parts += [col, arm]
            kind += [np.zeros(2500, dtype=np.int8)]
        for sp in range(2):
            s0, s1 = LINE_STATIONS[sp], LINE_STATIONS[sp + 1]
            z0, z1 = LINE_BASES[sp] + 21.0, LINE_BASES[sp + 1] + 21.0
            st = s0 + np.arange(int(round((s1 - s0) * 10)) + 1) * 0.1
            tau = (st - s0) / (s1 - s0)
            z = z0 + (z1 - z0) * tau - 4.0 * LINE_SAGS[sp] * tau * (1.0 - tau)
            for c, lat in enumerate(LINE_OFFSETS):
                line = np.concatenate([_line_xy(st, np.full_like(st, lat)), z[:, None]], axis=1)
                parts.append(line + rng.normal(0.0, 0.02, line.shape))
                kind.append(np.full(len(st), 1 + 3 * sp + c, dtype=np.int8))
        blob = np.concatenate([_line_xy(np.array([40.0]), np.array([22.0])), [[12.0]]], axis=1)
        parts.append(blob + rng.normal(0.0, 1.5, (800, 3)))
        kind.append(np.full(800, 7, dtype=np.int8))
        st = 110.0 + np.arange(61) * 0.1
        bar = np.concatenate([_line_xy(st, np.full_like(st, -22.0)), np.full((61, 1), 14.0)], axis=1)
        parts.append(bar + rng.normal(0.0, 0.02, bar.shape))
        kind.append(np.full(61, 8, dtype=np.int8))
        P = np.vstack(parts)
        kind = np.concatenate(kind)
        perm = rng.permutation(len(P))
        X = P.astype(np.float32)[perm]
        kind = kind[perm]
        for a in (X, kind):
            a.setflags(write=False)
        _LINE["case"] = (X, kind)
    return _LINE["case"]


def scene_towers():
    """the axes' feet of ``shape_cases.scene``'s two towers"""
    return np.array([[0.0, 0.0, 0.0], [60.0, 0.0, 0.0]])


def reference(name):
    """the reference answers the CPU and the GPU tests share, computed once: name in 'scene', 'scene_cut', 'line',
    'line_cut' (cut: with the towers given, cut_radius 9)"""
    if name not in _REF:
        base = name.split("_")[0]
        X = sc.scene()[0] if base == "scene" else line_scene()[0]
        if "mask_" + base not in _REF:
            _REF["mask_" + base] = sc.drop_mask_reference(X, **sc.SCENE_RULE)
        towers = None if not name.endswith("_cut") else (scene_towers() if base == "scene" else line_towers())
        _REF[name] = conductor_spans_reference(X, towers=towers, mask=_REF["mask_" + base])
    return _REF[name]
