"""Tower profile: the numpy statement of include/pch_hip.h's rule - the slice table per (table, slice), looped literally
-, a second statement (a sort by (slot, slice), then ``np.minimum.reduceat`` on the keys), ``levels_reference`` (cross-arm
levels, top, heights) and the scene: ``span_cases.line_scene`` / ``terrain_cases.terrain_scene``, whose towers are a 30 m
column tapering from 8 m to 2 m wide with a 16 m arm at 25 - 27 m above the base (TEST INFRASTRUCTURE, pure numpy; imported
by the CPU and the GPU tests, not a conftest).  Nothing here knows about blocks, waves or atomics."""
import numpy as np

import span_cases as sp
import terrain_cases as tc

U = 2.0 ** -53
EMPTY = (np.inf, -np.inf, np.inf, -np.inf)
DZS = (0.25, 0.5, 1.0)
MIN_ROWS, ARM_WINDOW, ARM_EXCESS, MAX_LEVELS = 3, 3.0, 4.0, 8
EXCESS_MARGIN = 2.0                              # every w - body is at least this far from ARM_EXCESS in the scene
BOUNDARY_MARGIN = 1.9e-5                         # no scene row is nearer than this to a slice boundary, metres
ARM_LOW, TOWER_TOP = 25.0, 30.0                  # above the base


# ------------------------------------------------------------------ keys
def key64(v):
    """key(v) = bits(v) ^ (bits(v) >> 63 ? 0xFFFFFFFFFFFFFFFF : 0x8000000000000000)"""
    bits = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return bits ^ np.where(bits >> np.uint64(63), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0x8000000000000000))


def unkey64(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return (k ^ np.where(k >> np.uint64(63), np.uint64(0x8000000000000000), np.uint64(0xFFFFFFFFFFFFFFFF))).view(np.float64)


# ------------------------------------------------------------------ the slice table
def row_terms(P, rows, f, dz):
    """(s, t, q) per row of a cluster with frame f = (cx, cy, z0, ux, uy), the rule's parentheses"""
    p = np.asarray(P, dtype=np.float32).reshape(-1, 3)[rows].astype(np.float64)
    with np.errstate(all="ignore"):
        dx, dy, h = p[:, 0] - f[0], p[:, 1] - f[1], p[:, 2] - f[2]
        s = (dx * f[3]) + (dy * f[4])
        t = (dy * f[3]) - (dx * f[4])
        q = np.floor(h / dz)
    return s, t, q


def takes_part(frames5, slot, T):
    frames5 = np.asarray(frames5, dtype=np.float64).reshape(-1, 5)
    slot = np.asarray(slot).reshape(-1)
    return (slot >= 0) & (slot < T) & np.isfinite(frames5).all(axis=1)


def slices_reference(P, perm, offsets, frames5, slot, T, dz, B):
    """(count int32 [T,B], ext float64 [T,B,4], outside int64 [T,2]): one loop over the clusters and their rows"""
    frames5 = np.asarray(frames5, dtype=np.float64).reshape(-1, 5)
    K = len(offsets) - 1
    count = np.zeros((T, B), dtype=np.int32)
    kmin = np.full((T, B, 2), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    kmax = np.zeros((T, B, 2), dtype=np.uint64)
    outside = np.zeros((T, 2), dtype=np.int64)
    part = takes_part(frames5, slot, T)
    for k in range(K):
        if not part[k]:
            continue
        rows = perm[offsets[k]:offsets[k + 1]]
        if not len(rows):
            continue
        s, t, q = row_terms(P, rows, frames5[k], dz)
        ks, kt = key64(s), key64(t)
        for i in range(len(rows)):
            if q[i] < 0:
                outside[slot[k], 0] += 1
            if q[i] >= B:
                outside[slot[k], 1] += 1
            if not (0 <= q[i] < B and np.isfinite(s[i]) and np.isfinite(t[i])):
                continue
            b = int(q[i])
            count[slot[k], b] += 1
            kmin[slot[k], b, 0] = min(kmin[slot[k], b, 0], ks[i])
            kmax[slot[k], b, 0] = max(kmax[slot[k], b, 0], ks[i])
            kmin[slot[k], b, 1] = min(kmin[slot[k], b, 1], kt[i])
            kmax[slot[k], b, 1] = max(kmax[slot[k], b, 1], kt[i])
    ext = np.empty((T, B, 4), dtype=np.float64)
    ext[:] = EMPTY
    has = count > 0
    for c, (src, j) in enumerate(((kmin, 0), (kmax, 0), (kmin, 1), (kmax, 1))):
        ext[..., c][has] = unkey64(src[..., j][has])
    return count, ext, outside


def slices_by_sort(P, perm, offsets, frames5, slot, T, dz, B):
    """the same through a sort of the binned rows by (slot, slice) and ``reduceat`` over the runs"""
    frames5 = np.asarray(frames5, dtype=np.float64).reshape(-1, 5)
    K = len(offsets) - 1
    part = takes_part(frames5, slot, T)
    S, Tt, Q, W = [], [], [], []
    for k in range(K):
        rows = perm[offsets[k]:offsets[k + 1]]
        if part[k] and len(rows):
            s, t, q = row_terms(P, rows, frames5[k], dz)
            S.append(s), Tt.append(t), Q.append(q), W.append(np.full(len(rows), slot[k], dtype=np.int64))
    count = np.zeros((T, B), dtype=np.int32)
    ext = np.empty((T, B, 4), dtype=np.float64)
    ext[:] = EMPTY
    outside = np.zeros((T, 2), dtype=np.int64)
    if not S:
        return count, ext, outside
    s, t, q, w = (np.concatenate(v) for v in (S, Tt, Q, W))
    with np.errstate(invalid="ignore"):
        np.add.at(outside[:, 0], w[q < 0], 1)
        np.add.at(outside[:, 1], w[q >= B], 1)
        binned = (q >= 0) & (q < B) & np.isfinite(s) & np.isfinite(t)
    s, t, e = s[binned], t[binned], w[binned] * B + q[binned].astype(np.int64)
    if not len(e):
        return count, ext, outside
    order = np.argsort(e, kind="stable")
    s, t, e = s[order], t[order], e[order]
    entries, first, counts = np.unique(e, return_index=True, return_counts=True)
    count.reshape(-1)[entries] = counts
    flat = ext.reshape(-1, 4)
    ks, kt = key64(s), key64(t)
    flat[entries, 0] = unkey64(np.minimum.reduceat(ks, first))
    flat[entries, 1] = unkey64(np.maximum.reduceat(ks, first))
    flat[entries, 2] = unkey64(np.minimum.reduceat(kt, first))
    flat[entries, 3] = unkey64(np.maximum.reduceat(kt, first))
    return count, ext, outside


# ------------------------------------------------------------------ levels
def widths(count, ext, min_rows):
    """(occ bool [B], w float64 [B]) of one table row"""
    occ = np.asarray(count) >= min_rows
    ext = np.asarray(ext, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        w = np.where(occ, np.maximum(ext[:, 1] - ext[:, 0], ext[:, 3] - ext[:, 2]), np.nan)
    return occ, w


def body_of(occ, w, G):
    B = len(w)
    body = np.full(B, np.nan)
    for b in range(B):
        lo, hi = max(0, b - G), min(B - 1, b + G)
        v = w[lo:hi + 1][occ[lo:hi + 1]]
        if len(v):
            body[b] = v.min()
    return body


def levels_reference(count, ext, z0, dz, ground=None, min_rows=3, arm_window=3.0, arm_excess=4.0, max_levels=8):
    """ops.tower_levels' dict as numpy arrays, one loop per table row and slice: ``n_levels`` int64 [T], ``z_low``,
    ``z_high``, ``width``, ``rows`` float64 [T, max_levels] (NaN-padded), ``top`` [T]; with ``ground`` [T] also
    ``tower_height`` and ``nominal_height``"""
    count = np.asarray(count).reshape(-1, np.asarray(count).shape[-1])
    T, B = count.shape
    ext = np.asarray(ext, dtype=np.float64).reshape(T, B, 4)
    z0 = np.broadcast_to(np.asarray(z0, dtype=np.float64), (T,))
    G = int(np.ceil(float(arm_window) / float(dz)))
    out = dict(n_levels=np.zeros(T, dtype=np.int64), top=np.full(T, np.nan))
    for key in ("z_low", "z_high", "width", "rows"):
        out[key] = np.full((T, max_levels), np.nan)
    for k in range(T):
        occ, w = widths(count[k], ext[k], min_rows)
        body = body_of(occ, w, G)
        with np.errstate(invalid="ignore"):
            arm = occ & ((w - body) >= arm_excess)
        b, n = 0, 0
        while b < B:
            if not arm[b]:
                b += 1
                continue
            e = b
            while e + 1 < B and arm[e + 1]:
                e += 1
            if n < max_levels:
                out["z_low"][k, n] = z0[k] + float(b) * dz
                out["z_high"][k, n] = z0[k] + float(e + 1) * dz
                out["width"][k, n] = w[b:e + 1].max()
                out["rows"][k, n] = float(count[k, b:e + 1].sum())
                n += 1
            b = e + 1
        out["n_levels"][k] = n
        if occ.any():
            out["top"][k] = z0[k] + float(np.flatnonzero(occ).max() + 1) * dz
    if ground is not None:
        ground = np.broadcast_to(np.asarray(ground, dtype=np.float64), (T,))
        out["tower_height"] = out["top"] - ground
        out["nominal_height"] = out["z_low"][:, 0] - ground
    return out


def margins(P, perm, offsets, frames5, slot, T, dz, B, min_rows=MIN_ROWS, arm_window=ARM_WINDOW,
            arm_excess=ARM_EXCESS):
    """(excess, boundary): the smallest |(w - body) - arm_excess| over the occupied slices of the statement's tables,
    and the smallest distance in metres of a row of a cluster that takes part from a slice boundary"""
    frames5 = np.asarray(frames5, dtype=np.float64).reshape(-1, 5)
    count, ext, _ = slices_by_sort(P, perm, offsets, frames5, slot, T, dz, B)
    G = int(np.ceil(float(arm_window) / float(dz)))
    excess = np.inf
    for k in range(T):
        occ, w = widths(count[k], ext[k], min_rows)
        if occ.any():
            excess = min(excess, float(np.abs((w - body_of(occ, w, G))[occ] - arm_excess).min()))
    boundary = np.inf
    part = takes_part(frames5, slot, T)
    for k in range(len(offsets) - 1):
        rows = perm[offsets[k]:offsets[k + 1]]
        if part[k] and len(rows):
            h = np.asarray(P, dtype=np.float32).reshape(-1, 3)[rows, 2].astype(np.float64) - frames5[k, 2]
            boundary = min(boundary, float(np.abs(h - np.round(h / dz) * dz).min()))
    return excess, boundary


def ext_tolerance(P, perm, offsets, frames5=None):
    """float64 [K]: how far an ``s`` or ``t`` of cluster k may lie from the same figure in a frame whose sums were taken
    in another order (the library's).  The moments differ by at most ``span_cases.sum_bounds``; the centre is a mean of
    first moments (a bound divided by n); the direction is half an atan2 of centred second moments, whose perturbation
    over the anisotropy ``hypot(cxx - cyy, 2 cxy)`` bounds the angle, and an angle moves a point at radius r by r times
    it.  64 is slack for the chained divisions, the centring products, atan2, cos and sin (a few u relative each)."""
    P = np.asarray(P, dtype=np.float32).reshape(-1, 3)
    count, origin, M, A = sp.moments_reference(P, perm, offsets)
    bound = sp.sum_bounds(count, A)
    n = np.maximum(count.astype(np.float64), 1.0)
    tol = np.zeros(len(count))
    for k in range(len(count)):
        if not count[k]:
            continue
        mu = M[k, 0:3] / n[k]
        dmu = bound[k, 0:3] / n[k] + U * np.abs(origin[k].astype(np.float64) + mu)
        cxx, cyy, cxy = M[k, 3] / n[k] - mu[0] ** 2, M[k, 4] / n[k] - mu[1] ** 2, M[k, 6] / n[k] - mu[0] * mu[1]
        d2 = (bound[k, [3, 4, 6]] / n[k]).max() + 2.0 * np.abs(mu[:2]).max() * dmu[:2].max() + 4.0 * U * A[k, 3:5].max() / n[k]
        aniso = np.hypot(cxx - cyy, 2.0 * cxy)
        dtheta = 2.0 * d2 / aniso if aniso > 0 else np.pi
        rows = perm[offsets[k]:offsets[k + 1]]
        r = np.abs(P[rows, :2].astype(np.float64) - (origin[k, :2].astype(np.float64) + mu[:2])).sum(axis=1).max()
        tol[k] = 64.0 * (2.0 * dmu[:2].max() + r * dtheta + 4.0 * U * r)
    return tol


# ------------------------------------------------------------------ the scene
_SCENE = {}


def scene_towers():
    """(X float32 [n,3], perm int32, offsets int64 [4], frames float64 [3,6]): the tower rows (kind 0) of
    ``span_cases.line_scene`` grouped by the nearest tower axis, with ``span_cases.frames_reference``'s frames"""
    if "towers" not in _SCENE:
        X, kind = sp.line_scene()
        T = sp.line_towers()
        d = np.linalg.norm(X[:, None, :2].astype(np.float64) - T[None, :, :2], axis=2)
        labels = np.where(kind == 0, d.argmin(axis=1), -1).astype(np.int32)
        perm, offsets = sp.group_reference(labels, 3)
        count, origin, M, _ = sp.moments_reference(X, perm, offsets)
        _SCENE["towers"] = (X, perm, offsets, sp.frames_reference(count, origin, M))
    return _SCENE["towers"]


def frames5_of(frames, z0):
    """[K,5] = (cx, cy, z0, ux, uy) from ``span_frames``' six values and a z0 per cluster"""
    frames = np.asarray(frames, dtype=np.float64).reshape(-1, 6)
    return np.stack([frames[:, 0], frames[:, 1], np.broadcast_to(np.asarray(z0, dtype=np.float64), (len(frames),)),
                     frames[:, 3], frames[:, 4]], axis=1)


def assert_scene(P, perm, offsets, frames5, dz, B, base, what):
    """the scene's statement for tower clusters with the given frames: exactly one level per tower with ``z_low`` in the
    slice that holds ``base + 25`` and ``top`` in the one that ends at or above ``base + 30``, and both margins"""
    T = len(offsets) - 1
    slot = np.arange(T, dtype=np.int32)
    count, ext, outside = slices_by_sort(P, perm, offsets, frames5, slot, T, dz, B)
    lv = levels_reference(count, ext, frames5[:, 2], dz, min_rows=MIN_ROWS, arm_window=ARM_WINDOW,
                          arm_excess=ARM_EXCESS, max_levels=MAX_LEVELS)
    excess, boundary = margins(P, perm, offsets, frames5, slot, T, dz, B)
    assert (lv["n_levels"] == 1).all(), (what, lv["n_levels"])
    assert excess >= EXCESS_MARGIN, (what, excess)
    assert boundary >= BOUNDARY_MARGIN, (what, boundary)
    base = np.asarray(base, dtype=np.float64)
    low, top = lv["z_low"][:, 0], lv["top"]
    assert ((low <= base + ARM_LOW) & (base + ARM_LOW < low + dz)).all(), (what, low - base)
    assert ((top - dz < base + TOWER_TOP) & (base + TOWER_TOP <= top)).all(), (what, top - base)
    return dict(count=count, ext=ext, outside=outside, levels=lv, excess=excess, boundary=boundary)


def scene_reference(dz, cut=0.0):
    """the scene at z0 = base for one slice height, asserted: z_low = base + 25 and top = base + 30 exactly.  ``cut``:
    the rows lower than base + cut are taken out first (what a ground rule does to a tower's feet)"""
    key = ("scene", float(dz), float(cut))
    if key not in _SCENE:
        X, perm, offsets, frames = scene_towers()
        base = np.array(sp.LINE_BASES)
        if cut:
            lab = np.full(len(X), -1, dtype=np.int32)
            for k in range(3):
                rows = perm[offsets[k]:offsets[k + 1]]
                lab[rows[X[rows, 2] >= base[k] + cut]] = k
            perm, offsets = sp.group_reference(lab, 3)
        f5 = frames5_of(frames, base)
        B = int(np.ceil(64.0 / dz))
        out = assert_scene(X, perm, offsets, f5, dz, B, base, key)
        lv = out["levels"]
        assert np.array_equal(lv["z_low"][:, 0], base + ARM_LOW) and np.array_equal(lv["top"], base + TOWER_TOP), key
        out.update(perm=perm, offsets=offsets, frames5=f5, B=B)
        _SCENE[key] = out
    return _SCENE[key]
