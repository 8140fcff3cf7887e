"""Terrain grid: the numpy statement of include/pch_hip.h's rule - row frame, cell, lowest return, opening, ground and
fill, the ground under a position, row heights, the span ground profile -, an independent statement of the lowest return
(a sort by (cell, key)) and of the bilinear sample (np.interp on the cell centres), and the scene:
``clearance_cases.tree_scene`` with a ground sheet under the line and one flat-roofed building (TEST INFRASTRUCTURE,
pure numpy; imported by the CPU and the GPU tests, not a conftest).  Nothing here knows about tiles, tables or atomics."""
import numpy as np

import clearance_cases as cc
import span_cases as sp

U = 2.0 ** -53
NAN32 = np.float32(np.nan)
CELL, WINDOW_CELLS, DH, MAX_GAP, SEGMENTS, LIMIT = 1.0, 6, 0.5, 16, 32, 7.0
BREACH_LIMIT = 18.4                              # between the scene's smallest ground clearance and the next one


def grid(x0=0.0, y0=0.0, cell=1.0, nx=1, ny=1):
    return dict(x0=float(x0), y0=float(y0), cell=float(cell), nx=int(nx), ny=int(ny))


def same(a, b):
    """bit for bit, one NaN being as good as another: both NaN at the same places and equal bits elsewhere"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(bits), b[~nb].view(bits)))


# ------------------------------------------------------------------ row frame, cell, key
def frame(X, sub=None):
    """P = fl32(xyz - sub3) per component, a float32 subtraction; no subtraction without sub"""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    if sub is None:
        return X
    with np.errstate(all="ignore"):
        return (X - np.asarray(sub, dtype=np.float32).reshape(1, 3)).astype(np.float32)


def cell_of(g, X, Y):
    """(inside bool, fx, fy int64) of float64 positions: fx = floor((X - x0) / cell), inside iff 0 <= fx < nx and
    0 <= fy < ny (NaN and inf fail the comparisons); fx, fy are 0 where the position is outside"""
    with np.errstate(all="ignore"):
        qx = np.floor((np.asarray(X, dtype=np.float64) - g["x0"]) / g["cell"])
        qy = np.floor((np.asarray(Y, dtype=np.float64) - g["y0"]) / g["cell"])
        inside = (qx >= 0) & (qx < g["nx"]) & (qy >= 0) & (qy < g["ny"])
    fx = np.where(inside, qx, 0).astype(np.int64)
    fy = np.where(inside, qy, 0).astype(np.int64)
    return inside, fx, fy


def key_of(z):
    """key(z) = bits(z) ^ (bits(z) >> 31 ? 0xFFFFFFFF : 0x80000000)"""
    bits = np.ascontiguousarray(z, dtype=np.float32).view(np.uint32)
    return bits ^ np.where(bits >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return (k ^ np.where(k >> 31, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def takes_part(X, g, sub=None, skip=None):
    """(part bool [n], cell int64 [n], P float32 [n,3])"""
    P = frame(X, sub)
    inside, fx, fy = cell_of(g, P[:, 0].astype(np.float64), P[:, 1].astype(np.float64))
    part = inside & np.isfinite(P[:, 2])
    if skip is not None:
        part &= np.asarray(skip).reshape(-1) == 0
    return part, fy * g["nx"] + fx, P


# ------------------------------------------------------------------ lowest return
def low_reference(X, g, sub=None, skip=None):
    """(low float32 [ny,nx], count int32 [ny,nx]), one loop over the rows"""
    part, cell, P = takes_part(X, g, sub, skip)
    ncells = g["nx"] * g["ny"]
    best = np.full(ncells, 0xFFFFFFFF, dtype=np.uint32)
    count = np.zeros(ncells, dtype=np.int32)
    keys = key_of(P[:, 2])
    for i in np.flatnonzero(part):
        c = cell[i]
        count[c] += 1
        if keys[i] < best[c]:
            best[c] = keys[i]
    low = np.where(count > 0, unkey(best), NAN32).astype(np.float32)
    return low.reshape(g["ny"], g["nx"]), count.reshape(g["ny"], g["nx"])


def low_by_sort(X, g, sub=None, skip=None):
    """the same through a sort of the rows by (cell, key): the first row of every run is the lowest return"""
    part, cell, P = takes_part(X, g, sub, skip)
    ncells = g["nx"] * g["ny"]
    rows = np.flatnonzero(part)
    order = rows[np.lexsort((key_of(P[rows, 2]), cell[rows]))]
    cells, first, counts = np.unique(cell[order], return_index=True, return_counts=True)
    low = np.full(ncells, NAN32, dtype=np.float32)
    count = np.zeros(ncells, dtype=np.int32)
    low[cells] = P[order[first], 2]
    count[cells] = counts
    return low.reshape(g["ny"], g["nx"]), count.reshape(g["ny"], g["nx"])


# ------------------------------------------------------------------ opening, ground and fill
def _pass(a, R, axis, domax):
    """one pass of the opening along x (axis 1 of the [ny,nx] array) or y (axis 0): per cell the clipped window in
    ascending index, replaced only by a value that compares smaller (larger)"""
    a = np.asarray(a, dtype=np.float32)
    out = np.full(a.shape, NAN32, dtype=np.float32)
    n = a.shape[axis]
    for at in range(n):
        acc = np.full(a.shape[1 - axis], NAN32, dtype=np.float32)
        for k in range(max(at - R, 0), min(at + R, n - 1) + 1):
            v = a[:, k] if axis == 1 else a[k, :]
            ok = ~np.isnan(v)
            first = ok & np.isnan(acc)
            with np.errstate(invalid="ignore"):
                better = ok & ~np.isnan(acc) & ((v > acc) if domax else (v < acc))
            acc = np.where(first | better, v, acc)
        if axis == 1:
            out[:, at] = acc
        else:
            out[at, :] = acc
    return out


def open_reference(low, R):
    """erosion along x, then y, dilation along x, then y"""
    return _pass(_pass(_pass(_pass(low, R, 1, False), R, 0, False), R, 1, True), R, 0, True)


def ground_reference(low, R, dh, G):
    """(open float32, ground float32, state uint8), all [ny,nx]; the fill is one loop per cell"""
    low = np.asarray(low, dtype=np.float32)
    ny, nx = low.shape
    opened = open_reference(low, R)
    with np.errstate(invalid="ignore"):
        isg = ~np.isnan(low) & ((low.astype(np.float64) - opened.astype(np.float64)) <= float(dh))
    ground = np.full(low.shape, NAN32, dtype=np.float32)
    state = np.zeros(low.shape, dtype=np.uint8)
    for fy in range(ny):
        for fx in range(nx):
            rows = 0 if np.isnan(low[fy, fx]) else 4
            if isg[fy, fx]:
                ground[fy, fx], state[fy, fx] = low[fy, fx], 1 | rows
                continue
            num, den, found = 0.0, 0.0, False
            for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                for d in range(1, G + 1):
                    x, y = fx + d * dx, fy + d * dy
                    if x < 0 or x >= nx or y < 0 or y >= ny:
                        break
                    if isg[y, x]:
                        num = num + (float(low[y, x]) / float(d))
                        den = den + (1.0 / float(d))
                        found = True
                        break
            if found:
                ground[fy, fx] = np.float32(num / den)
            state[fy, fx] = (2 if found else 0) | rows
    return opened, ground, state


# ------------------------------------------------------------------ the ground under a position
def _axis(pos, o, cell, nc):
    with np.errstate(all="ignore"):
        u = ((pos - o) / cell) - 0.5
        f = np.where(np.isfinite(u), np.floor(u), 0.0)
    i0 = np.clip(f, 0, max(nc - 2, 0)).astype(np.int64)
    i1 = np.minimum(i0 + 1, nc - 1)
    with np.errstate(all="ignore"):
        a = u - i0.astype(np.float64)
        a = np.where(a < 0, 0.0, a)
        a = np.where(a > 1, 1.0, a)
    return i0, i1, a


def ground_at(g, ground, X, Y):
    """float64 [m]: g(X, Y) of the rule"""
    ground = np.asarray(ground, dtype=np.float32).reshape(g["ny"], g["nx"])
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    inside, fx, fy = cell_of(g, X, Y)
    i0, i1, a = _axis(X, g["x0"], g["cell"], g["nx"])
    j0, j1, b = _axis(Y, g["y0"], g["cell"], g["ny"])
    G = ground.astype(np.float64)
    g00, g10, g01, g11 = G[j0, i0], G[j0, i1], G[j1, i0], G[j1, i1]
    with np.errstate(all="ignore"):
        bil = (((g00 * (1.0 - a)) + (g10 * a)) * (1.0 - b)) + (((g01 * (1.0 - a)) + (g11 * a)) * b)
    four = ~(np.isnan(g00) | np.isnan(g10) | np.isnan(g01) | np.isnan(g11))
    return np.where(inside, np.where(four, bil, G[fy, fx]), np.nan)


def height_reference(X, g, ground, sub=None):
    """(height float32 [n], ground float32 [n])"""
    P = frame(X, sub)
    D = P.astype(np.float64)
    fin = np.isfinite(P).all(axis=1)
    gv = np.where(fin, ground_at(g, ground, D[:, 0], D[:, 1]), np.nan)
    with np.errstate(all="ignore"):
        h = (D[:, 2] - gv).astype(np.float32)
    return np.where(np.isnan(gv), NAN32, h).astype(np.float32), gv.astype(np.float32)


def sample_by_interp(g, ground, X, Y):
    """the bilinear value by np.interp on the cell centres, first along x for every grid line, then along y per
    position; np.interp holds the end values beyond the outer centres, which is the rule's clamp.  Only meaningful
    where the four cells around the position have ground."""
    ground = np.asarray(ground, dtype=np.float64).reshape(g["ny"], g["nx"])
    xc = g["x0"] + (np.arange(g["nx"]) + 0.5) * g["cell"]
    yc = g["y0"] + (np.arange(g["ny"]) + 0.5) * g["cell"]
    lines = np.stack([np.interp(X, xc, ground[j]) for j in range(g["ny"])])            # [ny, m]
    return np.array([np.interp(Y[p], yc, lines[:, p]) for p in range(len(X))])


# ------------------------------------------------------------------ span ground profile
def span_ground_reference(curves, S, g, ground, limit):
    """the rule's table per piece, one loop per piece and vertex"""
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 10)
    K = len(curves)
    out = dict(clearance=np.full((K, S + 1), np.nan), ground=np.full((K, S + 1), np.nan),
               covered=np.zeros(K, dtype=np.int64), min_clearance=np.full(K, np.inf),
               min_vertex=np.full(K, -1, dtype=np.int64), min_at=np.full((K, 3), np.nan),
               violation=np.zeros(K, dtype=bool), X=np.zeros((K, S + 1)), Y=np.zeros((K, S + 1)))
    for k in range(K):
        cx, cy, cz, ux, uy, a, b, c, m0, m1 = curves[k]
        step = (m1 - m0) / float(S)
        m = np.array([m0 + float(j) * step for j in range(S)] + [m1])
        z = np.array([a + mj * (b + c * mj) for mj in m])
        X, Y, W = cx + (m * ux), cy + (m * uy), cz + z
        gv = ground_at(g, ground, X, Y)
        out["X"][k], out["Y"][k] = X, Y
        out["ground"][k] = gv
        out["clearance"][k] = W - gv
        for j in range(S + 1):
            if np.isnan(gv[j]):
                continue
            out["covered"][k] += 1
            if out["clearance"][k, j] < out["min_clearance"][k]:
                out["min_clearance"][k], out["min_vertex"][k] = out["clearance"][k, j], j
                out["min_at"][k] = (X[j], Y[j], gv[j])
        out["violation"][k] = out["min_clearance"][k] <= limit
    return out


# ------------------------------------------------------------------ the scene: the line on a ground sheet
SHEET_STATIONS, SHEET_LATERALS = 380, 120        # every 0.5 m from station -20 and lateral -30
ROOF = (100.0, 12.0, 8.0, 6.0)                   # station, lateral of the low corner; edge; height
_SCENE = {}
_REF = {}


def sheet_z(station, lateral):
    """the true ground: through the tower bases at their stations (level beyond the outer ones), cross-slope 0.05"""
    return np.interp(station, sp.LINE_STATIONS, sp.LINE_BASES) + 0.05 * lateral


def terrain_scene():
    """(X float32 [n,3], kind int8): ``clearance_cases.tree_scene`` (kinds 0..12) followed by the ground sheet - one
    row every 0.5 m of station and lateral with +-0.2 m of jitter in both and N(0, 0.03) in z, none under the building
    (kind 20) - and the roof of the building, 8 x 8 m, 6 m above the ground at its middle, a row every 0.5 m (kind 21)"""
    if not _SCENE:
        X, kind = cc.tree_scene()
        rng = np.random.default_rng(41)
        st, lat = np.meshgrid(-20.0 + 0.5 * np.arange(SHEET_STATIONS), -30.0 + 0.5 * np.arange(SHEET_LATERALS),
                              indexing="ij")
        st = st.reshape(-1) + rng.uniform(-0.2, 0.2, st.size)
        lat = lat.reshape(-1) + rng.uniform(-0.2, 0.2, lat.size)
        s0, l0, edge, high = ROOF
        under = (st >= s0 - 0.25) & (st <= s0 + edge + 0.25) & (lat >= l0 - 0.25) & (lat <= l0 + edge + 0.25)
        st, lat = st[~under], lat[~under]
        sheet = np.concatenate([sp._line_xy(st, lat), (sheet_z(st, lat) + rng.normal(0.0, 0.03, st.size))[:, None]],
                               axis=1)
        rs, rl = np.meshgrid(s0 + 0.25 + 0.5 * np.arange(16), l0 + 0.25 + 0.5 * np.arange(16), indexing="ij")
        rs, rl = rs.reshape(-1), rl.reshape(-1)
        top = float(sheet_z(s0 + 0.5 * edge, l0 + 0.5 * edge)) + high
        roof = np.concatenate([sp._line_xy(rs, rl), top + rng.normal(0.0, 0.02, (rs.size, 1))], axis=1)
        X = np.vstack([X, sheet.astype(np.float32), roof.astype(np.float32)])
        kind = np.concatenate([kind, np.full(len(sheet), 20, dtype=np.int8), np.full(len(roof), 21, dtype=np.int8)])
        for a in (X, kind):
            a.setflags(write=False)
        _SCENE["case"] = (X, kind)
    return _SCENE["case"]


def scene_grid(X, cell, sub=None):
    """ops.terrain_grid's grid, from numpy: the box of the rows finite in all three coordinates"""
    P = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    fin = np.isfinite(P).all(axis=1)
    s = np.zeros(3, np.float32) if sub is None else np.asarray(sub, dtype=np.float32)
    out = dict(cell=float(cell))
    for k, name in enumerate("xy"):
        a = float(np.float32(P[fin, k].min()) - s[k])
        b = float(np.float32(P[fin, k].max()) - s[k])
        out[name + "0"], out["n" + name] = a, int(np.floor((b - a) / cell)) + 1
    return out


def reference():
    """the scene's reference answers, computed once: ``grid``, ``low``, ``count``, ``open``, ``ground``, ``state``,
    ``height`` / ``under`` per row, the accepted pieces' ``curves`` and ``chord`` (clearance_cases' reference: the rows
    the ground rule would keep are tree_scene's), the span ground ``profile`` and ``tol``.  The scene's margins are
    asserted here, on the host, so that pipeline-level comparisons may be exact."""
    if not _REF:
        X, kind = terrain_scene()
        g = scene_grid(X, CELL)
        low, count = low_reference(X, g)
        opened, ground, state = ground_reference(low, WINDOW_CELLS, DH, MAX_GAP)
        height, under = height_reference(X, g, ground)
        r = cc.reference()
        curves = r["curves"]
        profile = span_ground_reference(curves, SEGMENTS, g, ground, LIMIT)
        # how far the device's span table may move a vertex's clearance: the curve (a, b·m, c·m², the centre) by
        # clearance_cases' tol, and the vertex in the plane by as much, which moves the ground under it by the steepest
        # slope between neighbouring cells (per cell, both axes) times that
        G = ground.astype(np.float64)
        with np.errstate(invalid="ignore"):
            slope = max(np.nanmax(np.abs(np.diff(G, axis=0))), np.nanmax(np.abs(np.diff(G, axis=1)))) / CELL
        tol = r["tol"] * (1.0 + 2.0 * float(slope))
        assert tol < 1e-4, tol
        # no ground cell within 10 tol of the dh decision (the device's low and open are the statement's bit for bit;
        # the margin keeps the scene away from a decision on the last bits all the same)
        has = ~np.isnan(low)
        diff = low[has].astype(np.float64) - opened[has].astype(np.float64)
        assert np.abs(diff - DH).min() > 10.0 * tol, np.abs(diff - DH).min()
        # no span minimum within 10 tol of the limit, no two vertices of a span tied for the minimum within that
        clr = np.sort(np.where(np.isnan(profile["clearance"]), np.inf, profile["clearance"]), axis=1)
        assert (profile["covered"] >= 2).all()
        assert np.abs(profile["min_clearance"] - LIMIT).min() > 10.0 * tol
        assert np.abs(profile["min_clearance"] - BREACH_LIMIT).min() > 10.0 * tol
        assert (profile["min_clearance"] <= BREACH_LIMIT).sum() == 1 and not (profile["min_clearance"] <= LIMIT).any()
        assert (clr[:, 1] - clr[:, 0]).min() > 10.0 * tol, (clr[:, 1] - clr[:, 0]).min()
        _REF.update(grid=g, low=low, count=count, open=opened, ground=ground, state=state, height=height, under=under,
                    curves=curves, chord=r["chord"], idx=r["idx"], spans=r["spans"], profile=profile, tol=tol,
                    kind=kind)
    return _REF
