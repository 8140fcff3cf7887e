"""Tree fall: the numpy statement of include/pch_hip.h's rule - row frame, ground, height, participation, reach, the
distance from the foot, per row, per span, statistics -, a second, vectorised statement of the winner (argmin over the
[K,n] distances with per-row R2), the binning of hazard rows into ``trees`` records, and the scene:
``terrain_cases.terrain_scene`` with four stems and the bank one of them stands on (TEST INFRASTRUCTURE, pure numpy;
imported by the CPU and the GPU tests, not a conftest).  The statement loops spans and segments over all rows; nothing
here knows about tiles, bounds or culling."""
import numpy as np

import clearance_cases as cc
import shape_cases as sc
import span_cases as sp
import terrain_cases as tc

NAN32 = np.float32(np.nan)
CLEAR, NEAR, STRIKE = 0, 1, 2
OUTPUTS = ("dist2", "span", "height", "hazard", "count", "strikes", "min_dist2", "min_row", "max_height", "max_row")


# ------------------------------------------------------------------ feet and distances
def feet(X, g, ground, sub=None):
    """(F float64 [n,3] = (X, Y, g), H float64 [n], fin bool [n]): the row frame and the ground of the terrain rule.
    g - and with it H - is NaN for a row that is not finite in all three coordinates"""
    P = tc.frame(X, sub)
    D = P.astype(np.float64)
    fin = np.isfinite(P).all(axis=1)
    gv = np.where(fin, tc.ground_at(g, ground, D[:, 0], D[:, 1]), np.nan)
    with np.errstate(all="ignore"):
        H = D[:, 2] - gv
    return np.stack([D[:, 0], D[:, 1], gv], axis=1), H, fin


def foot_distances(F, curves, segs):
    """float64 [K,n]: the rule's d2 from every foot (float64 points) to every span; spans that take no part have +inf"""
    F = np.asarray(F, dtype=np.float64).reshape(-1, 3)
    curves = np.asarray(curves, dtype=np.float64)
    segs = np.asarray(segs, dtype=np.float64)
    K, S = segs.shape[0], segs.shape[1]
    X, Y, gv = F[:, 0], F[:, 1], F[:, 2]
    out = np.full((K, len(F)), np.inf)
    with np.errstate(all="ignore"):
        for k in range(K):
            if not (np.isfinite(curves[k, :5]).all() and np.isfinite(segs[k]).all()):
                continue
            cx, cy, cz, ux, uy = curves[k, :5]
            dx = X - cx
            dy = Y - cy
            w = gv - cz
            m = (dx * ux) + (dy * uy)
            t = (dy * ux) - (dx * uy)
            gmin = np.full(len(F), np.inf)
            for j in range(S):
                mj, zj, dm, dz, inv = segs[k, j]
                rm, rw = m - mj, w - zj
                q = ((rm * dm) + (rw * dz)) * inv
                q = np.where(q < 0, 0.0, q)
                q = np.where(q > 1, 1.0, q)
                em, ew = rm - (q * dm), rw - (q * dz)
                d = (em * em) + (ew * ew)
                gmin = np.where(d < gmin, d, gmin)
            out[k] = gmin + (t * t)
    return out


def reach_of(H, grow, limit):
    """(s2, R2) float64 [n] of the rule"""
    with np.errstate(all="ignore"):
        reach = H + float(grow)
        s2 = reach * reach
        R = reach + float(limit)
        R2 = R * R
    return s2, R2


def takes_part(X, H, fin, h_min, h_max, skip=None):
    """(part bool [n], uncovered bool [n])"""
    alive = fin.copy() if skip is None else fin & (np.asarray(skip).reshape(-1) == 0)
    with np.errstate(invalid="ignore"):
        part = alive & ~np.isnan(H) & (float(h_min) <= H) & (H <= float(h_max))
    return part, alive & np.isnan(H)


def height32(H):
    """out_height: (float)H, the one NaN where there is no ground or the row is not finite"""
    with np.errstate(all="ignore"):
        return np.where(np.isnan(H), NAN32, H.astype(np.float32)).astype(np.float32)


def table_of(best, who, hazard, height, K):
    """the per-span outputs over the rows with who == k, one loop per span"""
    out = dict(count=np.zeros(K, dtype=np.int64), strikes=np.zeros(K, dtype=np.int64), min_dist2=np.full(K, np.inf),
               min_row=np.full(K, -1, dtype=np.int64), max_height=np.full(K, NAN32, dtype=np.float32),
               max_row=np.full(K, -1, dtype=np.int64))
    for k in range(K):
        rows = np.flatnonzero(who == k)
        out["count"][k] = len(rows)
        out["strikes"][k] = int((hazard[rows] == STRIKE).sum())
        if len(rows):
            out["min_dist2"][k] = best[rows].min()
            out["min_row"][k] = rows[best[rows] == out["min_dist2"][k]][0]
            keys = tc.key_of(height[rows])
            out["max_height"][k] = height[rows][int(np.argmax(keys))]
            out["max_row"][k] = rows[keys == keys.max()][0]
    return out


# ------------------------------------------------------------------ the rule, looped literally
def treefall_reference(X, g, ground, curves, segs, h_min, h_max, grow, limit, sub=None, skip=None):
    """dict of OUTPUTS and ``stats`` int64 [2] (the rows that took part, the uncovered rows): spans in ascending k,
    ``if d2 <= R2 and d2 < best``"""
    K = np.asarray(segs).shape[0]
    F, H, fin = feet(X, g, ground, sub)
    n = len(F)
    part, bare = takes_part(X, H, fin, h_min, h_max, skip)
    s2, R2 = reach_of(H, grow, limit)
    d2 = foot_distances(F, curves, segs)
    best = np.full(n, np.inf)
    who = np.full(n, -1, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for k in range(K):
            take = part & (d2[k] <= R2) & (d2[k] < best)
            best = np.where(take, d2[k], best)
            who = np.where(take, np.int32(k), who)
        hazard = np.where(who < 0, CLEAR, np.where(best <= s2, STRIKE, NEAR)).astype(np.uint8)
    height = height32(H)
    out = dict(dist2=best, span=who, height=height, hazard=hazard,
               stats=np.array([part.sum(), bare.sum()], dtype=np.int64))
    out.update(table_of(best, who, hazard, height, K))
    return out


# ------------------------------------------------------------------ a second, vectorised statement
def treefall_by_argmin(F, H, part, d2, s2, R2):
    """(dist2, span, hazard) from the feet as float64 points [n,3] and the distances [K,n] with per-row R2: the winner
    is the argmin over the spans within R2 - np.argmin returns the first, i.e. the lowest index on a tie"""
    K, n = d2.shape
    with np.errstate(invalid="ignore"):
        masked = np.where(part[None, :] & (d2 <= R2[None, :]), d2, np.inf)
    if K == 0:
        return np.full(n, np.inf), np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    who = np.argmin(masked, axis=0)
    best = masked[who, np.arange(n)]
    found = best < np.inf                        # (d2 = +inf is never taken: it is not below best = +inf)
    who = np.where(found, who, -1).astype(np.int32)
    best = np.where(found, best, np.inf)
    with np.errstate(invalid="ignore"):
        hazard = np.where(~found, CLEAR, np.where(best <= s2, STRIKE, NEAR)).astype(np.uint8)
    return best, who, hazard


# ------------------------------------------------------------------ trees: hazard rows binned into xy cells
TREE_KEYS = ("row", "x", "y", "ground", "height", "span", "distance", "margin", "hazard")


def trees_reference(X, ground_under, height, span, dist2, hazard, cell, grow):
    """the ``trees`` records of pipeline.danger_trees, one loop over the hazard rows: they are binned into xy cells of
    ``cell`` metres (floor(x / cell), floor(y / cell)); per occupied cell the tallest hazard row, ties to the lowest
    row index; records ordered by (span, row).  ``ground_under`` float64 [n]: g under each row"""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    tallest = {}
    for i in np.flatnonzero(np.asarray(hazard) >= NEAR):
        c = (int(np.floor(float(X[i, 0]) / cell)), int(np.floor(float(X[i, 1]) / cell)))
        j = tallest.get(c)
        if j is None or height[i] > height[j]:
            tallest[c] = int(i)
    rows = sorted(tallest.values(), key=lambda i: (int(span[i]), i))
    out = []
    for i in rows:
        dist = float(np.sqrt(dist2[i]))
        h = float(height[i])
        out.append(dict(row=i, x=float(X[i, 0]), y=float(X[i, 1]), ground=float(ground_under[i]), height=h,
                        span=int(span[i]), distance=dist, margin=dist - (h + float(grow)), hazard=int(hazard[i])))
    return out


# ------------------------------------------------------------------ the rule's boundaries on level ground
def level_case():
    """level ground at z = 0 on a 16 x 16 grid of 8 m cells around the origin and level straight wires along x with
    dyadic values: span 0 at y = 0, 8 m up; span 1 the same wire again (a tie); span 2 with a NaN; span 3 at y = 40"""
    g = tc.grid(x0=-64.0, y0=-64.0, cell=8.0, nx=16, ny=16)
    ground = np.zeros((16, 16), dtype=np.float32)
    curves = np.stack([cc.curve(cz=8.0, m0=-32.0, m1=32.0), cc.curve(cz=8.0, m0=-32.0, m1=32.0),
                       cc.curve(cz=8.0, a=np.nan, m0=-32.0, m1=32.0), cc.curve(cy=40.0, cz=8.0, m0=-32.0, m1=32.0)])
    segs, _ = cc.segments_reference(curves, 4)
    return g, ground, curves, segs


def boundary_rows():
    """(X float32 [15,3], skip uint8 [15]) for ``level_case`` at h_min = 2, h_max = 12, grow = 0, limit = 3: a foot at
    (0, 6, 0) is 10 m from the wire 8 m up, d2 = 36 + 64 = 100 exactly"""
    below = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    above = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    X = np.array([[0.0, 6.0, 10.0],            # 0: reach = 10, d2 == s2: strikes
                  [0.0, 6.0, below(10.0)],     # 1: just short: near
                  [0.0, 6.0, 7.0],             # 2: R = 10, d2 == R2: near
                  [0.0, 6.0, below(7.0)],      # 3: just outside R: clear
                  [0.0, 6.0, 2.0],             # 4: H == h_min: takes part (clear: R = 5)
                  [0.0, 6.0, below(2.0)],      # 5: below h_min
                  [0.0, 6.0, 12.0],            # 6: H == h_max: strikes
                  [0.0, 6.0, above(12.0)],     # 7: above h_max
                  [np.inf, 6.0, 10.0], [0.0, -np.inf, 10.0], [0.0, 6.0, np.inf], [np.nan, 6.0, 10.0],   # 8..11
                  [0.0, 6.0, 10.0],            # 12: skipped
                  [100.0, 6.0, 10.0],          # 13: outside the grid: uncovered
                  [0.0, 36.0, 11.0]],          # 14: 4 m beside span 3 only: d2 = 16 + 64 = 80, strikes
                 dtype=np.float32)
    skip = np.zeros(len(X), dtype=np.uint8)
    skip[12] = 1
    return X, skip


BOUNDARY_HAZARD = (2, 1, 1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 2)
BOUNDARY_SPAN = (0, 0, 0, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1, -1, 3)        # the tie goes to span 0


# ------------------------------------------------------------------ the scene: the line, its ground, four stems
H_MIN, H_MAX, GROW, LIMIT, SEGMENTS, CELL = 3.0, 45.0, 0.0, 3.0, 32, 2.0
# name, station, lateral, the top's height above the true ground
STEMS = (("strike", 55.0, 16.0, 24.0), ("near", 25.0, -16.0, 20.5), ("far", 130.0, 27.0, 22.0),
         ("bank", 40.0, 39.0, 31.5))
BANK = (20.0, 60.0, 31.0, 47.0, 24.0)            # stations, laterals and z of the bank beside the first span
STEM_STEP = 0.25
_SCENE = {}
_REF = {}


def true_ground(station, lateral):
    s0, s1, l0, l1, z = BANK
    on_bank = (station >= s0) & (station <= s1) & (lateral >= l0) & (lateral <= l1)
    return np.where(on_bank, z, tc.sheet_z(station, lateral))


def stem_scene():
    """(X float32 [n,3], kind int8, points bool [n]): ``terrain_cases.terrain_scene`` (kinds 0..21) followed by the
    bank - level ground at z = 24 beside the first span, laterals 31..47 and stations 20..60, one row every 0.5 m,
    N(0, 0.03) in z (kind 30): higher than the lowest point of the wires beside it - and four stems (kinds 40..43),
    each a thin column of rows every 0.25 m from 2 m above the ground to its top with 0.05 m of jitter in x and y:
    "strike" 10 m beside an outer conductor and tall enough to reach it, "near" which ends short of the wire but
    within LIMIT of it, "far" which is tall and too far away, and "bank" on the bank, whose foot is above its wire.
    ``points``: the rows a ground rule would keep - ``clearance_cases.tree_scene`` and the stems."""
    if not _SCENE:
        X, kind = tc.terrain_scene()
        rng = np.random.default_rng(59)
        s0, s1, l0, l1, z = BANK
        st, lat = np.meshgrid(np.arange(s0 + 0.25, s1, 0.5), np.arange(l0 + 0.25, l1, 0.5), indexing="ij")
        st, lat = st.reshape(-1), lat.reshape(-1)
        bank = np.concatenate([sp._line_xy(st, lat), z + rng.normal(0.0, 0.03, (st.size, 1))], axis=1)
        parts, kinds = [X, bank.astype(np.float32)], [kind, np.full(len(bank), 30, dtype=np.int8)]
        for i, (_, station, lateral, top) in enumerate(STEMS):
            up = np.arange(2.0, top + 1e-9, STEM_STEP)
            base = float(true_ground(np.float64(station), np.float64(lateral)))
            xy = sp._line_xy(np.full(len(up), station), np.full(len(up), lateral)) + rng.uniform(-0.05, 0.05, (len(up), 2))
            parts.append(np.concatenate([xy, (base + up)[:, None]], axis=1).astype(np.float32))
            kinds.append(np.full(len(up), 40 + i, dtype=np.int8))
        X, kind = np.vstack(parts), np.concatenate(kinds)
        points = (kind <= 12) | (kind >= 40)
        for a in (X, kind, points):
            a.setflags(write=False)
        _SCENE["case"] = (X, kind, points)
    return _SCENE["case"]


def reference():
    """the scene's reference answers, computed once: ``grid`` and ``ground`` (the terrain rule on the whole scene),
    ``points`` (the rows kept), ``skip``, clearance_cases' ``spans`` / ``idx`` / ``curves`` / ``segs`` / ``chord``, the
    outputs of ``treefall_reference`` over the points at H_MIN, H_MAX, GROW, LIMIT, ``under`` (g per row), ``trees``
    and ``tol``.  The scene's margins are asserted here, on the host, so that the pipeline's class, span and counts may
    be compared exactly."""
    if not _REF:
        X, kind, keep = stem_scene()
        r = cc.reference()
        g = tc.scene_grid(X, tc.CELL)
        low, _ = tc.low_reference(X, g)
        _, ground, _ = tc.ground_reference(low, tc.WINDOW_CELLS, tc.DH, tc.MAX_GAP)
        P, pk = X[keep], kind[keep]
        n0 = len(cc.tree_scene()[0])
        assert np.array_equal(P[:n0], cc.tree_scene()[0])
        # the wire rule looks 2 m around a row: no stem row lies that close to a row of tree_scene, so the all-pairs
        # mask of the points is clearance_cases' followed by the stems' own - and a vertical column is no wire
        stems = P[n0:].astype(np.float64)
        gap = min(float(np.sqrt(((stems[:, None, :] - P[None, i:min(i + 2048, n0), :]) ** 2).sum(2).min()))
                  for i in range(0, n0, 2048))
        assert gap > 2.0 * sc.SCENE_RULE["radius"], gap
        assert not sc.drop_mask_reference(P[n0:], **sc.SCENE_RULE)[0].any()
        spans = r["spans"]
        tw = sp.line_towers()
        near = (((P[:, None, :2].astype(np.float64) - tw[None, :, :2]) ** 2).sum(2) <= 9.0 * 9.0).any(axis=1)
        skip = np.concatenate([r["skip"], np.zeros(len(P) - n0, dtype=np.uint8)])
        assert np.array_equal(skip[:n0] != 0, spans["wire"] | near[:n0]) and not near[n0:].any()
        curves, segs = r["curves"], r["segs"]
        out = treefall_reference(P, g, ground, curves, segs, H_MIN, H_MAX, GROW, LIMIT, skip=skip)
        F, H, fin = feet(P, g, ground)
        part, _ = takes_part(P, H, fin, H_MIN, H_MAX, skip)
        s2, R2 = reach_of(H, GROW, LIMIT)
        d2 = foot_distances(F, curves, segs)
        # how far the device's span table may move a distance: clearance_cases' tol; the ground grid is the rule's bit
        # for bit, so H is not moved at all
        tol = r["tol"]
        assert tol < 2e-5, tol
        # no H within 10 tol of h_min or h_max
        alive = fin & (skip == 0) & ~np.isnan(H)
        assert np.abs(H[alive] - H_MIN).min() > 10.0 * tol and np.abs(H[alive] - H_MAX).min() > 10.0 * tol
        # every stem top - and every other row that takes part - keeps 10 tol between its distances and its reach and
        # R; the two nearest spans of a row within R are further apart than that
        dist = np.sqrt(d2[:, part])
        reach, R = np.sqrt(s2[part]), np.sqrt(R2[part])
        assert np.abs(dist - reach[None, :]).min() > 10.0 * tol and np.abs(dist - R[None, :]).min() > 10.0 * tol
        tops = [np.flatnonzero(pk == 40 + i)[-1] for i in range(len(STEMS))]
        assert part[tops].all()
        two = np.sort(dist, axis=0)[:2]
        assert (two[1] - two[0])[two[0] <= R].min() > 10.0 * tol
        # per span, the two smallest distances and the two largest heights of its rows differ by more than 10 tol
        for k in np.flatnonzero(out["count"] > 1):
            rows = np.flatnonzero(out["span"] == k)
            d = np.sort(np.sqrt(out["dist2"][rows]))
            h = np.sort(out["height"][rows].astype(np.float64))
            assert d[1] - d[0] > 10.0 * tol and h[-1] - h[-2] > 10.0 * tol, k
        trees = trees_reference(P, F[:, 2], out["height"], out["span"], out["dist2"], out["hazard"], CELL, GROW)
        _REF.update(out, grid=g, ground=ground, points=P, kind=pk, skip=skip, spans=spans, idx=r["idx"], curves=curves,
                    segs=segs, chord=r["chord"], under=F[:, 2], d2=d2, part=part, tops=np.array(tops), trees=trees,
                    tol=tol)
    return _REF
