"""Canopy grid and tree crowns: the numpy statement of include/pch_hip.h's rule, looped literally - rows in ascending
order, the smoothing additions in the stated order, windows enumerated cell by cell, chains followed one step at a time
-, independent second statements of three of its parts (the canopy top by a sort, the tops for r1 = 0 by a sliding
maximum under the disc footprint, the roots by a union of every cell with its parent) and the scene:
``treefall_cases.stem_scene`` with planted trees (TEST INFRASTRUCTURE, pure numpy; imported by the CPU and the GPU tests,
not a conftest).  Nothing here knows about tiles, tables or atomics."""
import math

import numpy as np

import terrain_cases as tc
import treefall_cases as tf
import span_cases as sp

NAN32 = np.float32(np.nan)
MAX_SMOOTH, MAX_WINDOW, MAX_CROWN = 8, 32, 256
TABLE_KEYS = ("top_cell", "cells", "rows", "max_height", "max_row")
same = tc.same


# ------------------------------------------------------------------ participation and the canopy top
def takes_part(X, tg, ground, cg, h_min, h_max, sub=None, skip=None):
    """(part bool [n], cell int64 [n], Hd float64 [n], height float32 [n]): Hd = Z - g(X, Y) on the terrain grid; a row
    takes part iff it is not skipped, finite, inside the canopy grid, over ground and h_min <= Hd <= h_max on the double.
    height is (float)Hd for every finite row, NaN where g is NaN"""
    P = tc.frame(X, sub)
    D = P.astype(np.float64)
    fin = np.isfinite(P).all(axis=1)
    inside, fx, fy = tc.cell_of(cg, D[:, 0], D[:, 1])
    gv = np.where(fin, tc.ground_at(tg, ground, D[:, 0], D[:, 1]), np.nan)
    with np.errstate(all="ignore"):
        Hd = D[:, 2] - gv
        part = fin & inside & ~np.isnan(gv) & (h_min <= Hd) & (Hd <= h_max)
        height = np.where(np.isnan(gv), NAN32, Hd.astype(np.float32)).astype(np.float32)
    if skip is not None:
        part &= np.asarray(skip).reshape(-1) == 0
    return part, fy * cg["nx"] + fx, Hd, height


def pack(h, row):
    """(key(H) << 32) | ~row as Python integers"""
    return (int(tc.key_of(np.float32(h)).reshape(-1)[0]) << 32) | (~int(row) & 0xFFFFFFFF)


def top_reference(X, tg, ground, cg, h_min, h_max, sub=None, skip=None):
    """dict(top float32, top_row int32, count int32, all [ny,nx]; height float32 [n]), one loop over the rows"""
    part, cell, _, height = takes_part(X, tg, ground, cg, h_min, h_max, sub, skip)
    ncells = cg["nx"] * cg["ny"]
    best = [0] * ncells
    count = np.zeros(ncells, dtype=np.int32)
    top = np.full(ncells, NAN32, dtype=np.float32)
    top_row = np.full(ncells, -1, dtype=np.int32)
    keys = tc.key_of(height)
    for i in np.flatnonzero(part):
        c = cell[i]
        count[c] += 1
        k = (int(keys[i]) << 32) | (~int(i) & 0xFFFFFFFF)
        if k > best[c]:
            best[c], top[c], top_row[c] = k, height[i], i
    shape = (cg["ny"], cg["nx"])
    return dict(top=top.reshape(shape), top_row=top_row.reshape(shape), count=count.reshape(shape), height=height)


def top_by_sort(X, tg, ground, cg, h_min, h_max, sub=None, skip=None):
    """the same through a sort on (cell, key descending, row ascending): the first row of every run"""
    part, cell, _, height = takes_part(X, tg, ground, cg, h_min, h_max, sub, skip)
    ncells = cg["nx"] * cg["ny"]
    rows = np.flatnonzero(part)
    order = rows[np.lexsort((rows, -tc.key_of(height[rows]).astype(np.int64), cell[rows]))]
    cells, first, counts = np.unique(cell[order], return_index=True, return_counts=True)
    top = np.full(ncells, NAN32, dtype=np.float32)
    top_row = np.full(ncells, -1, dtype=np.int32)
    count = np.zeros(ncells, dtype=np.int32)
    top[cells], top_row[cells], count[cells] = height[order[first]], order[first], counts
    shape = (cg["ny"], cg["nx"])
    return dict(top=top.reshape(shape), top_row=top_row.reshape(shape), count=count.reshape(shape), height=height)


# ------------------------------------------------------------------ smoothing, tops, parents, roots, crowns, table
def smooth_reference(top, S):
    top = np.asarray(top, dtype=np.float32)
    ny, nx = top.shape
    sm = np.full(top.shape, NAN32, dtype=np.float32)
    vals = top.astype(np.float64).tolist()
    for fy in range(ny):
        for fx in range(nx):
            if math.isnan(vals[fy][fx]):
                continue
            total, cnt = 0.0, 0
            for y in range(max(fy - S, 0), min(fy + S, ny - 1) + 1):
                line = vals[y]
                for x in range(max(fx - S, 0), min(fx + S, nx - 1) + 1):
                    v = line[x]
                    if v == v:
                        total = total + v
                        cnt = cnt + 1
            sm[fy, fx] = np.float32(total / float(cnt))
    return sm


def window_of(s, cell, r0, r1):
    """W of a cell with smoothed height s"""
    with np.errstate(all="ignore"):
        q = np.floor((np.float64(r0) + (np.float64(r1) * np.float64(s))) / np.float64(cell))
    if not q >= 1.0:
        return 1
    return MAX_WINDOW if q > MAX_WINDOW else int(q)


def segment_reference(top, top_row, count, cell, S, r0, r1, top_min, crown_frac, Rc, sm=None):
    """steps 2 - 8 of the rule on the [ny,nx] grids: dict(smooth, window, is_top, parent, root, tree, ntrees and the five
    table columns over all trees)"""
    top = np.asarray(top, dtype=np.float32)
    ny, nx = top.shape
    n = nx * ny
    sm = smooth_reference(top, S) if sm is None else np.asarray(sm, dtype=np.float32)
    s = sm.reshape(-1).astype(np.float64).tolist()          # float32 values, compared as such
    has = [v == v for v in s]

    def beats(a, b):
        return s[a] > s[b] or (s[a] == s[b] and a < b)

    window = np.zeros(n, dtype=np.int32)
    is_top = np.zeros(n, dtype=bool)
    parent = list(range(n))
    live = [c for c in range(n) if has[c]]
    for c in live:
        fy, fx = divmod(c, nx)
        W = window_of(s[c], cell, r0, r1)
        window[c] = W
        best = -1
        for y in range(max(fy - W, 0), min(fy + W, ny - 1) + 1):
            for x in range(max(fx - W, 0), min(fx + W, nx - 1) + 1):
                dx, dy = x - fx, y - fy
                k = y * nx + x
                if k == c or dx * dx + dy * dy > W * W or not has[k]:
                    continue
                if best < 0 or beats(k, best):
                    best = k
        beaten = best >= 0 and beats(best, c)
        is_top[c] = s[c] >= top_min and not beaten
        nb = -1
        for y in range(max(fy - 1, 0), min(fy + 1, ny - 1) + 1):
            for x in range(max(fx - 1, 0), min(fx + 1, nx - 1) + 1):
                k = y * nx + x
                if k == c or not has[k]:
                    continue
                if nb < 0 or beats(k, nb):
                    nb = k
        if nb >= 0 and beats(nb, c):
            parent[c] = nb
        elif beaten:
            parent[c] = best
    root = list(range(n))
    for c in live:
        r = c
        while parent[r] != r:
            r = parent[r]
        root[c] = r
    tops = np.flatnonzero(is_top)
    id_of = np.full(n, -1, dtype=np.int64)
    id_of[tops] = np.arange(len(tops))
    tree = np.full(n, -1, dtype=np.int32)
    for c in live:
        r = root[c]
        if not is_top[r]:
            continue
        dx, dy = c % nx - r % nx, c // nx - r // nx
        if s[c] >= (crown_frac * s[r]) and dx * dx + dy * dy <= Rc * Rc:
            tree[c] = id_of[r]
    T = len(tops)
    cells = np.zeros(T, dtype=np.int32)
    rows = np.zeros(T, dtype=np.int64)
    key = [0] * T
    max_height = np.full(T, NAN32, dtype=np.float32)
    max_row = np.full(T, -1, dtype=np.int32)
    tf_, tr_, cn_ = top.reshape(-1), np.asarray(top_row).reshape(-1), np.asarray(count).reshape(-1)
    for c in live:
        t = tree[c]
        if t < 0:
            continue
        cells[t] += 1
        rows[t] += int(cn_[c])
        k = pack(tf_[c], tr_[c])
        if k > key[t]:
            key[t], max_height[t], max_row[t] = k, tf_[c], tr_[c]
    return dict(smooth=sm, window=window.reshape(ny, nx), is_top=is_top.reshape(ny, nx),
                parent=np.array(parent, dtype=np.int64), root=np.array(root, dtype=np.int64), tree=tree.reshape(ny, nx),
                ntrees=T, top_cell=tops.astype(np.int32), cells=cells, rows=rows, max_height=max_height, max_row=max_row)


def rows_reference(X, tg, ground, cg, h_min, h_max, tree, sub=None, skip=None):
    part, cell, _, _ = takes_part(X, tg, ground, cg, h_min, h_max, sub, skip)
    return np.where(part, np.asarray(tree).reshape(-1)[cell], -1).astype(np.int32)


# ------------------------------------------------------------------ second statements
def tops_by_sliding_maximum(sm, W, top_min):
    """for one W (r1 = 0): a cell is a top iff it reaches top_min, no cell of the disc that comes before it in index
    order is >= it and none that comes after it is > it - two sliding maxima, one per half of the footprint"""
    from numpy.lib.stride_tricks import sliding_window_view
    sm = np.asarray(sm, dtype=np.float32)
    a = np.where(np.isnan(sm), -np.inf, sm.astype(np.float64))
    pad = np.pad(a, W, constant_values=-np.inf)
    view = sliding_window_view(pad, (2 * W + 1, 2 * W + 1))
    dy, dx = np.mgrid[-W:W + 1, -W:W + 1]
    disc = dx * dx + dy * dy <= W * W
    before = disc & ((dy < 0) | ((dy == 0) & (dx < 0)))
    after = disc & ((dy > 0) | ((dy == 0) & (dx > 0)))
    hi_before = np.where(before, view, -np.inf).max(axis=(2, 3))
    hi_after = np.where(after, view, -np.inf).max(axis=(2, 3))
    with np.errstate(invalid="ignore"):
        return ~np.isnan(sm) & (sm.astype(np.float64) >= top_min) & (hi_before < a) & (hi_after <= a)


def roots_by_union(sm, parent):
    """every cell united with its parent; a set's root is its greatest member under "beats" """
    s = np.asarray(sm, dtype=np.float32).reshape(-1)
    n = len(s)
    rep = list(range(n))

    def find(a):
        while rep[a] != a:
            rep[a] = rep[rep[a]]
            a = rep[a]
        return a

    for c in range(n):
        a, b = find(c), find(int(parent[c]))
        if a != b:
            rep[a] = b
    groups = {}
    for c in range(n):
        groups.setdefault(find(c), []).append(c)
    root = np.arange(n)
    for members in groups.values():
        m = np.array(members)
        if np.isnan(s[m]).any():
            continue                                          # a cell without a value is alone
        order = np.lexsort((m, -s[m].astype(np.float64)))
        root[m] = m[order[0]]
    return root


# ------------------------------------------------------------------ the scene: the line, its ground, planted trees
CELL, H_MIN, H_MAX, SMOOTH, R0, R1, TOP_MIN, CROWN_FRAC, CROWN_RADIUS = 0.5, 2.0, 45.0, 1, 1.5, 0.05, 5.0, 0.5, 8.0
# name, station, lateral, height of the top, crown radius, crown depth
PLANTED = (("low", 140.0, -18.0, 9.0, 2.5, 4.0), ("mid", 10.0, -22.0, 12.0, 3.0, 6.0), ("high", 70.0, -20.0, 16.0, 4.0, 8.0),
           ("left", 90.0, -22.0, 18.0, 4.5, 9.0), ("right", 96.0, -22.0, 24.0, 4.0, 10.0),
           ("twin", 120.0, 20.0, 14.0, 3.0, 6.0), ("shrub", 30.0, 22.0, 3.0, 1.0, 1.0),
           ("banked", 30.0, 39.0, 10.0, 2.5, 5.0))
TWIN = (1.5, 13.6)                               # the second maximum of "twin": metres along the station, height
LATTICE = 0.25
# the overlapping pair, computed on the CPU from the statement alone and recorded here: of the pair's rows that got a
# tree, how many went to "right" - the figure the device must reproduce exactly
OVERLAP_RIGHT_SHARE = (1068, 1872)
_SCENE = {}
_REF = {}


def _crown(rng, station, lateral, base, height, radius, depth, extra=None):
    """a stem every 0.25 m from 1 m up to the crown's base and a paraboloid crown on a 0.25 m lattice: the surface
    z = base + height - depth (d / radius)^2 within the radius (``extra``: a second paraboloid, the higher one counts),
    with 0.03 m of jitter in x and y and N(0, 0.02) in z"""
    k = int(math.ceil(radius / LATTICE)) + (8 if extra else 0)
    ds, dl = np.meshgrid(LATTICE * np.arange(-k, k + 1), LATTICE * np.arange(-k, k + 1), indexing="ij")
    ds, dl = ds.reshape(-1), dl.reshape(-1)
    d2 = ds * ds + dl * dl
    z = np.where(d2 <= radius * radius, height - depth * d2 / (radius * radius), -np.inf)
    if extra:
        e2 = (ds - extra[0]) ** 2 + dl * dl
        z = np.maximum(z, np.where(e2 <= radius * radius, extra[1] - depth * e2 / (radius * radius), -np.inf))
    on = np.isfinite(z)
    ds, dl, z = ds[on], dl[on], z[on]
    up = np.arange(1.0, height - depth, LATTICE)
    st = np.concatenate([station + ds, np.full(len(up), station)]) + rng.uniform(-0.03, 0.03, len(z) + len(up))
    lat = np.concatenate([lateral + dl, np.full(len(up), lateral)]) + rng.uniform(-0.03, 0.03, len(z) + len(up))
    zz = base + np.concatenate([z, up]) + rng.normal(0.0, 0.02, len(z) + len(up))
    return np.concatenate([sp._line_xy(st, lat), zz[:, None]], axis=1).astype(np.float32)


def canopy_scene():
    """(X float32 [n,3], kind int8, skip uint8 [n]): ``treefall_cases.stem_scene`` (kinds 0..43) followed by the planted
    trees (kinds 50..57, in PLANTED's order).  ``skip`` marks what is neither ground nor vegetation: the rows of
    ``clearance_cases.tree_scene`` (the line, its clutter and the cones that hang in the air, kinds 0..12) and the roof
    (kind 21)."""
    if not _SCENE:
        X, kind, _ = tf.stem_scene()
        rng = np.random.default_rng(68)
        parts, kinds = [X], [kind]
        for i, (name, station, lateral, height, radius, depth) in enumerate(PLANTED):
            base = float(tf.true_ground(np.float64(station), np.float64(lateral)))
            parts.append(_crown(rng, station, lateral, base, height, radius, depth, TWIN if name == "twin" else None))
            kinds.append(np.full(len(parts[-1]), 50 + i, dtype=np.int8))
        X, kind = np.vstack(parts), np.concatenate(kinds)
        skip = ((kind <= 12) | (kind == 21)).astype(np.uint8)
        for a in (X, kind, skip):
            a.setflags(write=False)
        _SCENE["case"] = (X, kind, skip)
    return _SCENE["case"]


def canopy_grid_of(tg, cell):
    """the canopy grid over the terrain grid's extent: ops._terrain_grid_of's arithmetic on the extent's corners"""
    out = dict(cell=float(cell))
    for name in ("x", "y"):
        a = tg[name + "0"]
        b = a + tg["n" + name] * tg["cell"]
        out[name + "0"], out["n" + name] = a, int(math.floor((b - a) / cell)) + 1
    return out


def crown_cells_of(cell, crown_radius):
    return max(1, int(math.ceil(crown_radius / cell)))


def _axis_cell(cg, station, lateral):
    xy = sp._line_xy(np.array([station]), np.array([lateral]))[0]
    return int(math.floor((xy[0] - cg["x0"]) / cg["cell"])), int(math.floor((xy[1] - cg["y0"]) / cg["cell"]))


def reference():
    """the scene's reference answers, computed once, with its margins asserted on the host so that the pipeline's integer
    outputs may be compared exactly: ``grid`` / ``ground`` (the terrain rule on the whole scene, nothing skipped),
    ``canopy_grid``, the outputs of ``top_reference`` and ``segment_reference``, ``row_tree``, ``planted`` (tree id per
    PLANTED entry, -1 for the shrub), ``stems`` (tree id per treefall stem), ``share`` and ``tol``"""
    if not _REF:
        X, kind, skip = canopy_scene()
        tol = 1.2e-5
        tg = tc.scene_grid(X, tc.CELL)
        low, _ = tc.low_reference(X, tg)
        _, ground, _ = tc.ground_reference(low, tc.WINDOW_CELLS, tc.DH, tc.MAX_GAP)
        cg = canopy_grid_of(tg, CELL)
        Rc = crown_cells_of(CELL, CROWN_RADIUS)
        t = top_reference(X, tg, ground, cg, H_MIN, H_MAX, skip=skip)
        seg = segment_reference(t["top"], t["top_row"], t["count"], CELL, SMOOTH, R0, R1, TOP_MIN, CROWN_FRAC, Rc)
        row_tree = rows_reference(X, tg, ground, cg, H_MIN, H_MAX, seg["tree"], skip=skip)
        part, cell, Hd, _ = takes_part(X, tg, ground, cg, H_MIN, H_MAX, skip=skip)
        # no Hd within 10 tol of h_min or h_max, no smoothed height within 10 tol of top_min
        alive = (skip == 0) & ~np.isnan(Hd)
        assert min(np.abs(Hd[alive] - H_MIN).min(), np.abs(Hd[alive] - H_MAX).min()) > 10.0 * tol
        s = seg["smooth"].reshape(-1).astype(np.float64)
        live = np.flatnonzero(~np.isnan(s))
        assert np.abs(s[live] - TOP_MIN).min() > 10.0 * tol
        # no cell within 10 tol of its crown_frac decision (where its root is a top)
        root, is_top = seg["root"], seg["is_top"].reshape(-1)
        rooted = live[is_top[root[live]]]
        assert np.abs(s[rooted] - CROWN_FRAC * s[root[rooted]]).min() > 10.0 * tol
        # no two cells whose order decides a top or a parent within 10 tol, unless exactly equal: every cell against
        # the greatest of its window and of its neighbours, and each of those against the runner-up
        nx, ny = cg["nx"], cg["ny"]
        S2 = seg["smooth"]
        worst = np.inf
        for c in live:
            fy, fx = divmod(int(c), nx)
            W = int(seg["window"].reshape(-1)[c])
            for R in (W, 1):
                y0, y1, x0, x1 = max(fy - R, 0), min(fy + R, ny - 1), max(fx - R, 0), min(fx + R, nx - 1)
                blk = S2[y0:y1 + 1, x0:x1 + 1].astype(np.float64)
                dy, dx = np.mgrid[y0 - fy:y1 - fy + 1, x0 - fx:x1 - fx + 1]
                inw = ~np.isnan(blk) & ((dx != 0) | (dy != 0)) & ((dx * dx + dy * dy <= W * W) if R == W else True)
                v = np.sort(blk[inw])[::-1]
                gaps = []
                if len(v):
                    gaps.append(abs(v[0] - s[c]))
                if len(v) > 1 and v[0] > s[c]:
                    gaps.append(v[0] - v[1])
                for gp in gaps:
                    if gp != 0.0:
                        worst = min(worst, gp)
        assert worst > 10.0 * tol, worst
        # the trees: one per planted tree at or above top_min and one per stem; every top within one cell of its axis
        axes = [(p[1], p[2]) for p in PLANTED] + [(st[1], st[2]) for st in tf.STEMS]
        want = [p[3] >= TOP_MIN for p in PLANTED] + [True] * len(tf.STEMS)
        assert seg["ntrees"] == sum(want), (seg["ntrees"], sum(want))
        ids = []
        for (station, lateral), w in zip(axes, want):
            ax, ay = _axis_cell(cg, station, lateral)
            near = [k for k, c in enumerate(seg["top_cell"]) if abs(c % nx - ax) <= 1 and abs(c // nx - ay) <= 1]
            assert len(near) == (1 if w else 0), (station, lateral, near)
            ids.append(near[0] if w else -1)
        planted, stems = np.array(ids[:len(PLANTED)]), np.array(ids[len(PLANTED):])
        names = [p[0] for p in PLANTED]
        # the shrub's rows get -1; every row of a separated tree that takes part carries its tree's id
        shrub = kind == 50 + names.index("shrub")
        assert part[shrub].any() and (row_tree[shrub] == -1).all()
        for name in ("low", "mid", "high", "twin", "banked"):
            i = names.index(name)
            mine = part & (kind == 50 + i)
            assert mine.sum() > 100 and (row_tree[mine] == planted[i]).all(), name
        # the overlapping pair: how many of the pair's rows that got a tree went to "right" - a recorded result
        pair = part & ((kind == 50 + names.index("left")) | (kind == 50 + names.index("right")))
        owned = pair & (row_tree >= 0)
        assert np.isin(row_tree[owned], planted[[names.index("left"), names.index("right")]]).all()
        share = (int((row_tree[owned] == planted[names.index("right")]).sum()), int(owned.sum()))
        _REF.update(t, **seg)
        _REF.update(grid=tg, ground=ground, canopy_grid=cg, crown_cells=Rc, row_tree=row_tree, part=part, planted=planted,
                    stems=stems, share=share, tol=tol, kind=kind, skip=skip)
    return _REF
