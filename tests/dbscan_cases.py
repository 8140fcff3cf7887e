"""Inputs that put DBSCAN's eps predicate on its boundary, and all-pairs statements of what stage C's calls return
(TEST INFRASTRUCTURE, pure numpy; imported by the CPU and the GPU tests, not a conftest).

The instrument is the float64 matrix of squared distances ``pair_d2``: coordinates promoted from float32, the three
squares accumulated in order - the arithmetic of ``oracle.dbscan.radius_neighbors_bruteforce`` and of sklearn's
``euclidean_rdist``.  Every ``eps`` and ``min_samples`` below is read off that matrix, never counted by hand:

* lattices with power-of-two spacing: a lattice sphere passes exactly through lattice points, so pairs sit at
  ``d2 == eps*eps`` in float32 and float64 alike;
* k-distance picks: ``eps_at(d2)`` gives the smallest double ``e`` with ``e*e >= d2`` and its predecessor ``em``; a
  point is core at ``e`` and not at ``em``, and ``e*e`` / ``em*em`` round to one float32;
* two clumps whose closest cross pair decides one cluster or two; a lone point whose nearest core point decides
  label or noise.
"""
import math

import numpy as np

EPSG = np.array([437000.0, 3139000.0, 80.0])


# ------------------------------------------------------------------ the instrument
def pair_d2(X, Q=None):
    """float64 [len(Q), len(X)] squared distances (Q defaults to X; both float32 coordinates)"""
    X64 = np.ascontiguousarray(np.asarray(X), dtype=np.float64)
    Q64 = X64 if Q is None else np.ascontiguousarray(np.asarray(Q), dtype=np.float64).reshape(-1, 3)
    d = np.zeros((Q64.shape[0], X64.shape[0]), dtype=np.float64)
    for j in range(3):                                   # d += tmp*tmp, j ascending
        t = Q64[:, j:j + 1] - X64[None, :, j]
        d += t * t
    return d


def neighbour_counts(X, eps_list, strict=False, block=1024):
    """int64 [len(eps_list), n]: neighbours of every row (self included) under d2 <= eps*eps, or d2 < eps*eps with
    ``strict``, for every eps of the list (one pass over the matrix)"""
    X = np.asarray(X)
    r2 = [float(e) * float(e) for e in eps_list]
    out = np.empty((len(r2), len(X)), dtype=np.int64)
    for s in range(0, len(X), block):
        d = pair_d2(X, X[s:s + block])
        for k, r in enumerate(r2):
            out[k, s:s + block] = ((d < r) if strict else (d <= r)).sum(1)
    return out


def eps_at(d2):
    """(e, em): e the smallest double with e*e >= d2 (the product as the kernels and sklearn form it), em its
    predecessor - a pair at squared distance d2 is inside at e and outside at em"""
    d2 = float(d2)
    assert d2 > 0.0
    e = math.sqrt(d2)
    while e * e >= d2:
        e = math.nextafter(e, 0.0)
    while e * e < d2:
        e = math.nextafter(e, math.inf)
    em = math.nextafter(e, 0.0)
    assert e * e >= d2 > em * em
    return e, em


def f32_only_core(X, eps, ms):
    """the strawman: float32 arithmetic only, d32 <= float32(eps*eps).  Proves that a fixture is hard."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
    r2 = np.float32(float(eps) * float(eps))
    cnt = np.zeros(len(X), dtype=np.int64)
    for s in range(0, len(X), 1024):
        d = np.zeros((len(X[s:s + 1024]), len(X)), dtype=np.float32)
        for j in range(3):
            t = X[s:s + 1024, j:j + 1] - X[None, :, j]
            d += t * t
        cnt[s:s + 1024] = (d <= r2).sum(1)
    return (cnt >= int(ms)).astype(np.uint8)


# ------------------------------------------------------------------ the grid stage C lays over a fit
def grid_cells(X, eps, origin=None):
    """int64 [n,3] cell of every row: floor((x - origin) / s) with s = eps/sqrt(3) * (1 - 2^-16) and the origin at
    the lower corner of the box (float32), as stage C computes it"""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    o = X64.min(0) if origin is None else np.asarray(origin, dtype=np.float32).astype(np.float64)
    inv = 1.0 / (float(eps) / 1.7320508075688772 * (1.0 - 1.0 / 65536.0))
    return np.floor((X64 - o) * inv).astype(np.int64)


def cell_census(X, eps, origin=None):
    """(cnt [n], tot [n]): rows in the row's own cell, and rows in the 5x5x5 block of cells around it - what
    db_core_k branches on (cnt >= min_samples: dense; cnt < 24: one query at a time; tot >= 8192: long sweep)"""
    c = grid_cells(X, eps, origin)
    c = c - c.min(0)
    dims = c.max(0) + 1
    H = np.zeros(tuple(dims + 4), dtype=np.int64)
    np.add.at(H, (c[:, 0] + 2, c[:, 1] + 2, c[:, 2] + 2), 1)
    S = H
    for ax in range(3):                                   # box sum of width 5 per axis
        S = sum(np.roll(S, k, axis=ax) for k in (-2, -1, 0, 1, 2))
    idx = (c[:, 0] + 2, c[:, 1] + 2, c[:, 2] + 2)
    return H[idx], S[idx]


def count_cells(X, eps, chunk_size=0):
    """occupied cells, summed over the chunks (each chunk has its own cells; one box for all)"""
    c = grid_cells(X, eps)
    cs = int(chunk_size) if int(chunk_size) > 0 else len(X)
    return sum(len(np.unique(c[s:s + cs], axis=0)) for s in range(0, len(X), cs))


# ------------------------------------------------------------------ a. lattices
def _lattice(dims, h, offset, seed):
    g = np.stack(np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    X64 = g * h + np.asarray(offset, dtype=np.float64)
    X = X64.astype(np.float32)
    assert (X.astype(np.float64) == X64).all(), "lattice not representable in float32"
    return X[np.random.default_rng(seed).permutation(len(X))]


def lattice_few():
    """spacing 0.5 at the EPSG offset, eps 1.5: cells of 1..8 points (one query at a time), 30 ties per sphere"""
    return _lattice((12, 12, 12), 0.5, EPSG, 101), 1.5


def lattice_tile():
    """spacing 0.5 at the origin, eps 3.0: cells of 27..64 points (staged tiles), below every min_samples"""
    return _lattice((16, 16, 16), 0.5, (0.0, 0.0, 0.0), 102), 3.0


def lattice_long():
    """spacing 0.5 at the EPSG offset, eps 4.5 (102 ties per sphere): a 5x5x5 block of cells spans 26 lattice steps,
    more than 8192 candidates.  A cavity in the middle, wider than two cells, keeps every third lattice point per
    axis: cells of a few points amid the full blocks"""
    g = np.stack(np.meshgrid(*[np.arange(26)] * 3, indexing="ij"), -1).reshape(-1, 3)
    inside = ((g >= 8) & (g < 19)).all(1)
    keep = ~inside | (g % 3 == 2).all(1)
    X64 = g[keep] * 0.5 + EPSG
    X = X64.astype(np.float32)
    assert (X.astype(np.float64) == X64).all()
    return X[np.random.default_rng(103).permutation(len(X))], 4.5


def lattice_dense():
    """a block of spacing 0.125 (cells of up to 343 points: dense at the min_samples taken here) beside a lattice of
    spacing 0.5 whose points reach into the block, eps 1.5 (float32 has no 0.125 steps at EPSG northings: a small
    offset instead)"""
    d = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.125
    s = np.stack(np.meshgrid(np.arange(8), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3) * 0.5
    s = s + np.array([-4.75, -1.5, -1.5])                # x = -4.75 .. -1.25: 1.25 in front of the block's face
    X64 = np.vstack([d, s]) + np.array([437.0, 3139.0, 80.0])
    X = X64.astype(np.float32)
    assert (X.astype(np.float64) == X64).all()
    return X[np.random.default_rng(104).permutation(len(X))], 1.5


LATTICES = {"few": lattice_few, "tile": lattice_tile, "long": lattice_long, "dense": lattice_dense}


def lattice_probe(name, X, eps):
    """the row whose neighbourhood sets min_samples: it has pairs exactly at eps, and for the branch fixtures it
    sits in the kind of cell the fixture is built for"""
    em = math.nextafter(float(eps), 0.0)
    ce, cm = neighbour_counts(X, [eps, em])
    cnt, tot = cell_census(X, eps)
    ok = ce > cm
    if name == "few":
        ok &= (cnt < 24) & (ce == ce.max())
    elif name == "tile":
        ok &= (cnt >= 24) & (ce == ce.max())
    elif name == "long":
        ok &= (cnt < 24) & (tot >= 8192)
    elif name == "dense":
        ok &= (cnt < 24) & (cm + 1 <= cnt.max())
    rows = np.flatnonzero(ok)
    assert len(rows), name
    p = rows[np.argmax(ce[rows])]
    return int(p), ce, cm


_LATTICE_CACHE = {}


def lattice_case(name):
    """(X, eps, em, [count at eps (probe core), that + 1 (not core), count at em + 1 (core at eps only)], probe
    row), em = nextafter(eps, 0); computed once per process"""
    if name not in _LATTICE_CACHE:
        X, eps = LATTICES[name]()
        p, ce, cm = lattice_probe(name, X, eps)
        X.setflags(write=False)
        _LATTICE_CACHE[name] = (X, eps, math.nextafter(eps, 0.0), [int(ce[p]), int(ce[p]) + 1, int(cm[p]) + 1], p)
    return _LATTICE_CACHE[name]


# ------------------------------------------------------------------ b. k-distance picks
def blob_cloud(epsg, seed=7):
    """two blobs of 700 points and 300 clutter; local coordinates carry full 24-bit mantissas"""
    rng = np.random.default_rng(seed)
    X = np.vstack([rng.normal([10.0, 12.0, 20.0], [2.5, 2.5, 6.0], (700, 3)),
                   rng.normal([32.0, 15.0, 22.0], [2.5, 2.5, 6.0], (700, 3)),
                   rng.uniform(0.0, 45.0, (300, 3))])
    X = X[rng.permutation(len(X))]
    if epsg:
        X = X + EPSG
    return X.astype(np.float32)


def tight_cloud(seed=5):
    """1700 points around the origin, spread 0.6: neighbours are as far apart as the coordinates are large, so the
    float32 differences round as well (between neighbours of the clouds above they are exact) and the float32
    distance strays furthest from the float64 one - the input that needs the full width of the guard band"""
    return np.random.default_rng(seed).normal(0.0, 0.6, (1700, 3)).astype(np.float32)


KDIST_CLOUDS = {"local": lambda: blob_cloud(False), "epsg": lambda: blob_cloud(True), "tight": tight_cloud}


def banded_count(X, i, eps, band):
    """(neighbours of row i as a float32 pre-filter with a relative guard band of ``band`` around eps*eps counts them -
    exact arithmetic inside the band only, as db_within2 does - , neighbours by the matrix)"""
    X = np.asarray(X, dtype=np.float32)
    e2 = float(eps) * float(eps)
    lo = np.nextafter(np.float32(e2 * (1.0 - band)), np.float32(-np.inf))
    hi = np.nextafter(np.float32(e2 * (1.0 + band)), np.float32(np.inf))
    t = [(X[i, j] - X[:, j]).astype(np.float64) for j in range(3)]       # float32 differences; squares exact in float64
    d = (t[0] * t[0]).astype(np.float32).astype(np.float64)
    d = (t[1] * t[1] + d).astype(np.float32).astype(np.float64)          # fma: one rounding
    d = (t[2] * t[2] + d).astype(np.float32)
    D = pair_d2(X, X[i])[0]
    inside = np.where(d <= lo, True, np.where(d >= hi, False, D <= e2))
    return int(inside.sum()), int((D <= e2).sum())


KDIST_MS = (1, 2, 8, 20, 80)
KDIST_PICKS = 32


def kdist_picks(X, D, ms, npick=KDIST_PICKS, seed=0):
    """([(row, e, em, j)], skipped) for seeded rows: the k-th smallest entry of the row of D (self included), the
    distance to row j, sets eps: the row is core at e and not at em.  A row whose k-th distance ties with the
    (k-1)-th or (k+1)-th is skipped.  For min_samples = 1 every point is core at any eps and the 1st distance is 0:
    the pick takes k = 2, where the nearest neighbour j enters - at e the two rows share a cluster, at em they do not
    unless a third row links them, which the CPU test rules out from the oracle."""
    rng = np.random.default_rng(1000 * int(ms) + seed)
    rows = rng.choice(len(X), npick, replace=False)
    picks, skipped = [], 0
    k = max(int(ms), 2)
    for i in rows:
        order = np.argsort(D[i], kind="stable")
        d = D[i][order]
        if d[k - 1] == d[k - 2] or (k < len(d) and d[k - 1] == d[k]):
            skipped += 1
            continue
        e, em = eps_at(d[k - 1])
        picks.append((int(i), e, em, int(order[k - 1])))
    return picks, skipped


def f32_only_within(x, y, eps):
    """the strawman on one pair: float32 differences, squares and sum against float32(eps*eps)"""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    t = x - y
    d = np.float32(0.0)
    for j in range(3):
        d = np.float32(d + t[j] * t[j])
    return bool(d <= np.float32(float(eps) * float(eps)))


# ------------------------------------------------------------------ c. link at the boundary
DIRECTIONS = {"x": (1.0, 0.0, 0.0), "xy": (1.0, 1.0, 0.0), "xyz": (1.0, 1.0, 1.0), "generic": (0.62, -0.41, 0.67)}


def _clump(rng, centre, n, radius):
    v = rng.normal(size=(n, 3))
    v *= (radius * rng.uniform(0.2, 1.0, (n, 1))) / np.linalg.norm(v, axis=1, keepdims=True)
    return np.asarray(centre) + v


def link_case(direction, halo=False, epsg=False, seed=0, eps0=None, ms=12):
    """(X, ms, e, em, (rows of clump A, rows of clump B)).  Two clumps within 1e-3*eps0, eps0 apart along the
    direction; d2* is the smallest cross entry of D, at e one cluster, at em two.  With ``halo`` the clumps hold
    ms - 4 points and a sparse ring of radius 0.9*eps0 around each centre supplies the rest: no cell holds ms points,
    so no cell is dense and the link is found by the sweeping union kernels."""
    if eps0 is None:
        eps0 = 16.0 if epsg else 2.0                     # float32 steps of 0.25 at EPSG northings: a larger figure
    rng = np.random.default_rng(500 + seed + 17 * sorted(DIRECTIONS).index(direction) + (1 if halo else 0))
    u = np.asarray(DIRECTIONS[direction])
    u = u / np.linalg.norm(u)
    ca = np.array([3.37, 5.11, 2.93]) + (EPSG if epsg else 0.0)
    cb = ca + eps0 * u
    nc = ms - 4 if halo else ms + 3
    parts = [_clump(rng, ca, nc, 1e-3 * eps0 / 2), _clump(rng, cb, nc, 1e-3 * eps0 / 2)]
    if halo:
        # a ring around each centre in the plane across the direction: within eps of its own clump, 1.34*eps0 from the
        # other clump; the second ring is turned by half a step, so ring points of the two sides stay 1.02*eps0 apart
        w = np.cross(u, [0.3, 0.5, 0.81])
        w /= np.linalg.norm(w)
        w2 = np.cross(u, w)
        for c, phase in ((ca, 0.0), (cb, np.pi / 12)):
            ang = phase + np.arange(12) * (2 * np.pi / 12)
            parts.append(c + 0.9 * eps0 * (np.cos(ang)[:, None] * w + np.sin(ang)[:, None] * w2)
                         + rng.normal(0, 1e-4, (12, 3)))
    X = np.vstack(parts).astype(np.float32)
    perm = rng.permutation(len(X))
    inv = np.argsort(perm)
    X = X[perm]
    a, b = np.sort(inv[np.arange(nc)]), np.sort(inv[np.arange(nc, 2 * nc)])
    e, em = eps_at(pair_d2(X[b], X[a]).min())
    return X, ms, e, em, (a, b)


# ------------------------------------------------------------------ d. border at the boundary
def border_case(two=False, epsg=False, seed=0, eps0=2.0, ms=12):
    """(X, ms, e, em, lone row, rows of clump A[, rows of clump B]).  A clump of ms + 2 points and a lone point eps0
    away; d2* is the smallest entry of D between them: the lone point is labelled at e and noise at em.  With ``two``
    a second clump is the mirror image of the first through the lone point (coordinates on a 2^-12 grid, so the image
    is exact in float32 and every distance to it equals its twin's in float64): the lone point sits at its boundary
    distance from both clusters at once, and the smaller id wins.  File order: clump A, the lone point, clump B."""
    rng = np.random.default_rng(900 + seed + (1 if two else 0))
    ca = np.array([7.13, 2.57, 4.21]) + (EPSG if epsg else 0.0)
    u = np.array([0.53, 0.31, -0.79])
    u /= np.linalg.norm(u)
    nc = ms + 2
    A = _clump(rng, ca, nc, 1e-3 * eps0 / 2)
    lone = ca + eps0 * u
    if two:
        assert not epsg, "the mirror image needs more fraction bits than float32 has at EPSG coordinates"
        A, lone = np.round(A * 4096.0) / 4096.0, np.round(lone * 4096.0) / 4096.0
        X64 = np.vstack([A, lone[None, :], 2.0 * lone - A])
        X = X64.astype(np.float32)
        assert (X.astype(np.float64) == X64).all()
    else:
        X = np.vstack([A, lone[None, :]]).astype(np.float32)
    a, lone_row = np.arange(nc), nc
    e, em = eps_at(pair_d2(X[a], X[lone_row]).min())
    if two:
        b = np.arange(nc + 1, 2 * nc + 1)
        assert pair_d2(X[b], X[lone_row]).min() == pair_d2(X[a], X[lone_row]).min()
        return X, ms, e, em, lone_row, a, b
    return X, ms, e, em, lone_row, a


# ------------------------------------------------------------------ all-pairs statements of the continuation calls
def relabel_reference(X, core, labels, cmap, eps, chunk_size=0):
    """pch_dbscan_relabel_i32 per chunk of chunk_size rows (0: the whole array): core rows take cmap[label] (ids
    outside [0, len(cmap)) give -1); non-core rows take the smallest new id >= 0 among their core neighbours within
    eps in the same chunk, else -1"""
    X = np.asarray(X, dtype=np.float32)
    core = np.asarray(core).astype(bool)
    labels = np.asarray(labels).astype(np.int64)
    cmap = np.asarray(cmap).astype(np.int64)
    n = len(X)
    out = np.full(n, -1, dtype=np.int64)
    ok = core & (labels >= 0) & (labels < len(cmap))
    out[ok] = cmap[labels[ok]]
    r2 = float(eps) * float(eps)
    cs = int(chunk_size) if int(chunk_size) > 0 else max(n, 1)
    big = np.iinfo(np.int64).max
    for s in range(0, n, cs):
        sl = slice(s, min(s + cs, n))
        c_rows = s + np.flatnonzero(core[sl] & (out[sl] >= 0))
        q_rows = s + np.flatnonzero(~core[sl])
        if not len(c_rows) or not len(q_rows):
            continue
        for q0 in range(0, len(q_rows), 512):
            q = q_rows[q0:q0 + 512]
            hit = pair_d2(X[c_rows], X[q]) <= r2
            best = np.where(hit, out[c_rows][None, :], big).min(1)
            out[q] = np.where(best == big, -1, best)
    return out.astype(np.int32)


def first_core_rows_reference(core, labels, k):
    """smallest core row of every cluster id 0..k-1"""
    core = np.asarray(core).astype(bool)
    labels = np.asarray(labels)
    out = np.full(int(k), -1, dtype=np.int32)
    rows = np.flatnonzero(core & (labels >= 0))
    first = np.full(int(k), np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, labels[rows], rows)
    out[:] = first
    return out


def bridge_cloud(n, seed, epsg=False):
    """blobs, a thin bridge between two of them, clutter, and rows between neighbouring blobs that touch both"""
    rng = np.random.default_rng(seed)
    k = 6
    centres = np.column_stack([np.arange(k) * 14.0 + 8.0, rng.uniform(8, 14, k), rng.uniform(8, 14, k)])
    per = int(n * 0.7) // k
    sigma = 2.2 * (n / 12000.0) ** (1.0 / 3.0)                      # the same density at every n
    parts = [rng.normal(c, sigma, (per, 3)) for c in centres]
    nb = n // 20
    t = rng.uniform(0, 1, (nb, 1))
    parts.append(centres[0] + t * (centres[1] - centres[0]) + rng.normal(0, 0.25, (nb, 3)))   # the bridge
    nt = n // 40
    for a in range(2, k - 1):                                          # sparse rows half way: border candidates
        mid = (centres[a] + centres[a + 1]) / 2
        parts.append(mid + rng.normal(0, [0.8, 3.0, 3.0], (nt // (k - 3) + 1, 3)))
    rest = n - sum(len(p) for p in parts)
    parts.append(np.column_stack([rng.uniform(-5, k * 14.0 + 5, rest), rng.uniform(-5, 27, rest), rng.uniform(-5, 27, rest)]))
    X = np.vstack(parts)[:n]
    X = X[rng.permutation(len(X))]
    if epsg:
        X = X + EPSG
    return X.astype(np.float32)
