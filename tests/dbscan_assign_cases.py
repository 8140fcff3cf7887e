"""The all-pairs statement of pch_dbscan_assign_f32 and the queries its tests use (TEST INFRASTRUCTURE, pure numpy;
imported by the CPU and the GPU tests, not a conftest).

``assign_reference`` says what ``ops.DbscanFit.assign`` returns: for every query the smallest label among the fit's
core rows within eps under ``dbscan_cases.pair_d2`` (float64, three squares accumulated in order), else -1; one fit
per chunk.  Nothing here knows about cells, keys or pieces.
"""
import math

import numpy as np

import dbscan_cases as dc


# ------------------------------------------------------------------ the statement
def _coarse(P, side):
    return np.floor(np.asarray(P, dtype=np.float64) / side).astype(np.int64)


def assign_reference(X, core, labels, Q, eps, chunk_size=0, query_chunk=None, sub=None, prune=False):
    """int32 [len(Q)].  X, core, labels: the fitted rows, their core flags and their CURRENT labels (a core row whose
    label is < 0 - its cluster was dropped by a relabel - attracts nothing).  q = float32(Q) - float32(sub), a float32
    subtraction.  chunk_size > 0: the fit is one fit per chunk_size rows and query_chunk[i] names the chunk query i is
    held against; an index outside [0, nchunks), a chunk holding NaN/inf, and a query holding NaN/inf give -1.

    ``prune`` changes the cost, not the statement: fit rows and queries are bucketed into cubes of side 1.001*eps and
    a query meets only the core rows of the 27 cubes around its own.  Two rows whose cubes are two or more apart on
    an axis differ by more than eps on it, so their squared distance exceeds eps*eps: every skipped pair is outside.
    """
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32)).reshape(-1, 3)
    q = np.ascontiguousarray(np.asarray(Q, dtype=np.float32)).reshape(-1, 3)
    if sub is not None:
        q = q - np.asarray(sub, dtype=np.float32)[None, :]
        assert q.dtype == np.float32
    core = np.asarray(core).astype(bool)
    labels = np.asarray(labels).astype(np.int64)
    n, nq = len(X), len(q)
    cs = int(chunk_size) if 0 < int(chunk_size) < n else max(n, 1)
    nchunks = max(-(-n // cs), 1)
    if query_chunk is None:
        assert nchunks == 1, "a chunked fit needs query_chunk"
        qc = np.zeros(nq, dtype=np.int64)
    else:
        qc = np.asarray(query_chunk).astype(np.int64)
    out = np.full(nq, -1, dtype=np.int64)
    r2 = float(eps) * float(eps)
    big = np.iinfo(np.int64).max
    finite_q = np.isfinite(q).all(1)
    for c in range(nchunks):
        lo, hi = c * cs, min((c + 1) * cs, n)
        if not np.isfinite(X[lo:hi]).all():                        # sklearn refuses the chunk: no fit
            continue
        c_rows = lo + np.flatnonzero(core[lo:hi] & (labels[lo:hi] >= 0))
        q_rows = np.flatnonzero((qc == c) & finite_q)
        if not len(c_rows) or not len(q_rows):
            continue
        Xc, Lc = X[c_rows], labels[c_rows]
        if not prune:
            groups = [(q_rows[s:s + 512], slice(None)) for s in range(0, len(q_rows), 512)]
        else:
            side = 1.001 * float(eps)
            with np.errstate(over="ignore", invalid="ignore"):
                cq = np.clip(np.floor(q[q_rows].astype(np.float64) / side), -2.0 ** 40, 2.0 ** 40).astype(np.int64)
            cx = _coarse(Xc, side)
            uq, inv = np.unique(cq, axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            order = np.argsort(inv, kind="stable")
            bounds = np.searchsorted(inv[order], np.arange(len(uq) + 1))
            groups = []
            for u in range(len(uq)):
                near = np.flatnonzero((np.abs(cx - uq[u][None, :]) <= 1).all(1))
                if len(near):
                    groups.append((q_rows[order[bounds[u]:bounds[u + 1]]], near))
        for qr, sel in groups:
            for s in range(0, len(qr), 512):
                part = qr[s:s + 512]
                hit = dc.pair_d2(Xc[sel], q[part]) <= r2
                best = np.where(hit, Lc[sel][None, :], big).min(1)
                out[part] = np.where(best == big, -1, best)
    return out.astype(np.int32)


def reach_counts(X, core, labels, Q, eps):
    """int64 [len(Q)]: how many different clusters have a core row within eps of each query (single fit)"""
    X = np.asarray(X, dtype=np.float32)
    q = np.asarray(Q, dtype=np.float32).reshape(-1, 3)
    rows = np.flatnonzero(np.asarray(core).astype(bool) & (np.asarray(labels) >= 0))
    lab = np.asarray(labels)[rows]
    k = int(lab.max()) + 1 if len(lab) else 0
    out = np.zeros(len(q), dtype=np.int64)
    fin = np.flatnonzero(np.isfinite(q).all(1))
    for s in range(0, len(fin), 512):
        part = fin[s:s + 512]
        hit = dc.pair_d2(X[rows], q[part]) <= float(eps) * float(eps)
        seen = np.zeros((len(part), k), dtype=bool)
        for c in range(k):
            seen[:, c] = hit[:, lab == c].any(1)
        out[part] = seen.sum(1)
    return out


# ------------------------------------------------------------------ queries
def cell_side(eps):
    return float(eps) / 1.7320508075688772 * (1.0 - 1.0 / 65536.0)


def bridge_queries(X, eps, seed=77):
    """float32 [20012,3] for a fit on X: 12 000 uniform in X's box widened by 3 eps, 6 000 rows of X jittered by
    N(0, 0.4), the first 2 000 rows of X as they are, and twelve rows by hand: NaN, +inf and -inf in one component
    each, +1e30 and -1e30, a row of -0.0 components, and a point 2.5 cells outside each of the six faces of X's box
    (within two cells of the grid on the low side: the clamped path; on the high side the grid's slack cell decides)"""
    X = np.asarray(X, dtype=np.float32)
    rng = np.random.default_rng(seed)
    lo, hi = X.min(0).astype(np.float64), X.max(0).astype(np.float64)
    uni = rng.uniform(lo - 3.0 * eps, hi + 3.0 * eps, (12000, 3))
    jit = X[rng.choice(len(X), 6000, replace=False)].astype(np.float64) + rng.normal(0.0, 0.4, (6000, 3))
    mid = (lo + hi) / 2.0
    hand = [np.array([np.nan, mid[1], mid[2]]), np.array([mid[0], np.inf, mid[2]]), np.array([mid[0], mid[1], -np.inf]),
            np.array([1e30, mid[1], mid[2]]), np.array([mid[0], -1e30, mid[2]]), np.array([-0.0, -0.0, -0.0])]
    s = cell_side(eps)
    for a in range(3):
        for edge, sign in ((lo, -1.0), (hi, 1.0)):
            p = mid.copy()
            p[a] = edge[a] + sign * 2.5 * s
            hand.append(p)
    return np.vstack([uni, jit, X[:2000].astype(np.float64), np.vstack(hand)]).astype(np.float32)


def mixed_chunks(nq, nchunks, seed=78):
    """int32 [nq]: seeded chunk indices in [0, nchunks) with -1 and nchunks (both outside) mixed in"""
    rng = np.random.default_rng(seed)
    qc = rng.integers(0, nchunks, nq).astype(np.int32)
    bad = rng.choice(nq, max(nq // 50, 2), replace=False)
    qc[bad[::2]] = -1
    qc[bad[1::2]] = nchunks
    return qc


def ring26(centre, radius):
    """float32 [26,3]: centre + radius * u for the 26 directions of {-1, 0, 1}^3"""
    g = np.stack(np.meshgrid(*[np.array([-1.0, 0.0, 1.0])] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[(g != 0).any(1)]
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return (np.asarray(centre, dtype=np.float64) + float(radius) * g).astype(np.float32)


def clump_fit(X, groups, ms, em):
    """(core, labels) of a fit on X whose rows are the clumps ``groups`` (row index arrays, in file order of their
    first rows): asserted from the distance matrix - every row has ms neighbours even at em, rows of different clumps
    are further apart than any eps used - so the fit is known without running one"""
    cnt = dc.neighbour_counts(X, [em])[0]
    assert (cnt >= ms).all()
    labels = np.full(len(X), -1, dtype=np.int32)
    for k, g in enumerate(groups):
        labels[g] = k
        for h in groups[k + 1:]:
            assert dc.pair_d2(X[g], X[h]).min() > 1.5 * em * em
    assert (labels >= 0).all()
    return np.ones(len(X), dtype=np.uint8), labels


def boundary_cases():
    """[(name, X_fit, ms, e, em, (core, labels), query row)]: dc.border_case with the lone row taken out of the fit
    and used as the only query.  "two": the query sits at its boundary distance from both clumps, the smaller id
    wins.  "one-epsg": EPSG coordinates, eps0 16; the query lies outside the fit's box on all three axes and in a
    cell below the grid's origin in z."""
    out = []
    X, ms, e, em, lone, a, b = dc.border_case(True)
    keep = np.delete(np.arange(len(X)), lone)
    Xf = np.ascontiguousarray(X[keep])
    ga, gb = np.arange(len(a)), np.arange(len(a), len(a) + len(b))
    out.append(("two", Xf, ms, e, em, clump_fit(Xf, [ga, gb], ms, em), X[lone:lone + 1].copy()))
    X, ms, e, em, lone, a = dc.border_case(False, epsg=True, eps0=16.0)
    Xf = np.ascontiguousarray(X[a])
    q = X[lone:lone + 1].copy()
    tz = math.floor((float(q[0, 2]) - float(Xf[:, 2].min())) / cell_side(e))
    assert ((q[0] < Xf.min(0)) | (q[0] > Xf.max(0))).all() and tz < 0, (q, tz)      # a cell below the grid's origin
    out.append(("one-epsg", Xf, ms, e, em, clump_fit(Xf, [np.arange(len(a))], ms, em), q))
    return out


def ring_case(eps0=2.0, ms=12):
    """(X_fit, ms, eps0, (core, labels), queries at 0.98 eps0, queries at 1.02 eps0): one clump of radius 5e-4 eps0 and
    the 26 directions around its centre - inside for every row of the clump, outside for every row"""
    X, ms, e, em, lone, a = dc.border_case(False, eps0=eps0, ms=ms)
    Xf = np.ascontiguousarray(X[a])
    centre = np.array([7.13, 2.57, 4.21])
    assert np.sqrt(dc.pair_d2(Xf, centre.astype(np.float32)[None, :]).max()) <= 1e-3 * eps0
    return (Xf, ms, eps0, clump_fit(Xf, [np.arange(len(a))], ms, math.nextafter(eps0, 0.0)),
            ring26(centre, 0.98 * eps0), ring26(centre, 1.02 * eps0))


LATTICE_STEP = {"few": 0.5, "tile": 0.5, "long": 0.5, "dense": 0.125}


def lattice_queries(name):
    """the lattice's own rows, then every row moved one lattice step along x (exact in float32): pairs at d2 == eps*eps
    for queries on rows of the fit and beside them"""
    X = dc.lattice_case(name)[0]
    S64 = X.astype(np.float64) + np.array([LATTICE_STEP[name], 0.0, 0.0])
    S = S64.astype(np.float32)
    assert (S.astype(np.float64) == S64).all()
    return np.vstack([X, S])


def kept_chunks(n, kept_index, chunk_size):
    """int32 [n] for a cloud whose rows kept_index (ascending) were fitted in chunks of chunk_size: a kept row names
    the chunk it was fitted in, a dropped row the chunk of the next kept row (the last chunk behind the last one)"""
    kept = np.zeros(n, dtype=np.int64)
    kept[np.asarray(kept_index, dtype=np.int64)] = 1
    before = np.cumsum(kept) - kept
    nchunks = max(-(-len(kept_index) // int(chunk_size)), 1)
    return np.minimum(before // int(chunk_size), nchunks - 1).astype(np.int32)
