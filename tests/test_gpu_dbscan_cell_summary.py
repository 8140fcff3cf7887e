"""The cell summary of the staged route: where the cell table comes from the staged lists and no chunk overflowed,
nobody sweeps the rows for the cells' core boxes and smallest core rows (db_cellstats).  db_cellscatter stages every
cell's smallest row, db_celltab makes it cell_min, and db_core writes the rest from what its wave holds: the cell's own
bounds as the box of a dense cell, the exact box and the smallest CORE row of a sparse one.

Every case compares labels, core flags, cluster count and the clusters' first core rows of the staged route with the
global sort of the same build (which runs db_cellstats) and with the CPU oracle, and reads from the launch profile that
db_cellstats ran on the global route only.  The clouds sit on the lattice of tests/test_gpu_dbscan_chunk_union.py: the
grid's origin is a row at 0.2 and the cell side is one unit, just under."""
import numpy as np
import pytest
import torch

from oracle import dbscan as odb
from pointcloudhookup_amd import _lib, ops
from test_gpu_dbscan_chunk_union import (EPS, KEYED, LIMIT, SEVEN, STAGED, _cells_of, _chunk_rows, _cloud, _far_pairs,
                                         _in_lds)

pytestmark = pytest.mark.gpu

FEW = 24                      # db_core_k: a sparse cell below this many rows takes the query loop, else the tile loop
SIDE = 1.0 - 2.0 ** -16       # the cell side in lattice units
F32 = np.float32


# ------------------------------------------------------------------------------------------------ runs
def _fit(X, cuda, ms, chunk, mode, workspace=None):
    """a DbscanFit made on the given route (in `workspace` when given) and the names of the kernels it launched"""
    xyz = torch.from_numpy(X).to(cuda)
    try:
        ops.set_dbscan_sort_mode(mode)
        ops.set_profiling(True)
        if workspace is None:
            fit = ops.DbscanFit(xyz, EPS, ms, chunk)
        else:
            fit = ops.DbscanFit.__new__(ops.DbscanFit)
            fit.n, fit.device, fit.chunk_size, fit.workspace = len(X), cuda, chunk, workspace
            with torch.cuda.device(cuda):
                fit.labels, fit.core, fit.nclusters = ops._dbscan_call(xyz, workspace, EPS, ms, chunk, None, True)
        ran = {name for name, _, launches in ops.get_profile() if launches > 0}
    finally:
        ops.set_profiling(False)
        ops.set_dbscan_sort_mode("auto")
    return fit, ran


def _results(fit):
    return fit.labels.cpu().numpy(), fit.core.cpu().numpy(), fit.nclusters, fit.first_core_rows().cpu().numpy()


def _oracle(X, ms, chunk):
    """labels, core flags and every cluster's smallest core row, chunk by chunk (a NaN/inf chunk stays noise)"""
    n = len(X)
    labels, core, first, k = np.full(n, -1, np.int32), np.zeros(n, np.uint8), [], 0
    for lo in range(0, n, chunk):
        P = X[lo:lo + chunk]
        if not np.isfinite(P).all():
            continue
        la, ca = odb.dbscan_fit_c(P, EPS, ms)
        kk = int(la.max()) + 1
        first += [lo + int(np.flatnonzero((la == j) & (ca != 0))[0]) for j in range(kk)]
        labels[lo:lo + chunk] = np.where(la >= 0, la + k, -1)
        core[lo:lo + chunk] = ca
        k += kk
    return labels, core, k, np.asarray(first, np.int32)


def _staged(ran):
    return _in_lds(ran) and "db_cellstats" not in ran


def _keyed(ran):
    return SEVEN <= ran and "db_chunkunion" not in ran and "db_cellstats" in ran


def _check(X, cuda, ms, chunk, between=None):
    """staged route == global sort == CPU oracle; db_cellstats ran on the global route only.  between(fit): called
    on the staged fit while it is the thread's live one, its result on the global fit is compared too.  Returns the
    staged results"""
    fit, ran = _fit(X, cuda, ms, chunk, "chunk")
    a = _results(fit) + ((between(fit),) if between else ())
    fit, ranb = _fit(X, cuda, ms, chunk, "global")
    b = _results(fit) + ((between(fit),) if between else ())
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    for u, v in zip(a, _oracle(X, ms, chunk)):
        np.testing.assert_array_equal(u, v)
    assert _staged(ran), sorted(ran)
    assert _keyed(ranb), sorted(ranb)
    return a


# ------------------------------------------------------------------------------------------------ clouds
def _cell_rows(rng, cell, rows, lo=0.05, hi=0.9):
    """rows points inside lattice cell `cell`"""
    return 0.2 + np.asarray(cell, np.float64) + rng.uniform(lo, hi, (rows, 3))


def _border_first(ms, sparse_rows):
    """One chunk, two clusters.  Row 0 is the grid's origin in cell (0,0,0); the other sparse_rows - 1 rows of that
    cell sit at its far side in x, within eps of the dense cell (2,0,0) and so core - row 0 is beyond eps of that cell
    and has only its cell mates: a border row of that cluster, whose core rows come last.  Between them the rows of a
    dense cell far away: the cluster with the smaller first core row"""
    rng = np.random.default_rng(7)
    far = np.array([1.1, 0.2, 0.2]) + rng.uniform(0.0, 0.05, (sparse_rows - 1, 3))
    dense = _cell_rows(rng, (2, 0, 0), ms + 2, 0.05, 0.15)
    other = _cell_rows(rng, (12, 0, 0), ms + 2)
    return np.vstack([[[0.2, 0.2, 0.2]], other, far, dense]).astype(F32)


def _boundary_cloud(ms):
    """cells of exactly ms and ms - 1 rows side by side along x; a cell of ms - 1 rows on its own (noise) and one of ms
    (a cluster); and a cell of ms - 1 rows spread along x beside a single row two cells on that reaches only some of
    them: a cell with core and non-core rows.  Shuffled; the origin is a row of cell (0,0,0)"""
    rng = np.random.default_rng(11 + ms)
    parts = [_cell_rows(rng, (i, 0, 0), (ms if i % 2 == 0 else ms - 1) - (i == 0)) for i in range(6)]
    parts += [_cell_rows(rng, (10, 0, 0), ms - 1), _cell_rows(rng, (14, 0, 0), ms)]
    spread = np.full((ms - 1, 3), 0.7)
    spread[:, 0] = 18.25 + 0.85 * np.arange(ms - 1) / (ms - 2)
    parts += [spread + rng.uniform(0.0, 1e-3, spread.shape), [[20.6, 0.7, 0.7]]]
    X = np.vstack(parts)
    rng.shuffle(X)
    return np.vstack([X, [[0.2, 0.2, 0.2]]]).astype(F32)


def _reach(v, d):
    """the float32 coordinates furthest from v in direction d (+1 / -1) still within eps of it, and the next one on"""
    def within(t):
        return (np.float64(t) - np.float64(v)) ** 2 <= EPS * EPS
    away = F32(d * np.inf)
    t = F32(np.float64(v) + d * EPS)
    while within(t):
        t = np.nextafter(t, away)
    while not within(t):
        t = np.nextafter(t, -away)
    return t, np.nextafter(t, away)


BOUND_MS = 5


def _bound_group(axis, v, base, dirs, step=0.05):
    """BOUND_MS rows that share the coordinate v on `axis` - a dense cell whose rows all lie on one plane - in a line
    from `base` along the next axis; for every direction of dirs two rows in line with the first of them along `axis`:
    one at the last float32 within eps of it, one at the next float32.  Returns the rows and the indices of the first
    row, of the rows that border it and of the rows just beyond"""
    R = np.array(base, F32)
    R[axis] = v
    rows = [R.copy() for _ in range(BOUND_MS)]
    for j in range(1, BOUND_MS):
        rows[j][(axis + 1) % 3] += F32(step * j)
    inside, beyond = [], []
    for d in dirs:
        for t, into in zip(_reach(v, d), (inside, beyond)):
            P = R.copy()
            P[axis] = t
            into.append(len(rows))
            rows.append(P)
    return np.array(rows, F32), 0, inside, beyond


def _grid_cells(X):
    """the cell of every row as the library computes it: floor((x - origin) / side) in float64"""
    side = EPS / 1.7320508075688772 * SIDE
    return np.floor((X.astype(np.float64) - X.min(0).astype(np.float64)) * (1.0 / side)).astype(np.int64)


def _bounds_cloud():
    """dense cells with rows exactly on the grid's origin, on cell faces (0.2 + 3 * side rounded to float32 and the
    float32 below it, on every axis) and at the far corner of the grid's last cell, each with rows at eps and just
    beyond.  Returns the cloud and, per group, (first row, bordering rows, rows beyond) as indices into it"""
    face = F32(0.2 + 3 * SIDE)
    groups = []
    for a in range(3):
        for i, v in enumerate((face, np.nextafter(face, F32(-np.inf)))):
            base = np.full(3, 0.5)
            base[(a + 1) % 3] += 8.0 * (1 + 2 * a + i)    # every group on its own, eight cells from the next
            groups.append(_bound_group(a, v, base, (-1, 1)))
    origin = _bound_group(0, F32(0.2), (0.2, 0.2, 0.2), (1,))
    far = _bound_group(0, F32(60.9), (60.9, 60.9, 60.9), (-1,), step=-0.05)
    X, index = [], []
    for rows, first, inside, beyond in [origin] + groups + [far]:
        at = sum(len(x) for x in X)
        X.append(rows)
        index.append((at + first, [at + i for i in inside], [at + i for i in beyond]))
    return np.vstack(X).astype(F32), index


# ------------------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize("ms,sparse_rows", [(4, 3), (80, 30)])
def test_numbering_through_a_sparse_cell(cuda, oracle_clib, ms, sparse_rows):
    """the smallest row of a sparse cell is a border row, below every core row of the other cluster: with the staged
    smallest row of ALL the cell's rows left in place the two cluster ids would swap.  Twice, in two chunks; both
    sparse paths of db_core"""
    assert (sparse_rows < FEW) == (ms == 4) and sparse_rows < ms
    P = _border_first(ms, sparse_rows)
    X = np.vstack([P, P])
    la, ca, ka, first = _check(X, cuda, ms, len(P))
    n0 = 1 + ms + 2                                       # the first row of the sparse cell's core rows
    for lo, k0 in ((0, 0), (len(P), 2)):
        assert not ca[lo] and ca[lo + 1:lo + len(P)].all()
        assert la[lo] == k0 + 1 and la[lo + 1] == k0 and la[lo + n0] == k0 + 1
        assert list(first[k0:k0 + 2]) == [lo + 1, lo + n0]
    assert ka == 4


def test_numbering_through_a_dense_cell(cuda, oracle_clib):
    """every cell dense, rows shuffled, three chunks: every cluster's first core row is the smallest row of some dense
    cell, wherever the scatter put it among the cell's sorted rows"""
    chunk, ms = 2500, 5
    X = _cloud(21, chunk, [40, 25, 33], last_rows=1700, grid=(12, 12, 6))
    X[1:ms] = (0.2 + np.random.default_rng(22).uniform(0.0, 0.3, (ms - 1, 3))).astype(F32)    # the origin's cell: dense too
    c = _cells_of(X)
    for lo in range(0, len(X), chunk):
        _, cnt = np.unique(c[lo:lo + chunk], axis=0, return_counts=True)
        assert cnt.min() >= ms
    la, ca, ka, first = _check(X, cuda, ms, chunk)
    assert ca.all() and ka > 6 and (first >= chunk).sum() > 3 and (np.diff(first) > 0).all()


@pytest.mark.parametrize("ms", [4, 80])
def test_the_dense_boundary(cuda, oracle_clib, ms):
    """cells of min_samples rows (dense: the cell's bounds, the staged row) beside cells of min_samples - 1 (sparse: the
    exact values; the query loop for 3 rows, the tile loop for 79), with and without core rows"""
    assert (ms - 1 < FEW) == (ms == 4)
    X = _boundary_cloud(ms)
    c = _cells_of(X)
    _, inv, cnt = np.unique(c, axis=0, return_inverse=True, return_counts=True)
    assert sorted(cnt) == sorted([ms, ms - 1] * 3 + [ms - 1, ms, ms - 1, 1])
    la, ca, ka, first = _check(X, cuda, ms, len(X))
    ncore = np.bincount(inv.reshape(-1), weights=ca)
    assert ka == 3 and ((ncore > 0) & (ncore < cnt)).any() and ((ncore == 0) & (cnt == ms - 1)).any()
    assert ((ncore == cnt) & (cnt == ms - 1)).any() and (la == -1).sum() >= ms - 1


def test_rows_on_the_bounds_of_dense_cells(cuda, oracle_clib):
    """a dense cell's box is the cell's bounds, a little widened: rows on the origin, on cell faces and in the last
    cell's far corner lie inside it, so a row at the last float32 within eps of one is its border row, the next
    float32 is noise - as rows of the fit and as queries of DbscanFit.assign"""
    X, index = _bounds_cloud()
    c = _grid_cells(X)
    assert (c.min(0) == 0).all() and (c[index[-1][0]] == c.max(0)).all() and (X[index[0][0]] == F32(0.2)).all()
    on = [c[index[g][0]][(g - 1) // 2] for g in range(1, 7)]
    assert sorted(set(on)) == [2, 3]                      # the face values fall on either side of the face

    def queries(fit):
        return fit.assign(torch.from_numpy(X).to(cuda)).cpu().numpy()

    la, ca, ka, first, asg = _check(X, cuda, BOUND_MS, len(X), between=queries)
    np.testing.assert_array_equal(asg, la)
    assert ka == len(index)
    for row, inside, beyond in index:
        assert ca[row] and la[row] >= 0
        assert len(inside) > 0 and (la[inside] == la[row]).all() and not ca[inside].any()
        assert (la[beyond] == -1).all()


@pytest.mark.parametrize("scale,clusters", [(1.0 - 1e-4, 3), (1.0 + 1e-4, 6)])
def test_far_corners(cuda, oracle_clib, scale, clusters):
    """cells whose core points mass in the corners that face away from each other: the true core boxes are far
    apart, the cells' bounds are not, and exactly one pair (or none) is within eps"""
    X = _far_pairs(scale)
    la, ca, ka, first = _check(X, cuda, 5, len(X))
    assert ka == clusters and ca[:-1].all()


@pytest.mark.parametrize("last_rows", [3, 1])
def test_degenerate_chunks_side_by_side(cuda, oracle_clib, last_rows):
    """an ordinary chunk, a NaN chunk, a chunk that is one dense cell, an ordinary chunk and a last chunk of one sparse
    cell: three rows, or one"""
    chunk, ms = 1000, 5
    rng = np.random.default_rng(31)
    parts = [_chunk_rows(rng, 300, chunk, (12, 12, 6)),
             _chunk_rows(rng, 200, chunk, (12, 12, 6)),   # gets a NaN below
             _chunk_rows(rng, 1, chunk, (12, 12, 6)),
             _chunk_rows(rng, 350, chunk, (12, 12, 6)),
             _chunk_rows(rng, 1, last_rows, (12, 12, 6))]
    X = np.vstack(parts).astype(F32)
    X[5] = 0.2
    X[chunk + 123, 2] = np.nan
    la, ca, ka, first = _check(X, cuda, ms, chunk)
    assert (la[chunk:2 * chunk] == -1).all() and not ca[chunk:2 * chunk].any()
    assert ca[2 * chunk:3 * chunk].all() and len(np.unique(la[2 * chunk:3 * chunk])) == 1
    assert 2 * chunk in first                             # the one-cell chunk: its rows stay in place
    assert (la[4 * chunk:] == -1).all() and not ca[4 * chunk:].any()
    assert ca[:chunk].any() and ca[3 * chunk:4 * chunk].any()


def test_staged_then_fallback_then_staged_on_one_workspace(cuda, oracle_clib):
    """three fits of the same size in one workspace: staged, a chunk of 1 025 cells (db_cellstats and the seven
    kernels), staged again with other cells.  A staged smallest row or a cell_min left over would show"""
    chunk, last, ms = 4099, 1500, 5
    clouds = [_cloud(41, chunk, [400, 900, 60, 200], last_rows=last),
              _cloud(42, chunk, [400, LIMIT + 1, 7, 200], last_rows=last),
              _cloud(43, chunk, [30, 500, 1000, 1], last_rows=last, origin_row=chunk)]
    n = len(clouds[0])
    with torch.cuda.device(cuda):
        ws = torch.empty(int(_lib.lib().pch_dbscan_ws_bytes(n)) + 256, dtype=torch.uint8, device=cuda)
    got = []
    for X in clouds:                                      # back to back, nothing in between but the read-out
        fit, ran = _fit(X, cuda, ms, chunk, "chunk", workspace=ws)
        got.append(_results(fit) + (ran,))
    for X, res, keyed in zip(clouds, got, (False, True, False)):
        assert (_keyed(res[4]) and KEYED <= res[4]) if keyed else _staged(res[4]), sorted(res[4])
        fit, ranb = _fit(X, cuda, ms, chunk, "global")
        for u, v, w in zip(res, _results(fit), _oracle(X, ms, chunk)):
            np.testing.assert_array_equal(u, v)
            np.testing.assert_array_equal(u, w)
        assert res[2] > 0 and _keyed(ranb)


def test_strip_pairs_of_a_staged_fit(cuda, oracle_clib):
    """pch_dbscan_strip_pairs_i32 rejects cells by the x range of cell_box: the same pairs from the cells' bounds as
    from the exact boxes"""
    X = _cloud(51, 3000, [300], grid=(16, 8, 4))

    def pairs(fit):
        p, count = fit.strip_pairs(5.0, 9.5, cap=4096)
        k = int(count.item())
        assert 0 < k <= 4096
        p = p[:k].cpu().numpy()
        return p[np.lexsort((p[:, 1], p[:, 0]))]

    la, ca, ka, first, p = _check(X, cuda, 12, len(X), between=pairs)
    x = X[p[:, 0], 0]
    assert ((x >= 5.0) & (x < 9.5)).all() and (ca[p[:, 0]] != 0).all()
    np.testing.assert_array_equal(la[p[:, 0]], p[:, 1])
    c = _cells_of(X)
    strip = (ca != 0) & (X[:, 0] >= F32(5.0)) & (X[:, 0] < F32(9.5))
    assert len(p) == len(np.unique(c[strip], axis=0))
