"""db_chunkunion: on the staged route (every chunk holds at most 1 024 cells) one workgroup per chunk unites the chunk's
core cells in LDS and leaves root, comp_min and the clusters' first-row bits - the work of db_cellfin, db_union_pairs,
db_union0, db_flatten, db_union1, db_compmin and db_mark, which still run on every other route.

Every case compares labels, core flags and cluster count of the chunk-local route with the global sort's (which runs
the seven kernels) and with the CPU oracle, and reads from the library's launch profile which kernels ran.  The inputs
sit on a lattice of cells: the grid's origin is a row at 0.2, the cell side is one lattice unit (just under), so cell
(i, j, k) covers [0.2 + i, 1.2 + i) x ... and every chunk holds an exact number of cells."""
import math

import numpy as np
import pytest
import torch

from oracle import dbscan as odb
from pointcloudhookup_amd import ops, synth

pytestmark = pytest.mark.gpu

EPS = math.sqrt(3.0)          # cell side eps/sqrt(3) * (1 - 2^-16): one lattice unit, just under
LIMIT = 1024                  # cells a chunk may hold on the staged route (CT_CELLS)
GRID = (48, 48, 24)

STAGED = {"db_cellscatter", "db_chunkcells", "db_celltab"}
KEYED = {"db_heads", "db_cells"}
SEVEN = {"db_union_pairs", "db_union0", "db_union1", "db_flatten", "db_compmin", "db_mark", "db_cellfin"}


# ------------------------------------------------------------------------------------------------ clouds
def _chunk_rows(rng, ncells, rows, grid=GRID):
    """rows points in exactly ncells distinct cells of the grid (every cell holds at least one), jittered inside"""
    flat = rng.choice(int(np.prod(grid)), ncells, replace=False)
    cells = np.stack(np.unravel_index(flat, grid), 1).astype(np.float64)
    idx = np.concatenate([np.arange(ncells), rng.integers(0, ncells, rows - ncells)])
    rng.shuffle(idx)
    return cells[idx] + 0.5 + rng.uniform(-0.3, 0.3, (rows, 3))


def _cloud(seed, chunk, cells_per_chunk, last_rows=None, origin_row=0, grid=GRID):
    """one chunk per entry of cells_per_chunk (the last one of last_rows rows when given); row origin_row is the
    grid's origin - and may add a cell to that row's chunk"""
    rng = np.random.default_rng(seed)
    parts = []
    for i, nc in enumerate(cells_per_chunk):
        rows = last_rows if (last_rows is not None and i == len(cells_per_chunk) - 1) else chunk
        parts.append(_chunk_rows(rng, nc, rows, grid))
    X = np.vstack(parts).astype(np.float32)
    X[origin_row] = 0.2
    return X


def _cells_of(X):
    """lattice cell of every row"""
    return np.floor((X.astype(np.float64) - 0.2) / (1.0 - 2.0 ** -16) + 1e-9).astype(np.int64)


def _snake_cells(n=LIMIT, run=16, rows=8):
    """n cells on one path: runs of `run` cells along x at y = 0, 2, 4, ..., joined by one cell at alternating ends,
    layers at z = 0, 2, ... joined by one cell.  Cells that do not follow each other on the path are two cells apart
    or meet at a turn, so with points within 0.1 of the cell centres only neighbours on the path link"""
    path, x, y, z, dx, dy = [], 0, 0, 0, 1, 1
    while len(path) < n:
        for r in range(rows):
            for _ in range(run):
                path.append((x, y, z))
                x += dx
            x -= dx
            dx = -dx
            if r < rows - 1:
                path.append((x, y + dy, z))
                y += 2 * dy
        dy = -dy
        path.append((x, y, z + 1))
        z += 2
    return np.array(path[:n], dtype=np.float64)


def _snake(cut=()):
    """four rows in every cell of the snake (min_samples 4: every cell is core), in shuffled order; cut: positions on
    the path whose cell is left out (in the middle of a run: the path's two sides are then 1.8 apart at least)"""
    cells = _snake_cells()
    keep = np.ones(len(cells), bool)
    keep[list(cut)] = False
    cells = cells[keep]
    rng = np.random.default_rng(31)
    idx = np.repeat(np.arange(len(cells)), 4)
    rng.shuffle(idx)
    X = (cells[idx] + 0.7 + rng.uniform(-0.1, 0.1, (len(idx), 3))).astype(np.float32)
    X[np.flatnonzero(idx == 0)[0]] = 0.2                  # the origin, in the path's first cell (0, 0, 0)
    return X, len(cells)


def _far_pair(offset, pa, toward, scale, mass=70):
    """cells (0,0,0) and `offset` with mass core points each, massed in the corners that face away from each other,
    plus one point each: pa and the point at distance EPS * scale from it in direction `toward`"""
    rng = np.random.default_rng(41)
    off = np.asarray(offset, np.float64)
    A = 0.2 + rng.uniform(0.01, 0.05, (mass, 3))
    B = 0.2 + off + rng.uniform(0.90, 0.95, (mass, 3))
    u = np.asarray(toward, np.float64)
    pa = np.asarray(pa, np.float64)
    pb = pa + u / np.linalg.norm(u) * EPS * scale
    return np.vstack([A, pa[None], B, pb[None]])


def _far_pairs(scale):
    """three such pairs, 10 cells apart in x: face neighbours (1,0,0) and two pairs that meet only through an outer
    neighbour row, (2,1,1) and (0,2,2).  Rows in shuffled order"""
    parts = [_far_pair((1, 0, 0), (0.25, 0.25, 0.45), (1.25, 0.8, 0.6), scale),
             _far_pair((2, 1, 1), (1.15, 1.15, 1.15), (1.6, 0.5, 0.43), scale) + (10.0, 0.0, 0.0),
             _far_pair((0, 2, 2), (0.7, 1.15, 1.15), (0.0, 1.0, 1.0), scale) + (20.0, 0.0, 0.0)]
    X = np.vstack(parts)
    np.random.default_rng(42).shuffle(X)
    X = np.vstack([X, [[0.2, 0.2, 0.2]]]).astype(np.float32)
    for base, off in zip((0, 10, 20), ((1, 0, 0), (2, 1, 1), (0, 2, 2))):   # the construction holds in float32
        c = _cells_of(X)
        a = X[(c == (base, 0, 0)).all(1)].astype(np.float64)
        b = X[(c == (base + off[0], off[1], off[2])).all(1)].astype(np.float64)
        assert len(a) >= 71 and len(b) == 71
        d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(2)
        assert (d2 <= 3.0).sum() == (1 if scale < 1 else 0)
    return X


def _bridge_block():
    """min_samples 6.  Two core cells, six points on a line each, (0,0,0) and (4,0,0); between them one point p in
    cell (2,0,0) that is within eps of two points of either line: 5 neighbours, not core, so the lines stay two
    clusters although p borders both.  Cell (0,1,0) holds two points: e1 within eps of the whole first line (core),
    e2 beyond eps of everything but e1 (not core): a cell with 0 < core points < points"""
    line = np.linspace(0.25, 1.15, 6)
    D1 = np.stack([line, np.full(6, 0.3), np.full(6, 0.3)], 1)
    D2 = D1 + (4.0, 0.0, 0.0)
    return np.vstack([D1, D2, [[2.7, 0.3, 0.3]], [[0.7, 1.25, 0.3]], [[0.7, 2.15, 1.15]]])


# ------------------------------------------------------------------------------------------------ runs
def _run(X, cuda, ms, chunk, mode, profile=False):
    """labels, core flags, cluster count and - with profile - the names of the kernels that were launched"""
    ran = None
    try:
        ops.set_dbscan_sort_mode(mode)
        if profile:
            ops.set_profiling(True)
        lab, core, k = ops.dbscan(torch.from_numpy(X).to(cuda), EPS, ms, chunk, want_core=True)
        if profile:
            ran = {name for name, _, launches in ops.get_profile() if launches > 0}
    finally:
        if profile:
            ops.set_profiling(False)
        ops.set_dbscan_sort_mode("auto")
    return lab.cpu().numpy(), core.cpu().numpy(), k, ran


def _in_lds(ran):
    return STAGED <= ran and not (KEYED & ran) and "db_chunkunion" in ran and not (SEVEN & ran)


def _check(X, cuda, ms, chunk, lds=True):
    """chunk-local route == global sort == CPU oracle, and the kernels that united the cells: db_chunkunion (lds) or
    the seven; returns the chunk-local results"""
    la, ca, ka, ran = _run(X, cuda, ms, chunk, "chunk", profile=True)
    lb, cb, kb, ranb = _run(X, cuda, ms, chunk, "global", profile=True)
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(ca, cb)
    assert ka == kb
    np.testing.assert_array_equal(la, odb.dbscan_chunked(X, EPS, ms, chunk, fit="c"))
    assert SEVEN <= ranb and "db_chunkunion" not in ranb
    assert _in_lds(ran) if lds else (SEVEN <= ran and "db_chunkunion" not in ran)
    return la, ca, ka


# ------------------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize("cut,clusters", [((), 1), ((200, 700), 3)])
def test_snake_of_1024_cells(cuda, oracle_clib, cut, clusters):
    """one chunk whose cells are a single path with runs along x, y and z: every cell hooks under its predecessor, so
    the forest starts as chains as long as the runs; whole it is the limit of 1 024 cells.  Cut twice: three clusters"""
    X, ncells = _snake(cut)
    assert ncells == LIMIT - len(cut) and len(np.unique(_cells_of(X), axis=0)) == ncells
    la, ca, ka = _check(X, cuda, 4, len(X))
    assert ka == clusters and ca.all()
    assert (np.bincount(la) > 0).all()


@pytest.mark.parametrize("scale,clusters", [(1.0 - 1e-4, 3), (1.0 + 1e-4, 6)])
def test_links_only_the_exhaustive_search_finds(cuda, oracle_clib, scale, clusters):
    """pairs of cells with 71 core points each of which exactly one pair is within eps (or none: just outside) - a
    face pair, a (2,1,1) pair and a (0,2,2) pair; the first points of a cell say nothing"""
    X = _far_pairs(scale)
    la, ca, ka = _check(X, cuda, 5, len(X))
    assert ka == clusters and ca[:-1].all()


def test_links_through_edges_corners_and_outer_rows(cuda, oracle_clib):
    """a sparse random lattice with min_samples 3: most links are no face links"""
    chunk = 3001
    X = _cloud(51, chunk, [500, 900, 300], last_rows=1400, grid=(24, 24, 12))
    la, ca, ka = _check(X, cuda, 3, chunk)
    assert ka > 10 and (la == -1).any()
    c = _cells_of(X[:chunk])                              # core cells that link although they share no face
    core_cells = np.unique(c[ca[:chunk] != 0], axis=0)
    have = {tuple(v) for v in core_cells}
    lab_of = {tuple(v): la[:chunk][(c == v).all(1) & (ca[:chunk] != 0)][0] for v in core_cells}
    faces = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)]
    lonely = [v for v in have if not any((v[0] + d[0], v[1] + d[1], v[2] + d[2]) in have for d in faces)]
    sizes = np.bincount(la[la >= 0])
    assert any(sizes[lab_of[v]] > (la[:chunk][(c == v).all(1)] == lab_of[v]).sum() for v in lonely)


def test_partly_core_and_non_core_cells(cuda, oracle_clib):
    """cells with core and non-core points side by side, and cells without a core point between core cells: they
    border clusters and never join them"""
    rng = np.random.default_rng(61)
    block = _bridge_block()
    chunk = 2 * len(block) + 3000
    rand = _chunk_rows(rng, 900, chunk - len(block), grid=(24, 24, 12)) + (0.0, 0.0, 6.0)
    rand2 = _chunk_rows(rng, 500, chunk - len(block), grid=(24, 24, 12)) + (0.0, 0.0, 6.0)
    X = np.vstack([block, rand, rand2, block]).astype(np.float32)
    X = np.vstack([X, [[0.2, 0.2, 0.2]] * 7]).astype(np.float32)     # the origin (seven rows: a core cell of its own)
    la, ca, ka = _check(X, cuda, 6, chunk)
    assert ca[:12].all() and not ca[12] and ca[13] and not ca[14]
    assert la[0] != la[6] and la[12] == min(la[0], la[6]) and la[13] == la[0] and la[14] == la[0]
    c = _cells_of(X[:chunk])
    _, inv = np.unique(c, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    size, ncore = np.bincount(inv), np.bincount(inv, weights=ca[:chunk])
    assert ((ncore > 0) & (ncore < size)).sum() > 20 and (ncore == 0).sum() > 20 and (ncore == size).sum() > 20


def test_chunks_are_independent(cuda, oracle_clib):
    """the same rows in two consecutive chunks of 4 099 and their first 1 777 once more as a ragged last chunk: the
    same clusters again, numbered on, never one cluster across a chunk boundary"""
    chunk, last = 4099, 1777
    P = _cloud(71, chunk, [900], grid=(24, 24, 12))
    X = np.vstack([P, P, P[:last]])
    la, ca, ka = _check(X, cuda, 4, chunk)
    a, b = la[:chunk], la[chunk:2 * chunk]
    k1 = a.max() + 1
    assert k1 > 5 and (a == -1).any()
    np.testing.assert_array_equal(b, np.where(a >= 0, a + k1, -1))
    np.testing.assert_array_equal(ca[:chunk], ca[chunk:2 * chunk])
    assert la[2 * chunk:].max() == ka - 1 and la[2 * chunk:][la[2 * chunk:] >= 0].min() == 2 * k1


def test_degenerate_chunks_side_by_side(cuda, oracle_clib):
    """a NaN chunk (one cell, never core), a chunk of one cell, of two cells, a chunk without a core cell (1 000 cells
    three apart) and ordinary chunks around them"""
    chunk = 1000
    rng = np.random.default_rng(81)
    lone = np.stack(np.unravel_index(np.arange(chunk), (10, 10, 10)), 1) * 3.0 + 0.7
    parts = [_chunk_rows(rng, 300, chunk, (12, 12, 6)),
             _chunk_rows(rng, 200, chunk, (12, 12, 6)),   # gets an inf below
             _chunk_rows(rng, 1, chunk, (12, 12, 6)),
             _chunk_rows(rng, 2, chunk, (12, 12, 6)),
             lone,
             _chunk_rows(rng, 350, chunk, (12, 12, 6))[:613]]
    X = np.vstack(parts).astype(np.float32)
    X[4 * chunk] = 0.2                                    # the origin: cell (0,0,0) of the chunk without a core cell
    X[chunk + 77, 1] = np.inf
    la, ca, ka = _check(X, cuda, 5, chunk)
    assert (la[chunk:2 * chunk] == -1).all() and not ca[chunk:2 * chunk].any()
    assert ca[2 * chunk:4 * chunk].all() and len(np.unique(la[2 * chunk:3 * chunk])) == 1
    assert len(np.unique(la[3 * chunk:4 * chunk])) in (1, 2)
    assert (la[4 * chunk:5 * chunk] == -1).all() and not ca[4 * chunk:5 * chunk].any()
    assert ca[:chunk].any() and ca[5 * chunk:].any()


def test_a_chunk_of_1025_cells_takes_the_seven_kernels(cuda, oracle_clib):
    """one chunk beyond the limit among small ones: the table is read off the keys and the global kernels unite"""
    chunk = 4099
    X = _cloud(91, chunk, [300, 1, LIMIT + 1, 77, LIMIT, 500], last_rows=2222)
    la, ca, ka, ran = _run(X, cuda, 5, chunk, "chunk", profile=True)
    assert STAGED <= ran and KEYED <= ran and "db_chunksort" in ran
    la2, _, ka2 = _check(X, cuda, 5, chunk, lds=False)
    np.testing.assert_array_equal(la, la2)
    assert ka == ka2 and ka > 5


def test_staged_then_fallback_then_staged_on_one_workspace(cuda, oracle_clib):
    """three calls of the same sizes on the same workspace: db_chunkunion, the seven kernels (chunk 1 overflows),
    db_chunkunion again with other cell counts.  A root, a first-row bit or a forest left over from the call before
    would show"""
    chunk, last = 4099, 1500
    clouds = [_cloud(92, chunk, [400, 900, 60, 200], last_rows=last),
              _cloud(93, chunk, [400, LIMIT + 200, 7, 200], last_rows=last),
              _cloud(94, chunk, [30, 500, 1000, 1], last_rows=last, origin_row=chunk)]
    got = [_run(X, cuda, 5, chunk, "chunk", profile=True) for X in clouds]      # back to back, nothing in between
    for X, (la, ca, ka, ran), keyed in zip(clouds, got, (False, True, False)):
        assert (SEVEN <= ran and "db_chunkunion" not in ran and KEYED <= ran) if keyed else _in_lds(ran)
        lb, cb, kb, _ = _run(X, cuda, 5, chunk, "global")
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(ca, cb)
        assert ka == kb and ka > 0
        np.testing.assert_array_equal(la, odb.dbscan_chunked(X, EPS, 5, chunk, fit="c"))


def test_assign_continues_a_fit_united_in_lds(cuda, oracle_clib):
    """DbscanFit.assign reads the cell table, cell_box and the cells' labels of the fit: the same answers on a fit
    whose cells db_chunkunion united as on a global-sort fit, and so do first_core_rows (the bitmap)"""
    chunk = 4099
    X = _cloud(95, chunk, [200, 37, 1000, 90], last_rows=1777)
    rng = np.random.default_rng(96)
    pick = rng.integers(0, len(X), 3000)
    Q = (X[pick] + rng.uniform(-0.8, 0.8, (len(pick), 3))).astype(np.float32)
    qc = rng.integers(0, 4, len(pick)).astype(np.int32)
    qc[::2] = (pick[::2] // chunk).astype(np.int32)       # half of them against the chunk they were drawn from
    out, ran = {}, {}
    for mode in ("chunk", "global"):
        try:
            ops.set_dbscan_sort_mode(mode)
            ops.set_profiling(True)
            fit = ops.DbscanFit(torch.from_numpy(X).to(cuda), EPS, 5, chunk)
            ran[mode] = {name for name, _, launches in ops.get_profile() if launches > 0}
        finally:
            ops.set_profiling(False)
            ops.set_dbscan_sort_mode("auto")
        got = fit.assign(torch.from_numpy(Q).to(cuda), chunk=torch.from_numpy(qc).to(cuda)).cpu().numpy()
        first = fit.first_core_rows().cpu().numpy()
        out[mode] = (fit.labels.cpu().numpy(), fit.core.cpu().numpy(), fit.nclusters, got, first)
    for a, b in zip(out["chunk"], out["global"]):
        np.testing.assert_array_equal(a, b)
    assert _in_lds(ran["chunk"])
    assert SEVEN <= ran["global"] and "db_chunkunion" not in ran["global"]
    np.testing.assert_array_equal(out["chunk"][0], odb.dbscan_chunked(X, EPS, 5, chunk, fit="c"))
    assert (out["chunk"][3] >= 0).any() and (out["chunk"][3] == -1).any()


def test_tower_clusters_with_the_chunk_route_forced(cuda):
    """the fused entry point (ground filter, DBSCAN, grouping) on a small corridor: labels, perm, offsets and stats
    are the global route's, bit for bit"""
    raw = torch.from_numpy(synth.corridor_numpy(120000, seed=synth.SEED0, kind="corridor", offset=True,
                                                towers=3).astype(np.float32)).to(cuda)
    out, ran = {}, {}
    for mode in ("chunk", "global"):
        try:
            ops.set_dbscan_sort_mode(mode)
            ops.set_profiling(True)
            g, labels, k, perm, offsets, stats = ops.tower_clusters(raw, 8.0, 80, 5000)
            ran[mode] = {name for name, _, launches in ops.get_profile() if launches > 0}
        finally:
            ops.set_profiling(False)
            ops.set_dbscan_sort_mode("auto")
        out[mode] = (k, g["count"], labels.cpu().numpy(), perm.cpu().numpy(), offsets.cpu().numpy(),
                     stats.cpu().numpy().view(np.uint32))
    assert out["chunk"][0] == out["global"][0] > 0 and out["chunk"][1] == out["global"][1]
    for a, b in zip(out["chunk"][2:], out["global"][2:]):
        np.testing.assert_array_equal(a, b)
    assert "db_chunkunion" in ran["chunk"] and not (SEVEN & ran["chunk"])
    assert SEVEN <= ran["global"] and "db_chunkunion" not in ran["global"]
