"""The cell table of the chunk-local route.  db_cellscatter stages every chunk's sorted cell list (keys, first rows,
cell count) instead of a key per row; db_chunkcells scans the counts, and db_celltab writes the table from the staged
lists - or, when a chunk overflowed the counting table, the keys of the other chunks, and the table is read off the keys
as before (db_heads / db_cells).  Runs with more chunks than db_chunkcells' one workgroup scans keep the keys.

Every case compares labels, core flags and cluster count of the chunk-local route with the global sort's and with the
CPU oracle, and reads from the library's launch profile which route ran.  The inputs sit on a lattice of cells (one
lattice unit = one grid cell), so every chunk holds an exact number of cells."""
import math

import numpy as np
import pytest
import torch

from oracle import dbscan as odb
from pointcloudhookup_amd import ops

pytestmark = pytest.mark.gpu

EPS = math.sqrt(3.0)          # cell side eps/sqrt(3) * (1 - 2^-16): one lattice unit, just under
LIMIT = 1024                  # cells a chunk may hold in the counting table (CT_CELLS)
MAX_CHUNKS = 16384            # chunks a run may have on the staged route (DB_TABLE_MAX_CHUNKS)
GRID = (48, 48, 24)

STAGED = {"db_cellscatter", "db_chunkcells", "db_celltab"}
KEYED = {"db_heads", "db_cells"}


def _chunk_rows(rng, ncells, rows, grid=GRID):
    """rows points in exactly ncells distinct cells of the grid (every cell holds at least one), jittered inside"""
    flat = rng.choice(int(np.prod(grid)), ncells, replace=False)
    cells = np.stack(np.unravel_index(flat, grid), 1).astype(np.float64)
    idx = np.concatenate([np.arange(ncells), rng.integers(0, ncells, rows - ncells)])
    rng.shuffle(idx)
    return cells[idx] + 0.5 + rng.uniform(-0.3, 0.3, (rows, 3))


def _cloud(seed, chunk, cells_per_chunk, last_rows=None, origin_row=0):
    """one chunk per entry of cells_per_chunk (the last one of last_rows rows when given).  Row origin_row is the
    grid's origin, which makes a lattice cell exactly one grid cell - and may add a cell to that row's chunk"""
    rng = np.random.default_rng(seed)
    parts = []
    for i, nc in enumerate(cells_per_chunk):
        rows = last_rows if (last_rows is not None and i == len(cells_per_chunk) - 1) else chunk
        parts.append(_chunk_rows(rng, nc, rows))
    X = np.vstack(parts).astype(np.float32)
    X[origin_row] = 0.2
    return X


def _crowd(seed, rows, grid=(7, 6, 4)):
    """rows points spread over a small block of cells: neighbours are frequent even inside chunks of a few rows"""
    rng = np.random.default_rng(seed)
    X = (rng.integers(0, grid, (rows, 3)) + 0.5 + rng.uniform(-0.3, 0.3, (rows, 3))).astype(np.float32)
    X[0] = 0.2
    return X


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


def _check(X, cuda, ms, chunk):
    """chunk-local route == global sort == CPU oracle; returns the chunk-local results and what it launched"""
    la, ca, ka, ran = _run(X, cuda, ms, chunk, "chunk", profile=True)
    lb, cb, kb, _ = _run(X, cuda, ms, chunk, "global")
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(ca, cb)
    assert ka == kb
    np.testing.assert_array_equal(la, odb.dbscan_chunked(X, EPS, ms, chunk, fit="c"))
    return la, ca, ka, ran


def test_staged_route_with_awkward_sizes(cuda, oracle_clib):
    """five chunks of 4 099 rows (no multiple of 8: threads of db_celltab and its 2 048-row tiles straddle chunks), a
    ragged last chunk, every chunk below the table limit: the table comes from the staged lists, no key is read"""
    chunk = 4099
    X = _cloud(11, chunk, [200, 37, 1000, 513, 90], last_rows=1777)
    la, ca, ka, ran = _check(X, cuda, 5, chunk)
    assert STAGED <= ran and not (KEYED & ran)
    assert ka > 5 and ca.any() and not ca.all() and (la == -1).any()


def test_chunks_of_two_cells_the_limit_and_one_cell(cuda, oracle_clib):
    """exactly 2 cells, exactly 1 024 (the table's limit: still staged) and 1 cell (rows stay in place, the single
    cell is staged) side by side in one call"""
    chunk = 4096
    X = _cloud(12, chunk, [2, LIMIT, 1, 300, LIMIT, 1, 2], last_rows=1001, origin_row=3 * chunk)
    la, ca, ka, ran = _check(X, cuda, 4, chunk)
    assert STAGED <= ran and not (KEYED & ran)
    for c in (0, 2, 5):                                   # thousands of rows in one or two cells: all core
        assert ca[c * chunk:(c + 1) * chunk].all()


def test_nan_chunks_on_the_staged_route(cuda, oracle_clib):
    """NaN/inf chunks first, side by side and last: each is one staged cell that never holds a core point"""
    chunk = 3001
    X = _cloud(13, chunk, [150, 40, 700, 700, 30, 260], last_rows=1200, origin_row=chunk)    # in a finite chunk
    bad = (0, 2, 3, 5)
    for c, col, val in zip(bad, (0, 1, 2, 0), (np.nan, np.inf, np.nan, -np.inf)):
        X[c * chunk + 17 + c, col] = val
    la, ca, _, ran = _check(X, cuda, 5, chunk)
    assert STAGED <= ran and not (KEYED & ran)
    for c in bad:
        assert (la[c * chunk:(c + 1) * chunk] == -1).all() and not ca[c * chunk:(c + 1) * chunk].any()
    for c in (1, 4):
        assert ca[c * chunk:(c + 1) * chunk].any()


def test_one_overflowing_chunk_falls_back_to_the_keys(cuda, oracle_clib):
    """one chunk of 1 025 cells among chunks below the limit: db_chunksort writes that chunk's keys, db_celltab
    regenerates the keys of all other chunks (one of them a single cell, one with a NaN) from their staged lists, and
    db_heads / db_cells read the table off them"""
    chunk = 4099
    X = _cloud(14, chunk, [300, 1, LIMIT + 1, 77, LIMIT, 500], last_rows=2222)
    X[3 * chunk + 5, 2] = np.nan
    la, ca, ka, ran = _check(X, cuda, 5, chunk)
    assert STAGED <= ran and KEYED <= ran and "db_chunksort" in ran
    assert (la[3 * chunk:4 * chunk] == -1).all() and ka > 5


@pytest.mark.parametrize("chunk,rows", [(5, 403), (3, 250)])
def test_tiny_chunks(cuda, oracle_clib, chunk, rows):
    """chunks of 5 and 3 rows: the 8 rows of one db_celltab thread lie in two to four chunks"""
    X = _crowd(15 + chunk, rows)
    la, _, ka, ran = _check(X, cuda, 2, chunk)
    assert STAGED <= ran and not (KEYED & ran)
    assert ka > 10 and (la == -1).any()


def test_one_chunk_more_than_the_staged_route_takes(cuda, oracle_clib):
    """16 385 chunks of 2 rows (the last of 1): the host chooses the keyed route, db_cellscatter writes keys"""
    chunk = 2
    X = _crowd(16, 2 * MAX_CHUNKS + 1)
    la, _, ka, ran = _check(X, cuda, 2, chunk)
    assert "db_cellscatter" in ran and KEYED <= ran and not ({"db_chunkcells", "db_celltab"} & ran)
    assert ka > 100 and (la == -1).any()
    # and the largest run that is staged
    Y = X[:2 * MAX_CHUNKS - 1]
    _, _, _, ran = _check(Y, cuda, 2, chunk)
    assert STAGED <= ran and not (KEYED & ran)


def test_staged_then_fallback_then_staged_on_one_workspace(cuda, oracle_clib):
    """three calls of the same sizes in one process, so on the same workspace: staged, fallback (chunk 1 overflows;
    chunk 2 holds fewer cells than before), staged again with other cell counts.  A route word, a cell count or a
    staged list left over from the call before would show"""
    chunk, last = 4099, 1500
    clouds = [_cloud(17, chunk, [400, 900, 60, 200], last_rows=last),
              _cloud(18, chunk, [400, LIMIT + 200, 7, 200], last_rows=last),
              _cloud(19, chunk, [30, 500, 1000, 1], last_rows=last, origin_row=chunk)]
    got = [_run(X, cuda, 5, chunk, "chunk", profile=True) for X in clouds]      # back to back, nothing in between
    for X, (la, ca, ka, ran), keyed in zip(clouds, got, (False, True, False)):
        assert STAGED <= ran and (KEYED <= ran if keyed else not (KEYED & ran))
        lb, cb, kb, _ = _run(X, cuda, 5, chunk, "global")
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(ca, cb)
        assert ka == kb and ka > 0
        np.testing.assert_array_equal(la, odb.dbscan_chunked(X, EPS, 5, chunk, fit="c"))


def test_assign_continues_a_staged_fit(cuda, oracle_clib):
    """DbscanFit.assign reads chunk_cells, the cell table and the sorted rows of the fit: the same answers on a fit
    whose table came from the staged lists (the launch profile says so) as on a global-sort fit, and the fit's labels
    are the oracle's"""
    chunk = 4099
    X = _cloud(20, chunk, [200, 37, 1000, 90], last_rows=1777)
    rng = np.random.default_rng(21)
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
        out[mode] = (fit.labels.cpu().numpy(), fit.core.cpu().numpy(), fit.nclusters, got)
    for a, b in zip(out["chunk"], out["global"]):
        np.testing.assert_array_equal(a, b)
    assert STAGED <= ran["chunk"] and not (KEYED & ran["chunk"])
    assert KEYED <= ran["global"] and not (STAGED & ran["global"])
    np.testing.assert_array_equal(out["chunk"][0], odb.dbscan_chunked(X, EPS, 5, chunk, fit="c"))
    assert (out["chunk"][3] >= 0).any() and (out["chunk"][3] == -1).any()
