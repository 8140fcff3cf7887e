"""The chunk-local cell grouping (one workgroup per chunk counts the chunk's cells in an LDS table and scatters the
rows; a chunk with more cells than the table takes goes through the radix chunk sort) feeds the same clustering as
the global sort.  The inputs put rows on a lattice of cells so that every chunk holds an exact number of cells: few,
just at the table's limit and just above it, side by side in one call."""
import math

import numpy as np
import pytest
import torch

from oracle import dbscan as odb
from pointcloudhookup_amd import ops

pytestmark = pytest.mark.gpu

EPS = math.sqrt(3.0)          # cell side eps/sqrt(3) * (1 - 2^-16): one lattice unit, just under
LIMIT = 1024                  # cells a chunk may hold in the counting table
GRID = (64, 64, 40)


def _lattice_chunk(rng, ncells, rows):
    """rows points in exactly ncells distinct cells (each cell holds at least one), jittered inside the cell"""
    flat = rng.choice(int(np.prod(GRID)), ncells, replace=False)
    cells = np.stack(np.unravel_index(flat, GRID), 1).astype(np.float64)
    idx = np.concatenate([np.arange(ncells), rng.integers(0, ncells, rows - ncells)])
    rng.shuffle(idx)
    return cells[idx] + 0.5 + rng.uniform(-0.3, 0.3, (rows, 3))


def _cloud(seed, chunk, cells_per_chunk, last_rows=None):
    """one chunk per entry of cells_per_chunk (the last one holds last_rows rows when given); the grid origin sits at
    0.2 on every axis, so a lattice cell is exactly one grid cell"""
    rng = np.random.default_rng(seed)
    parts = []
    for i, nc in enumerate(cells_per_chunk):
        rows = last_rows if (last_rows is not None and i == len(cells_per_chunk) - 1) else chunk
        parts.append(_lattice_chunk(rng, nc, rows))
    X = np.vstack(parts).astype(np.float32)
    X[0] = 0.2                                            # the box's lower corner: origin of the grid
    return X


def _run(X, cuda, ms, chunk, mode):
    try:
        ops.set_dbscan_sort_mode(mode)
        lab, core, k = ops.dbscan(torch.from_numpy(X).to(cuda), EPS, ms, chunk, want_core=True)
    finally:
        ops.set_dbscan_sort_mode("auto")
    return lab.cpu().numpy(), core.cpu().numpy(), k


def _check(X, cuda, ms, chunk, oracle=False):
    la, ca, ka = _run(X, cuda, ms, chunk, "chunk")
    lb, cb, kb = _run(X, cuda, ms, chunk, "global")
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(ca, cb)
    assert ka == kb
    if oracle:
        np.testing.assert_array_equal(la, odb.dbscan_chunked(X, EPS, ms, chunk, fit="c"))
    return la, ca, ka


def test_cells_below_at_and_above_the_table_limit_in_one_call(cuda, oracle_clib):
    """few cells, the limit, one above it, far above it and a ragged last chunk: both kernels write parts of the same
    output, and three runs give the same labels although rows of a cell land in a different order each time"""
    chunk = 20000
    X = _cloud(1, chunk, [40, LIMIT - 1, LIMIT, LIMIT + 1, 300, 12000, LIMIT + 1, 2500], last_rows=7001)
    la, ca, ka = _check(X, cuda, 6, chunk, oracle=True)
    assert ka > 8 and ca.any() and not ca.all() and (la == -1).any()
    for _ in range(2):
        lb, cb, kb = _run(X, cuda, 6, chunk, "chunk")
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(ca, cb)
        assert ka == kb


def test_nan_chunks_first_last_and_adjacent(cuda, oracle_clib):
    """NaN/inf chunks stay noise as a whole, in front, side by side (one of them above the table limit) and last"""
    chunk = 9000
    X = _cloud(2, chunk, [200, 50, LIMIT + 1, 700, 700, 30, 2000], last_rows=5000)
    for c, col, val in ((0, 0, np.nan), (2, 1, np.inf), (3, 2, np.nan), (6, 0, -np.inf)):
        X[c * chunk + 17 + c, col] = val
    X[chunk] = 0.2                                        # the origin again, in a finite chunk
    la, ca, _ = _check(X, cuda, 5, chunk, oracle=True)
    for c in (0, 2, 3, 6):
        assert (la[c * chunk:(c + 1) * chunk] == -1).all() and not ca[c * chunk:(c + 1) * chunk].any()


def test_one_cell_chunks(cuda, oracle_clib):
    """a chunk whose rows all share one cell keeps them in place: dense (all core), every row the same point, and a
    ragged last chunk of three rows (noise)"""
    chunk = 5000
    rng = np.random.default_rng(3)
    parts = [_lattice_chunk(rng, 300, chunk),
             np.asarray((10.5, 20.5, 5.5)) + rng.uniform(-0.3, 0.3, (chunk, 3)),
             _lattice_chunk(rng, 1200, chunk),
             np.full((chunk, 3), 20.5),
             np.asarray((60.5, 60.5, 2.5)) + rng.uniform(-0.3, 0.3, (3, 3))]
    X = np.vstack(parts).astype(np.float32)
    X[0] = 0.2
    la, ca, _ = _check(X, cuda, 8, chunk, oracle=True)
    assert ca[chunk:2 * chunk].all() and ca[3 * chunk:4 * chunk].all() and (la[-3:] == -1).all()


@pytest.mark.parametrize("cells", [[3000, LIMIT + 1, 50], [LIMIT, 20, LIMIT + 500]])
def test_largest_chunk_size(cuda, cells):
    """chunk_size 131072, the largest the chunk-local route takes, with a ragged last chunk"""
    chunk = 131072
    X = _cloud(4, chunk, cells, last_rows=60001)
    _check(X, cuda, 50, chunk)


# The middle chunk of three takes every route of the two chunk kernels: rows per chunk, cells of the middle chunk, row
# of that chunk that holds a NaN.  The last case repeats the one before it with chunks of three row batches per thread:
# db_cellscatter_k stops sweeping behind the first batch, so only db_chunksort_k's own sweep meets the NaN.
CHUNK_SHAPES = {
    "few cells": (4096, 300, None),
    "above the table limit": (4096, LIMIT + 500, None),
    "one cell": (4096, 1, None),
    "NaN in the first rows": (4096, 300, 5),
    "above the limit, NaN in the last 64 rows": (4096, LIMIT + 500, 4096 - 10),
    "above the limit, NaN in the last 64 rows, swept in batches": (20000, LIMIT + 500, 20000 - 10),
}


@pytest.mark.parametrize("shape", list(CHUNK_SHAPES))
def test_chunk_shapes_of_the_shared_prologue(cuda, shape):
    """three chunks, the middle one of the shape under test: labels, core flags and cluster count of the chunk-local
    route equal the global sort's; a NaN chunk is noise as a whole, and a chunk above the limit went to db_chunksort"""
    chunk, cells, nan_row = CHUNK_SHAPES[shape]
    X = _cloud(5, chunk, [200, cells, 600])
    if nan_row is not None:
        X[chunk + nan_row, 1] = np.nan
    ops.set_profiling(True)
    try:
        la, ca, ka = _run(X, cuda, 4, chunk, "chunk")
        ran = {name for name, _, launches in ops.get_profile() if launches > 0}
    finally:
        ops.set_profiling(False)
    lb, cb, kb = _run(X, cuda, 4, chunk, "global")
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(ca, cb)
    assert ka == kb and ka > 0
    assert "db_cellscatter" in ran
    if cells > LIMIT:
        assert "db_chunksort" in ran
    if nan_row is not None:
        assert (la[chunk:2 * chunk] == -1).all() and not ca[chunk:2 * chunk].any()
    for c in (0, 2):
        assert (la[c * chunk:(c + 1) * chunk] >= 0).any() and ca[c * chunk:(c + 1) * chunk].any()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 2017, 2048, 2049])
def test_first_core_rows_and_identity_relabel_at_the_bitmap_boundaries(cuda, n):
    """n at the word and 64-word boundaries of the row bitmap and of its scanned word counts, which the fit and its
    continuation calls take from one carving.  Two blobs far apart, the second one in the last word: the first core
    row of every cluster is read back from the fit's own labels and core flags, and the identity map leaves the
    labels as they are"""
    rng = np.random.default_rng(n)
    nb = min((n - 1) % 32 + 1, n - 1)                     # the second blob starts with the bitmap's last word
    X = rng.uniform(-0.4, 0.4, (n, 3)) + np.where(np.arange(n)[:, None] >= n - nb, 50.0, 0.0)
    fit = ops.DbscanFit(torch.from_numpy(X.astype(np.float32)).to(cuda), 2.0, 1, 0)
    assert fit.nclusters == min(n, 2)
    labels, core = fit.labels.clone(), fit.core.bool()
    rows = torch.arange(n, device=cuda)
    want = [int(rows[core & (labels == k)].min()) for k in range(fit.nclusters)]
    assert fit.first_core_rows().cpu().tolist() == want
    ident = torch.arange(fit.nclusters, dtype=torch.int32, device=cuda)
    assert torch.equal(fit.relabel(ident), labels)
