"""The staged route's labels have one owner per row: db_label (db_filelabel_k) takes tiles of consecutive INPUT rows,
finds every row's cell among its chunk's sorted keys in LDS and writes the rows of dense cells (every row core) in file
order; db_border writes every row of every other cell.  db_prelabel makes the cells' labels in front of both, and
db_celltab builds the cell table and the neighbour-row table per cell, one workgroup per chunk, with no cid column.

Every case compares labels, core flags, cluster count and the clusters' first core rows of the staged route with the
global sort's (db_label_k, db_rowtab_k, the per-row owners of old) and with the CPU oracle (oracle.dbscan.dbscan_fit_c,
chunk by chunk), and reads the route from the library's launch profile.  The clouds sit on the lattice of
tests/test_gpu_dbscan_chunk_union.py: cell (i, j, k) covers [0.2 + i, 1.2 + i) x ..., eps = sqrt(3).

A cell's diagonal is shorter than eps, so a cell that holds a core row holds no noise row: the mixed cells here are
core + border and border + noise.

Run once against a build with two deliberate mistakes - the dense flag taken as ncore > 0, db_border_k's early exit left
in front of its writes - 6 of the 9 cases fail: the shuffled chunk, both awkward chunk sizes, the three fits on one
workspace, the cluster boxes at (2, 10) and the continuation (by its core flags); the overflowing chunk (old kernels),
the cluster boxes at (8, 80) and the profile pass.
All 9 pass on the final sources."""
import numpy as np
import pytest
import torch

from oracle import dbscan as odb
from pointcloudhookup_amd import ops, pipeline, synth
from test_gpu_dbscan_chunk_union import (EPS, KEYED, LIMIT, SEVEN, _cells_of, _chunk_rows, _cloud, _in_lds)

pytestmark = pytest.mark.gpu

TILE = 2048                   # input rows per workgroup of db_filelabel_k (DB_LAB_TILE)


# ------------------------------------------------------------------------------------------------ runs
def _oracle(X, ms, chunk):
    """labels, core flags, cluster count and first core rows: dbscan_fit_c chunk by chunk, numbered on as
    oracle.dbscan.dbscan_chunked numbers; a NaN/inf chunk stays noise"""
    n = len(X)
    labels, core, k = np.full(n, -1, np.int32), np.zeros(n, np.uint8), 0
    for lo in range(0, n, chunk):
        part = X[lo:lo + chunk]
        if not np.isfinite(part).all():
            continue
        la, co = odb.dbscan_fit_c(part, EPS, ms)
        labels[lo:lo + chunk] = np.where(la >= 0, la + k, -1)
        core[lo:lo + chunk] = co
        if (la >= 0).any():
            k += int(la.max()) + 1
    first = np.array([np.flatnonzero((labels == c) & (core != 0))[0] for c in range(k)], np.int32)
    return labels, core, k, first


def _fit(X, cuda, ms, chunk, mode):
    """one fit on a workspace of its own: (labels, core, count, first core rows), the kernels launched, the fit"""
    try:
        ops.set_dbscan_sort_mode(mode)
        ops.set_profiling(True)
        fit = ops.DbscanFit(torch.from_numpy(X).to(cuda), EPS, ms, chunk)
        ran = {name for name, _, launches in ops.get_profile() if launches > 0}
    finally:
        ops.set_profiling(False)
        ops.set_dbscan_sort_mode("auto")
    first = fit.first_core_rows().cpu().numpy()
    return (fit.labels.cpu().numpy(), fit.core.cpu().numpy(), fit.nclusters, first), ran, fit


def _same(got, want):
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def _staged(ran):
    return _in_lds(ran) and "db_rowtab" not in ran and {"db_prelabel", "db_label", "db_border"} <= ran


def _check(X, cuda, ms, chunk, staged=True):
    """staged route == global sort == CPU oracle, and the route; returns the chunk-local results"""
    got, ran, _ = _fit(X, cuda, ms, chunk, "chunk")
    glob, ranb, _ = _fit(X, cuda, ms, chunk, "global")
    _same(got, glob)
    _same(got, _oracle(X, ms, chunk))
    assert SEVEN <= ranb and "db_chunkunion" not in ranb and "db_rowtab" in ranb
    assert _staged(ran) if staged else (KEYED <= ran and SEVEN <= ran and "db_chunkunion" not in ran)
    return got


# ------------------------------------------------------------------------------------------------ clouds
def _roles():
    """min_samples 4.  (name, rows) of hand-placed cells, coordinates absolute (cell i covers [0.2 + i, 1.2 + i)):
    origin   cell (0,0,0), six rows, one of them the grid's origin: dense
    D        cell (1,0,0), nine rows: eight low in y and t high in y: dense
    bn       cell (1,2,0), two rows: b within eps of t alone (border), n beyond eps of everything but b (noise)
    four     cell (3,0,0), exactly min_samples rows: dense, a cluster of its own
    three    cell (5,0,0), one row fewer, two cells from `four`: no core row, beyond eps of every core row -> noise,
             although a core cell lies in its neighbourhood (the border rule runs and finds nothing)
    S        cell (9,0,0), three rows, each within eps of the two others and of p1: all core though the cell holds
             fewer than min_samples rows
    cb       cell (10,0,0), two rows: p1 within eps of S (core), p2 within eps of p1 alone (border)
    far      cell (20,20,10), three rows, no core cell anywhere around: all -1 by the early exit"""
    j = np.random.default_rng(7).uniform(-0.01, 0.01, (64, 3))
    at = lambda k, x, y, z: np.array([x, y, z]) + j[k]
    return [("origin", np.vstack([[[0.2, 0.2, 0.2]]] + [at(k, 0.35, 0.35, 0.35)[None] for k in range(5)])),
            ("D", np.vstack([at(10 + k, 1.7, 0.35, 0.7)[None] for k in range(8)] + [at(18, 1.7, 1.15, 0.7)[None]])),
            ("bn", np.vstack([at(20, 1.7, 2.8, 0.7)[None], at(21, 1.7, 3.15, 0.7)[None]])),
            ("four", np.vstack([at(30 + k, 3.7, 0.7, 0.7)[None] for k in range(4)])),
            ("three", np.vstack([at(35 + k, 5.7, 0.7, 0.7)[None] for k in range(3)])),
            ("S", np.vstack([at(40 + k, 9.3, 0.7, 0.7)[None] for k in range(3)])),
            ("cb", np.vstack([at(45, 10.3, 0.7, 0.7)[None], at(46, 11.15, 0.7, 0.7)[None]])),
            ("far", np.vstack([at(50 + k, 20.7, 20.7, 10.7)[None] for k in range(3)]))]


def _shuffled_chunk():
    """the hand-placed cells and a random lattice of 300 cells 30 cells above them, all rows shuffled: one chunk of
    two label tiles and a few rows in which file order is not cell order; returns the cloud and where every
    hand-placed row went"""
    roles = _roles()
    rng = np.random.default_rng(8)
    filler = _chunk_rows(rng, 300, TILE + 77, grid=(12, 12, 6)) + (0.0, 0.0, 30.0)
    X = np.vstack([r for _, r in roles] + [filler]).astype(np.float32)
    order = rng.permutation(len(X))
    where, at = {}, 0
    inv = np.argsort(order)
    for name, r in roles:
        where[name] = inv[at:at + len(r)]
        at += len(r)
    return X[order], where


# ------------------------------------------------------------------------------------------------ cases
def test_shuffled_chunk_with_every_kind_of_cell(cuda, oracle_clib):
    X, w = _shuffled_chunk()
    assert len(X) > TILE and (X.min(0) == 0.2).all()
    c = _cells_of(X)
    for name, cell in (("origin", (0, 0, 0)), ("D", (1, 0, 0)), ("bn", (1, 2, 0)), ("four", (3, 0, 0)),
                       ("three", (5, 0, 0)), ("S", (9, 0, 0)), ("cb", (10, 0, 0)), ("far", (20, 20, 10))):
        assert (c[w[name]] == cell).all() and (c == cell).all(1).sum() == len(w[name])
    la, ca, ka, _ = _check(X, cuda, 4, len(X))
    assert ca[w["origin"]].all() and ca[w["D"]].all() and ca[w["four"]].all() and ca[w["S"]].all()
    assert len(set(la[np.concatenate([w["origin"], w["D"]])])) == 1 and la[w["D"][0]] >= 0
    b, n = w["bn"]
    assert not ca[b] and not ca[n] and la[b] == la[w["D"][0]] and la[n] == -1
    assert len(set(la[w["four"]])) == 1 and la[w["four"][0]] not in (-1, la[w["D"][0]])
    assert not ca[w["three"]].any() and (la[w["three"]] == -1).all()
    p1, p2 = w["cb"]
    assert ca[p1] and not ca[p2] and la[p1] == la[p2] == la[w["S"][0]] >= 0
    assert not ca[w["far"]].any() and (la[w["far"]] == -1).all()


@pytest.mark.parametrize("chunk", [4099, 4128])
def test_several_chunks_with_awkward_sizes(cuda, oracle_clib, chunk):
    """4 099 is no multiple of 32 (two chunks share a word of the row bitmap), 4 128 is one, neither is a multiple of
    the label tile.  A one-cell chunk, a NaN chunk in the middle, a chunk of exactly 1 024 cells, a last chunk of one
    row"""
    assert chunk % TILE and (chunk % 32 != 0) == (chunk == 4099)
    X = _cloud(101, chunk, [300, 1, 200, LIMIT, 500, 1], last_rows=1)
    X[2 * chunk + 1234, 2] = np.nan
    assert len(X) == 5 * chunk + 1
    assert len(np.unique(_cells_of(X[3 * chunk:4 * chunk]), axis=0)) == LIMIT
    la, ca, ka, first = _check(X, cuda, 4, chunk)
    assert ca[chunk:2 * chunk].all() and len(set(la[chunk:2 * chunk])) == 1
    assert (la[2 * chunk:3 * chunk] == -1).all() and not ca[2 * chunk:3 * chunk].any()
    assert la[-1] == -1 and not ca[-1]
    part_l, part_c = la[3 * chunk:4 * chunk], ca[3 * chunk:4 * chunk]        # the 1 024 cells: all three kinds of rows
    assert part_c.sum() > 1000 and ((part_l >= 0) & (part_c == 0)).sum() > 20 and (part_l == -1).sum() > 100
    assert ca[:chunk].sum() > 1000 and ca[4 * chunk:5 * chunk].sum() > 1000


def test_a_chunk_of_1025_cells_takes_the_old_kernels(cuda, oracle_clib):
    chunk = 4099
    X = _cloud(102, chunk, [300, LIMIT + 1, 77], last_rows=2222)
    la, ca, ka, first = _check(X, cuda, 4, chunk, staged=False)
    assert ka > 5


def test_three_clouds_on_one_workspace(cuda, oracle_clib):
    """ops.dbscan keeps one workspace per thread: three clouds of one size with other cell counts, back to back.  A
    cell label, a neighbour row or a bitmap word left from the fit before would show"""
    chunk, last = 4099, 1500
    clouds = [_cloud(103, chunk, [400, 900, 60, 200], last_rows=last),
              _cloud(104, chunk, [30, 500, 1000, 1], last_rows=last, origin_row=chunk),
              _cloud(105, chunk, [900, 20, 700, 300], last_rows=last)]
    got = []
    try:
        ops.set_dbscan_sort_mode("chunk")
        for X in clouds:                                  # nothing in between
            ops.set_profiling(True)
            lab, core, k = ops.dbscan(torch.from_numpy(X).to(cuda), EPS, 4, chunk, want_core=True)
            ran = {name for name, _, launches in ops.get_profile() if launches > 0}
            ops.set_profiling(False)
            got.append((lab.cpu().numpy(), core.cpu().numpy(), k, ran))
    finally:
        ops.set_profiling(False)
        ops.set_dbscan_sort_mode("auto")
    for X, (la, ca, ka, ran) in zip(clouds, got):
        assert _staged(ran)
        want = _oracle(X, 4, chunk)
        _same((la, ca, ka), want[:3])
        assert ka > 0


@pytest.mark.parametrize("eps,min_points,chunk", [(8.0, 80, 5000), (2.0, 10, 1000)])
def test_cluster_boxes(cuda, eps, min_points, chunk):
    """pipeline.cluster_points with the chunk route forced: a cluster's box is folded from the dense cells' rows in
    file order, the exact core boxes of the other cells and the border rows - it must be numpy's min / max over the
    cluster's rows.  By the CPU oracle the 11 772 kept rows hold 48 border rows and 15 cells with core and other rows
    at (8, 80) in chunks of 5 000 (176 cells at most), and 2 843 border rows, 4 269 noise rows and 215 such cells at
    (2, 10) in chunks of 1 000 (860 cells at most)"""
    raw = torch.from_numpy(synth.corridor_numpy(120000, seed=synth.SEED0, kind="corridor", offset=True,
                                                towers=3).astype(np.float32)).to(cuda)
    try:
        ops.set_dbscan_sort_mode("chunk")
        ops.set_profiling(True)
        cl = pipeline.cluster_points(raw, eps, min_points, chunk)
        ran = {name for name, _, launches in ops.get_profile() if launches > 0}
    finally:
        ops.set_profiling(False)
        ops.set_dbscan_sort_mode("auto")
    assert "db_chunkunion" in ran and "db_celltab" in ran and "db_rowtab" not in ran
    P = cl["ground"]["points"].cpu().numpy()
    la, k = cl["labels"].cpu().numpy(), int(cl["nclusters"])
    stats = cl["stats"].cpu().numpy()
    assert k > 0 and len(P) == len(la) > 5000 and ((la == -1).sum() > 4000) == (eps == 2.0)
    want = np.zeros((k, 8), np.float32)
    for c in range(k):
        rows = P[la == c]
        want[c, :3], want[c, 3:6] = rows.min(0), rows.max(0)
    np.testing.assert_array_equal(stats.view(np.uint32), want.view(np.uint32))


def test_assign_after_a_staged_fit(cuda, oracle_clib):
    """DbscanFit.assign reads the cells' labels (db_prelabel on the staged route, db_label on any other)"""
    chunk = 4099
    X = _cloud(106, chunk, [200, 37, 1000, 90], last_rows=1777)
    rng = np.random.default_rng(107)
    pick = rng.integers(0, len(X), 500)
    Q = torch.from_numpy((X[pick] + rng.uniform(-0.8, 0.8, (len(pick), 3))).astype(np.float32)).to(cuda)
    qc = torch.from_numpy((pick // chunk).astype(np.int32)).to(cuda)
    out = {}
    for mode in ("chunk", "global"):
        got, ran, fit = _fit(X, cuda, 4, chunk, mode)
        assert _staged(ran) if mode == "chunk" else "db_chunkunion" not in ran
        out[mode] = got + (fit.assign(Q, chunk=qc).cpu().numpy(),)
    _same(out["chunk"], out["global"])
    assert (out["chunk"][4] >= 0).any() and (out["chunk"][4] == -1).any()


def test_profile_of_the_staged_route(cuda):
    """db_celltab ran once, with the neighbour rows in its launch: no db_rowtab; the labels came from db_prelabel,
    db_label and db_border, one launch each"""
    X = _cloud(108, 4099, [300, 700], last_rows=2000)
    try:
        ops.set_dbscan_sort_mode("chunk")
        ops.set_profiling(True)
        ops.dbscan(torch.from_numpy(X).to(cuda), EPS, 4, 4099)
        prof = {name: launches for name, _, launches in ops.get_profile()}
    finally:
        ops.set_profiling(False)
        ops.set_dbscan_sort_mode("auto")
    for name in ("db_cellscatter", "db_chunkcells", "db_celltab", "db_chunkunion", "db_prelabel", "db_label", "db_border"):
        assert prof.get(name, 0) == 1, name
    for name in ("db_rowtab", "db_heads", "db_cells", "db_cellstats"):
        assert prof.get(name, 0) == 0, name
