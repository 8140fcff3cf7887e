"""Span sections on the device (pch_span_section_f32, ops.span_section, pipeline.span_sections, the drop-in's
PCH_SECTION): all seven outputs must equal the numpy statement of the rule (section_cases) bit for bit - whatever the
sweep culls and however the waves combine their rows."""
import csv

import numpy as np
import pytest
import torch

import clearance_cases as cc
import las_bytes
import section_cases as sn
import shape_cases as sc
import span_cases as sp
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

TILE = ops.CLEARANCE_TILE
EPSG = np.array([437000.0, 3139000.0, 80.0])
HALF, DEPTH, LIMIT = 12.0, 25.0, 6.0


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(cuda)


def _run(X, C, B, cuda, half=HALF, depth=DEPTH, limit=LIMIT, skip=None, want_stats=False):
    out = ops.span_section(_dev(X, cuda), _dev(np.asarray(C, dtype=np.float64).reshape(-1, 10), cuda), B, half, depth,
                           limit, skip=None if skip is None else _dev(skip, cuda), want_stats=want_stats)
    return {key: v.cpu().numpy() for key, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want, what):
    for key in sn.OUTPUTS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        if not np.array_equal(_bits(got[key]), _bits(want[key])):
            bad = np.argwhere(got[key] != want[key])[:5]
            raise AssertionError((what, key, bad.tolist(), [got[key][tuple(b)] for b in bad],
                                  [want[key][tuple(b)] for b in bad]))


def _check(X, C, B, cuda, what, half=HALF, depth=DEPTH, limit=LIMIT, skip=None):
    want = sn.section_reference(X, C, B, half, depth, limit, skip=skip)
    got = _run(X, C, B, cuda, half, depth, limit, skip=skip)
    _same(got, want, what)
    return got, want


# ------------------------------------------------------------------ rows, spans, stations
@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_row_and_span_counts(cuda, n):
    hits = 0
    for K in (0, 1, 64, 65):
        X, C = sn.random_case(n, K, seed=100 + K)
        _, want = _check(X, C, 16, cuda, (n, K))
        hits += int((want["span"] >= 0).sum())
        if K == 0:
            assert (want["span"] == -1).all() and np.isinf(want["v"]).all() and (want["station"] == -1).all()
            assert want["count"].shape == (0, 16)
    assert hits > 0 or n <= 1


@pytest.mark.parametrize("B", [1, 2, 64, 128])
def test_station_counts_over_several_tiles(cuda, B):
    X, C = sn.random_case(5 * TILE + 17, 65, seed=7, phases=True)
    got, want = _check(X, C, B, cuda, B)
    assert (want["count"].sum(axis=1) > 0).sum() > 40 and want["violations"].sum() > 500
    assert want["count"].sum() > (want["span"] >= 0).sum()                     # rows under more than one span
    assert (want["station"] < B).all() and (want["station"].max() == B - 1)


# ------------------------------------------------------------------ the rule's edges
def test_the_boundary_rows(cuda):
    X, skip, curves, rows = sn.edge_case()
    got, _ = _check(X, curves, sn.E_STATIONS, cuda, "edges", half=sn.E_HALF, depth=sn.E_DEPTH, limit=sn.E_LIMIT,
                    skip=skip)
    part = np.array([w[0] for w in rows])
    assert np.array_equal(got["span"], np.where(part, 1, -1))
    assert np.array_equal(got["station"], np.array([w[1] for w in rows]))
    assert got["v"][14] == 0.0 and got["v"][17] == 4.0 and got["v"][20] == 16.0
    assert got["violations"][1].tolist() == [1, 0, 4, 1] and got["count"][2].tolist() == got["count"][1].tolist()
    assert got["min_v"][1].tolist() == [1.0, 6.0, 0.0, 0.5] and got["min_row"][2].tolist() == [29, 8, 14, 30]
    # the same rows spread over three tiles, each among rows that are far from everything
    big = np.full((2 * TILE + 300, 3), 500.0, dtype=np.float32)
    where = np.arange(len(X)) * 71 + 5
    big[where] = X
    bskip = np.zeros(len(big), dtype=np.uint8)
    bskip[where] = skip
    got, _ = _check(big, curves, sn.E_STATIONS, cuda, "edges, three tiles", half=sn.E_HALF, depth=sn.E_DEPTH,
                    limit=sn.E_LIMIT, skip=bskip)
    assert np.array_equal(got["span"][where], np.where(part, 1, -1)) and (np.delete(got["span"], where) == -1).all()


# ------------------------------------------------------------------ attribution
def test_three_parallel_phases_count_a_row_in_all_three(cuda):
    rng = np.random.default_rng(5)
    phases = np.stack([cc.curve(cy=lat, cz=30.0, a=-2.0 + 0.25 * i, c=0.002, m0=-40.0, m1=40.0)
                       for i, lat in enumerate((-4.0, 0.0, 4.0))])
    n = TILE + 200
    X = np.stack([rng.uniform(-45.0, 45.0, n), rng.uniform(-20.0, 20.0, n), rng.uniform(0.0, 32.0, n)],
                 axis=1).astype(np.float32)
    got, want = _check(X, phases, 16, cuda, "phases")
    m, t = X[:, 0].astype(np.float64), X[:, 1].astype(np.float64)
    under_all = (np.abs(m) < 39.0) & (np.abs(t) < HALF - 4.5) & (X[:, 2] > 8.0) & (X[:, 2] < 27.0)
    assert under_all.sum() > 200
    j = np.floor((m + 40.0) / 5.0).astype(int)
    for k in range(3):
        assert (got["count"][k] >= np.bincount(j[under_all], minlength=16)).all()
    assert got["count"].sum() >= 3 * under_all.sum()
    # the wire that hangs lowest above the row gets it: here the first phase (a is lowest), whatever its index
    assert (got["span"][under_all] == 0).all()
    back, _ = _check(X, phases[::-1], 16, cuda, "phases reversed")
    assert (back["span"][under_all] == 2).all()
    for key in ("count", "violations", "min_v", "min_row"):
        assert np.array_equal(_bits(back[key][::-1]), _bits(got[key])), key
    assert np.array_equal(_bits(back["v"]), _bits(got["v"])) and np.array_equal(back["station"], got["station"])


def test_ties_between_identical_spans_go_to_the_lowest_index(cuda):
    X, C = sn.random_case(TILE + 300, 1, seed=3)
    got, _ = _check(X, np.concatenate([C, C, C]), 32, cuda, "three identical spans")
    assert (got["span"] <= 0).all() and (got["span"] == 0).sum() > 300
    for key in ("count", "violations", "min_v", "min_row"):                    # every cell of the copies is the first's
        assert np.array_equal(_bits(got[key][1]), _bits(got[key][0])), key
        assert np.array_equal(_bits(got[key][2]), _bits(got[key][0])), key


# ------------------------------------------------------------------ the lowest row of a minimum
def test_duplicate_rows_at_a_cells_minimum_give_the_lowest_row(cuda):
    """the row that is a cell's minimum stands at five places - two waves of one tile, two rounds of one wave, two
    other tiles - among rows that lie deeper in the same cell and in other cells"""
    rng = np.random.default_rng(11)
    wire = cc.curve(cz=30.0, c=0.004, m0=-40.0, m1=40.0).reshape(1, 10)
    n = 3 * TILE + 50
    X = np.stack([rng.uniform(-40.0, 40.0, n), rng.uniform(-10.0, 10.0, n), rng.uniform(8.0, 25.0, n)],
                 axis=1).astype(np.float32)
    top = np.array([12.5, 1.0, 29.0], dtype=np.float32)                        # zw = 30.625: v = 1.625, station 10 of 16
    places = [2 * TILE + 31, TILE + 700, 300 + 64, 300, 3 * TILE + 7]
    for order in (places, places[::-1]):
        for i in order:
            X[i] = top
        got, want = _check(X, wire, 16, cuda, "duplicates")
        assert got["min_row"][0, 10] == min(places) and got["min_v"][0, 10] == np.float32(1.625)
        assert got["count"][0, 10] > 100
    X[300] = X[0]
    got, _ = _check(X, wire, 16, cuda, "duplicates without the lowest")
    assert got["min_row"][0, 10] == 300 + 64


# ------------------------------------------------------------------ spans that take no part, odd directions
def test_spans_that_take_no_part_change_no_bit_of_the_others(cuda):
    X, C = sn.random_case(2 * TILE + 5, 9, seed=21)
    clean = _run(X, C, 32, cuda)
    _same(clean, sn.section_reference(X, C, 32, HALF, DEPTH, LIMIT), "clean")
    cases = [(col, v) for col in range(10) for v in (np.nan, np.inf if col % 2 else -np.inf)]
    for col, v in cases + [("no length", 0.0), ("backwards", -1.0)]:
        D = np.insert(C, 4, C[2], axis=0)
        if col == "no length":
            D[4, 9] = D[4, 8]
        elif col == "backwards":
            D[4, 8], D[4, 9] = D[4, 9], D[4, 8]
        else:
            D[4, col] = v
        assert not sn.takes_part(D)[4], (col, v)
        got, _ = _check(X, D, 32, cuda, (col, v))
        assert (got["span"] != 4).all() and got["count"][4].sum() == 0 and (got["min_row"][4] == -1).all()
        assert np.isinf(got["min_v"][4]).all()
        keep = np.array([0, 1, 2, 3, 5, 6, 7, 8, 9])
        moved = np.where(got["span"] > 4, got["span"] - 1, got["span"])
        assert np.array_equal(moved, clean["span"]) and np.array_equal(_bits(got["v"]), _bits(clean["v"]))
        assert np.array_equal(got["station"], clean["station"])
        for key in ("count", "violations", "min_v", "min_row"):
            assert np.array_equal(_bits(got[key][keep]), _bits(clean[key])), (col, key)


def test_a_span_whose_direction_is_not_unit_is_never_wrongly_culled(cuda):
    X, C = sn.random_case(3 * TILE, 6, seed=33, spread=4000.0)
    X = X[np.argsort(X[:, 0], kind="stable")]                                  # sorted: tight tile boxes
    C[1, 3:5] *= 1.5                                                           # stretches m and t by 1.5
    C[4, 3:5] *= 0.5
    C[5, 3:5] *= 1.0 + 1e-5                                                    # beyond the bounds' assumption
    far = X.copy()
    far[:, 0] += np.float32(9000.0)                                            # rows the true bounds would never meet
    for rows, what in ((X, "near"), (np.vstack([far, X]), "far and near")):
        got, want = _check(rows, C, 32, cuda, what, half=25.0, depth=40.0, limit=10.0)
    assert (want["count"][[1, 4, 5]].sum(axis=1) > 0).all()


# ------------------------------------------------------------------ mask and rows
def test_skip_mask_nonfinite_rows_and_tiles_with_no_acceptable_row(cuda):
    X, C = sn.random_case(3 * TILE + 100, 12, seed=51)
    rng = np.random.default_rng(52)
    skip = (rng.uniform(0.0, 1.0, len(X)) < 0.2).astype(np.uint8)
    skip[TILE:2 * TILE] = 1                                                    # a tile that is skipped entirely
    skip[5] = 255
    bad = {3: (0, np.nan), 64: (1, np.inf), 65: (2, -np.inf), 700: (0, np.inf), TILE - 1: (2, np.nan),
           2 * TILE: (1, np.nan), 3 * TILE + 99: (0, -np.inf), 2 * TILE + 1: (2, np.inf)}
    for i, (axis, v) in bad.items():
        X[i, axis] = v
    got, want = _check(X, C, 32, cuda, "skip", skip=skip)
    gone = np.union1d(np.flatnonzero(skip), np.array(sorted(bad)))
    assert (got["span"][gone] == -1).all() and np.isinf(got["v"][gone]).all() and (got["station"][gone] == -1).all()
    assert (got["span"][:TILE] >= 0).sum() > 100 and not np.isin(got["min_row"], gone).any()
    out = ops.span_section(_dev(X, cuda), _dev(C, cuda), 32, HALF, DEPTH, LIMIT, skip=_dev(skip != 0, cuda))
    assert np.array_equal(out["span"].cpu().numpy(), want["span"])             # a bool mask is taken as it is
    everything = _run(X, C, 32, cuda, skip=np.ones(len(X), dtype=np.uint8), want_stats=True)
    assert (everything["span"] == -1).all() and (everything["count"] == 0).all()
    assert everything["stats"].tolist() == [0, 0, 0]
    assert (everything["min_row"] == -1).all() and np.isinf(everything["min_v"]).all()
    allbad = np.full((TILE + 3, 3), np.nan, dtype=np.float32)                  # tiles without a finite row
    _check(allbad, C, 32, cuda, "no finite row")


def test_projected_coordinates_and_the_same_call_twice(cuda):
    X, C = sn.random_case(4 * TILE + 1, 65, seed=91, shift=EPSG)
    a, want = _check(X, C, 64, cuda, "EPSG scale")
    assert (want["span"] >= 0).sum() > 1500 and want["violations"].sum() > 300
    b = _run(X, C, 64, cuda)
    for key in sn.OUTPUTS:
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key


# ------------------------------------------------------------------ culling and contention
def test_two_hundred_spans_in_random_and_in_sorted_row_order(cuda):
    """K = 200 short spans over 10 km and 8 tiles of rows: shuffled, every tile meets nearly every span; sorted, most
    (tile, span) pairs are culled, and the tables are the same"""
    rng = np.random.default_rng(44)
    n, K, B = 8 * TILE, 200, 16
    X, C = sn.random_case(n, K, seed=45, spread=10000.0)
    C[:, 8], C[:, 9] = -rng.uniform(2.0, 6.0, K), rng.uniform(2.0, 6.0, K)
    C[:, 7] = rng.uniform(0.02, 0.2, K)                                       # short and deep
    k = rng.integers(0, K, n)
    m, t = rng.uniform(-8.0, 8.0, n), rng.normal(0.0, 6.0, n)
    near = np.stack([C[k, 0] + m * C[k, 3] - t * C[k, 4], C[k, 1] + m * C[k, 4] + t * C[k, 3],
                     C[k, 2] + C[k, 5] - rng.uniform(-4.0, 20.0, n)], axis=1).astype(np.float32)
    X = np.where((rng.uniform(0.0, 1.0, n) < 0.8)[:, None], near, X)
    X = X[rng.permutation(n)]
    want = sn.section_reference(X, C, B, HALF, DEPTH, LIMIT)
    assert (want["count"].sum(axis=1) > 0).sum() > 150 and want["violations"].sum() > 300
    shuffled = _run(X, C, B, cuda, want_stats=True)
    _same(shuffled, want, "random order")
    order = np.lexsort((X[:, 1], X[:, 0]))
    ordered = _run(X[order], C, B, cuda, want_stats=True)
    assert np.array_equal(_bits(ordered["v"]), _bits(want["v"][order]))
    assert np.array_equal(ordered["span"], want["span"][order])
    assert np.array_equal(ordered["station"], want["station"][order])
    for key in ("count", "violations", "min_v"):
        assert np.array_equal(_bits(ordered[key]), _bits(want[key])), key
    has = want["min_row"] >= 0
    assert np.array_equal(ordered["min_row"] >= 0, has)
    assert np.array_equal(X[order][ordered["min_row"][has]], X[want["min_row"][has]])   # the same point, wherever it is
    tiles = n // TILE
    print(f"(tile, span) pairs walked: {shuffled['stats'][1]} shuffled, {ordered['stats'][1]} sorted of {tiles * K}; "
          f"pairs that took part {shuffled['stats'][0]}; flushes {shuffled['stats'][2]} and {ordered['stats'][2]}")
    assert shuffled["stats"][0] == ordered["stats"][0] == want["count"].sum()
    assert shuffled["stats"][1] > 0.6 * tiles * K and ordered["stats"][1] < 0.25 * tiles * K
    assert ordered["stats"][2] <= shuffled["stats"][2] <= shuffled["stats"][0]


def test_rows_all_in_one_cell_reach_global_memory_once_per_wave(cuda):
    rng = np.random.default_rng(12)
    n = 4 * TILE
    wire = cc.curve(cz=30.0, c=0.004, m0=-40.0, m1=40.0).reshape(1, 10)
    X = np.stack([rng.uniform(10.1, 14.9, n), rng.uniform(-10.0, 10.0, n), rng.uniform(8.0, 28.0, n)],
                 axis=1).astype(np.float32)                                    # station 10 of 16: m in [10, 15)
    want = sn.section_reference(X, wire, 16, HALF, DEPTH, LIMIT)
    assert want["count"][0, 10] == n
    got = _run(X, wire, 16, cuda, want_stats=True)
    _same(got, want, "one cell")
    print(f"stats {got['stats'].tolist()} for {n} rows in one cell")
    assert got["stats"][0] == n and got["stats"][1] == 4 and 0 < got["stats"][2] <= -(-n // 64)


# ------------------------------------------------------------------ call level
def test_refusals(cuda):
    X, C = sn.random_case(100, 3, seed=95)
    dX, dC = _dev(X, cuda), _dev(C, cuda)
    for half, depth, limit in ((np.nan, 80.0, 7.0), (np.inf, 80.0, 7.0), (0.0, 80.0, 7.0), (-1.0, 80.0, 7.0),
                               (15.0, np.nan, 7.0), (15.0, np.inf, 7.0), (15.0, 80.0, np.nan), (15.0, 80.0, 0.0),
                               (15.0, 80.0, -1.0), (15.0, 5.0, 6.0), (15.0, 0.0, 0.0)):
        with pytest.raises(ValueError):
            ops.span_section(dX, dC, 16, half, depth, limit)
    for stations in (0, 129, 1.5, True):
        with pytest.raises(ValueError):
            ops.span_section(dX, dC, stations, 15.0, 80.0, 7.0)
    with pytest.raises(ValueError):
        ops.span_section(dX, dC[:, :5].contiguous(), 16, 15.0, 80.0, 7.0)
    with pytest.raises(ValueError):
        ops.span_section(dX, _dev(np.zeros((4097, 10)), cuda), 16, 15.0, 80.0, 7.0)
    with pytest.raises(ValueError):
        ops.span_section(dX, dC, 16, 15.0, 80.0, 7.0, skip=torch.zeros(99, dtype=torch.uint8, device=cuda))
    with pytest.raises(TypeError):
        ops.span_section(torch.from_numpy(X), dC, 16, 15.0, 80.0, 7.0)
    with pytest.raises(TypeError):
        ops.span_section(dX, dC.to(torch.float32), 16, 15.0, 80.0, 7.0)
    with pytest.raises(TypeError):
        pipeline.span_sections(torch.from_numpy(X), {})
    out = ops.span_section(dX, dC, 16, 15.0, 80.0, 80.0)                       # limit == depth is allowed
    assert torch.equal(out["count"], out["violations"]) and "stats" not in out


def test_the_raw_c_abi(cuda):
    L = _lib.lib()
    X, C = sn.random_case(TILE + 7, 4, seed=97)
    n, K, B = len(X), 4, 8
    want = sn.section_reference(X, C, B, HALF, DEPTH, LIMIT)
    assert want["count"].sum() > 200
    dX, dC = _dev(X, cuda), _dev(C, cuda)
    v = torch.full((n,), -1.0, dtype=torch.float32, device=cuda)
    span = torch.full((n,), 7, dtype=torch.int32, device=cuda)
    station = torch.full((n,), 7, dtype=torch.int32, device=cuda)
    tab = [torch.full((K, B), 7, dtype=dt, device=cuda) for dt in (torch.int64, torch.int64, torch.float32, torch.int64)]
    stats = torch.full((3,), 7, dtype=torch.int64, device=cuda)
    need = L.pch_span_section_ws_bytes(n, K, B)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def call(xyz=None, nn=n, kk=K, bb=B, half=HALF, depth=DEPTH, limit=LIMIT, out=None, ost=None, cnt=None, mrow=None,
             wsp=None, wb=None, cv=None):
        return L.pch_span_section_f32(p(dX) if xyz is None else xyz, 0, nn, p(dC) if cv is None else cv, kk, bb, half,
                                      depth, limit, p(v) if out is None else out, p(span),
                                      p(station) if ost is None else ost, p(tab[0]) if cnt is None else cnt, p(tab[1]),
                                      p(tab[2]), p(tab[3]) if mrow is None else mrow, p(stats),
                                      p(ws) if wsp is None else wsp, need if wb is None else wb, st)

    assert call() == 0
    got = dict(count=tab[0], violations=tab[1], min_v=tab[2], min_row=tab[3], v=v, span=span, station=station)
    _same({key: t.cpu().numpy() for key, t in got.items()}, want, "raw")
    assert stats[0].item() == want["count"].sum() and 0 < stats[1].item() <= 2 * K    # two tiles; a far span is culled
    assert 0 < stats[2].item() <= stats[0].item()
    before = [t.clone() for t in got.values()] + [stats.clone()]
    assert call(wb=need - 1) == -2 and b"workspace" in L.pch_last_error()      # PCH_ERR_WORKSPACE
    host = np.zeros(n, dtype=np.float64)
    nan, inf = float("nan"), float("inf")
    for rc in (call(nn=-1), call(nn=2 ** 32), call(kk=-1), call(kk=4097), call(bb=0), call(bb=129), call(half=nan),
               call(half=0.0), call(half=-1.0), call(half=inf), call(depth=nan), call(depth=inf), call(limit=nan),
               call(limit=0.0), call(limit=DEPTH + 0.5), call(xyz=0), call(out=0), call(ost=0), call(cnt=0),
               call(mrow=0), call(cv=0), call(wsp=0), call(wsp=host.ctypes.data)):
        assert rc == -1                                                        # PCH_ERR_ARG
    torch.cuda.synchronize()
    for t, b in zip(list(got.values()) + [stats], before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))           # a refused call writes nothing
    # no span: every row +inf / -1 / -1 and no table, without a pointer to read; no row: empty cells per span
    f = L.pch_span_section_f32
    assert f(p(dX), 0, n, 0, 0, B, HALF, DEPTH, LIMIT, p(v), p(span), p(station), 0, 0, 0, 0, p(stats), p(ws), need,
             st) == 0
    torch.cuda.synchronize()
    assert torch.isinf(v).all() and (span == -1).all() and (station == -1).all() and stats.tolist() == [0, 0, 0]
    stats.fill_(7)
    assert f(0, 0, 0, p(dC), K, B, HALF, DEPTH, LIMIT, 0, 0, 0, p(tab[0]), p(tab[1]), p(tab[2]), p(tab[3]), p(stats),
             p(ws), need, st) == 0
    torch.cuda.synchronize()
    assert (tab[0] == 0).all() and (tab[1] == 0).all() and torch.isinf(tab[2]).all() and (tab[3] == -1).all()
    assert stats.tolist() == [0, 0, 0]
    stats.fill_(7)                                                             # neither rows nor spans: stats all the same
    assert f(0, 0, 0, 0, 0, B, HALF, DEPTH, LIMIT, 0, 0, 0, 0, 0, 0, 0, p(stats), p(ws), need, st) == 0
    assert f(0, 0, 0, 0, 0, B, HALF, DEPTH, LIMIT, 0, 0, 0, 0, 0, 0, 0, 0, p(ws), need, st) == 0
    torch.cuda.synchronize()
    assert stats.tolist() == [0, 0, 0]


# ------------------------------------------------------------------ the scene, pipeline level
def test_span_sections_against_the_reference(cuda):
    r = sn.reference()
    X, kind = cc.tree_scene()
    points = _dev(X, cuda)
    spans = pipeline.conductor_spans(points, rule=dict(sc.SCENE_RULE), towers=sp.line_towers())
    out = pipeline.span_sections(points, spans, stations=sn.STATIONS, half_width=sn.HALF, depth=sn.DEPTH,
                                 limit=sn.LIMIT, towers=sp.line_towers(), cut_radius=9.0)
    K, idx = r["spans"]["nclusters"], r["idx"]
    assert np.array_equal(out["pieces"].cpu().numpy(), idx)
    # the pipeline's own curves through the statement: every tensor is equal
    curves = ops.span_curves(spans["table"], spans["frames"], spans["ext"])[out["pieces"]].cpu().numpy()
    near = pipeline._near_towers(points, sp.line_towers(), 9.0)
    skip = (spans["wire"] | near).cpu().numpy().astype(np.uint8)
    assert np.array_equal(skip, r["skip"])
    want = sn.section_reference(X, curves, sn.STATIONS, sn.HALF, sn.DEPTH, sn.LIMIT, skip=skip)
    got = {key: out[key].cpu().numpy() for key in ("count", "violations", "min_row", "v", "station")}
    got["min_v"] = out["min_vertical"].cpu().numpy()
    got["span"] = out["span"].cpu().numpy()
    want["span"] = np.where(want["span"] >= 0, idx[np.maximum(want["span"], 0)], -1).astype(np.int32)
    _same(got, want, "pipeline")
    has = want["min_row"] >= 0
    top = out["top"].cpu().numpy()
    assert np.array_equal(top[has], X[want["min_row"][has]]) and np.isnan(top[~has]).all()
    # against the host's curves: the same rows in the same cells wherever a row stands clear of a decision
    clear = r["margin"] > 10.0 * r["tol"] + 1e-6                               # (a skipped row's margin is +inf)
    assert clear[r["skip"] == 0].sum() > 0.99 * (r["skip"] == 0).sum()
    assert np.array_equal(got["station"][clear], r["station"][clear])
    assert np.array_equal(np.where(got["span"] >= 0, 1, 0)[clear], np.where(r["span"] >= 0, 1, 0)[clear])
    # the centres, the wire over them and the table
    B = sn.STATIONS
    m0, m1 = curves[:, 8:9], curves[:, 9:10]
    m = m0 + (np.arange(B)[None, :] + 0.5) * ((m1 - m0) / B)
    assert np.array_equal(out["m"].cpu().numpy(), m)
    assert np.allclose(out["xy"].cpu().numpy()[:, :, 0], curves[:, 0:1] + m * curves[:, 3:4], rtol=0, atol=1e-9)
    wire_z = curves[:, 2:3] + curves[:, 5:6] + m * (curves[:, 6:7] + curves[:, 7:8] * m)
    assert np.allclose(out["wire_z"].cpu().numpy(), wire_z, rtol=0, atol=1e-9)
    assert torch.isnan(out["ground"]).all() and out["ground"].shape == (len(idx), B)
    T = {key: v.cpu().numpy() for key, v in out["table"].items()}
    assert tuple(T) == pipeline.SECTION_TABLE_KEYS and all(len(v) == K for v in T.values())
    rest = np.setdiff1d(np.arange(K), idx)
    assert np.array_equal(T["count"][idx], want["count"].sum(axis=1))
    assert np.array_equal(T["violations"][idx], want["violations"].sum(axis=1))
    assert np.array_equal(T["min_vertical"][idx], want["min_v"].min(axis=1))
    assert np.array_equal(T["min_station"][idx], np.where(np.isfinite(want["min_v"].min(axis=1)),
                                                          want["min_v"].argmin(axis=1), -1))
    some = T["min_row"][idx] >= 0
    assert np.array_equal(T["min_row"][idx][some], want["min_row"][np.arange(len(idx)), want["min_v"].argmin(axis=1)][some])
    assert np.array_equal(T["min_point"][idx][some], X[T["min_row"][idx][some]])
    assert (T["count"][rest] == 0).all() and (T["min_row"][rest] == -1).all() and np.isnan(T["min_point"][rest]).all()
    # the breach tree: station 40 of the first span, top 17.0 m, 4.5 m below the middle wire: its cell violates at the
    # scene's limit of 7 m and the cell's highest return is one of the tree's rows
    breach = np.flatnonzero(kind == 10)
    assert (got["span"][breach] >= 0).all()
    apex = breach[np.argmin(got["v"][breach])]
    p, j = int(np.searchsorted(idx, got["span"][apex])), int(got["station"][apex])
    assert got["violations"][p, j] > 0 and kind[got["min_row"][p, j]] == 10 and 4.0 < got["min_v"][p, j] < 5.0
    a = np.radians(sp.LINE_AZIMUTH_DEG)
    xy = out["xy"].cpu().numpy()
    assert abs((xy[p, j, 0] * np.cos(a) + xy[p, j, 1] * np.sin(a)) - 40.0) < 0.5 * 70.0 / B + 0.3   # half a station
    # the near tree stands at lateral -6 m of the second span: inside the 15 m corridor of all its three phases, outside
    # the 5 m corridor of the phase at +6 m, whose cells it leaves
    narrow = pipeline.span_sections(points, spans, stations=sn.STATIONS, half_width=5.0, depth=sn.DEPTH, limit=sn.LIMIT,
                                    towers=sp.line_towers(), cut_radius=9.0)
    thin = sn.section_reference(X, curves, sn.STATIONS, 5.0, sn.DEPTH, sn.LIMIT, skip=skip)
    for key, name in (("count", "count"), ("violations", "violations"), ("min_v", "min_vertical"), ("min_row", "min_row"),
                      ("v", "v"), ("station", "station")):
        assert np.array_equal(_bits(narrow[name].cpu().numpy()), _bits(thin[key])), key
    tree = kind == 11
    lateral = -curves[:, 0] * np.sin(a) + curves[:, 1] * np.cos(a)
    along = curves[:, 0] * np.cos(a) + curves[:, 1] * np.sin(a)
    second = np.flatnonzero(along > 80.0)
    assert len(second) == 3
    far = int(second[np.argmax(lateral[second])])
    assert abs(lateral[far] - 6.0) < 0.2
    for f in second:
        assert sn.span_pairs(X, curves[f], sn.STATIONS, sn.HALF, sn.DEPTH)[0][tree].all()
    wide_far, _, cells = sn.span_pairs(X, curves[far], sn.STATIONS, sn.HALF, sn.DEPTH)
    assert not sn.span_pairs(X, curves[far], sn.STATIONS, 5.0, sn.DEPTH)[0][tree].any()
    cells = np.unique(cells[tree])
    lost = got["count"][far, cells].sum() - thin["count"][far, cells].sum()
    assert lost >= tree.sum() and (narrow["span"].cpu().numpy()[tree] >= 0).all()   # still under its own phase
    # with a terrain model of the same rows and a ground sheet the ground under the stations is finite
    rng = np.random.default_rng(1)
    sheet = np.concatenate([sp._line_xy(rng.uniform(-15.0, 165.0, 20000), rng.uniform(-30.0, 30.0, 20000)),
                            rng.uniform(0.0, 0.2, (20000, 1))], axis=1).astype(np.float32)
    terrain = pipeline.terrain_model(_dev(np.vstack([X, sheet]), cuda))
    with_ground = pipeline.span_sections(points, spans, terrain=terrain, stations=sn.STATIONS, half_width=sn.HALF,
                                         depth=sn.DEPTH, limit=sn.LIMIT, towers=sp.line_towers(), cut_radius=9.0)
    g = with_ground["ground"].cpu().numpy()
    assert np.isfinite(g).all() and (np.abs(g) < 1.0).all() and (out["wire_z"].cpu().numpy() - g > 10.0).all()
    assert torch.equal(with_ground["count"], out["count"])
    # no accepted piece: an empty result, nothing raised
    none = dict(spans, accepted=torch.zeros_like(spans["accepted"]))
    empty = pipeline.span_sections(points, none, towers=sp.line_towers())
    assert empty["pieces"].numel() == 0 and empty["count"].shape == (0, 64) and empty["top"].shape == (0, 64, 3)
    assert (empty["span"] == -1).all() and torch.isinf(empty["v"]).all() and (empty["table"]["count"] == 0).all()
    with pytest.raises(ValueError):
        pipeline.span_sections(points, spans, stations=129)


# ------------------------------------------------------------------ drop-in
def test_drop_in_knob_writes_the_section_table(cuda, tmp_path, monkeypatch):
    from pointcloudhookup_amd.utils import tower_extraction as te
    X, _ = cc.tree_scene()
    rng = np.random.default_rng(1)
    sheet = np.concatenate([sp._line_xy(rng.uniform(-15.0, 165.0, 20000), rng.uniform(-30.0, 30.0, 20000)),
                            rng.uniform(0.0, 0.2, (20000, 1))], axis=1).astype(np.float32)
    lifted = X.copy()
    lifted[:, 2] += np.float32(3.5)
    raw = np.vstack([lifted, sheet])
    scales, offsets = np.array([0.001, 0.001, 0.001]), np.array([0.0, 0.0, 0.0])
    path = str(tmp_path / "line.las")
    las_bytes.build(path, np.round(raw.astype(np.float64) / scales).astype(np.int32), scales=scales, offsets=offsets)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(te, "OBB_MODE", "upright")
    monkeypatch.setattr(te, "DROP_LINEAR", te.drop_linear_from_env("2,0.9,0.5,10"))
    monkeypatch.setattr(te, "SPANS", te.spans_from_env("1,5,9,20"))

    def run():
        logs = []
        return te.extract_towers(path, log_callback=logs.append, min_points=20), logs

    assert te.SECTION is None
    off, off_logs = run()
    table = tmp_path / "output_towers" / "section_info.csv"
    assert len(off) == 3 and not table.exists()
    monkeypatch.setattr(te, "SECTION", te.section_from_env("15,7,32,80", spans=True))
    on, logs = run()
    extra = [m for m in logs if "导线断面" in m]
    assert len(extra) == 1 and "越限区段" in extra[0], extra
    assert [m for m in logs if "导线断面" not in m] == off_logs
    assert len(on) == len(off)
    for a, b in zip(on, off):                                                  # the tower dicts are the same
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    with open(table, newline="", encoding="utf-8") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == te.SECTION_COLUMNS and len(lines) == 1 + 6 * 32  # one line per accepted piece and station
    col = {name: np.array([float(v[i]) for v in lines[1:]]) for i, name in enumerate(te.SECTION_COLUMNS) if i}
    assert np.isnan(col["ground_z"]).all()                                     # no terrain knob: no ground
    assert sorted(set(col["station"].tolist())) == list(range(32))
    breached = np.flatnonzero(col["violations"] > 0)
    assert f"越限区段 {len(breached)}/{6 * 32}" in extra[0] and len(breached) >= 1
    # the breach tree stands at station 40, lateral 0: the violating cells lie there and their highest return is the tree's
    a = np.radians(sp.LINE_AZIMUTH_DEG)
    station = col["x"] * np.cos(a) + col["y"] * np.sin(a)
    top_station = col["top_x"] * np.cos(a) + col["top_y"] * np.sin(a)
    top_lateral = -col["top_x"] * np.sin(a) + col["top_y"] * np.cos(a)
    worst = int(np.argmin(col["min_vertical"]))
    assert worst in breached and abs(station[worst] - 40.0) < 3.0
    assert abs(top_station[worst] - 40.0) < 2.1 and abs(top_lateral[worst]) < 2.1
    assert abs(col["top_z"][worst] - (17.0 + 3.5)) < 0.5 and abs(col["min_vertical"][worst] - 4.5) < 0.5
    assert (col["wire_z"] - col["top_z"])[col["count"] > 0].min() > 0.0
    # with the terrain knob the ground under the stations is the model's, in world coordinates: the sheet at z = 0 .. 0.2
    monkeypatch.setattr(te, "TERRAIN", te.terrain_from_env("1,12,0.5,7", spans=True))
    run()
    with open(table, newline="", encoding="utf-8") as f:
        lines = list(csv.reader(f))
    ground = {name: np.array([float(v[i]) for v in lines[1:]]) for i, name in enumerate(te.SECTION_COLUMNS) if i}
    assert len(lines) == 1 + 6 * 32 and np.isfinite(ground["ground_z"]).all()
    assert (np.abs(ground["ground_z"]) < 1.0).all() and (ground["wire_z"] - ground["ground_z"] > 10.0).all()
    for name in ("count", "violations", "min_vertical", "wire_z"):
        assert np.array_equal(ground[name], col[name]), name
    monkeypatch.setattr(te, "TERRAIN", None)
    monkeypatch.setattr(te, "SECTION", None)
    again, again_logs = run()
    assert again_logs == off_logs and len(again) == 3
