"""Conductor clearance on the device (pch_clearance_f32, ops.clearance, pipeline.conductor_clearance, the drop-in's
PCH_CLEARANCE): the reference's curve and segment tables are fed to the kernel, so every output must equal the numpy
statement of the rule (clearance_cases) bit for bit - whatever the sweep culls."""
import csv

import numpy as np
import pytest
import torch

import clearance_cases as cc
import las_bytes
import shape_cases as sc
import span_cases as sp
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

TILE = ops.CLEARANCE_TILE
EPSG = np.array([437000.0, 3139000.0, 80.0])


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(cuda)


def _case(n, K, seed, shift=None, spread=120.0):
    """(X float32 [n,3], curves float64 [K,10]): K random sagging spans in a square of ``spread`` metres and n rows, seven
    in ten of them scattered around a span (beyond its ends, beside and below it), the others anywhere"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-0.5 * np.pi, 0.5 * np.pi, K)
    half = rng.uniform(10.0, 35.0, K)
    C = np.stack([rng.uniform(0.0, spread, K), rng.uniform(0.0, spread, K), rng.uniform(15.0, 30.0, K), np.cos(ang),
                  np.sin(ang), rng.uniform(-0.5, 0.5, K), rng.uniform(-0.1, 0.1, K), rng.uniform(0.0, 0.004, K),
                  -half * rng.uniform(0.8, 1.0, K), half], axis=1).reshape(K, 10)
    X = np.concatenate([rng.uniform(-20.0, spread + 20.0, (n, 2)), rng.uniform(0.0, 40.0, (n, 1))], axis=1)
    if K:
        k = rng.integers(0, K, n)
        m = rng.uniform(C[k, 8] - 15.0, C[k, 9] + 15.0)
        t = rng.normal(0.0, 6.0, n)
        z = C[k, 2] + C[k, 5] + m * (C[k, 6] + C[k, 7] * m) - rng.uniform(-3.0, 14.0, n)
        near = np.stack([C[k, 0] + m * C[k, 3] - t * C[k, 4], C[k, 1] + m * C[k, 4] + t * C[k, 3], z], axis=1)
        X = np.where((rng.uniform(0.0, 1.0, n) < 0.7)[:, None], near, X)
    if shift is not None:
        X = X + shift
        C[:, 0:3] += shift
    return X.astype(np.float32), C


def _run(X, C, segs, cuda, radius=cc.RADIUS, limit=cc.LIMIT, skip=None, want_stats=False):
    out = ops.clearance(_dev(X, cuda), _dev(C, cuda), _dev(segs, cuda), radius, limit,
                        skip=None if skip is None else _dev(skip, cuda), want_stats=want_stats)
    return {key: v.cpu().numpy() for key, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want, what):
    for key in cc.OUTPUTS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        if not np.array_equal(_bits(got[key]), _bits(want[key])):
            bad = np.flatnonzero(got[key] != want[key])
            raise AssertionError((what, key, len(bad), bad[:5], got[key][bad[:5]], want[key][bad[:5]]))


def _check(X, C, S, cuda, what, radius=cc.RADIUS, limit=cc.LIMIT, skip=None):
    segs, _ = cc.segments_reference(C, S)
    want = cc.clearance_reference(X, C, segs, radius, limit, skip=skip)
    got = _run(X, C, segs, cuda, radius, limit, skip=skip)
    _same(got, want, what)
    return got, want


# ------------------------------------------------------------------ rows, spans, segments
@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_row_span_and_segment_counts(cuda, n):
    hits = 0
    for K in (0, 1, 64, 65):
        X, C = _case(n, K, seed=100 + K)
        for S in (1, 2, 32, 128):
            _, want = _check(X, C, S, cuda, (n, K, S))
            hits += int((want["span"] >= 0).sum())
            if K == 0:
                assert (want["span"] == -1).all() and np.isinf(want["dist2"]).all() and want["count"].shape == (0,)
    assert hits > 0 or n == 1


def test_several_tiles_and_a_wide_radius(cuda):
    X, C = _case(5 * TILE + 17, 65, seed=7)
    got, want = _check(X, C, 32, cuda, "five tiles")
    assert (want["count"] > 0).sum() > 40 and want["violations"].sum() > 100
    _check(X, C, 5, cuda, "five tiles, radius 60", radius=60.0, limit=59.0)
    _check(X, C, 5, cuda, "five tiles, radius 1 mm", radius=1e-3, limit=1e-3)


# ------------------------------------------------------------------ thresholds and ties
@pytest.mark.parametrize("which", ["radius", "limit"])
def test_a_row_exactly_at_the_threshold_is_inside_and_the_next_float_is_not(cuda, which):
    """a level span along x and rows straight above one of its vertices: d2 is the height squared, exactly"""
    C = cc.curve(m0=-8.0, m1=8.0).reshape(1, 10)
    h = np.float32(10.0 if which == "radius" else 6.0)
    up = np.nextafter(h, np.float32(np.inf))
    X = np.array([[1.0, 0.0, h], [1.0, 0.0, up], [1.0, 0.0, -h], [1.0, 0.0, -up]], dtype=np.float32)
    got, _ = _check(X, C, 32, cuda, which)
    at, above = float(h) * float(h), float(up) * float(up)
    if which == "radius":
        assert got["span"].tolist() == [0, -1, 0, -1] and got["dist2"][0] == at == got["dist2"][2]
        assert np.isinf(got["dist2"][[1, 3]]).all() and got["count"][0] == 2 and got["violations"][0] == 0
    else:
        assert got["span"].tolist() == [0, 0, 0, 0] and got["dist2"].tolist() == [at, above, at, above]
        assert got["count"][0] == 4 and got["violations"][0] == 2             # dist2 <= l2 holds at the limit only
    assert got["min_row"][0] == 0


def test_ties_between_spans_go_to_the_lowest_index(cuda):
    one = cc.curve(cx=3.0, cy=-2.0, cz=20.0, ux=0.8, uy=0.6, a=0.3, b=0.01, c=0.002, m0=-20.0, m1=25.0)
    rng = np.random.default_rng(3)
    m, t = rng.uniform(-30.0, 35.0, 300), rng.normal(0.0, 5.0, 300)
    X = np.stack([3.0 + m * 0.8 - t * 0.6, -2.0 + m * 0.6 + t * 0.8, 20.0 - rng.uniform(-3.0, 9.0, 300)],
                 axis=1).astype(np.float32)
    got, _ = _check(X, np.stack([one, one]), 32, cuda, "two identical spans")
    assert (got["span"] <= 0).all() and (got["span"] == 0).sum() > 50 and got["count"][1] == 0
    assert got["min_row"][1] == -1 and np.isinf(got["min_dist2"][1])
    # midway between two parallel spans with ux = 1: t = -3 and +3, the same m and w, hence the same d2
    pair = np.stack([cc.curve(cy=3.0, cz=5.0, m0=-30.0, m1=30.0), cc.curve(cy=-3.0, cz=5.0, m0=-30.0, m1=30.0)])
    Y = np.stack([np.linspace(-35.0, 35.0, 141), np.zeros(141), np.linspace(0.0, 9.0, 141)], axis=1).astype(np.float32)
    got, _ = _check(Y, pair, 32, cuda, "midway")
    assert (got["span"] == 0).sum() > 100 and (got["span"] != 1).all() and got["count"].tolist()[1] == 0
    got, _ = _check(Y, pair[::-1].copy(), 32, cuda, "midway, the table reversed")
    assert (got["span"] != 1).all()


# ------------------------------------------------------------------ geometry
def test_rows_beyond_both_ends_and_the_end_vertices(cuda):
    C = cc.curve(cx=1.0, cy=2.0, cz=10.0, ux=0.6, uy=0.8, a=0.5, b=0.05, c=0.01, m0=-8.0, m1=12.0).reshape(1, 10)
    m = np.concatenate([np.linspace(-17.0, -8.0, 40), [-8.0, 12.0], np.linspace(12.0, 21.0, 40)])
    z0, z1 = 0.5 + -8.0 * (0.05 + 0.01 * -8.0), 0.5 + 12.0 * (0.05 + 0.01 * 12.0)
    rows = []
    for t in (-4.0, 0.0, 2.5):
        for dz in (-3.0, 0.0, 3.0):
            w = np.where(m < 2.0, z0, z1) + dz
            rows.append(np.stack([1.0 + m * 0.6 - t * 0.8, 2.0 + m * 0.8 + t * 0.6, 10.0 + w], axis=1))
    X = np.vstack(rows).astype(np.float32)
    for S in (1, 3, 32):
        got, _ = _check(X, C, S, cuda, ("beyond the ends", S))
        # the statement in space agrees; a metre and a half beyond an end the answer is the distance to the end vertex
        # (both clamp branches)
        P = X.astype(np.float64)
        hit = got["span"] == 0
        dist = np.sqrt(got["dist2"])
        assert hit.sum() > 300 and np.abs(dist - cc.polyline_distance(P, cc.polyline_world(C, S)[0]))[hit].max() < 1e-12
        ends = cc.polyline_world(C, 1)[0]
        mm = np.tile(m, 9)
        for end, side in ((ends[0], mm < -9.5), (ends[1], mm > 13.5)):
            assert (hit & side).sum() > 100
            assert np.abs(dist - np.linalg.norm(P - end, axis=1))[hit & side].max() < 1e-12


def test_rows_above_a_deep_parabola_where_two_segments_compete(cuda):
    C = cc.curve(cz=0.0, c=0.5, m0=-4.0, m1=4.0).reshape(1, 10)
    x = np.linspace(-1.5, 1.5, 61)
    X = np.concatenate([np.stack([x, np.full(61, t), np.full(61, z)], axis=1) for t in (0.0, 0.5) for z in (3.0, 6.0, 9.0)])
    for S in (2, 8, 32):
        got, _ = _check(X.astype(np.float32), C, S, cuda, ("deep parabola", S), radius=8.0, limit=4.0)
        assert (got["span"] == 0).sum() > 200
    mid = np.array([[0.0, 0.0, 6.0]], dtype=np.float32)                        # on the axis: both arms are equally near
    got, _ = _check(mid, C, 8, cuda, "on the axis", radius=8.0, limit=4.0)
    V = cc.polyline_world(C, 8)[0]
    assert abs(np.sqrt(got["dist2"][0]) - cc.polyline_distance(mid.astype(np.float64), V)[0]) < 1e-12


def test_a_span_without_length_is_a_point(cuda):
    C = np.stack([cc.curve(a=1.0, b=0.5, m0=2.0, m1=2.0)])                     # the point (2, 0, 2)
    X = np.array([[2.0, 0.0, 5.0], [6.0, 0.0, 2.0], [2.0, -3.0, 6.0], [2.0, 0.0, 2.0], [20.0, 0.0, 2.0]], dtype=np.float32)
    for S in (1, 4, 128):
        segs, _ = cc.segments_reference(C, S)
        assert (segs[0, :, 4] == 0).all()
        got, _ = _check(X, C, S, cuda, ("point", S))
        assert got["dist2"].tolist() == [9.0, 16.0, 25.0, 0.0, np.inf] and got["min_row"][0] == 3


# ------------------------------------------------------------------ spans that do not take part
def test_a_span_with_a_nan_takes_no_part_and_changes_no_bit_of_the_others(cuda):
    X, C = _case(2 * TILE + 5, 9, seed=21)
    segs, _ = cc.segments_reference(C, 32)
    clean = _run(X, C, segs, cuda)
    for where in ("coefficient", "centre", "segment", "inv"):
        D, dsegs = np.insert(C, 4, C[2], axis=0), np.insert(segs, 4, segs[2], axis=0)
        if where == "coefficient":
            D[4, 7] = np.nan
            dsegs, _ = cc.segments_reference(D, 32)                             # every z of that span is NaN
        elif where == "centre":
            D[4, 1] = np.inf
        elif where == "segment":
            dsegs[4, 17, 3] = np.nan
        else:
            dsegs[4, 31, 4] = -np.inf
        got = _run(X, D, dsegs, cuda)
        _same(got, cc.clearance_reference(X, D, dsegs, cc.RADIUS, cc.LIMIT), where)
        assert (got["span"] != 4).all() and got["count"][4] == 0 and got["min_row"][4] == -1
        keep = np.array([0, 1, 2, 3, 5, 6, 7, 8, 9])
        moved = np.where(got["span"] > 4, got["span"] - 1, got["span"])
        assert np.array_equal(moved, clean["span"]) and np.array_equal(_bits(got["dist2"]), _bits(clean["dist2"]))
        for key in ("count", "violations", "min_dist2", "min_row"):
            assert np.array_equal(_bits(got[key][keep]), _bits(clean[key])), (where, key)


def test_a_span_whose_direction_is_not_unit_is_never_culled(cuda):
    X, C = _case(3 * TILE, 6, seed=33, spread=4000.0)
    X = X[np.argsort(X[:, 0], kind="stable")]                                  # sorted: tight tile boxes
    C[1, 3:5] *= 1.5                                                           # stretches m and t by 1.5
    C[4, 3:5] *= 0.5
    C[5, 3:5] *= 1.0 + 1e-5                                                  # beyond the bounds' assumption
    far = X.copy()
    far[:, 0] += np.float32(9000.0)                                            # rows the true bounds would never meet
    for rows, what in ((X, "near"), (np.vstack([far, X]), "far and near")):
        got, want = _check(rows, C, 16, cuda, what, radius=25.0, limit=10.0)
    assert (want["count"][[1, 4, 5]] > 0).all()


# ------------------------------------------------------------------ culling stress
def test_two_hundred_short_spans_in_random_and_in_sorted_row_order(cuda):
    rng = np.random.default_rng(44)
    n, K = 8 * TILE, 200
    X, C = _case(n, K, seed=45, spread=10000.0)
    C[:, 8], C[:, 9] = -rng.uniform(2.0, 6.0, K), rng.uniform(2.0, 6.0, K)
    k = rng.integers(0, K, n)
    m, t = rng.uniform(-12.0, 12.0, n), rng.normal(0.0, 5.0, n)
    near = np.stack([C[k, 0] + m * C[k, 3] - t * C[k, 4], C[k, 1] + m * C[k, 4] + t * C[k, 3],
                     C[k, 2] - rng.uniform(-2.0, 9.0, n)], axis=1).astype(np.float32)
    X = np.where((rng.uniform(0.0, 1.0, n) < 0.8)[:, None], near, X)
    X = X[rng.permutation(n)]
    segs, _ = cc.segments_reference(C, 32)
    want = cc.clearance_reference(X, C, segs, cc.RADIUS, cc.LIMIT)
    assert (want["count"] > 0).sum() > 150 and want["violations"].sum() > 1000
    shuffled = _run(X, C, segs, cuda, want_stats=True)
    _same(shuffled, want, "random order")
    order = np.lexsort((X[:, 1], X[:, 0]))
    ordered = _run(X[order], C, segs, cuda, want_stats=True)
    assert np.array_equal(_bits(ordered["dist2"]), _bits(want["dist2"][order]))
    assert np.array_equal(ordered["span"], want["span"][order])
    for key in ("count", "violations", "min_dist2"):
        assert np.array_equal(_bits(ordered[key]), _bits(want[key])), key
    back = np.where(ordered["min_row"] >= 0, order[np.maximum(ordered["min_row"], 0)], -1)
    has = want["min_row"] >= 0
    assert np.array_equal(back >= 0, has)
    assert np.array_equal(X[back[has]], X[want["min_row"][has]])               # the same point, wherever it sits
    # every tile of the shuffled cloud covers all but the outermost spans; sorted, most spans are culled and the answer
    # is the same
    tiles = n // TILE
    print(f"(tile, span) pairs walked: {shuffled['loops'][1]} shuffled, {ordered['loops'][1]} sorted of {tiles * K}; "
          f"segment loops run: {shuffled['loops'][0]} and {ordered['loops'][0]} of {n * K} (row, span) pairs")
    assert shuffled["loops"][1] > 0.9 * tiles * K and ordered["loops"][1] < tiles * K // 4
    assert shuffled["loops"][0] < n * K // 20                                  # the per-row tests stop the others


# ------------------------------------------------------------------ mask and rows
def test_skip_mask_with_a_tile_that_is_skipped_entirely(cuda):
    X, C = _case(3 * TILE + 100, 12, seed=51)
    rng = np.random.default_rng(52)
    skip = (rng.uniform(0.0, 1.0, len(X)) < 0.2).astype(np.uint8)
    skip[TILE:2 * TILE] = 1
    skip[5] = 255
    got, want = _check(X, C, 32, cuda, "skip", skip=skip)
    assert (got["span"][skip != 0] == -1).all() and np.isinf(got["dist2"][skip != 0]).all()
    assert (got["span"][:TILE] >= 0).sum() > 100
    none = _run(X, C, cc.segments_reference(C, 32)[0], cuda, skip=np.zeros(len(X), dtype=np.uint8))
    _same(none, cc.clearance_reference(X, C, cc.segments_reference(C, 32)[0], cc.RADIUS, cc.LIMIT), "all-zero mask")
    out = ops.clearance(_dev(X, cuda), _dev(C, cuda), _dev(cc.segments_reference(C, 32)[0], cuda), cc.RADIUS, cc.LIMIT,
                        skip=_dev(skip != 0, cuda))                            # a bool mask is taken as it is
    assert np.array_equal(out["span"].cpu().numpy(), want["span"])
    everything = _run(X, C, cc.segments_reference(C, 32)[0], cuda, skip=np.ones(len(X), dtype=np.uint8))
    assert (everything["span"] == -1).all() and (everything["count"] == 0).all()
    assert (everything["min_row"] == -1).all() and np.isinf(everything["min_dist2"]).all()


def test_nonfinite_rows_get_nothing(cuda):
    X, C = _case(TILE + 40, 8, seed=61)
    bad = {3: (0, np.nan), 64: (1, np.inf), 65: (2, -np.inf), 700: (0, np.inf), TILE - 1: (2, np.nan), TILE: (1, np.nan),
           TILE + 39: (0, -np.inf)}
    for i, (axis, v) in bad.items():
        X[i, axis] = v
    X[701] = np.nan
    got, _ = _check(X, C, 32, cuda, "non-finite rows")
    rows = sorted(bad) + [701]
    assert (got["span"][rows] == -1).all() and np.isinf(got["dist2"][rows]).all() and (got["span"] >= 0).sum() > 300
    allbad = np.full((TILE + 3, 3), np.nan, dtype=np.float32)                  # a tile without a finite row
    _check(allbad, C, 32, cuda, "no finite row")


def test_coordinates_at_projected_scale(cuda):
    X, C = _case(2 * TILE + 9, 20, seed=71, shift=EPSG)
    got, want = _check(X, C, 32, cuda, "EPSG scale")
    assert (want["span"] >= 0).sum() > 500 and want["violations"].sum() > 50


def test_duplicate_rows_at_the_minimum_give_the_lowest_row(cuda):
    X, C = _case(2 * TILE, 5, seed=81)
    segs, _ = cc.segments_reference(C, 32)
    first = cc.clearance_reference(X, C, segs, cc.RADIUS, cc.LIMIT)
    k = int(np.argmax(first["count"]))
    p = X[first["min_row"][k]].copy()
    for i in (TILE + 300, 17, TILE - 1, 900):
        X[i] = p
    got, want = _check(X, C, 32, cuda, "duplicates")
    assert got["min_row"][k] == min(17, int(first["min_row"][k])) and want["min_dist2"][k] == first["min_dist2"][k]


# ------------------------------------------------------------------ call level
def test_the_same_call_twice_gives_the_same_bits(cuda):
    X, C = _case(4 * TILE + 1, 65, seed=91, shift=EPSG)
    segs, _ = cc.segments_reference(C, 32)
    a, b = _run(X, C, segs, cuda), _run(X, C, segs, cuda)
    for key in cc.OUTPUTS:
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key


def test_refusals(cuda):
    X, C = _case(100, 3, seed=95)
    segs, _ = cc.segments_reference(C, 4)
    dX, dC, dS = _dev(X, cuda), _dev(C, cuda), _dev(segs, cuda)
    for radius, limit in ((np.nan, 1.0), (np.inf, 1.0), (10.0, np.nan), (10.0, np.inf), (0.0, 0.0), (-1.0, -2.0),
                          (10.0, 0.0), (10.0, -1.0), (5.0, 6.0)):
        with pytest.raises(ValueError):
            ops.clearance(dX, dC, dS, radius, limit)
    with pytest.raises(ValueError):
        ops.clearance(dX, dC, _dev(np.zeros((3, 129, 5)), cuda), 10.0, 6.0)
    with pytest.raises(ValueError):
        ops.clearance(dX, dC, _dev(np.zeros((3, 0, 5)), cuda), 10.0, 6.0)
    with pytest.raises(ValueError):
        ops.clearance(dX, _dev(np.zeros((4097, 10)), cuda), _dev(np.zeros((4097, 1, 5)), cuda), 10.0, 6.0)
    with pytest.raises(ValueError):
        ops.clearance(dX, dC, dS[:2], 10.0, 6.0)
    with pytest.raises(ValueError):
        ops.clearance(dX, dC, dS, 10.0, 6.0, skip=torch.zeros(99, dtype=torch.uint8, device=cuda))
    with pytest.raises(TypeError):
        ops.clearance(torch.from_numpy(X), dC, dS, 10.0, 6.0)
    with pytest.raises(TypeError):
        ops.clearance(dX.double(), dC, dS, 10.0, 6.0)
    with pytest.raises(TypeError):
        ops.span_segments(torch.from_numpy(C), 4)
    with pytest.raises(ValueError):
        ops.span_segments(dC, 129)
    with pytest.raises(TypeError):
        pipeline.conductor_clearance(torch.from_numpy(X), {})
    ok = ops.clearance(dX, dC[:, :5].contiguous(), dS, 10.0, 10.0)             # [K,5] curves, limit == radius
    assert np.array_equal(ok["count"].cpu().numpy(), ok["violations"].cpu().numpy())


def test_the_raw_c_abi(cuda):
    L = _lib.lib()
    X, C = _case(TILE + 7, 4, seed=97)
    n, K, S = len(X), 4, 8
    segs, _ = cc.segments_reference(C, S)
    want = cc.clearance_reference(X, C, segs, 10.0, 6.0)
    dX, dC, dS = _dev(X, cuda), _dev(C[:, :5], cuda), _dev(segs, cuda)
    d2 = torch.full((n,), -1.0, dtype=torch.float64, device=cuda)
    span = torch.full((n,), 7, dtype=torch.int32, device=cuda)
    tab = [torch.full((K,), 7, dtype=dt, device=cuda) for dt in (torch.int64, torch.int64, torch.float64, torch.int64)]
    need = L.pch_clearance_ws_bytes(n, K, S)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def call(xyz=None, nn=n, kk=K, ss=S, radius=10.0, limit=6.0, out=None, cnt=None, wsp=None, wb=None, curves=None):
        return L.pch_clearance_f32(p(dX) if xyz is None else xyz, 0, nn, p(dC) if curves is None else curves, p(dS), kk,
                                   ss, radius, limit, p(d2) if out is None else out, p(span),
                                   p(tab[0]) if cnt is None else cnt, p(tab[1]), p(tab[2]), p(tab[3]), 0,
                                   p(ws) if wsp is None else wsp, need if wb is None else wb, st)

    assert call() == 0
    got = dict(dist2=d2, span=span, count=tab[0], violations=tab[1], min_dist2=tab[2], min_row=tab[3])
    _same({key: v.cpu().numpy() for key, v in got.items()}, want, "raw")
    before = [t.clone() for t in got.values()]
    assert call(wb=need - 1) == -2 and b"workspace" in L.pch_last_error()      # PCH_ERR_WORKSPACE
    host = np.zeros(n, dtype=np.float64)
    for rc in (call(nn=-1), call(nn=2 ** 32), call(kk=-1), call(kk=4097), call(ss=0), call(ss=129),
               call(radius=float("nan")), call(limit=float("inf")), call(limit=0.0), call(limit=10.5), call(radius=-1.0),
               call(xyz=0), call(out=0), call(cnt=0), call(curves=0), call(wsp=0), call(wsp=host.ctypes.data)):
        assert rc == -1                                                        # PCH_ERR_ARG
    torch.cuda.synchronize()
    for t, b in zip(got.values(), before):
        assert torch.equal(t, b)                                               # a refused call writes nothing
    # no span: every row +inf / -1 and no table, without a pointer to read; no row: an empty table per span
    assert L.pch_clearance_f32(p(dX), 0, n, 0, 0, 0, S, 10.0, 6.0, p(d2), p(span), 0, 0, 0, 0, 0, p(ws), need, st) == 0
    assert L.pch_clearance_f32(0, 0, 0, p(dC), p(dS), K, S, 10.0, 6.0, 0, 0, p(tab[0]), p(tab[1]), p(tab[2]), p(tab[3]),
                               0, p(ws), need, st) == 0
    assert L.pch_clearance_f32(0, 0, 0, 0, 0, 0, S, 10.0, 6.0, 0, 0, 0, 0, 0, 0, 0, p(ws), need, st) == 0
    torch.cuda.synchronize()
    assert torch.isinf(d2).all() and (span == -1).all()
    assert (tab[0] == 0).all() and (tab[1] == 0).all() and torch.isinf(tab[2]).all() and (tab[3] == -1).all()


# ------------------------------------------------------------------ pipeline level
def test_conductor_clearance_against_the_reference(cuda):
    r = cc.reference()
    X, kind = cc.tree_scene()
    points = _dev(X, cuda)
    spans = pipeline.conductor_spans(points, rule=dict(sc.SCENE_RULE), towers=sp.line_towers())
    assert {"frames", "ext"} <= set(spans)
    F, E = spans["frames"].cpu().numpy(), spans["ext"].cpu().numpy()
    assert np.abs(F - r["spans"]["frames"]).max() < 1e-6 and np.abs(E - r["spans"]["ext"]).max() < 1e-6
    out = pipeline.conductor_clearance(points, spans, radius=cc.RADIUS, limit=cc.LIMIT, segments=cc.SEGMENTS,
                                       towers=sp.line_towers(), cut_radius=9.0)
    K, idx = r["spans"]["nclusters"], r["idx"]
    span_ref = np.where(r["span"] >= 0, idx[np.maximum(r["span"], 0)], -1).astype(np.int32)
    assert np.array_equal(out["span"].cpu().numpy(), span_ref)
    assert np.array_equal(out["violating"].cpu().numpy(), r["dist2"] <= cc.LIMIT * cc.LIMIT)
    T = {key: v.cpu().numpy() for key, v in out["table"].items()}
    assert tuple(T) == pipeline.CLEARANCE_TABLE_KEYS and all(len(v) == K for v in T.values())
    rest = np.setdiff1d(np.arange(K), idx)
    assert np.array_equal(T["count"][idx], r["count"]) and np.array_equal(T["violations"][idx], r["violations"])
    assert np.array_equal(T["min_row"][idx], r["min_row"])
    assert (T["count"][rest] == 0).all() and (T["min_row"][rest] == -1).all() and np.isnan(T["chord_error"][rest]).all()
    tol = r["tol"]
    got, want = np.sqrt(out["dist2"].cpu().numpy()), np.sqrt(r["dist2"])
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    worst = float(np.abs(got[fin] - want[fin]).max())
    print(f"pipeline distances: worst difference {worst:.3e} m, tol {tol:.3e} m")
    assert worst <= tol
    has = r["count"] > 0
    assert np.abs(T["min_distance"][idx][has] - np.sqrt(r["min_dist2"][has])).max() <= tol
    assert np.isinf(T["min_distance"][idx][~has]).all() and np.isnan(T["min_point"][idx][~has]).all()
    assert np.array_equal(T["min_point"][idx][has], X[r["min_row"][has]])
    assert np.abs(T["chord_error"][idx] - r["chord"]).max() <= tol
    # no accepted piece: an empty result, nothing raised
    none = dict(spans, accepted=torch.zeros_like(spans["accepted"]))
    out = pipeline.conductor_clearance(points, none, towers=sp.line_towers())
    assert (out["span"] == -1).all() and not out["violating"].any() and (out["table"]["count"] == 0).all()
    blob = _dev(np.random.default_rng(2).normal(0.0, 1.5, (500, 3)).astype(np.float32), cuda)
    out = pipeline.conductor_clearance(blob, pipeline.conductor_spans(blob))
    assert out["span"].shape == (500,) and (out["span"] == -1).all() and out["table"]["count"].shape == (0,)


# ------------------------------------------------------------------ drop-in
def test_drop_in_knob_writes_the_clearance_table(cuda, tmp_path, monkeypatch):
    from pointcloudhookup_amd.utils import tower_extraction as te
    r = cc.reference()
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

    assert te.CLEARANCE is None
    off, off_logs = run()
    table = tmp_path / "output_towers" / "clearance_info.csv"
    assert len(off) == 3 and not table.exists()
    monkeypatch.setattr(te, "CLEARANCE", te.clearance_from_env("10,6,32", spans=True))
    on, logs = run()
    extra = [m for m in logs if "导线净空" in m]
    assert len(extra) == 1 and "越限线段 1/6" in extra[0], extra
    assert [m for m in logs if "导线净空" not in m] == off_logs
    assert len(on) == len(off)
    for a, b in zip(on, off):                                                  # the tower dicts are the same
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    with open(table, newline="", encoding="utf-8") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == te.CLEARANCE_COLUMNS and len(lines) == 1 + 6     # one line per accepted piece
    col = {name: np.array([float(v[i]) for v in lines[1:]]) for i, name in enumerate(te.CLEARANCE_COLUMNS) if i}
    # the file is the scene in millimetres, lifted: the counts may move by the few rows that sit a millimetre from a
    # threshold, the breached piece is the one above the breaching tree, as the scene says
    assert sorted(col["count"].tolist(), reverse=True)[3:] == [0.0, 0.0, 0.0]
    assert np.abs(np.sort(col["count"])[3:] - np.sort(r["count"])[3:]).max() <= 3
    breached = np.flatnonzero(col["violations"])
    assert len(breached) == 1 and abs(col["violations"][breached[0]] - r["violations"].max()) <= 3
    b = breached[0]
    assert abs(col["min_distance"][b] - np.sqrt(r["min_dist2"].min())) < 2e-3
    a = np.radians(sp.LINE_AZIMUTH_DEG)
    station = col["x"][b] * np.cos(a) + col["y"][b] * np.sin(a)
    lateral = -col["x"][b] * np.sin(a) + col["y"][b] * np.cos(a)
    assert abs(station - 40.0) < 2.1 and abs(lateral) < 2.1 and 11.0 + 3.5 <= col["z"][b] <= 17.0 + 3.5 + 0.01
    assert (col["chord_error"] > 1e-3).all() and (col["chord_error"] < 2e-3).all()
    monkeypatch.setattr(te, "CLEARANCE", None)
    again, again_logs = run()
    assert again_logs == off_logs and len(again) == 3
