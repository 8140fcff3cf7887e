"""Wind swing clearance on the device (pch_swing_clearance_f32, ops.swing_clearance, pipeline.wind_clearance, the
drop-in's PCH_WIND): the reference's head and segment tables are fed to the kernel, so all seven outputs must equal the
numpy statement of the rule (swing_cases) bit for bit - whatever the sweep culls."""
import csv

import numpy as np
import pytest
import torch

import clearance_cases as cc
import las_bytes
import shape_cases as sc
import span_cases as sp
import swing_cases as sw
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

TILE = ops.CLEARANCE_TILE
EPSG = np.array([437000.0, 3139000.0, 80.0])
RADIUS, LIMIT = 10.0, 6.0


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(cuda)


def _run(X, heads, segs, cuda, radius=RADIUS, limit=LIMIT, skip=None, want_stats=False):
    out = ops.swing_clearance(_dev(X, cuda), _dev(heads, cuda), _dev(segs, cuda), radius, limit,
                              skip=None if skip is None else _dev(skip, cuda), want_stats=want_stats)
    return {key: v.cpu().numpy() for key, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _differ(got, want, key):
    bad = np.flatnonzero((got[key] != want[key]) & ~(np.isnan(got[key].astype(np.float64))
                                                     & np.isnan(want[key].astype(np.float64))))
    return len(bad), bad[:5], got[key][bad[:5]], want[key][bad[:5]]


def _same(got, want, what):
    for key in sw.OUTPUTS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        if not np.array_equal(_bits(got[key]), _bits(want[key])):
            raise AssertionError((what, key) + _differ(got, want, key))


def _tables(C, deg, S):
    return sw.heads_reference(C, deg), sw.segments_reference(C, S)


def _check(X, heads, segs, cuda, what, radius=RADIUS, limit=LIMIT, skip=None):
    want = sw.swing_reference(X, heads, segs, radius, limit, skip=skip)
    got = _run(X, heads, segs, cuda, radius, limit, skip=skip)
    _same(got, want, what)
    return got, want


# ------------------------------------------------------------------ rows, spans, segments
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4 * TILE + 1])
def test_row_span_and_segment_counts(cuda, n):
    hits = 0
    for K in (0, 1, 64, 65):
        X, C, deg = sw.random_case(n, K, seed=100 + K)
        for S in (1, 32, 128):
            heads, segs = _tables(C, deg, S)
            _, want = _check(X, heads, segs, cuda, (n, K, S))
            hits += int((want["span"] >= 0).sum())
            if K == 0:
                assert (want["span"] == -1).all() and np.isinf(want["dist2"]).all() and np.isnan(want["sin"]).all()
                assert want["count"].shape == (0,)
    assert hits > 0 or n <= 1


@pytest.mark.parametrize("S", [1, 32, 128])
def test_two_hundred_spans_in_random_and_in_sorted_row_order(cuda, S):
    """K = 200 short spans over 10 km: shuffled, every tile meets nearly every span; sorted, most (tile, span) pairs are
    culled - spans far from every tile - and the answer is the same"""
    rng = np.random.default_rng(44)
    n, K = 2 * TILE + 1, 200
    X, C, deg = sw.random_case(n, K, seed=45, spread=10000.0)
    C[:, 8], C[:, 9] = -rng.uniform(2.0, 6.0, K), rng.uniform(2.0, 6.0, K)
    C[:, 7] = rng.uniform(0.02, 0.2, K)                                       # short and deep: a sag of up to 7 m
    k = rng.integers(0, K, n)
    m, t = rng.uniform(-12.0, 12.0, n), rng.normal(0.0, 5.0, n)
    near = np.stack([C[k, 0] + m * C[k, 3] - t * C[k, 4], C[k, 1] + m * C[k, 4] + t * C[k, 3],
                     C[k, 2] - rng.uniform(-4.0, 9.0, n)], axis=1).astype(np.float32)
    X = np.where((rng.uniform(0.0, 1.0, n) < 0.8)[:, None], near, X)
    X = X[rng.permutation(n)]
    heads, segs = _tables(C, deg, S)
    want = sw.swing_reference(X, heads, segs, RADIUS, LIMIT)
    assert (want["count"] > 0).sum() > 150 and want["violations"].sum() > 300
    shuffled = _run(X, heads, segs, cuda, want_stats=True)
    _same(shuffled, want, "random order")
    order = np.lexsort((X[:, 1], X[:, 0]))
    ordered = _run(X[order], heads, segs, cuda, want_stats=True)
    for key in ("dist2", "sin"):
        assert np.array_equal(_bits(ordered[key]), _bits(want[key][order])), key
    assert np.array_equal(ordered["span"], want["span"][order])
    for key in ("count", "violations", "min_dist2"):
        assert np.array_equal(_bits(ordered[key]), _bits(want[key])), key
    back = np.where(ordered["min_row"] >= 0, order[np.maximum(ordered["min_row"], 0)], -1)
    has = want["min_row"] >= 0
    assert np.array_equal(back >= 0, has)
    assert np.array_equal(X[back[has]], X[want["min_row"][has]])               # the same point, wherever it sits
    tiles = -(-n // TILE)
    print(f"(tile, span) pairs walked: {shuffled['loops'][1]} shuffled, {ordered['loops'][1]} sorted of {tiles * K}; "
          f"segment loops run: {shuffled['loops'][0]} and {ordered['loops'][0]} of {n * K} (row, span) pairs")
    assert shuffled["loops"][1] > 0.6 * tiles * K and ordered["loops"][1] < 0.7 * tiles * K
    assert ordered["loops"][1] < shuffled["loops"][1] and shuffled["loops"][0] < n * K // 10


def test_several_tiles_wide_and_narrow_radii_and_projected_coordinates(cuda):
    X, C, deg = sw.random_case(3 * TILE + 17, 65, seed=7)
    heads, segs = _tables(C, deg, 8)
    got, want = _check(X, heads, segs, cuda, "three tiles")
    assert (want["count"] > 0).sum() > 40 and want["violations"].sum() > 100
    _check(X, heads, segs, cuda, "radius 60", radius=60.0, limit=59.0)
    _check(X, heads, segs, cuda, "radius 1 mm", radius=1e-3, limit=1e-3)
    X, C, deg = sw.random_case(2 * TILE + 9, 20, seed=71, shift=EPSG)
    got, want = _check(X, *_tables(C, deg, 32), cuda, "EPSG scale")
    assert (want["span"] >= 0).sum() > 500 and want["violations"].sum() > 50


# ------------------------------------------------------------------ sqrt and /
def test_rows_inside_the_sector_pin_sqrt_and_division_to_numpys_bits(cuda):
    """4096 rows below one deep span, all inside its sector: out_sin is t/sqrt(t*t + bb*bb) of 4096 different operand
    pairs, bit for bit numpy's correctly rounded sqrt and /"""
    rng = np.random.default_rng(9)
    C = cc.curve(cx=5.0, cy=-3.0, cz=40.0, ux=0.8, uy=0.6, a=0.25, b=0.02, c=0.02, m0=-30.0, m1=34.0).reshape(1, 10)
    heads, segs = _tables(C, 60.0, 32)
    m = rng.uniform(-29.0, 33.0, 4096)
    sag_below = heads[0, 7] + (m - heads[0, 5]) * heads[0, 8]                 # the chord's height over the centre
    bb = rng.uniform(1.0, 24.0, 4096)
    t = bb * np.tan(np.radians(rng.uniform(-55.0, 55.0, 4096)))               # the sector ends at 60 degrees
    X = np.stack([5.0 + m * 0.8 - t * 0.6, -3.0 + m * 0.6 + t * 0.8, 40.0 + sag_below - bb], axis=1).astype(np.float32)
    got, want = _check(X, heads, segs, cuda, "inside the sector", radius=45.0, limit=10.0)
    hit = want["span"] == 0
    sT = heads[0, 9]
    assert hit.sum() > 3500 and (np.abs(want["sin"][hit]) < sT).all()         # none at the sector's end
    assert len(np.unique(want["sin"][hit])) > 3400


# ------------------------------------------------------------------ the rule's boundaries
def test_the_boundary_rows(cuda):
    heads, segs = sw.level_case()
    X, skip = sw.boundary_rows()
    got, _ = _check(X, heads, segs, cuda, "boundary", radius=sw.B_RADIUS, limit=sw.B_LIMIT, skip=skip)
    assert tuple(got["span"].tolist()) == sw.BOUNDARY_SPAN
    assert got["dist2"][0] == 100.0 and np.isinf(got["dist2"][1]) and got["dist2"][2] == 36.0
    assert got["violations"][4] == int((got["dist2"][got["span"] == 4] <= 36.0).sum()) and got["dist2"][3] > 36.0
    assert got["sin"][4] == 8.0 / np.sqrt(128.0) and got["sin"][5] == sw.B_SIN and np.signbit(got["sin"][18])
    assert np.isnan(got["sin"][[1, 14, 15, 16, 17]]).all() and got["count"][:sw.NOPART].sum() == 0
    assert got["count"][5] == 0 and got["min_row"][5] == -1                   # the tie goes to the lower span
    # the same rows spread over three tiles, each among rows that are far from everything
    big = np.full((2 * TILE + 300, 3), 500.0, dtype=np.float32)
    where = np.arange(len(X)) * 113 + 5
    big[where] = X
    bskip = np.zeros(len(big), dtype=np.uint8)
    bskip[where] = skip
    got, want = _check(big, heads, segs, cuda, "boundary, three tiles", radius=sw.B_RADIUS, limit=sw.B_LIMIT, skip=bskip)
    assert tuple(got["span"][where].tolist()) == sw.BOUNDARY_SPAN and (np.delete(got["span"], where) == -1).all()


def test_ties_between_identical_spans_go_to_the_lowest_index(cuda):
    X, C, deg = sw.random_case(TILE + 300, 1, seed=3)
    heads, segs = _tables(np.concatenate([C, C]), np.concatenate([deg, deg]) * 0.0 + 50.0, 32)
    got, _ = _check(X, heads, segs, cuda, "two identical spans")
    assert (got["span"] <= 0).all() and (got["span"] == 0).sum() > 300 and got["count"][1] == 0
    assert got["min_row"][1] == -1 and np.isinf(got["min_dist2"][1])


# ------------------------------------------------------------------ spans that do not take part, odd directions
def test_spans_that_take_no_part_change_no_bit_of_the_others(cuda):
    X, C, deg = sw.random_case(2 * TILE + 5, 9, seed=21)
    heads, segs = _tables(C, deg, 32)
    clean = _run(X, heads, segs, cuda)
    _same(clean, sw.swing_reference(X, heads, segs, RADIUS, LIMIT), "clean")
    for where in ("segment", "centre", "no length", "cosine zero", "not a turn", "sine negative", "kap"):
        H, G = np.insert(heads, 4, heads[2], axis=0), np.insert(segs, 4, segs[2], axis=0)
        if where == "segment":
            G[4, 17, 5] = np.nan
        elif where == "centre":
            H[4, 1] = np.inf
        elif where == "no length":
            H[4, 6] = H[4, 5]
        elif where == "cosine zero":
            H[4, 9:11] = (1.0, 0.0)
        elif where == "not a turn":
            H[4, 9:11] = H[4, 9:11] * np.sqrt(1.0 + 1e-5)
        elif where == "sine negative":
            H[4, 9] = -H[4, 9] - 0.1
            H[4, 10] = np.sqrt(1.0 - H[4, 9] * H[4, 9])
        else:
            H[4, 8] = -np.inf
        assert not sw.takes_part(H, G)[4], where
        got, _ = _check(X, H, G, cuda, where)
        assert (got["span"] != 4).all() and got["count"][4] == 0 and got["min_row"][4] == -1
        keep = np.array([0, 1, 2, 3, 5, 6, 7, 8, 9])
        moved = np.where(got["span"] > 4, got["span"] - 1, got["span"])
        assert np.array_equal(moved, clean["span"]) and np.array_equal(_bits(got["dist2"]), _bits(clean["dist2"]))
        assert np.array_equal(_bits(got["sin"]), _bits(clean["sin"]))
        for key in ("count", "violations", "min_dist2", "min_row"):
            assert np.array_equal(_bits(got[key][keep]), _bits(clean[key])), (where, key)


def test_a_span_whose_direction_is_not_unit_is_never_culled(cuda):
    X, C, deg = sw.random_case(3 * TILE, 6, seed=33, spread=4000.0)
    X = X[np.argsort(X[:, 0], kind="stable")]                                  # sorted: tight tile boxes
    C[1, 3:5] *= 1.5                                                           # stretches m and t by 1.5
    C[4, 3:5] *= 0.5
    C[5, 3:5] *= 1.0 + 1e-5                                                    # beyond the bounds' assumption
    far = X.copy()
    far[:, 0] += np.float32(9000.0)                                            # rows the true bounds would never meet
    heads, segs = _tables(C, deg, 16)
    for rows, what in ((X, "near"), (np.vstack([far, X]), "far and near")):
        got, want = _check(rows, heads, segs, cuda, what, radius=25.0, limit=10.0)
    assert (want["count"][[1, 4, 5]] > 0).all()


# ------------------------------------------------------------------ mask and rows
def test_skip_mask_nonfinite_rows_and_tiles_with_no_acceptable_row(cuda):
    X, C, deg = sw.random_case(3 * TILE + 100, 12, seed=51)
    heads, segs = _tables(C, deg, 32)
    rng = np.random.default_rng(52)
    skip = (rng.uniform(0.0, 1.0, len(X)) < 0.2).astype(np.uint8)
    skip[TILE:2 * TILE] = 1                                                    # a tile that is skipped entirely
    skip[5] = 255
    bad = {3: (0, np.nan), 64: (1, np.inf), 65: (2, -np.inf), 700: (0, np.inf), TILE - 1: (2, np.nan),
           2 * TILE: (1, np.nan), 3 * TILE + 99: (0, -np.inf)}
    for i, (axis, v) in bad.items():
        X[i, axis] = v
    got, want = _check(X, heads, segs, cuda, "skip", skip=skip)
    gone = np.union1d(np.flatnonzero(skip), np.array(sorted(bad)))
    assert (got["span"][gone] == -1).all() and np.isinf(got["dist2"][gone]).all() and np.isnan(got["sin"][gone]).all()
    assert (got["span"][:TILE] >= 0).sum() > 100
    out = ops.swing_clearance(_dev(X, cuda), _dev(heads, cuda), _dev(segs, cuda), RADIUS, LIMIT,
                              skip=_dev(skip != 0, cuda))                      # a bool mask is taken as it is
    assert np.array_equal(out["span"].cpu().numpy(), want["span"])
    everything = _run(X, heads, segs, cuda, skip=np.ones(len(X), dtype=np.uint8), want_stats=True)
    assert (everything["span"] == -1).all() and (everything["count"] == 0).all() and everything["loops"].tolist() == [0, 0]
    assert (everything["min_row"] == -1).all() and np.isinf(everything["min_dist2"]).all()
    allbad = np.full((TILE + 3, 3), np.nan, dtype=np.float32)                  # tiles without a finite row
    _check(allbad, heads, segs, cuda, "no finite row")


# ------------------------------------------------------------------ call level
def test_the_same_call_twice_and_with_the_rows_shuffled(cuda):
    X, C, deg = sw.random_case(4 * TILE + 1, 65, seed=91, shift=EPSG)
    heads, segs = _tables(C, deg, 32)
    a, b = _run(X, heads, segs, cuda), _run(X, heads, segs, cuda)
    for key in sw.OUTPUTS:
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key
    assert (a["span"] >= 0).sum() > 1000
    perm = np.random.default_rng(92).permutation(len(X))
    c = _run(X[perm], heads, segs, cuda)
    for key in ("dist2", "span", "sin"):
        assert np.array_equal(_bits(c[key]), _bits(a[key][perm])), key
    for key in ("count", "violations", "min_dist2"):
        assert np.array_equal(_bits(c[key]), _bits(a[key])), key
    has = a["min_row"] >= 0
    assert np.array_equal(c["min_row"] >= 0, has)
    assert np.array_equal(X[perm][c["min_row"][has]], X[a["min_row"][has]])


def test_refusals(cuda):
    X, C, deg = sw.random_case(100, 3, seed=95)
    heads, segs = _tables(C, deg, 4)
    dX, dH, dS = _dev(X, cuda), _dev(heads, cuda), _dev(segs, cuda)
    for radius, limit in ((np.nan, 1.0), (np.inf, 1.0), (10.0, np.nan), (10.0, np.inf), (0.0, 0.0), (-1.0, -2.0),
                          (10.0, 0.0), (10.0, -1.0), (5.0, 6.0)):
        with pytest.raises(ValueError):
            ops.swing_clearance(dX, dH, dS, radius, limit)
    with pytest.raises(ValueError):
        ops.swing_clearance(dX, dH, _dev(np.zeros((3, 129, 6)), cuda), 10.0, 6.0)
    with pytest.raises(ValueError):
        ops.swing_clearance(dX, dH, _dev(np.zeros((3, 4, 5)), cuda), 10.0, 6.0)
    with pytest.raises(ValueError):
        ops.swing_clearance(dX, dH[:, :10].contiguous(), dS, 10.0, 6.0)
    with pytest.raises(ValueError):
        ops.swing_clearance(dX, _dev(np.zeros((4097, 11)), cuda), _dev(np.zeros((4097, 1, 6)), cuda), 10.0, 6.0)
    with pytest.raises(ValueError):
        ops.swing_clearance(dX, dH, dS[:2], 10.0, 6.0)
    with pytest.raises(ValueError):
        ops.swing_clearance(dX, dH, dS, 10.0, 6.0, skip=torch.zeros(99, dtype=torch.uint8, device=cuda))
    with pytest.raises(TypeError):
        ops.swing_clearance(torch.from_numpy(X), dH, dS, 10.0, 6.0)
    with pytest.raises(TypeError):
        ops.swing_segments(torch.from_numpy(C), 4)
    with pytest.raises(ValueError):
        ops.swing_segments(_dev(C, cuda), 129)
    with pytest.raises(ValueError):
        ops.swing_heads(_dev(C, cuda), 90.0)
    with pytest.raises(ValueError):
        ops.swing_heads(_dev(C, cuda), [10.0, 20.0])
    with pytest.raises(TypeError):
        pipeline.wind_clearance(torch.from_numpy(X), {}, 45.0)
    # the device tables are the reference's, bit for bit
    assert np.array_equal(ops.swing_heads(_dev(C, cuda), deg).cpu().numpy().view(np.uint64), heads.view(np.uint64))
    assert np.array_equal(ops.swing_segments(_dev(C, cuda), 4).cpu().numpy().view(np.uint64), segs.view(np.uint64))


def test_the_raw_c_abi(cuda):
    L = _lib.lib()
    X, C, deg = sw.random_case(TILE + 7, 4, seed=97)
    n, K, S = len(X), 4, 8
    heads, segs = _tables(C, deg, S)
    want = sw.swing_reference(X, heads, segs, 10.0, 6.0)
    dX, dH, dS = _dev(X, cuda), _dev(heads, cuda), _dev(segs, cuda)
    d2 = torch.full((n,), -1.0, dtype=torch.float64, device=cuda)
    span = torch.full((n,), 7, dtype=torch.int32, device=cuda)
    sin = torch.full((n,), 7.0, dtype=torch.float64, device=cuda)
    tab = [torch.full((K,), 7, dtype=dt, device=cuda) for dt in (torch.int64, torch.int64, torch.float64, torch.int64)]
    need = L.pch_swing_clearance_ws_bytes(n, K, S)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def call(xyz=None, nn=n, kk=K, ss=S, radius=10.0, limit=6.0, out=None, osin=None, cnt=None, wsp=None, wb=None,
             hd=None):
        return L.pch_swing_clearance_f32(p(dX) if xyz is None else xyz, 0, nn, p(dH) if hd is None else hd, p(dS), kk,
                                         ss, radius, limit, p(d2) if out is None else out, p(span),
                                         p(sin) if osin is None else osin, p(tab[0]) if cnt is None else cnt, p(tab[1]),
                                         p(tab[2]), p(tab[3]), 0, p(ws) if wsp is None else wsp,
                                         need if wb is None else wb, st)

    assert call() == 0
    got = dict(dist2=d2, span=span, sin=sin, count=tab[0], violations=tab[1], min_dist2=tab[2], min_row=tab[3])
    _same({key: v.cpu().numpy() for key, v in got.items()}, want, "raw")
    before = [t.clone() for t in got.values()]
    assert call(wb=need - 1) == -2 and b"workspace" in L.pch_last_error()      # PCH_ERR_WORKSPACE
    host = np.zeros(n, dtype=np.float64)
    for rc in (call(nn=-1), call(nn=2 ** 32), call(kk=-1), call(kk=4097), call(ss=0), call(ss=129),
               call(radius=float("nan")), call(limit=float("inf")), call(limit=0.0), call(limit=10.5), call(radius=-1.0),
               call(xyz=0), call(out=0), call(osin=0), call(cnt=0), call(hd=0), call(wsp=0),
               call(wsp=host.ctypes.data)):
        assert rc == -1                                                        # PCH_ERR_ARG
    torch.cuda.synchronize()
    for t, b in zip(got.values(), before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))           # a refused call writes nothing
    # no span: every row +inf / -1 / NaN and no table, without a pointer to read; no row: an empty table per span
    f = L.pch_swing_clearance_f32
    assert f(p(dX), 0, n, 0, 0, 0, S, 10.0, 6.0, p(d2), p(span), p(sin), 0, 0, 0, 0, 0, p(ws), need, st) == 0
    assert f(0, 0, 0, p(dH), p(dS), K, S, 10.0, 6.0, 0, 0, 0, p(tab[0]), p(tab[1]), p(tab[2]), p(tab[3]), 0, p(ws), need,
             st) == 0
    assert f(0, 0, 0, 0, 0, 0, S, 10.0, 6.0, 0, 0, 0, 0, 0, 0, 0, 0, p(ws), need, st) == 0
    torch.cuda.synchronize()
    assert torch.isinf(d2).all() and (span == -1).all() and torch.isnan(sin).all()
    assert (tab[0] == 0).all() and (tab[1] == 0).all() and torch.isinf(tab[2]).all() and (tab[3] == -1).all()


# ------------------------------------------------------------------ the scene, op and pipeline level
def test_the_scene_bit_for_bit(cuda):
    r = sw.reference()
    X, _ = sw.wind_scene()
    got = _run(X, r["heads"], r["segs"], cuda, radius=sw.RADIUS, limit=sw.LIMIT, skip=r["skip"])
    _same(got, {key: r[key] for key in sw.OUTPUTS}, "scene")


def test_wind_clearance_against_the_reference(cuda):
    r = sw.reference()
    X, kind = sw.wind_scene()
    points = _dev(X, cuda)
    spans = pipeline.conductor_spans(points, rule=dict(sc.SCENE_RULE), towers=sp.line_towers())
    out = pipeline.wind_clearance(points, spans, sw.ANGLE, radius=sw.RADIUS, limit=sw.LIMIT, segments=sw.SEGMENTS,
                                  towers=sp.line_towers(), cut_radius=9.0)
    K, idx = r["spans"]["nclusters"], r["idx"]
    span_ref = np.where(r["span"] >= 0, idx[np.maximum(r["span"], 0)], -1).astype(np.int32)
    assert np.array_equal(out["span"].cpu().numpy(), span_ref)
    lim2 = sw.LIMIT * sw.LIMIT
    assert np.array_equal(out["violating"].cpu().numpy(), r["dist2"] <= lim2)
    T = {key: v.cpu().numpy() for key, v in out["table"].items()}
    assert tuple(T) == pipeline.WIND_TABLE_KEYS and all(len(v) == K for v in T.values())
    rest = np.setdiff1d(np.arange(K), idx)
    assert np.array_equal(T["count"][idx], r["count"]) and np.array_equal(T["violations"][idx], r["violations"])
    assert np.array_equal(T["min_row"][idx], r["min_row"])
    assert (T["count"][rest] == 0).all() and (T["min_row"][rest] == -1).all() and np.isnan(T["min_angle"][rest]).all()
    tol = r["tol"]
    got, want = out["distance"].cpu().numpy(), np.sqrt(r["dist2"])
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    worst = float(np.abs(got[fin] - want[fin]).max())
    print(f"pipeline distances: worst difference {worst:.3e} m, tol {tol:.3e} m")
    assert worst <= tol
    has = r["count"] > 0
    assert np.abs(T["min_distance"][idx][has] - np.sqrt(r["min_dist2"][has])).max() <= tol
    assert np.array_equal(T["min_point"][idx][has], X[r["min_row"][has]])
    angle = out["angle"].cpu().numpy()
    assert np.array_equal(np.isnan(angle), ~fin) and np.abs(angle[fin]).max() <= sw.ANGLE + 1e-9
    assert np.abs(angle[fin] - np.degrees(np.arcsin(r["sin"][fin]))).max() < 1e-3
    assert np.array_equal(T["min_angle"][idx][has], angle[r["min_row"][has]])
    # the 14 m column: a violation under wind, none at rest
    column = kind == 20
    clear = pipeline.conductor_clearance(points, spans, radius=sw.RADIUS, limit=sw.LIMIT, segments=sw.SEGMENTS,
                                         towers=sp.line_towers(), cut_radius=9.0)
    windy, calm = out["violating"].cpu().numpy(), clear["violating"].cpu().numpy()
    assert windy[column].sum() > 5 and not calm[column].any()
    assert np.array_equal(calm, r["rest"]["dist2"] <= lim2)
    assert (np.abs(angle[column & windy] + sw.ANGLE) < 1e-9).sum() > 5       # met at the full angle, on its side
    # no accepted piece: an empty result, nothing raised
    none = dict(spans, accepted=torch.zeros_like(spans["accepted"]))
    out = pipeline.wind_clearance(points, none, 45.0, towers=sp.line_towers())
    assert (out["span"] == -1).all() and not out["violating"].any() and (out["table"]["count"] == 0).all()
    assert torch.isnan(out["angle"]).all() and torch.isinf(out["distance"]).all()
    with pytest.raises(ValueError):
        pipeline.wind_clearance(points, spans, 90.0)


# ------------------------------------------------------------------ drop-in
def test_drop_in_knob_writes_the_wind_table(cuda, tmp_path, monkeypatch):
    from pointcloudhookup_amd.utils import tower_extraction as te
    r = sw.reference()
    X, _ = sw.wind_scene()
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

    assert te.WIND is None
    off, off_logs = run()
    table = tmp_path / "output_towers" / "wind_clearance_info.csv"
    assert len(off) == 3 and not table.exists()
    monkeypatch.setattr(te, "WIND", te.wind_from_env("45,7.5,10", spans=True))
    on, logs = run()
    extra = [m for m in logs if "风偏净空" in m]
    assert len(extra) == 1 and "越限线段" in extra[0], extra
    assert [m for m in logs if "风偏净空" not in m] == off_logs
    assert len(on) == len(off)
    for a, b in zip(on, off):                                                  # the tower dicts are the same
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    with open(table, newline="", encoding="utf-8") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == te.WIND_COLUMNS and len(lines) == 1 + 6          # one line per accepted piece
    col = {name: np.array([float(v[i]) for v in lines[1:]]) for i, name in enumerate(te.WIND_COLUMNS) if i}
    # the file is the scene in millimetres, lifted: counts may move by the few rows that sit a millimetre from a
    # threshold; the piece beside the column is breached, and its nearest row is a column row met at the full angle
    assert np.abs(np.sort(col["count"]) - np.sort(r["count"])).max() <= 3
    assert (col["violations"] > 0).sum() == (r["violations"] > 0).sum()
    a = np.radians(sp.LINE_AZIMUTH_DEG)
    station = col["x"] * np.cos(a) + col["y"] * np.sin(a)
    lateral = -col["x"] * np.sin(a) + col["y"] * np.cos(a)
    beside = np.flatnonzero((np.abs(station - 40.0) < 0.2) & (np.abs(lateral + 14.0) < 0.2))
    assert len(beside) == 1 and col["violations"][beside[0]] > 5 and abs(col["angle_deg"][beside[0]] + 45.0) < 1e-9
    k = int(np.unique(r["span"][(r["kind"] == 20) & (r["span"] >= 0)])[0])
    # unlike a distance at rest, a swung one depends on where the piece ends: f is measured from the chord through the
    # piece's own ends, and here the cut is made 9 m from the centres of the tower boxes, which may stand up to half a
    # metre from the true axes.  A piece of L = 62 m with c = 4*2/80^2 whose ends move by dL = 0.5 m changes f by at
    # most c*L*dL = 0.04 m, and the distance by no more than that
    assert abs(col["min_distance"][beside[0]] - np.sqrt(r["min_dist2"][k])) < 0.04 + 2e-3
    assert (np.abs(col["angle_deg"][np.isfinite(col["angle_deg"])]) <= 45.0 + 1e-9).all()
    monkeypatch.setattr(te, "WIND", None)
    again, again_logs = run()
    assert again_logs == off_logs and len(again) == 3
