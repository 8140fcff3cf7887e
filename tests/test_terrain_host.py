"""Terrain grid on the CPU: the new symbols and workspace sizes, the numpy statement of the rule (terrain_cases) against
an independent statement of its two cheap parts, identities of the opening, the torch twins of the span ground profile
against numpy, the scene's numbers and margins and the drop-in's knob (no kernel runs here)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import clearance_cases as cc
import span_cases as sp
import terrain_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
NEW_SYMBOLS = ("pch_terrain_low_ws_bytes", "pch_terrain_low_f32", "pch_terrain_ground_ws_bytes",
               "pch_terrain_ground_f32", "pch_terrain_height_f32", "pch_terrain_sample_f64")


def test_new_symbols_and_workspace_bytes():
    from pointcloudhookup_amd import _lib, ops, pipeline
    header = open(os.path.join(ROOT, "include", "pch_hip.h"), encoding="utf-8").read()
    declared = set(re.findall(r"\b(pch_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    L = _lib.lib()
    low, ground = L.pch_terrain_low_ws_bytes, L.pch_terrain_ground_ws_bytes
    assert low(0, 1) > 0 and low(0, 1) == low(2 ** 31 - 1, 1)                 # per cell, not per row
    assert 4 * 2 ** 24 <= low(0, 2 ** 24) <= 4 * 2 ** 24 + 1024               # one key per cell and the two figures
    for n, cells in ((-1, 1), (2 ** 31, 1), (1, 0), (1, -1), (1, 2 ** 24 + 1)):
        assert low(n, cells) == 0, (n, cells)
    assert ground(1) > 0 and 13 * 2 ** 24 <= ground(2 ** 24) <= 13 * 2 ** 24 + 2048    # three grids and a flag
    for cells in (0, -1, 2 ** 24 + 1):
        assert ground(cells) == 0, cells
    assert ops.TERRAIN_TILE == 1024 and ops.TERRAIN_MAX_CELLS == 2 ** 24
    assert ops.TERRAIN_MAX_WINDOW == 64 and ops.TERRAIN_MAX_GAP == 256
    for name in ("terrain_grid", "terrain_low", "terrain_ground", "terrain_height", "terrain_sample",
                 "span_ground_profile", "_terrain_grid_of", "_span_vertices_of", "_span_vertex_positions_of",
                 "_span_ground_minima_of"):
        assert callable(getattr(ops, name)), name
    for name in ("terrain_model", "height_above_ground", "span_ground_clearance", "terrain_cells"):
        assert callable(getattr(pipeline, name)), name
    # the rule is in the header word for word: the lines a reader checks the numpy statement against
    for line in ("key(z) = bits(z) ^ (bits(z) >> 31 ? 0xFFFFFFFF : 0x80000000)",
                 "fx = floor((X - x0) / cell) and fy = floor((Y - y0) / cell)",
                 "((double)low[c] - (double)open[c]) <= dh",
                 "num = num + ((double)low_k / (double)d_k)   and   den = den + (1.0 / (double)d_k)",
                 "u = ((X - x0) / cell) - 0.5",
                 "g = (((g00*(1 - a)) + (g10*a))*(1 - b)) + (((g01*(1 - a)) + (g11*a))*b)",
                 "X = cx + (m*ux), Y = cy + (m*uy), W = cz + z"):
        assert line in header, line


# ------------------------------------------------------------------ the two statements
def _awkward_rows(g, n, seed):
    """rows over and around a grid: inside, outside on every side, on cell edges, with NaN / inf, with both zeros"""
    rng = np.random.default_rng(seed)
    w, h = g["nx"] * g["cell"], g["ny"] * g["cell"]
    X = np.stack([g["x0"] + rng.uniform(-0.2 * w - 1, 1.2 * w + 1, n), g["y0"] + rng.uniform(-0.2 * h - 1, 1.2 * h + 1, n),
                  rng.normal(0.0, 5.0, n)], axis=1)
    edge = rng.uniform(0, 1, n) < 0.2
    X[edge, 0] = g["x0"] + np.round((X[edge, 0] - g["x0"]) / g["cell"]) * g["cell"]
    X[edge, 1] = g["y0"] + np.round((X[edge, 1] - g["y0"]) / g["cell"]) * g["cell"]
    X = X.astype(np.float32)
    for k, v in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
        X[(7 * k + 3) % n, k % 3] = v
    X[rng.integers(0, n, n // 10), 2] = np.float32(-0.0)
    X[rng.integers(0, n, n // 10), 2] = np.float32(0.0)
    return X


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (3, 3), (57, 30)])
def test_lowest_return_by_a_loop_and_by_a_sort(shape):
    g = tc.grid(x0=-3.25, y0=10.5, cell=0.75, nx=shape[0], ny=shape[1])
    X = _awkward_rows(g, 3000, seed=shape[0] * 100 + shape[1])
    skip = (np.arange(len(X)) % 5 == 0).astype(np.uint8)
    for sub, sk in ((None, None), (np.array([1.5, -2.0, 0.25], np.float32), skip)):
        low, count = tc.low_reference(X, g, sub=sub, skip=sk)
        low2, count2 = tc.low_by_sort(X, g, sub=sub, skip=sk)
        assert tc.same(low, low2) and np.array_equal(count, count2)
        assert np.array_equal(np.isnan(low), count == 0) and count.sum() == tc.takes_part(X, g, sub, sk)[0].sum()
        assert 0 < count.sum() < len(X)


def test_both_zeros_in_one_cell_give_the_negative_one():
    g = tc.grid(nx=1, ny=1)
    for z in ([0.0, -0.0], [-0.0, 0.0]):
        X = np.array([[0.5, 0.5, z[0]], [0.5, 0.5, z[1]]], dtype=np.float32)
        low, count = tc.low_reference(X, g)
        assert np.signbit(low[0, 0]) and low[0, 0] == 0 and count[0, 0] == 2
    assert tc.key_of(np.float32(-0.0)) < tc.key_of(np.float32(0.0))
    z = np.array([-np.inf, -3.0, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], dtype=np.float32)
    assert (np.diff(tc.key_of(z).astype(np.int64)) > 0).all() and tc.same(tc.unkey(tc.key_of(z)), z)


def test_bilinear_rule_against_interp_on_the_cell_centres():
    """the rule takes a = u - i0 from u = (X - x0)/cell - 0.5; np.interp takes (X - xc_i)/(xc_{i+1} - xc_i) from centres
    it computed itself.  Each takes a handful of roundings relative to the position in cells, q, so the two weights
    differ by a few u·q and the values by that times the largest step D between neighbouring cells, plus a few u of the
    largest value M - once along x and once along y; 64 u·(M + D·q) leaves room for both."""
    r = tc.reference()
    g, ground = r["grid"], r["ground"]
    X, _ = tc.terrain_scene()
    P = X[::23].astype(np.float64)
    rng = np.random.default_rng(3)
    strip = np.stack([g["x0"] + rng.uniform(0, 0.5, 200) * g["cell"] + (g["nx"] - 0.5) * (rng.uniform(0, 1, 200) < 0.5),
                      g["y0"] + rng.uniform(0, g["ny"], 200) * g["cell"]], axis=1)        # the half-cell border strip
    XY = np.concatenate([P[:, :2], strip])
    want = tc.ground_at(g, ground, XY[:, 0], XY[:, 1])
    i0, i1, _ = tc._axis(XY[:, 0], g["x0"], g["cell"], g["nx"])
    j0, j1, _ = tc._axis(XY[:, 1], g["y0"], g["cell"], g["ny"])
    G = ground.astype(np.float64)
    four = ~(np.isnan(G[j0, i0]) | np.isnan(G[j0, i1]) | np.isnan(G[j1, i0]) | np.isnan(G[j1, i1])) & ~np.isnan(want)
    assert four.sum() > 2000
    filled = np.where(np.isnan(G), 0.0, G)                                   # (np.interp has no NaN rule; unused cells)
    got = tc.sample_by_interp(g, filled, XY[four, 0], XY[four, 1])
    M = float(np.nanmax(np.abs(G)))
    D = float(max(np.nanmax(np.abs(np.diff(G, axis=0))), np.nanmax(np.abs(np.diff(G, axis=1)))))
    q = (float(np.abs(XY).max()) + abs(g["x0"]) + abs(g["y0"])) / g["cell"] + g["nx"] + g["ny"]
    bound = 64.0 * U * (M + D * q)
    worst = float(np.abs(got - want[four]).max())
    print(f"bilinear rule against np.interp: worst difference {worst:.3e} m over {four.sum()} positions, bound "
          f"{bound:.3e} m ({worst / (U * (M + D * q)):.1f} u of the scale)")
    assert worst <= bound


def test_ground_under_a_position_clamps_and_falls_back():
    g = tc.grid(x0=0.0, y0=0.0, cell=2.0, nx=3, ny=2)
    ground = np.array([[1.0, 2.0, 4.0], [3.0, 5.0, 9.0]], dtype=np.float32)
    at = lambda x, y, gr=ground, gg=g: float(tc.ground_at(gg, gr, np.array([x]), np.array([y]))[0])
    assert at(1.0, 1.0) == 1.0 and at(3.0, 1.0) == 2.0 and at(5.0, 3.0) == 9.0        # cell centres
    assert at(2.0, 1.0) == 1.5 and at(2.0, 2.0) == 0.25 * (1 + 2 + 3 + 5)             # between them
    assert at(0.0, 0.0) == 1.0 and at(0.5, 0.25) == 1.0 and at(5.75, 3.9) == 9.0      # the border strip is level
    for x, y in ((-0.001, 1.0), (6.0, 1.0), (1.0, -0.001), (1.0, 4.0), (np.nan, 1.0), (1.0, np.inf)):
        assert np.isnan(at(x, y))
    hole = ground.copy()
    hole[0, 1] = np.nan
    assert at(0.5, 0.5, hole) == 1.0 and at(1.5, 1.5, hole) == 1.0                    # the position's own cell
    assert np.isnan(at(3.0, 1.0, hole)) and at(5.5, 3.5, hole) == 9.0
    one = tc.grid(cell=1.0, nx=1, ny=1)
    assert float(tc.ground_at(one, np.array([[7.0]], np.float32), np.array([0.9]), np.array([0.1]))[0]) == 7.0


# ------------------------------------------------------------------ the opening
def test_opening_identities():
    rng = np.random.default_rng(11)
    low = rng.normal(0.0, 2.0, (23, 31)).astype(np.float32)
    low[rng.uniform(0, 1, low.shape) < 0.15] = np.nan
    assert tc.same(tc.open_reference(low, 0), low)                           # R = 0 is the identity
    for R in (1, 3, 6, 40):
        opened = tc.open_reference(low, R)
        has = ~np.isnan(low)
        assert not np.isnan(opened[has]).any() and (opened[has] <= low[has]).all()
    assert np.isnan(tc.open_reference(np.full((4, 5), np.nan, np.float32), 2)).all()
    # a plane away from the border is reproduced exactly; at the border the clipped window can only lower it
    yy, xx = np.mgrid[0:40, 0:50]
    plane = (0.25 * xx - 0.125 * yy + 3.0).astype(np.float32)
    opened = tc.open_reference(plane, 6)
    assert np.array_equal(opened[6:-6, 6:-6], plane[6:-6, 6:-6]) and (opened <= plane).all()
    # a spike narrower than the window goes, a plateau wider than it stays
    spike = np.full((40, 50), 3.0, np.float32)
    spike[20, 25] += 5.0
    assert (tc.open_reference(spike, 6) == 3.0).all() and tc.open_reference(spike, 0)[20, 25] == 8.0
    wide = np.zeros((40, 50), np.float32)
    wide[10:30, 10:30] = 4.0                                                 # 20 cells, window 13
    narrow = np.zeros((40, 50), np.float32)
    narrow[10:18, 10:18] = 4.0                                               # 8 cells
    assert np.array_equal(tc.open_reference(wide, 6), wide) and not tc.open_reference(narrow, 6).any()
    _, ground, state = tc.ground_reference(narrow, 6, 0.5, 16)
    assert (state[10:18, 10:18] == 6).all() and (ground[10:18, 10:18] == 0).all() and (state[0] == 5).all()


def test_fill_directions_gap_and_states():
    low = np.full((5, 7), np.nan, dtype=np.float32)
    low[2, 0], low[2, 6], low[0, 3], low[4, 3] = 1.0, 2.0, 4.0, 8.0
    _, ground, state = tc.ground_reference(low, 0, 0.0, 3)
    # (2, 3): -x at 3 (1.0), +x at 3 (2.0), -y at 2 (4.0), +y at 2 (8.0)
    num = ((((0.0 + 1.0 / 3.0) + 2.0 / 3.0) + 4.0 / 2.0) + 8.0 / 2.0)
    den = ((((0.0 + 1.0 / 3.0) + 1.0 / 3.0) + 1.0 / 2.0) + 1.0 / 2.0)
    assert ground[2, 3] == np.float32(num / den) and state[2, 3] == 2
    assert ground[2, 2] == np.float32((1.0 / 2.0) / (1.0 / 2.0)) and state[2, 2] == 2   # +x is 4 away: beyond the gap
    assert np.isnan(ground[1, 1]) and state[1, 1] == 0 and state[2, 0] == 5
    _, ground, state = tc.ground_reference(low, 0, 0.0, 0)
    assert (state[np.isnan(low)] == 0).all() and np.isnan(ground[np.isnan(low)]).all()
    # a cell with rows that is rejected and finds no ground: state 4
    low = np.zeros((1, 30), dtype=np.float32)
    low[0, 10:14] = 5.0
    _, ground, state = tc.ground_reference(low, 3, 0.5, 1)
    assert state[0, 10:14].tolist() == [6, 4, 4, 6] and np.isnan(ground[0, 11]) and ground[0, 10] == 0.0


# ------------------------------------------------------------------ the torch twins
def test_torch_twins_give_the_reference_bit_for_bit():
    from pointcloudhookup_amd import ops
    r = tc.reference()
    g, ground = r["grid"], r["ground"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    extra = np.stack([cc.curve(cx=30.0, cy=5.0, cz=20.0, ux=0.6, uy=0.8, a=3.0, b=-0.01, c=0.004, m0=-40.0, m1=50.0),
                      cc.curve(cx=1e4, m0=2.0, m1=2.0), cc.curve(cx=-28.0, cy=-34.0, cz=9.0, m0=-3.0, m1=3.0)])
    for S in (1, 2, 7, 32, 128):
        for C in (r["curves"], extra):
            for limit in (tc.LIMIT, tc.BREACH_LIMIT):
                want = tc.span_ground_reference(C, S, g, ground, limit)
                m, z, _ = ops._span_vertices_of(t(C), S)
                X, Y, W = ops._span_vertex_positions_of(t(C), m, z)
                assert np.array_equal(X.numpy().view(np.uint64), want["X"].view(np.uint64))
                assert np.array_equal(Y.numpy().view(np.uint64), want["Y"].view(np.uint64))
                gv = tc.ground_at(g, ground, X.numpy().reshape(-1), Y.numpy().reshape(-1)).reshape(X.shape)
                got = {k: v.numpy() for k, v in ops._span_ground_minima_of(X, Y, W, t(gv), limit).items()}
                for key in ("clearance", "ground", "covered", "min_clearance", "min_vertex", "min_at", "violation"):
                    assert tc.same(got[key], want[key]), (S, key)
    assert want["covered"][1] == 0 and not want["violation"][1]               # outside the grid: nothing covered
    assert want["min_vertex"][1] == -1 and np.isinf(want["min_clearance"][1]) and np.isnan(want["min_at"][1]).all()
    # span_segments' vertices are the shared helper's: its table is clearance_cases' bit for bit
    segs, chord = ops._span_segments_of(t(r["curves"]), tc.SEGMENTS)
    ws, wc = cc.segments_reference(r["curves"], tc.SEGMENTS)
    assert np.array_equal(segs.numpy().view(np.uint64), ws.view(np.uint64))
    assert np.array_equal(chord.numpy().view(np.uint64), wc.view(np.uint64))


def test_grid_of_the_bounds():
    from pointcloudhookup_amd import ops
    X, _ = tc.terrain_scene()
    for sub in (None, np.array([3.5, -7.25, 1.0], np.float32)):
        for cell in (1.0, 0.5, 3.0):
            want = tc.scene_grid(X, cell, sub)
            got = ops._terrain_grid_of(X[:, :2].min(0), X[:, :2].max(0), np.zeros(2, np.float32) if sub is None else sub,
                                       cell)
            assert got == want
            inside, _, _ = tc.cell_of(want, tc.frame(X, sub)[:, 0].astype(np.float64),
                                      tc.frame(X, sub)[:, 1].astype(np.float64))
            assert inside.all()                                              # the far edge's rows are inside
    none = ops._terrain_grid_of([np.inf, np.inf], [-np.inf, -np.inf], np.zeros(2, np.float32), 1.0)
    assert (none["nx"], none["ny"], none["x0"], none["y0"]) == (1, 1, 0.0, 0.0)
    with pytest.raises(ValueError, match="smallest cell that fits is") as e:
        ops._terrain_grid_of([0.0, 0.0], [5000.0, 5000.0], np.zeros(2, np.float32), 1.0)
    fits = float(str(e.value).rsplit(" ", 1)[1])
    ok = ops._terrain_grid_of([0.0, 0.0], [5000.0, 5000.0], np.zeros(2, np.float32), fits)
    assert ok["nx"] * ok["ny"] <= 2 ** 24 and 1.2 < fits < 1.25


def test_metres_to_cells_and_their_limits():
    from pointcloudhookup_amd import pipeline
    assert pipeline.terrain_cells(1.0, 12.0, 16.0) == (6, 16) and pipeline.terrain_cells(0.5, 12.0, 16.0) == (12, 32)
    assert pipeline.terrain_cells(1.0, 0.0, 0.0) == (0, 0) and pipeline.terrain_cells(2.0, 13.0, 3.0) == (4, 2)
    assert pipeline.terrain_cells(1.0, 128.0, 256.0) == (64, 256)
    with pytest.raises(ValueError, match="64 cells"):
        pipeline.terrain_cells(1.0, 128.5, 16.0)
    with pytest.raises(ValueError, match="256 cells"):
        pipeline.terrain_cells(1.0, 12.0, 256.5)
    for bad in ((0.0, 1.0, 1.0), (np.nan, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, np.inf)):
        with pytest.raises(ValueError):
            pipeline.terrain_cells(*bad)


# ------------------------------------------------------------------ the scene
def test_scene_numbers_and_margins():
    r = tc.reference()
    X, kind = tc.terrain_scene()
    g, state, ground = r["grid"], r["state"].reshape(-1), r["ground"].reshape(-1)
    assert len(X) == sp.LINE_ROWS + 3 * cc.TREE_ROWS + 45311 + 256 and (g["nx"], g["ny"]) == (199, 121)
    assert r["tol"] < 2e-5
    part, cell, _ = tc.takes_part(X, g)
    assert part.all()
    ncells = g["nx"] * g["ny"]
    has = lambda sel: np.bincount(cell[sel], minlength=ncells) > 0
    sheet, roof = has(kind == 20), has(kind == 21)
    # every cell with a ground-sheet row is accepted; no cell that holds only roof rows is, and all are filled
    assert sheet.sum() == 11492 and (state[sheet] == 5).all()
    only = roof & ~sheet & ~has(kind < 20)
    assert only.sum() == 61 and (state[only] == 6).all()
    assert {int(s): int((state == s).sum()) for s in np.unique(state)} == {0: 6504, 2: 6022, 5: 11492, 6: 61}
    # the model against the true ground at the cell centres
    a = np.radians(sp.LINE_AZIMUTH_DEG)
    xc, yc = np.meshgrid(g["x0"] + (np.arange(g["nx"]) + 0.5) * g["cell"], g["y0"] + (np.arange(g["ny"]) + 0.5) * g["cell"])
    truth = tc.sheet_z(xc * np.cos(a) + yc * np.sin(a), -xc * np.sin(a) + yc * np.cos(a)).reshape(-1)
    err = ground.astype(np.float64) - truth
    print(f"under the roof: {err[only].min():+.3f} .. {err[only].max():+.3f} m; sheet cells: "
          f"{err[sheet].min():+.3f} .. {err[sheet].max():+.3f} m")
    assert -0.07 < err[only].min() and err[only].max() < 0.05
    # a sheet cell's lowest return lies below its centre's ground by the slope over half a cell and the noise - except
    # where tower-foot rows, which line_scene places level with the tower's base, lie below the sloped sheet
    feet = sheet & has(kind == 0)
    assert np.abs(err[sheet & ~feet]).max() < 0.2 and -0.75 < err[feet].min() and (np.abs(err[feet]) > 0.2).sum() >= 1
    # heights: the sheet near 0, the roof near 6, every tree and conductor above the ground
    h = r["height"]
    assert not np.isnan(h).any()
    assert -0.1 < h[kind == 20].min() and h[kind == 20].max() < 0.45
    assert 5.4 < h[kind == 21].min() and h[kind == 21].max() < 6.6
    wires = (kind >= 1) & (kind <= 6)
    assert 17.0 < h[wires].min() < 19.0
    # the span table: six pieces, every vertex over ground, none within the limit; the three conductors of a span hang
    # at one height over a cross-slope, so the one over the highest ground reports the smallest clearance
    p = r["profile"]
    assert len(p["min_clearance"]) == 6 and (p["covered"] == tc.SEGMENTS + 1).all() and not p["violation"].any()
    assert 18.0 < p["min_clearance"].min() < p["min_clearance"].max() < 19.5
    assert (np.abs(p["min_vertex"] - tc.SEGMENTS // 2) <= 2).all()
    station = p["min_at"][:, 0] * np.cos(a) + p["min_at"][:, 1] * np.sin(a)
    for trio in (station < sp.LINE_STATIONS[1], station > sp.LINE_STATIONS[1]):
        by_ground = np.argsort(p["min_at"][trio, 2])
        assert trio.sum() == 3 and (np.diff(p["min_clearance"][trio][by_ground]) < 0).all()


def test_knob_parser_and_its_refusals():
    from pointcloudhookup_amd.utils import tower_extraction as te
    assert te.terrain_from_env(None) is None and te.terrain_from_env("  ") is None
    assert te.terrain_from_env(None, spans=False, frame="las") is None      # off needs nothing
    assert te.terrain_from_env("1, 12, 0.5") == dict(cell=1.0, window=12.0, dh=0.5, limit=7.0)
    assert te.terrain_from_env("0.5,12,0.25,6.5") == dict(cell=0.5, window=12.0, dh=0.25, limit=6.5)
    assert te.terrain_from_env("1,128,0") == dict(cell=1.0, window=128.0, dh=0.0, limit=7.0)
    for bad in ("1", "1,12", "1,12,0.5,7,8", "0,12,0.5", "-1,12,0.5", "inf,12,0.5", "1,-1,0.5", "1,nan,0.5", "1,12,-0.5",
                "1,12,inf", "1,12,0.5,nan", "1,129,0.5", "a,b,c"):
        with pytest.raises(ValueError):
            te.terrain_from_env(bad)
    with pytest.raises(ValueError, match="64 cells"):
        te.terrain_from_env("0.5,65,0.5")
    with pytest.raises(ValueError, match="PCH_SPANS"):
        te.terrain_from_env("1,12,0.5", spans=False)
    with pytest.raises(ValueError, match="PCH_FRAME"):
        te.terrain_from_env("1,12,0.5", frame="las")
    assert te.TERRAIN is None or te.SPANS is not None
    assert te.TERRAIN_COLUMNS[0] == "ID" and "min_clearance" in te.TERRAIN_COLUMNS


def test_knob_without_the_span_knob_or_in_the_las_frame_fails_at_import():
    """PCH_TERRAIN without PCH_SPANS, or with PCH_FRAME=las: a clear ValueError when the drop-in is imported (a fresh
    interpreter, since the knobs are read once at import)"""
    env = {k: v for k, v in os.environ.items() if k not in ("PCH_SPANS", "PCH_TERRAIN", "PCH_FRAME", "PCH_CLEARANCE")}
    code = "import pointcloudhookup_amd.utils.tower_extraction as te; print(te.TERRAIN)"
    run = lambda **kw: subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, **kw), capture_output=True,
                                      text=True)
    bad = run(PCH_TERRAIN="1,12,0.5")
    assert bad.returncode != 0 and "ValueError" in bad.stderr and "PCH_SPANS" in bad.stderr
    bad = run(PCH_TERRAIN="1,12,0.5", PCH_SPANS="1,5,9,20", PCH_FRAME="las")
    assert bad.returncode != 0 and "ValueError" in bad.stderr and "PCH_FRAME" in bad.stderr
    good = run(PCH_TERRAIN="1,12,0.5,6", PCH_SPANS="1,5,9,20")
    assert good.returncode == 0 and "'limit': 6.0" in good.stdout, good.stderr
    off = run()
    assert off.returncode == 0 and off.stdout.strip() == "None", off.stderr
