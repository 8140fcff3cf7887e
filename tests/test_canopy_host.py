"""Canopy grid and tree crowns on the CPU: the new symbols and workspace sizes, the header's lines, the numpy statement of
the rule (canopy_cases) against its independent second statements, identities of the rule, the scene's figures,
danger_trees_by_tree's records on hand-made inputs and the drop-in's knob (no kernel runs here)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import canopy_cases as cn
import terrain_cases as tc
import treefall_cases as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pch_canopy_top_ws_bytes", "pch_canopy_top_f32", "pch_canopy_trees_ws_bytes", "pch_canopy_trees_f32",
               "pch_canopy_rows_f32")


def test_new_symbols_and_workspace_bytes():
    from pointcloudhookup_amd import _lib, ops, pipeline
    header = open(os.path.join(ROOT, "include", "pch_hip.h"), encoding="utf-8").read()
    declared = set(re.findall(r"\b(pch_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    L = _lib.lib()
    top, trees = L.pch_canopy_top_ws_bytes, L.pch_canopy_trees_ws_bytes
    assert top(0, 1) > 0 and top(0, 1) == top(2 ** 31 - 1, 1)                 # per cell, not per row
    assert 8 * 2 ** 24 <= top(0, 2 ** 24) <= 8 * 2 ** 24 + 1024               # one 64-bit key per cell and the two figures
    for n, cells in ((-1, 1), (2 ** 31, 1), (1, 0), (1, -1), (1, 2 ** 24 + 1)):
        assert top(n, cells) == 0, (n, cells)
    # five 32-bit grids, the flags, one count per block of 256 cells and one key per table entry
    assert trees(1, 1) > 0 and 21 * 2 ** 24 + 8 <= trees(2 ** 24, 1) <= 21 * 2 ** 24 + 2 ** 18 + 4096
    assert trees(2 ** 24, 2 ** 20) - trees(2 ** 24, 1) == 8 * 2 ** 20 - 256
    for cells, cap in ((0, 1), (-1, 1), (2 ** 24 + 1, 1), (1, 0), (1, -1), (1, 2 ** 24 + 1)):
        assert trees(cells, cap) == 0, (cells, cap)
    assert ops.CANOPY_TILE == 1024
    assert (ops.CANOPY_MAX_SMOOTH, ops.CANOPY_MAX_WINDOW, ops.CANOPY_MAX_CROWN) == (8, 32, 256)
    assert (cn.MAX_SMOOTH, cn.MAX_WINDOW, cn.MAX_CROWN) == (8, 32, 256) and ops.CANOPY_TABLE_KEYS == cn.TABLE_KEYS
    for m in re.finditer(r"#define PCH_CANOPY_MAX_(SMOOTH|WINDOW|CROWN)\s+(\d+)", header):
        assert int(m.group(2)) == getattr(ops, "CANOPY_MAX_" + m.group(1))
    for name in ("check_canopy_rule", "canopy_grid", "canopy_top", "canopy_trees", "canopy_rows"):
        assert callable(getattr(ops, name)), name
    for name in ("tree_segments", "danger_trees_by_tree", "canopy_cells", "_by_tree_records"):
        assert callable(getattr(pipeline, name)), name
    # the rule is in the header word for word: the lines a reader checks the numpy statement against
    for line in ("g = g(X, Y) on the terrain grid;  Hd = Z - g;  H = (float)Hd",
                 "h_min <= Hd and Hd <= h_max",
                 "sum = sum + (double)top[c'];  cnt = cnt + 1",
                 "sm[c] = (float)(sum / (double)cnt)",
                 "c' beats c iff sm[c'] > sm[c], or sm[c'] == sm[c] and c' < c",
                 "r = r0 + (r1 * (double)sm[c]);  W = (int)floor(r / cell), clamped to [1, PCH_CANOPY_MAX_WINDOW]",
                 "(double)sm[c] >= (crown_frac * (double)sm[root[c]])",
                 "(key(H) << 32) | ~row"):
        assert line in header, line


def test_rule_checks_and_metres_to_cells():
    from pointcloudhookup_amd import ops, pipeline
    assert ops.check_canopy_rule(2, 45, 1, 1, 0.05, 5, 0.5, 16) == (2.0, 45.0, 1, 1.0, 0.05, 5.0, 0.5, 16)
    for bad in (dict(h_min=-1.0), dict(h_min=3.0, h_max=2.0), dict(h_max=np.inf), dict(smooth=9), dict(smooth=0.5),
                dict(r0=-0.1), dict(r1=np.nan), dict(top_min=-1.0), dict(crown_frac=1.5), dict(crown_cells=0),
                dict(crown_cells=257), dict(crown_cells=True)):
        with pytest.raises(ValueError):
            ops.check_canopy_rule(**bad)
    assert pipeline.canopy_cells(0.5, 8.0) == 16 and pipeline.canopy_cells(0.5, 0.0) == 1
    assert pipeline.canopy_cells(1.0, 2.5) == 3 and pipeline.canopy_cells(0.5, 128.0) == 256
    with pytest.raises(ValueError, match="256 cells"):
        pipeline.canopy_cells(0.5, 128.5)
    for bad in ((0.0, 1.0), (np.nan, 1.0), (1.0, -1.0), (1.0, np.inf)):
        with pytest.raises(ValueError):
            pipeline.canopy_cells(*bad)
    g = tc.grid(x0=-3.5, y0=2.25, cell=1.0, nx=199, ny=121)
    assert ops.canopy_grid(g, 0.5) == cn.canopy_grid_of(g, 0.5) == dict(cell=0.5, x0=-3.5, y0=2.25, nx=399, ny=243)
    with pytest.raises(ValueError, match="2\\^24"):
        ops.canopy_grid(tc.grid(cell=1.0, nx=4096, ny=4096), 0.5)
    with pytest.raises(ValueError):
        ops.canopy_grid(g, 0.0)


# ------------------------------------------------------------------ the two statements
def _case(nx, ny, n, seed):
    rng = np.random.default_rng(seed)
    cg = tc.grid(x0=-3.0, y0=2.0, cell=0.5, nx=nx, ny=ny)
    tx, ty = int(np.ceil(nx * 0.5 / 2.0)) + 2, int(np.ceil(ny * 0.5 / 2.0)) + 2
    tg = tc.grid(x0=-5.0, y0=0.0, cell=2.0, nx=tx, ny=ty)
    ground = rng.normal(0.0, 0.5, (ty, tx)).astype(np.float32)
    ground[rng.uniform(0, 1, ground.shape) < 0.08] = np.nan
    ground[1, 1] = 0.25                                                      # the canopy grid's first cell has ground
    X = np.stack([-3.0 + rng.uniform(-0.1, 1.1, n) * nx * 0.5, 2.0 + rng.uniform(-0.1, 1.1, n) * ny * 0.5,
                  np.round(rng.uniform(-1.0, 30.0, n) * 8.0) / 8.0], axis=1).astype(np.float32)
    for k, v in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
        X[(7 * k + 3) % n, k % 3] = v
    return tg, ground, cg, X


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (33, 17)])
def test_canopy_top_by_a_loop_and_by_a_sort(shape):
    tg, ground, cg, X = _case(shape[0], shape[1], 3000, seed=shape[0] * 100 + shape[1])
    skip = (np.arange(len(X)) % 5 == 0).astype(np.uint8)
    for sub, sk in ((None, None), (np.array([0.125, -0.125, 0.25], np.float32), skip)):
        a = cn.top_reference(X, tg, ground, cg, 2.0, 25.0, sub=sub, skip=sk)
        b = cn.top_by_sort(X, tg, ground, cg, 2.0, 25.0, sub=sub, skip=sk)
        for key in ("top", "top_row", "count", "height"):
            assert cn.same(a[key], b[key]), key
        part, cell, Hd, height = cn.takes_part(X, tg, ground, cg, 2.0, 25.0, sub=sub, skip=sk)
        assert a["count"].sum() == part.sum() and np.array_equal(np.isnan(a["top"]), a["count"] == 0)
        assert np.array_equal(a["top_row"] == -1, a["count"] == 0)
        assert cn.same(height, tc.height_reference(X, tg, ground, sub=sub)[0])       # terrain_height's, bit for bit
        rows = a["top_row"][a["count"] > 0]
        assert part[rows].all() and cn.same(height[rows], a["top"][a["count"] > 0])
        assert cn.same(cn.rows_reference(X, tg, ground, cg, 2.0, 25.0, a["top_row"], sub=sub, skip=sk)[part],
                       a["top_row"].reshape(-1)[cell[part]])
    assert 0 < part.sum() < len(X)


@pytest.mark.parametrize("W", [1, 2, 4, 32])
def test_tops_by_the_window_loop_and_by_a_sliding_maximum(W):
    tg, ground, cg, X = _case(33, 17, 4000, seed=W)
    t = cn.top_reference(X, tg, ground, cg, 2.0, 25.0)
    for S in (0, 1):
        seg = cn.segment_reference(t["top"], t["top_row"], t["count"], 0.5, S, 0.5 * W, 0.0, 5.0, 0.5, 8)
        live = ~np.isnan(seg["smooth"])
        assert (seg["window"][live] == W).all() and live.sum() > 300
        assert np.array_equal(seg["is_top"], cn.tops_by_sliding_maximum(seg["smooth"], W, 5.0))
        assert np.array_equal(seg["root"], cn.roots_by_union(seg["smooth"], seg["parent"]))
        assert seg["ntrees"] == seg["is_top"].sum() >= 1
    # ties: a lattice of equal values - the index decides, in both statements
    flat = np.full((9, 12), 7.0, np.float32)
    flat[4, 5:8] = np.nan
    seg = cn.segment_reference(flat, np.zeros_like(flat, np.int32), np.ones_like(flat, np.int32), 1.0, 0, float(W), 0.0,
                               5.0, 0.5, 8)
    assert np.array_equal(seg["is_top"], cn.tops_by_sliding_maximum(flat, W, 5.0)) and seg["ntrees"] == 1
    assert np.array_equal(seg["root"], cn.roots_by_union(flat, seg["parent"]))


# ------------------------------------------------------------------ identities
def _grid_case(top):
    top = np.asarray(top, dtype=np.float32)
    has = ~np.isnan(top)
    return dict(top=top, top_row=np.where(has, np.arange(top.size).reshape(top.shape), -1).astype(np.int32),
                count=has.astype(np.int32) * 3)


def test_identities_of_the_rule():
    rng = np.random.default_rng(5)
    top = rng.uniform(3.0, 20.0, (23, 31)).astype(np.float32)
    top[rng.uniform(0, 1, top.shape) < 0.2] = np.nan
    assert cn.same(cn.smooth_reference(top, 0), top)                          # S = 0 is the identity
    sm = cn.smooth_reference(top, 2)
    assert np.array_equal(np.isnan(sm), np.isnan(top))                        # empty cells are not filled
    assert np.nanmin(top) <= np.nanmin(sm) and np.nanmax(sm) <= np.nanmax(top)
    # a level plateau: exactly one top, the lowest-index cell; the crown is cut at Rc
    level = _grid_case(np.full((30, 40), 9.0, np.float32))
    seg = cn.segment_reference(**level, cell=0.5, S=1, r0=1.0, r1=0.0, top_min=5.0, crown_frac=0.5, Rc=8)
    dy, dx = np.mgrid[0:30, 0:40]
    assert seg["ntrees"] == 1 and seg["top_cell"].tolist() == [0] and (seg["root"] == 0).all()
    assert np.array_equal(seg["tree"] == 0, dx * dx + dy * dy <= 64) and seg["rows"][0] == 3 * seg["cells"][0]
    assert seg["max_height"][0] == 9.0 and seg["max_row"][0] == 0
    # W clamps at 1 and at 32
    assert cn.window_of(0.0, 0.5, 0.0, 0.0) == 1 and cn.window_of(10.0, 0.5, 0.0, 0.01) == 1
    assert cn.window_of(10.0, 0.5, 1.0, 0.05) == 3 and cn.window_of(10.0, 0.5, 16.0, 0.0) == 32
    assert cn.window_of(30.0, 0.5, 100.0, 1.0) == 32 and cn.window_of(np.inf, 0.5, 1.0, 0.0) == 1
    # crown_frac = 0: every cell whose root is a top within Rc; crown_frac = 1: only cells as tall as their top
    t = _grid_case(top)
    loose = cn.segment_reference(**t, cell=0.5, S=1, r0=1.0, r1=0.05, top_min=5.0, crown_frac=0.0, Rc=256)
    tight = cn.segment_reference(**t, cell=0.5, S=1, r0=1.0, r1=0.05, top_min=5.0, crown_frac=1.0, Rc=256)
    live = ~np.isnan(loose["smooth"]).reshape(-1)
    rooted = live & loose["is_top"].reshape(-1)[loose["root"]]
    assert np.array_equal(loose["tree"].reshape(-1) >= 0, rooted) and 1 < loose["ntrees"] == tight["ntrees"]
    assert (tight["cells"] >= 1).all() and tight["cells"].sum() < loose["cells"].sum() == rooted.sum()
    s = tight["smooth"].reshape(-1)
    own = np.flatnonzero(tight["tree"].reshape(-1) >= 0)
    assert (s[own] == s[tight["root"][own]]).all()
    # chains rise strictly: every parent beats its cell
    p = loose["parent"]
    moved = np.flatnonzero(p != np.arange(len(p)))
    assert ((s[p[moved]] > s[moved]) | ((s[p[moved]] == s[moved]) & (p[moved] < moved))).all()
    # the table is the crown's: cells, rows and the tallest top of every tree
    for k in range(loose["ntrees"]):
        mine = loose["tree"] == k
        assert loose["cells"][k] == mine.sum() and loose["rows"][k] == t["count"][mine].sum()
        assert loose["max_height"][k] == t["top"][mine].max() and mine.reshape(-1)[loose["top_cell"][k]]


def test_scene_figures_and_margins():
    r = cn.reference()
    X, kind, skip = cn.canopy_scene()
    assert r["share"] == cn.OVERLAP_RIGHT_SHARE and 0.4 < r["share"][0] / r["share"][1] < 0.8
    assert r["ntrees"] == 11 and (r["planted"] >= 0).sum() == 7 and len(set(r["stems"].tolist())) == 4
    cg = r["canopy_grid"]
    assert (cg["nx"], cg["ny"]) == (2 * r["grid"]["nx"] + 1, 2 * r["grid"]["ny"] + 1) and r["crown_cells"] == 16
    names = [p[0] for p in cn.PLANTED]
    # heights: every tree's tallest return within 0.35 m of what was planted (the ground model and the jitter)
    for name, _, _, height, _, _ in cn.PLANTED:
        k = r["planted"][names.index(name)]
        if k >= 0:
            assert abs(float(r["max_height"][k]) - height) < 0.35, (name, r["max_height"][k])
    for (name, _, _, top), k in zip(tf.STEMS, r["stems"]):
        assert abs(float(r["max_height"][k]) - top) < 0.6 and r["cells"][k] <= 4, name
    # the twin crown is one tree that holds the rows of both maxima
    twin = r["planted"][names.index("twin")]
    assert (r["row_tree"][r["part"] & (kind == 50 + names.index("twin"))] == twin).all()
    # crown areas: a paraboloid of radius R, cut at half its top's height, covers at most pi R^2
    for name, _, _, _, radius, _ in cn.PLANTED:
        k = r["planted"][names.index(name)]
        if k >= 0:
            assert 4 < r["cells"][k] * cn.CELL ** 2 < np.pi * (radius + 1.0) ** 2, name
    # skipped rows and rows below h_min carry no tree
    assert (r["row_tree"][skip != 0] == -1).all() and (r["row_tree"][kind == 20] == -1).all()
    assert (r["row_tree"] >= 0).sum() == r["rows"].sum()


# ------------------------------------------------------------------ danger_trees_by_tree on hand-made inputs
def test_hazard_rows_per_tree_on_hand_made_inputs():
    from pointcloudhookup_amd import pipeline
    rows = np.array([3, 8, 9, 20, 21, 40, 41])
    xyz = np.array([[1.0, 1.0, 9], [1.2, 1.1, 12], [1.4, 0.9, 11], [30.0, 5.0, 8], [30.5, 5.5, 7], [50.1, 9.0, 6],
                    [57.0, 9.0, 6]], dtype=np.float32)
    under = np.zeros(7)
    height = np.array([9, 12, 11, 8, 7, 6, 6], dtype=np.float32)
    span = np.array([2, 2, 2, 0, 0, 1, 1], dtype=np.int32)
    dist2 = np.array([100.0, 144.0, 100.0, 81.0, 49.0, 49.0, 36.0])
    hazard = np.array([2, 2, 2, 1, 2, 1, 1], dtype=np.uint8)
    row_tree = np.array([4, 4, 4, 1, 1, -1, -1], dtype=np.int32)
    trees = dict(max_row=np.arange(100, 105), x=np.arange(5.0), y=np.arange(5.0) * 2, ground=np.full(5, 0.5),
                 max_height=np.array([0, 8.5, 0, 0, 12.5], np.float32))
    recs = pipeline._by_tree_records(rows, xyz, under, height, span, dist2, hazard, row_tree, trees, 2.0, 1.0)
    assert [tuple(r) for r in recs] == [pipeline.BY_TREE_KEYS] * 4
    assert [(r["span"], r["tree"]) for r in recs] == [(0, 1), (1, -1), (1, -1), (2, 4)]
    assert sum(r["rows"] for r in recs) == len(rows)                          # no hazard row is lost
    a, f1, f2, b = recs
    assert (a["row"], a["rows"], a["strikes"], a["hazard"], a["min_row"]) == (101, 2, 1, 2, 21)
    assert a["margin"] == 7.0 - (7.0 + 1.0) and a["distance"] == 7.0 and (a["x"], a["y"], a["height"]) == (1.0, 2.0, 8.5)
    # margins 10 - (9 + 1), 12 - (12 + 1) and 10 - (11 + 1): row 9 has the smallest
    assert (b["row"], b["rows"], b["strikes"], b["min_row"], b["margin"], b["span"]) == (104, 3, 3, 9, -2.0, 2)
    assert (f1["row"], f2["row"]) == (40, 41) and f1["rows"] == f2["rows"] == 1 and f1["min_row"] == 40
    assert f1["margin"] == 7.0 - (6.0 + 1.0) and f2["margin"] == 6.0 - 7.0
    # a tie for the smallest margin goes to the lowest row: 9 - (8 + 1) and 8 - (7 + 1)
    tied = pipeline._by_tree_records(rows, xyz, under, height, span, np.where(rows == 21, 64.0, dist2), hazard, row_tree,
                                     trees, 2.0, 1.0)
    assert (tied[0]["tree"], tied[0]["min_row"], tied[0]["margin"], tied[0]["distance"]) == (1, 20, 0.0, 9.0)
    # the records of no tree are _tree_records' own, bin for bin
    free = row_tree < 0
    plain = pipeline._tree_records(rows[free], xyz[free], under[free], height[free], span[free], dist2[free],
                                   hazard[free], 2.0, 1.0)
    assert [(p["row"], p["margin"], p["x"]) for p in plain] == [(f["row"], f["margin"], f["x"]) for f in (f1, f2)]
    # two free rows in one 2 m cell: one record that counts both
    xyz[6, 0] = 50.9
    recs = pipeline._by_tree_records(rows, xyz, under, height, span, dist2, hazard, row_tree, trees, 2.0, 1.0)
    assert len(recs) == 3 and recs[1]["tree"] == -1 and recs[1]["rows"] == 2 and recs[1]["row"] == 40
    assert pipeline._by_tree_records(rows[:0], xyz[:0], under[:0], height[:0], span[:0], dist2[:0], hazard[:0],
                                     row_tree[:0], trees, 2.0, 0.0) == []


# ------------------------------------------------------------------ the drop-in's knob
def test_knob_parser_and_its_refusals():
    from pointcloudhookup_amd.utils import tower_extraction as te
    assert te.trees_from_env(None) is None and te.trees_from_env("  ") is None
    assert te.trees_from_env(None, terrain=False, frame="las") is None       # off needs nothing
    assert te.trees_from_env("0.5, 5") == dict(cell=0.5, top_min=5.0, crown_radius=8.0, smooth=1)
    assert te.trees_from_env("1,4,10,0") == dict(cell=1.0, top_min=4.0, crown_radius=10.0, smooth=0)
    assert te.trees_from_env("0.5,5,128,8") == dict(cell=0.5, top_min=5.0, crown_radius=128.0, smooth=8)
    for bad in ("0.5", "0.5,5,8,1,2", "0,5", "-1,5", "inf,5", "0.5,-1", "0.5,nan", "0.5,5,-1", "0.5,5,inf", "0.5,5,8,9",
                "0.5,5,8,0.5", "0.5,5,8,-1", "a,b"):
        with pytest.raises(ValueError):
            te.trees_from_env(bad)
    with pytest.raises(ValueError, match="256 cells"):
        te.trees_from_env("0.5,5,128.5")
    with pytest.raises(ValueError, match="PCH_TERRAIN"):
        te.trees_from_env("0.5,5", terrain=False)
    with pytest.raises(ValueError, match="PCH_FRAME"):
        te.trees_from_env("0.5,5", frame="las")
    assert te.TREES is None or te.TERRAIN is not None
    assert te.TREES_COLUMNS[0] == "ID" and "crown_area" in te.TREES_COLUMNS and "margin" in te.TREES_FALL_COLUMNS


def test_knob_without_the_terrain_knob_or_in_the_las_frame_fails_at_import():
    """PCH_TREES without PCH_TERRAIN, or with PCH_FRAME=las: a clear ValueError when the drop-in is imported (a fresh
    interpreter, since the knobs are read once at import)"""
    drop = ("PCH_SPANS", "PCH_TERRAIN", "PCH_FRAME", "PCH_CLEARANCE", "PCH_TREEFALL", "PCH_TREES")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    code = "import pointcloudhookup_amd.utils.tower_extraction as te; print(te.TREES)"
    run = lambda **kw: subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, **kw), capture_output=True,
                                      text=True)
    bad = run(PCH_TREES="0.5,5")
    assert bad.returncode != 0 and "ValueError" in bad.stderr and "PCH_TERRAIN" in bad.stderr
    bad = run(PCH_TREES="0.5,5", PCH_TERRAIN="1,12,0.5", PCH_SPANS="1,5,9,20", PCH_FRAME="las")
    assert bad.returncode != 0 and "ValueError" in bad.stderr and "PCH_FRAME" in bad.stderr
    good = run(PCH_TREES="0.5,5,6", PCH_TERRAIN="1,12,0.5", PCH_SPANS="1,5,9,20")
    assert good.returncode == 0 and "'crown_radius': 6.0" in good.stdout, good.stderr
    off = run()
    assert off.returncode == 0 and off.stdout.strip() == "None", off.stderr
