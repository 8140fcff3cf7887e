"""Tree fall on the CPU: the new symbols and the workspace size, the header's lines, the two numpy statements of the rule
(treefall_cases) against each other on the rule's boundaries, the scene's numbers, the binning of hazard rows into
``trees`` records and the drop-in's knob (no kernel runs here)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import terrain_cases as tc
import treefall_cases as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pch_treefall_ws_bytes", "pch_treefall_f32")


def test_new_symbols_and_workspace_bytes():
    from pointcloudhookup_amd import _lib, ops, pipeline
    header = open(os.path.join(ROOT, "include", "pch_hip.h"), encoding="utf-8").read()
    declared = set(re.findall(r"\b(pch_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    L = _lib.lib()
    ws = L.pch_treefall_ws_bytes
    assert ws(0, 0, 1) > 0 and ws(0, 0, 1) == ws(10 ** 8, 1, 128)            # per span, not per row
    assert ws(0, 4096, 128) > ws(0, 1, 128) and ws(2 ** 31 - 1, 4096, 128) == ws(0, 4096, 1)
    assert ws(0, 4096, 128) <= 4096 * 128                                     # tallies, bounds and a flag per span
    for n, K, S in ((-1, 1, 1), (2 ** 31, 1, 1), (1, -1, 1), (1, 4097, 1), (1, 1, 0), (1, 1, 129)):
        assert ws(n, K, S) == 0, (n, K, S)
    assert ops.TREEFALL_TILE == 1024 and ops.TREEFALL_OUTPUTS == tf.OUTPUTS
    assert (ops.TREEFALL_CLEAR, ops.TREEFALL_NEAR, ops.TREEFALL_STRIKE) == (tf.CLEAR, tf.NEAR, tf.STRIKE) == (0, 1, 2)
    assert callable(ops.treefall) and callable(pipeline.danger_trees)
    assert pipeline.TREEFALL_TABLE_KEYS == ("count", "strikes", "min_distance", "min_row", "max_height", "max_row",
                                            "chord_error")
    assert pipeline.TREEFALL_TREE_KEYS == tf.TREE_KEYS
    for bad in ((-1.0, 45.0, 0.0, 3.0), (3.0, 2.0, 0.0, 3.0), (2.0, 45.0, -0.5, 3.0), (2.0, 45.0, 0.0, -1.0),
                (float("nan"), 45.0, 0.0, 3.0), (2.0, float("inf"), 0.0, 3.0), (2.0, 45.0, float("inf"), 3.0),
                (2.0, 45.0, 0.0, float("nan"))):
        with pytest.raises(ValueError):
            ops.check_treefall_rule(*bad)
    assert ops.check_treefall_rule(0, 0, 0, 0) == (0.0, 0.0, 0.0, 0.0)


def test_the_rule_is_in_the_header_word_for_word():
    """the lines a reader checks the numpy statement against, and the three class constants"""
    header = open(os.path.join(ROOT, "include", "pch_hip.h"), encoding="utf-8").read()
    at = header.index("tree fall, opt-in (DESIGN.md 5h)")
    rule = header[at:header.index("pch_treefall_f32(", at)]
    for line in ("H = Z - g", "h_min <= H and H <= h_max", "reach = H + grow;  s2 = reach*reach",
                 "R = reach + limit;  R2 = R*R", "dx = X - cx;  dy = Y - cy;  w = g - cz",
                 "m = (dx*ux) + (dy*uy);  t = (dy*ux) - (dx*uy)", "q = ((rm*dm_j) + (rw*dz_j))*inv_j",
                 "em = rm - (q*dm_j);  ew = rw - (q*dz_j)", "d2 = gmin + (t*t)",
                 "if d2 <= R2 and d2 < best: best = d2; who = k", "Ties go to the lowest k",
                 "P = fl32(xyz[i] - sub3)", "all 5 + 5*S of its values are finite", "tallied as uncovered",
                 "PCH_TREEFALL_NEAR   = 1: best <= R2 and best > s2", "PCH_TREEFALL_STRIKE = 2: best <= s2",
                 "0 <= h_min <= h_max, grow >= 0 and limit >= 0", "NEAREST span within its own R only"):
        assert line in rule, line
    for name, value in (("PCH_TREEFALL_CLEAR", tf.CLEAR), ("PCH_TREEFALL_NEAR", tf.NEAR),
                        ("PCH_TREEFALL_STRIKE", tf.STRIKE)):
        assert re.search(rf"#define {name}\s+{value}\b", header), name


def _both(X, g, ground, curves, segs, h_min, h_max, grow, limit, sub=None, skip=None):
    """the looped statement, and the vectorised one checked against it bit for bit"""
    want = tf.treefall_reference(X, g, ground, curves, segs, h_min, h_max, grow, limit, sub=sub, skip=skip)
    F, H, fin = tf.feet(X, g, ground, sub)
    part, bare = tf.takes_part(X, H, fin, h_min, h_max, skip)
    s2, R2 = tf.reach_of(H, grow, limit)
    best, who, hazard = tf.treefall_by_argmin(F, H, part, tf.foot_distances(F, curves, segs), s2, R2)
    assert tc.same(best, want["dist2"]) and np.array_equal(who, want["span"]) and np.array_equal(hazard, want["hazard"])
    assert want["stats"].tolist() == [int(part.sum()), int(bare.sum())]
    T = tf.table_of(best, who, hazard, tf.height32(H), np.asarray(segs).shape[0])
    for key, v in T.items():
        assert tc.same(v, want[key]), key
    return want


def test_statements_agree_on_the_boundaries_of_the_rule():
    g, ground, curves, segs = tf.level_case()
    X, skip = tf.boundary_rows()
    out = _both(X, g, ground, curves, segs, 2.0, 12.0, 0.0, 3.0, skip=skip)
    assert tuple(out["hazard"].tolist()) == tf.BOUNDARY_HAZARD and tuple(out["span"].tolist()) == tf.BOUNDARY_SPAN
    assert out["dist2"][[0, 1, 2, 6]].tolist() == [100.0] * 4 and out["dist2"][14] == 80.0
    assert np.isinf(out["dist2"][[3, 4, 5, 7, 8, 9, 10, 11, 12, 13]]).all()
    assert out["stats"].tolist() == [7, 1]
    assert np.isnan(out["height"][[8, 9, 10, 11, 13]]).all() and out["height"][12] == 10.0 and out["height"][5] < 2.0
    assert out["count"].tolist() == [4, 0, 0, 1] and out["strikes"].tolist() == [2, 0, 0, 1]
    assert out["min_row"].tolist() == [0, -1, -1, 14] and out["max_row"].tolist() == [6, -1, -1, 14]
    assert out["max_height"][0] == 12.0 and np.isnan(out["max_height"][1:3]).all()
    # limit = 0: R2 == s2, class 1 is empty; grow: the reach grows, the height does not
    zero = _both(X, g, ground, curves, segs, 2.0, 12.0, 0.0, 0.0, skip=skip)
    assert set(zero["hazard"].tolist()) == {0, 2} and zero["hazard"][[0, 1, 2]].tolist() == [2, 0, 0]
    grown = _both(X, g, ground, curves, segs, 2.0, 12.0, 3.0, 0.0, skip=skip)
    assert grown["hazard"][[0, 1, 2, 3]].tolist() == [2, 2, 2, 0] and tc.same(grown["height"], out["height"])
    # NaN ground under the rows: nothing takes part, every finite row that is not skipped is uncovered
    holes = np.full_like(ground, np.nan)
    none = _both(X, g, holes, curves, segs, 2.0, 12.0, 0.0, 3.0, skip=skip)
    assert none["stats"].tolist() == [0, 10] and (none["span"] == -1).all() and np.isnan(none["height"]).all()
    # sub3: the rows whose shift is exact in float32, given in another frame
    sub = np.array([512.0, -256.0, 64.0], dtype=np.float32)
    exact = np.array([0, 2, 4, 6, 8, 9, 10, 11, 12, 13, 14])
    here = _both(X[exact], g, ground, curves, segs, 2.0, 12.0, 0.0, 3.0, skip=skip[exact])
    moved = _both((X[exact] + sub).astype(np.float32), g, ground, curves, segs, 2.0, 12.0, 0.0, 3.0, sub=sub,
                  skip=skip[exact])
    for key in tf.OUTPUTS:
        assert tc.same(moved[key], here[key]), key
    # no span, no row
    empty = _both(X, g, ground, curves[:0], segs[:0], 2.0, 12.0, 0.0, 3.0)
    assert (empty["span"] == -1).all() and len(empty["count"]) == 0 and tc.same(empty["height"][:8], out["height"][:8])
    assert len(_both(X[:0], g, ground, curves, segs, 2.0, 12.0, 0.0, 3.0)["dist2"]) == 0


def test_heights_are_the_terrain_rule_s():
    rng = np.random.default_rng(3)
    g = tc.grid(x0=-3.0, y0=1.0, cell=0.75, nx=13, ny=9)
    ground = rng.normal(0.0, 2.0, (9, 13)).astype(np.float32)
    ground[rng.uniform(size=ground.shape) < 0.2] = np.nan
    X = np.stack([rng.uniform(-4.0, 8.0, 500), rng.uniform(0.0, 9.0, 500), rng.normal(5.0, 5.0, 500)],
                 axis=1).astype(np.float32)
    X[::37, 1] = np.nan
    _, H, _ = tf.feet(X, g, ground)
    assert tc.same(tf.height32(H), tc.height_reference(X, g, ground)[0])


def test_scene_numbers_and_margins():
    r = tf.reference()
    X, kind, keep = tf.stem_scene()
    assert len(r["points"]) == int(keep.sum()) and 4e-6 < r["tol"] < 7e-6
    pk, hz, tops = r["kind"], r["hazard"], r["tops"]
    # only stem rows are hazards: the cones stand under the wires, lower than the wires hang above their feet
    assert set(np.unique(pk[hz > 0]).tolist()) == {40, 41, 43}
    assert hz[tops].tolist() == [tf.STRIKE, tf.NEAR, tf.CLEAR, tf.NEAR]
    dist, h = np.sqrt(r["dist2"][tops]), r["height"][tops].astype(np.float64)
    assert dist[0] < h[0] and h[1] < dist[1] < h[1] + tf.LIMIT and np.isinf(dist[2]) and h[3] < dist[3] < h[3] + tf.LIMIT
    # "far" is tall but too far away for its own R; "bank" stands higher than the lowest point of its wire
    far = np.sqrt(r["d2"][:, tops[2]].min())
    assert h[2] > h[1] and far > h[2] + tf.LIMIT
    k = r["span"][tops[3]]
    wire_low = r["curves"][k, 2] + (r["segs"][k, :, 1]).min()
    assert r["under"][tops[3]] > wire_low + 2.0 and r["points"][tops[3], 2] - wire_low > h[3] + tf.LIMIT
    assert r["count"].sum() == (hz > 0).sum() and r["strikes"].sum() == (hz == tf.STRIKE).sum() == 13
    for k in np.flatnonzero(r["count"]):
        assert r["span"][r["min_row"][k]] == k and r["dist2"][r["min_row"][k]] == r["min_dist2"][k]
        assert r["span"][r["max_row"][k]] == k and r["height"][r["max_row"][k]] == r["max_height"][k]
    assert r["stats"][1] == 0 and r["stats"][0] == r["part"].sum()
    # the trees: one record per stem that is a hazard - the stems are thinner than a cell, but may straddle two
    recs = r["trees"]
    assert 3 <= len(recs) <= 6
    assert {int(pk[t["row"]]) for t in recs} == {40, 41, 43}
    assert [(t["span"], t["row"]) for t in recs] == sorted((t["span"], t["row"]) for t in recs)
    for t in recs:
        assert abs(t["margin"] - (t["distance"] - t["height"] - tf.GROW)) < 1e-12 and (t["margin"] <= 0) == (t["hazard"] == 2)


def test_trees_binning_on_a_hand_made_case():
    from pointcloudhookup_amd import pipeline
    #        x     y     z      height span  dist2  hazard
    rows = [(0.5, 0.5, 10.0, 9.0, 1, 64.0, 2),       # 0: cell (0, 0)
            (1.5, 1.5, 12.0, 11.0, 1, 100.0, 2),     # 1: cell (0, 0), the tallest there
            (1.9, 0.1, 12.0, 11.0, 0, 144.0, 1),     # 2: cell (0, 0), as tall: the lower row (1) stays
            (2.0, 0.0, 5.0, 4.0, 0, 36.0, 1),        # 3: cell (1, 0), on the edge
            (-0.1, 0.0, 6.0, 5.0, 2, 25.0, 2),       # 4: cell (-1, 0)
            (-1.9, 1.9, 7.0, 6.5, 0, 49.0, 1),       # 5: cell (-1, 0), taller
            (9.0, 9.0, 30.0, 29.0, 0, 16.0, 0),      # 6: no hazard
            (2.5, 1.0, 5.0, 4.0, 0, 36.0, 2)]        # 7: cell (1, 0), as tall as 3: 3 stays
    a = np.array(rows)
    X, height = a[:, :3].astype(np.float32), a[:, 3].astype(np.float32)
    span, dist2, hazard = a[:, 4].astype(np.int32), a[:, 5].copy(), a[:, 6].astype(np.uint8)
    under = X[:, 2].astype(np.float64) - height
    want = tf.trees_reference(X, under, height, span, dist2, hazard, 2.0, 0.5)
    assert [t["row"] for t in want] == [3, 5, 1]                                   # by (span, row)
    sel = np.flatnonzero(hazard >= 1)
    got = pipeline._tree_records(sel, X[sel], under[sel], height[sel], span[sel], dist2[sel], hazard[sel], 2.0, 0.5)
    assert got == want and tuple(got[0]) == pipeline.TREEFALL_TREE_KEYS
    assert got[2] == dict(row=1, x=1.5, y=1.5, ground=1.0, height=11.0, span=1, distance=10.0, margin=-1.5, hazard=2)
    assert pipeline._tree_records(sel[:0], X[:0], under[:0], height[:0], span[:0], dist2[:0], hazard[:0], 2.0, 0.0) == []


def test_knob_parser_and_its_refusals():
    from pointcloudhookup_amd.utils import tower_extraction as te
    assert te.treefall_from_env(None) is None and te.treefall_from_env("  ") is None
    assert te.treefall_from_env(None, spans=False, terrain=False, frame="las") is None      # off needs nothing
    assert te.treefall_from_env("2, 3") == dict(h_min=2.0, limit=3.0, grow=0.0, h_max=45.0)
    assert te.treefall_from_env("2,3,1.5") == dict(h_min=2.0, limit=3.0, grow=1.5, h_max=45.0)
    assert te.treefall_from_env("0,0,0,0") == dict(h_min=0.0, limit=0.0, grow=0.0, h_max=0.0)
    assert te.treefall_from_env("5,3,1,60") == dict(h_min=5.0, limit=3.0, grow=1.0, h_max=60.0)
    for bad in ("2", "2,3,1,45,6", "-1,3", "2,-3", "2,3,-1", "50,3", "5,3,0,4", "nan,3", "2,inf", "2,3,nan", "2,3,0,inf",
                "a,b"):
        with pytest.raises(ValueError):
            te.treefall_from_env(bad)
    with pytest.raises(ValueError, match="PCH_SPANS"):
        te.treefall_from_env("2,3", spans=False)
    with pytest.raises(ValueError, match="PCH_TERRAIN"):
        te.treefall_from_env("2,3", terrain=False)
    with pytest.raises(ValueError, match="PCH_FRAME=las"):
        te.treefall_from_env("2,3", frame="las")
    assert te.TREEFALL is None or (te.SPANS is not None and te.TERRAIN is not None)
    assert te.TREEFALL_COLUMNS[0] == "ID" and "margin" in te.TREEFALL_COLUMNS and "hazard" in te.TREEFALL_COLUMNS


def test_knob_without_its_neighbours_fails_at_import():
    """PCH_TREEFALL without PCH_SPANS or PCH_TERRAIN, or with PCH_FRAME=las: a clear ValueError when the drop-in is
    imported (a fresh interpreter, since the knobs are read once at import)"""
    env = {k: v for k, v in os.environ.items()
           if k not in ("PCH_SPANS", "PCH_CLEARANCE", "PCH_TERRAIN", "PCH_TREEFALL", "PCH_FRAME")}
    code = "import pointcloudhookup_amd.utils.tower_extraction as te; print(te.TREEFALL)"
    run = lambda **kw: subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, **kw), capture_output=True,
                                      text=True)
    bad = run(PCH_TREEFALL="2,3")
    assert bad.returncode != 0 and "ValueError" in bad.stderr and "PCH_SPANS" in bad.stderr
    bad = run(PCH_TREEFALL="2,3", PCH_SPANS="1,5,9,20")
    assert bad.returncode != 0 and "ValueError" in bad.stderr and "PCH_TERRAIN" in bad.stderr
    bad = run(PCH_TREEFALL="2,3", PCH_SPANS="1,5,9,20", PCH_TERRAIN="1,12,0.5", PCH_FRAME="las")
    assert bad.returncode != 0 and "ValueError" in bad.stderr
    good = run(PCH_TREEFALL="2,3,1.5", PCH_SPANS="1,5,9,20", PCH_TERRAIN="1,12,0.5")
    assert good.returncode == 0 and "'grow': 1.5" in good.stdout, good.stderr
    off = run()
    assert off.returncode == 0 and off.stdout.strip() == "None"
