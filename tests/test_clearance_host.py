"""Conductor clearance on the CPU: the numpy statement of the rule (clearance_cases) against an independent statement,
the torch twins of the curve and segment tables against it, the scene's numbers and margins, the drop-in's knob, the
new symbols and the workspace size (no kernel runs here)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import clearance_cases as cc
import span_cases as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
NEW_SYMBOLS = ("pch_clearance_ws_bytes", "pch_clearance_f32")


def test_reference_against_point_to_polyline_in_space():
    """the rule measures in the span's frame (m, w, t); the same distance taken with np.linalg.norm on world-space
    vertices agrees within a few ulps of the scene's scale"""
    r = cc.reference()
    X, _ = cc.tree_scene()
    P = X.astype(np.float64)
    V = cc.polyline_world(r["curves"], cc.SEGMENTS)
    scale = float(np.abs(P).max() + np.abs(r["curves"][:, 8:10]).max())
    worst = 0.0
    for k in range(len(V)):
        want = cc.polyline_distance(P, V[k])
        got = np.sqrt(r["d2"][k])
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"frame statement against the statement in space: worst difference {worst:.3e} m at scale {scale:.1f} m "
          f"({worst / (U * scale):.1f} u)")
    # either statement takes a dozen roundings of quantities up to `scale`; 64 u of it leaves room for both
    assert worst <= 64.0 * U * scale


def test_polyline_lies_within_chord_error_of_the_curve():
    """distances to the 32-segment polyline against a 4096-segment one: they differ by at most chord_error, the bound
    |c|·((m1 - m0)/S)²/4 - and the finer polyline is never the farther one from a row below the wire"""
    r = cc.reference()
    X, kind = cc.tree_scene()
    some = (kind >= 10) | (np.arange(len(X)) % 16 == 0)                      # the trees and every sixteenth row
    P, kind = X[some].astype(np.float64), kind[some]
    fine = cc.polyline_world(r["curves"], 4096)
    coarse = cc.polyline_world(r["curves"], cc.SEGMENTS)
    worst, bound = 0.0, 0.0
    for k in range(len(fine)):
        d32, d4096 = cc.polyline_distance(P, coarse[k]), cc.polyline_distance(P, fine[k])
        diff = np.abs(d32 - d4096)
        assert (diff <= r["chord"][k] + 1e-12).all(), (k, diff.max(), r["chord"][k])
        below = (kind >= 10) & (d32 <= cc.RADIUS)
        assert (d32[below] >= d4096[below] - 1e-12).all()                    # over-estimated, never under
        worst, bound = max(worst, float(diff.max())), max(bound, float(r["chord"][k]))
    print(f"S = 32 against S = 4096: largest difference {worst * 1e3:.3f} mm, largest bound {bound * 1e3:.3f} mm")
    assert 0.5 * bound < worst <= bound                                      # (the bound is not slack: /8 would fail)


def test_torch_twins_give_the_reference_tables_bit_for_bit():
    from pointcloudhookup_amd import ops
    r = cc.reference()
    spans = r["spans"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    T = spans["table"]
    curves = ops._span_curves_of(t(T["a"]), t(T["b"]), t(T["c"]), t(spans["frames"]), t(spans["ext"]))
    want = cc.curves_reference(T, spans["frames"], spans["ext"])
    assert curves.dtype == torch.float64 and curves.shape == want.shape
    assert np.array_equal(curves.numpy().view(np.uint64), want.view(np.uint64))
    # every entry of a segment table is one correctly rounded IEEE operation on the ones before it - add, multiply,
    # divide, none fused across torch calls -, so torch's CPU arithmetic has no room to differ from numpy's
    extra = np.stack([cc.curve(a=3.0, b=-0.01, c=0.004, m0=-150.0, m1=170.0), cc.curve(m0=2.0, m1=2.0),
                      cc.curve(a=1.0, c=0.5, m0=-1.0, m1=1.0)])
    for S in (1, 2, 7, 32, 128):
        for C in (r["curves"], extra):
            segs, chord = ops._span_segments_of(t(C), S)
            ws, wc = cc.segments_reference(C, S)
            assert segs.shape == (len(C), S, 5) and chord.shape == (len(C),)
            assert np.array_equal(segs.numpy().view(np.uint64), ws.view(np.uint64)), S
            assert np.array_equal(chord.numpy().view(np.uint64), wc.view(np.uint64)), S
    segs, _ = cc.segments_reference(extra, 4)
    assert (segs[1, :, 2:] == 0).all() and (segs[1, :, 0] == 2.0).all()      # m0 == m1: no length, inv = 0
    for bad in (0, 129, 2.5, True):
        with pytest.raises(ValueError):
            ops.check_segments(bad)


def test_scene_numbers_and_margins():
    r = cc.reference()
    X, kind = cc.tree_scene()
    assert len(X) == sp.LINE_ROWS + 3 * cc.TREE_ROWS and 4e-6 < r["tol"] < 7e-6
    # only tree rows come within the radius: the conductors and the rows at the towers are skipped, the blob and the
    # bar stand 16 m and more aside
    near = r["span"] >= 0
    assert set(np.unique(kind[near]).tolist()) == {10, 11, 12}
    dist = np.sqrt(r["dist2"])
    breach, beside, between = (kind == 10), (kind == 11), (kind == 12)
    assert dist[breach].min() < cc.LIMIT and (dist[breach] <= cc.LIMIT).sum() > 10
    assert cc.LIMIT < dist[beside].min() < cc.RADIUS                        # inside the radius, outside the limit
    assert len(np.unique(r["span"][between & near])) == 2                   # attributed to two conductors
    assert r["count"].sum() == near.sum() and (r["count"] > 0).sum() == 3
    assert r["violations"].sum() == (dist <= cc.LIMIT).sum() > 0
    violated = set(np.flatnonzero(r["violations"]).tolist())
    assert violated == set(np.unique(r["span"][breach & near]).tolist())    # the pieces above the breaching tree
    for k in np.flatnonzero(r["count"]):
        assert r["span"][r["min_row"][k]] == k and r["dist2"][r["min_row"][k]] == r["min_dist2"][k]
    assert (r["min_row"][r["count"] == 0] == -1).all() and np.isinf(r["min_dist2"][r["count"] == 0]).all()
    assert (r["chord"] < 2e-3).all() and (r["chord"] > 1e-3).all()


def test_reference_handles_skips_ties_and_spans_that_take_no_part():
    C = np.stack([cc.curve(cy=-1.0), cc.curve(cy=1.0), cc.curve(cy=-1.0), cc.curve(a=np.nan)])
    segs, _ = cc.segments_reference(C, 4)
    X = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, 30.0, 0.0]], dtype=np.float32)
    out = cc.clearance_reference(X, C, segs, 10.0, 1.0, skip=np.array([0, 1, 0, 0], dtype=np.uint8))
    assert out["span"].tolist() == [0, -1, -1, -1] and out["dist2"][0] == 1.0 and np.isinf(out["dist2"][1:]).all()
    assert out["count"].tolist() == [1, 0, 0, 0] and out["violations"].tolist() == [1, 0, 0, 0]
    assert out["min_row"].tolist() == [0, -1, -1, -1]


def test_knob_parser_and_its_refusals():
    from pointcloudhookup_amd.utils import tower_extraction as te
    assert te.clearance_from_env(None) is None and te.clearance_from_env("  ") is None
    assert te.clearance_from_env(None, spans=False) is None                 # off needs nothing
    assert te.clearance_from_env("10, 6") == dict(radius=10.0, limit=6.0, segments=32)
    assert te.clearance_from_env("10,6,64") == dict(radius=10.0, limit=6.0, segments=64)
    assert te.clearance_from_env("6,6,1") == dict(radius=6.0, limit=6.0, segments=1)
    for bad in ("10", "10,6,32,1", "0,0", "-1,1", "10,0", "10,11", "inf,6", "10,nan", "10,6,0", "10,6,129", "10,6,2.5",
                "a,b"):
        with pytest.raises(ValueError):
            te.clearance_from_env(bad)
    with pytest.raises(ValueError, match="PCH_SPANS"):
        te.clearance_from_env("10,6", spans=False)
    assert te.CLEARANCE is None or te.SPANS is not None
    assert te.CLEARANCE_COLUMNS[0] == "ID" and "min_distance" in te.CLEARANCE_COLUMNS


def test_knob_without_the_span_knob_fails_at_import():
    """PCH_CLEARANCE without PCH_SPANS: a clear ValueError when the drop-in is imported (a fresh interpreter, since the
    knobs are read once at import)"""
    env = {k: v for k, v in os.environ.items() if k not in ("PCH_SPANS", "PCH_CLEARANCE")}
    code = "import pointcloudhookup_amd.utils.tower_extraction as te; print(te.CLEARANCE)"
    bad = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, PCH_CLEARANCE="10,6"),
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "ValueError" in bad.stderr and "PCH_SPANS" in bad.stderr
    good = subprocess.run([sys.executable, "-c", code], cwd=ROOT,
                          env=dict(env, PCH_CLEARANCE="10,6,16", PCH_SPANS="1,5,9,20"), capture_output=True, text=True)
    assert good.returncode == 0 and "'segments': 16" in good.stdout, good.stderr


def test_new_symbols_and_workspace_bytes():
    from pointcloudhookup_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "pch_hip.h"), encoding="utf-8").read()
    declared = set(re.findall(r"\b(pch_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    L = _lib.lib()
    ws = L.pch_clearance_ws_bytes
    assert ws(0, 0, 1) > 0 and ws(0, 0, 1) == ws(10 ** 8, 1, 128)            # per span, not per row
    assert ws(0, 4096, 128) > ws(0, 1, 128) and ws(2 ** 32 - 1, 4096, 128) == ws(0, 4096, 1)
    assert ws(0, 4096, 128) <= 4096 * 128                                     # tallies, bounds and a flag per span
    for n, K, S in ((-1, 1, 1), (2 ** 32, 1, 1), (1, -1, 1), (1, 4097, 1), (1, 1, 0), (1, 1, 129)):
        assert ws(n, K, S) == 0, (n, K, S)
    assert ops.CLEARANCE_TILE == 1024 and ops.CLEARANCE_MAX_SPANS == 4096 and ops.CLEARANCE_MAX_SEGMENTS == 128
    for name in ("span_curves", "span_segments", "clearance", "_span_curves_of", "_span_segments_of"):
        assert callable(getattr(ops, name))
    # the rule is in the header word for word: the lines a reader checks the numpy statement against
    for line in ("q = ((rm*dm_j) + (rw*dz_j))*inv_j", "em = rm - (q*dm_j);  ew = rw - (q*dz_j)", "d2 = g + (t*t)",
                 "if d2 <= r2 and d2 < best: best = d2; who = k", "NEAREST span only"):
        assert line in header, line
