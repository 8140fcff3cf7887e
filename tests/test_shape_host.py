"""Neighbourhood shapes, host side: the all-pairs reference (shape_cases.shape_reference) against an independent
statement, its edge rules, the corridor scene the wire-removal rule is meant for, the drop-in's knob, the radius check
and the C ABI's names.  No GPU."""
import os
import re

import numpy as np
import pytest

import shape_cases as sc
from pointcloudhookup_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the reference against scikit-learn and np.cov
def test_reference_against_radius_neighbors_and_cov():
    from sklearn.neighbors import NearestNeighbors
    rng = np.random.default_rng(3)
    X = np.vstack([rng.normal(0.0, 0.5, (400, 3)), rng.uniform(-3.0, 3.0, (400, 3))]).astype(np.float32)
    X[:, 0] += np.float32(4.0e5)                                 # projected-CRS scale: moments about the query survive
    Q = np.vstack([X[::7], (X[:40] + rng.normal(0.0, 0.3, (40, 3))).astype(np.float32)])
    r = 0.9
    count, M = sc.shape_reference(X, Q, r)
    sets = NearestNeighbors(radius=r, algorithm="brute").fit(X.astype(np.float64)).radius_neighbors(
        Q.astype(np.float64), return_distance=False)
    C, trace = sc.covariance(count, M)
    seen = 0
    for i, rows in enumerate(sets):
        d2 = ((X[rows].astype(np.float64) - Q[i].astype(np.float64)) ** 2).sum(1)
        if np.any(np.abs(d2 - r * r) < 1e-9):                    # sklearn decides such a row on the rooted distance
            continue
        assert count[i] == len(rows)
        if len(rows) < 2:
            continue
        want = np.cov(X[rows].astype(np.float64) - Q[i].astype(np.float64), rowvar=False, bias=True)
        assert np.abs(C[i] - want).max() <= 1e-12 * max(trace[i], np.trace(want))
        seen += 1
    assert seen > 100 and count.max() > 100


# ------------------------------------------------------------------ edge rules of the reference
def _lattice():
    g = np.arange(-6, 7, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def test_reference_tie_on_the_radius_is_in_and_the_next_float_is_out():
    X = _lattice()
    Q = np.zeros((1, 3), dtype=np.float32)
    count, M = sc.shape_reference(X, Q, 5.0)
    d2 = (X.astype(np.float64) ** 2).sum(1)
    assert count[0] == (d2 <= 25.0).sum() and (d2 == 25.0).sum() == 30
    for tie in ((3, 4, 0), (5, 0, 0), (0, 0, 5)):
        P = np.array([tie], dtype=np.float32)
        assert sc.shape_reference(P, Q, 5.0)[0][0] == 1
        out = P.copy()
        k = int(np.argmax(P[0]))
        out[0, k] = np.nextafter(out[0, k], np.float32(np.inf))
        assert sc.shape_reference(out, Q, 5.0)[0][0] == 0
        c, m = sc.shape_reference(np.vstack([P, out]), Q, 5.0)
        assert c[0] == 1 and np.array_equal(m[0, :3], P[0].astype(np.float64))
    # the lattice is symmetric about the query: first moments and mixed moments vanish, the squares are equal
    assert np.array_equal(M[0, :3], np.zeros(3)) and np.array_equal(M[0, 6:], np.zeros(3))
    assert M[0, 3] == M[0, 4] == M[0, 5] > 0


def test_reference_nan_query_bad_chunks_and_far_query():
    rng = np.random.default_rng(5)
    X = rng.uniform(0.0, 4.0, (300, 3)).astype(np.float32)
    eps = 1.0
    far = np.array([[4.0 + 7 * eps, 2.0, 2.0]])                          # 7 eps beyond the cloud's side
    Q = np.vstack([X[0:1], X[100:101], X[200:201], X[1:2], [[np.nan, 1, 1]], [[1, np.inf, 1]], X[4:6], far])
    Q = Q.astype(np.float32)
    nchunks = 3
    qc = np.array([0, 1, 2, 0, 0, 1, -1, nchunks, 1], dtype=np.int32)
    count, M = sc.shape_reference(X, Q, eps, chunk_size=100, query_chunk=qc)
    assert (count[:4] >= 1).all()                                        # a row of the chunk finds itself
    for i in (4, 5, 6, 7, 8):
        assert count[i] == 0 and not M[i].any(), i
    # a query is held against its chunk only
    c0, _ = sc.shape_reference(X[:100], Q[:1], eps)
    assert c0[0] == count[0]
    # a chunk holding NaN has no fit
    Xb = X.copy()
    Xb[150, 1] = np.nan
    cb, Mb = sc.shape_reference(Xb, Q, eps, chunk_size=100, query_chunk=qc)
    assert cb[1] == 0 and not Mb[1].any() and cb[0] == count[0] and cb[2] == count[2]


def test_moment_bounds_hold_between_two_summation_orders():
    """the bound the GPU test uses, tried on two orders here: numpy's pairwise sums against math.fsum"""
    import math
    X, _, _ = sc.scene()
    rows = np.arange(0, len(X), 97)
    count, M = sc.shape_reference(X, X[rows], 2.0)
    B = sc.moment_bounds(count, 2.0)
    worst = 0.0
    for i, row in enumerate(rows):
        d = X.astype(np.float64) - X[row].astype(np.float64)
        d = d[(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= 4.0]
        assert len(d) == count[i]
        terms = [d[:, 0], d[:, 1], d[:, 2], d[:, 0] ** 2, d[:, 1] ** 2, d[:, 2] ** 2, d[:, 0] * d[:, 1],
                 d[:, 0] * d[:, 2], d[:, 1] * d[:, 2]]
        for a, t in enumerate(terms):
            worst = max(worst, abs(math.fsum(t) - M[i, a]) / B[i, a])
    assert worst <= 1.0
    print(f"two summation orders: worst share of the bound {worst:.4f}")


# ------------------------------------------------------------------ the scene
def test_scene_one_cluster_before_two_after():
    from sklearn.cluster import DBSCAN
    X, wire, x0 = sc.scene()
    assert X.shape == (sc.SCENE_ROWS, 3) and X.dtype == np.float32 and wire.sum() == sc.SCENE_WIRE_ROWS
    for ms in (20, 80):
        lab = DBSCAN(eps=8.0, min_samples=ms).fit(X).labels_
        assert lab.max() + 1 == 1 and (lab < 0).sum() == 0
    mask, f, count = sc.drop_mask_reference(X, **sc.SCENE_RULE)
    assert mask[~wire].sum() == 0                                          # not one tower row
    assert round(100.0 * mask[wire].mean(), 1) == 91.9
    assert mask[wire & (x0 > 10) & (x0 < 50)].all()
    assert count.min() == 6 and count.max() == 366
    assert np.abs(f["linearity"] - 0.9).min() > 1e-6 and np.abs(f["verticality"] - 0.5).min() > 1e-6
    lab = DBSCAN(eps=8.0, min_samples=20).fit(X[~mask]).labels_
    assert lab.max() + 1 == 2 and (lab < 0).sum() == 0
    # Jacobi's ground: the eigenvalues np.linalg.eigh gives reproduce the trace
    assert np.abs(f["l1"] + f["l2"] + f["l3"] - f["trace"]).max() <= 1e-12 * f["trace"].max()


def test_scene_with_ground_keeps_the_scene_rows():
    from oracle import ground_filter as ogf
    raw = sc.scene_with_ground()
    ref = ogf.ground_filter(raw)
    assert len(ref["filtered"]) == sc.SCENE_ROWS and not ref.get("used_fallback", False)


# ------------------------------------------------------------------ the drop-in's knob
def test_drop_linear_from_env():
    from pointcloudhookup_amd.utils import tower_extraction as te
    assert te.drop_linear_from_env(None) is None
    assert te.drop_linear_from_env("") is None and te.drop_linear_from_env("   ") is None
    assert te.drop_linear_from_env("2,0.9,0.5,10") == dict(radius=2.0, linearity=0.9, verticality=0.5, min_rows=10)
    got = te.drop_linear_from_env(" 1.5 , 0.8,0.3 , 0 ")
    assert got == dict(radius=1.5, linearity=0.8, verticality=0.3, min_rows=0) and isinstance(got["min_rows"], int)
    for bad in ("2", "2,0.9,0.5", "2,0.9,0.5,10,1", "0,0.9,0.5,10", "-1,0.9,0.5,10", "nan,0.9,0.5,10",
                "inf,0.9,0.5,10", "2,nan,0.5,10", "2,0.9,0.5,-1", "2,0.9,0.5,ten", "a,b,c,d", "2,0.9,0.5,1.5"):
        with pytest.raises(ValueError):
            te.drop_linear_from_env(bad)
    assert te.DROP_LINEAR == te.drop_linear_from_env(os.environ.get("PCH_DROP_LINEAR"))
    knob = te.drop_linear_from_env("2,0.9,0.5,10")
    line = te.drop_linear_line(dict(n_dropped=7), 100, knob)
    assert "7/100" in line and "\n" not in line


# ------------------------------------------------------------------ the radius check needs no device
@pytest.mark.parametrize("radius", [0.0, -1.0, float("nan"), float("inf"), 2.0000001, 8.0])
def test_bad_radius_raises_before_any_device_call(radius):
    fit = ops.DbscanFit.__new__(ops.DbscanFit)            # no fit was made: nothing but the radius may be looked at
    fit.eps = 2.0
    with pytest.raises(ValueError):
        fit.shape(None, radius)
    with pytest.raises(ValueError):
        ops.check_shape_radius(radius, 2.0)


def test_good_radius_passes_the_check():
    assert ops.check_shape_radius(2.0, 2.0) == 2.0 and ops.check_shape_radius(0.5, 2.0) == 0.5
    from pointcloudhookup_amd import pipeline
    for radius in (0.0, float("nan"), -2.0):
        with pytest.raises(ValueError):
            pipeline.drop_linear_rows(dict(points=None), radius=radius)


# ------------------------------------------------------------------ the C ABI's names
def test_entry_points_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "pch_hip.h"), encoding="utf-8").read()
    names = _lib.exported_symbols()
    for name in ("pch_dbscan_shape_ws_bytes", "pch_dbscan_shape_f32", "pch_shape_features_f64"):
        assert name in names
        assert re.search(r"\b" + name + r"\s*\(", header), name
    for word in ("out_moments", "radius*radius", "2(n+1)"):      # the rule stands in the header
        assert word in header
