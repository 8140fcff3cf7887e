"""pch_dbscan_knn_f32 without a GPU: its all-pairs statement (knn_cases.knn_reference) against live sklearn and against
kdist_reference, the cut through ties, the edge rules, the sparse-row rule on the scene with stray returns, and the
argument errors that need no device."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dbscan_cases as dc
import kdist_cases as kc
import knn_cases as kn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _inputs(name):
    """(X, eps, min_samples, chunk) - the inputs of test_kdist_host.py::test_reference_against_live_sklearn"""
    if name in dc.KDIST_CLOUDS:
        return dc.KDIST_CLOUDS[name](), (0.45 if name == "tight" else 4.0), 20, 0
    d = np.load(os.path.join(GOLD, f"dbscan_{name}.npz"))
    return d["X"], float(d["eps"]), int(d["min_samples"]), int(d["chunk"])


# ------------------------------------------------------------------ 1. the statement against sklearn
@pytest.mark.parametrize("name", ["towers5000", "towers30000_chunk10000", "local", "epsg", "tight"])
def test_reference_against_live_sklearn(name):
    """per chunk: sqrt(d2) is kneighbors' distances bit for bit where finite; rows are its indices in every finite slot
    whose distance is tied neither with a neighbouring slot nor with slot k + 1; column k-1 and count are
    kdist_reference's"""
    pytest.importorskip("sklearn")
    from sklearn.neighbors import NearestNeighbors
    X, eps, ms, chunk = _inputs(name)
    n = len(X)
    cs = chunk if 0 < chunk < n else n
    qc = (np.arange(n) // cs).astype(np.int32) if cs < n else None
    k = ms
    rows, d2, count = kn.knn_reference(X, X, eps, k, chunk, qc)
    want, wcnt = kc.kdist_reference(X, X, eps, k, chunk, qc)
    np.testing.assert_array_equal(d2[:, k - 1].view(np.uint64), want.view(np.uint64))
    np.testing.assert_array_equal(count, wcnt)
    assert (d2[:, 0] == 0.0).all() and (d2[:, 1:] >= d2[:, :-1]).all()
    compared = total = 0
    for s in range(0, n, cs):
        Xc = X[s:s + cs]
        dist, ind = NearestNeighbors(algorithm="kd_tree").fit(Xc).kneighbors(Xc, n_neighbors=k + 1)
        mine, fin = d2[s:s + cs], np.isfinite(d2[s:s + cs])
        np.testing.assert_array_equal(np.sqrt(mine[fin]).view(np.uint64), dist[:, :k][fin].view(np.uint64))
        tied = np.zeros(dist.shape, dtype=bool)
        tied[:, 1:] |= dist[:, 1:] == dist[:, :-1]
        tied[:, :-1] |= dist[:, :-1] == dist[:, 1:]
        sure = fin & ~tied[:, :k]
        np.testing.assert_array_equal(rows[s:s + cs][sure], (ind[:, :k] + s)[sure])
        compared += int(sure.sum())
        total += int(fin.sum())
    print(f"{name}: k {k}, {compared} of {total} finite slots compared with kneighbors' indices")
    assert compared >= 0.9 * total
    if name in dc.KDIST_CLOUDS:
        assert k == 20 and compared == total                            # no ties in these clouds


def test_the_quick_reference_is_the_literal_stable_argsort():
    import dbscan_assign_cases as ac
    X, eps, _, _, _ = dc.lattice_case("few")                            # ties everywhere
    for k in (1, 7, 27, 200):
        for a, b in zip(kn.knn_reference(X, X[::5], eps, k), kn.knn_reference(X, X[::5], eps, k, literal=True)):
            np.testing.assert_array_equal(a, b)
    X = dc.bridge_cloud(6000, 31)
    Q = ac.bridge_queries(X, 1.0)[::9]
    qc = ac.mixed_chunks(len(Q), 3)
    for a, b in zip(kn.knn_reference(X, Q, 1.0, 12, 2000, qc), kn.knn_reference(X, Q, 1.0, 12, 2000, qc, literal=True)):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 2. the cut through ties
@pytest.mark.parametrize("name", ["few", "tile", "dense"])
def test_lattices_cut_ties_by_row(name):
    X, eps, _, _, _ = dc.lattice_case(name)
    cut = 0
    for k in (2, 7, 27):
        rows, d2, count = kn.knn_reference(X, X, eps, k)
        rows1, d21, count1 = kn.knn_reference(X, X, eps, k + 1)
        np.testing.assert_array_equal(rows1[:, :k], rows)
        np.testing.assert_array_equal(count1, count)
        tie = np.isfinite(d21[:, k]) & (d21[:, k - 1] == d21[:, k])     # slot k and slot k + 1 of the longer answer
        cut += int(tie.sum())
        assert (rows1[tie, k - 1] < rows1[tie, k]).all()                # the smaller row is the one that stays
        # within equal d2 the rows ascend, everywhere
        same = np.isfinite(d21[:, 1:]) & (d21[:, 1:] == d21[:, :-1])
        assert (rows1[:, 1:][same] > rows1[:, :-1][same]).all()
    print(f"lattice {name}: {cut} rows whose answer is cut inside a tie (k in 2, 7, 27)")
    assert cut > 0


# ------------------------------------------------------------------ 3. the edge rules
def test_reference_edge_rules():
    import dbscan_assign_cases as ac
    X = dc.bridge_cloud(6000, 31)
    Q = ac.bridge_queries(X, 1.0)
    Q = np.vstack([Q[:-12:7], Q[-12:]])
    k = 5
    rows, d2, cnt = kn.knn_reference(X, Q, 1.0, k)
    want, wcnt = kc.kdist_reference(X, Q, 1.0, k)
    np.testing.assert_array_equal(d2[:, k - 1], want)
    np.testing.assert_array_equal(cnt, wcnt)
    short = (cnt > 0) & (cnt < k)
    assert short.any() and (rows[short, -1] == -1).all() and np.isinf(d2[short, -1]).all()
    fin = rows >= 0
    i, j = np.nonzero(fin)
    np.testing.assert_array_equal(d2[fin], dc.pair_d2(X, Q)[i, rows[fin]])          # the rows are those distances' rows
    bad = ~np.isfinite(Q).all(1)
    assert bad.sum() == 3 and (cnt[bad] == 0).all() and (rows[bad] == -1).all() and np.isinf(d2[bad]).all()
    c = np.array([437000.0, 3139000.0, 80.0], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        raw = Q + c
        a = kn.knn_reference(X, raw, 1.0, k, sub=c)
        b = kn.knn_reference(X, raw - c, 1.0, k)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    qc = ac.mixed_chunks(len(Q), 3)
    grow, gd2, gcnt = kn.knn_reference(X, Q, 1.0, 3, 2000, qc)
    out = (qc < 0) | (qc > 2)
    assert out.any() and (gcnt[out] == 0).all() and (grow[out] == -1).all() and np.isinf(gd2[out]).all()
    for c_no in range(3):                                               # a chunk is its own fit, the rows are global
        sel = qc == c_no
        prow, pd2, pcnt = kn.knn_reference(X[2000 * c_no:2000 * (c_no + 1)], Q[sel], 1.0, 3)
        np.testing.assert_array_equal(gd2[sel], pd2)
        np.testing.assert_array_equal(gcnt[sel], pcnt)
        np.testing.assert_array_equal(grow[sel], np.where(prow >= 0, prow + 2000 * c_no, -1))
    assert (grow[qc == 2] >= 4000).sum() > 0
    Xb = X.copy()
    Xb[3000, 1] = np.nan
    brow, bd2, bcnt = kn.knn_reference(Xb, Q, 1.0, 3, 2000, qc)
    assert (bcnt[qc == 1] == 0).all() and (brow[qc == 1] == -1).all()
    np.testing.assert_array_equal(brow[qc != 1], grow[qc != 1])


def test_a_duplicate_with_a_smaller_row_comes_before_the_row_itself():
    rng = np.random.default_rng(12)
    A = rng.normal(0.0, 0.3, (300, 3)).astype(np.float32)
    X = np.vstack([A, A[:80]])[rng.permutation(380)]
    rows, d2, cnt = kn.knn_reference(X, X, 1.0, 2)
    own = np.arange(len(X))
    assert (d2[:, 0] == 0.0).all()
    later = rows[:, 0] != own                                           # the order decides, not identity
    assert later.sum() == 80 and (rows[later, 0] < own[later]).all() and (rows[later, 1] == own[later]).all()
    assert (d2[later, 1] == 0.0).all()
    np.testing.assert_array_equal(X[rows[later, 0]], X[own[later]])


# ------------------------------------------------------------------ 4. the scene with stray returns
@pytest.mark.parametrize("rule_no", [0, 1])
def test_scene_with_strays(rule_no):
    X, kind = kn.scene_with_strays()
    assert X.shape == (kn.STRAY_ROWS, 3) and X.dtype == np.float32
    assert [(kind == a).sum() for a in range(3)] == [5000, 1803, kn.N_STRAYS]
    r = kn.sparse_case(rule_no)
    d = r["dropped"]
    tower, wire, stray = (int(d[kind == a].sum()) for a in range(3))
    print(f"strays scene {kn.SPARSE_RULES[rule_no]}: thr {r['threshold']:.4f}; dropped {tower} tower, {wire} wire, "
          f"{stray} of {kn.N_STRAYS} stray ({int(r['by_count'].sum())} by count, {int(r['by_mean'].sum())} by mean); "
          f"margin {r['margin']:.3g}")
    assert wire == 0
    assert stray >= 150
    assert tower <= 0.05 * 5000
    assert r["margin"] >= 1e-4                                          # the GPU test may demand equal masks
    assert not (r["by_count"] & r["by_mean"]).any() and np.isinf(r["m"][r["by_count"]]).all()


def test_strays_join_the_towers_without_the_drop():
    """what the rule is for: at eps = 8 the strays near a tower become its border points"""
    pytest.importorskip("sklearn")
    from sklearn.cluster import DBSCAN
    import shape_cases as sc
    X, kind = kn.scene_with_strays()
    linear = np.zeros(len(X), dtype=bool)
    linear[:] = sc.drop_mask_reference(X, **sc.SCENE_RULE)[0]
    lab = DBSCAN(eps=8.0, min_samples=20).fit(X[~linear]).labels_
    inside = int((lab[kind[~linear] == 2] >= 0).sum())
    assert lab.max() + 1 == 2 and inside >= 50
    sparse = kn.sparse_case(0)["dropped"]
    Y, ykind = X[~sparse], kind[~sparse]
    linear = sc.drop_mask_reference(Y, **sc.SCENE_RULE)[0]
    assert linear[ykind == 0].sum() == 0 and linear[ykind == 1].sum() >= 1600
    lab = DBSCAN(eps=8.0, min_samples=20).fit(Y[~linear]).labels_
    left = int((lab[ykind[~linear] == 2] >= 0).sum())
    print(f"strays inside a tower cluster: {inside} with drop_linear alone, {left} with the sparse rows dropped first")
    assert lab.max() + 1 == 2 and (lab < 0).sum() == 0 and left <= 5


def test_mean_distance_reference_and_its_bound():
    import math
    X, _ = kn.scene_with_strays()
    r = kn.sparse_case(0)
    k = 8
    _, d2, count = kn.knn_reference(X[:500], X[:500], 2.0, k)
    m = kn.mean_distance_reference(d2, count, k)
    worst = 0.0
    for i in np.flatnonzero(count >= k):
        exact = math.fsum(math.sqrt(v) for v in d2[i]) / k
        worst = max(worst, abs(m[i] - exact) / exact / kn.mean_distance_bound(k))
    assert np.isinf(m[count < k]).all() and worst <= 0.5
    assert kn.threshold_bound(6800, 8, 2.0, 2.0) < 1e-4 * r["threshold"] * 1e-3      # far inside the scene's margin


# ------------------------------------------------------------------ 5. argument errors that need no device
def test_knn_argument_errors_need_no_device():
    from pointcloudhookup_amd import ops
    assert ops.KNN_MAX_K == 256
    fit = ops.DbscanFit.__new__(ops.DbscanFit)                          # no fit is made: every call below raises first
    fit.n, fit.chunk_size, fit.device = 10, 0, torch.device("cpu")
    q = torch.zeros((10, 3), dtype=torch.float32)
    for k in (0, -3, 257, 1000, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            fit.knn(None, k)                                            # before the query is looked at
    with pytest.raises(TypeError, match="CUDA/HIP"):
        fit.knn(q, 1)
    with pytest.raises(TypeError):
        fit.knn(q.double(), 1)
    with pytest.raises(TypeError):
        fit.knn(q.numpy(), 256)
    with pytest.raises(ValueError, match="own"):
        fit.knn(q, 1, chunk="mine")


def test_knn_mean_distance_on_the_host():
    from pointcloudhookup_amd import ops
    d2 = torch.tensor([[0.0, 1.0, 4.0], [0.0, 9.0, float("inf")], [float("inf")] * 3], dtype=torch.float64)
    count = torch.tensor([5, 2, 0], dtype=torch.int32)
    m = ops.knn_mean_distance(d2, count, 3)
    assert m.dtype == torch.float64 and m.tolist() == [1.0, float("inf"), float("inf")]
    assert ops.knn_mean_distance(d2, count, 2).tolist() == [0.5, 1.5, float("inf")]  # the first k slots only
    assert not torch.isnan(ops.knn_mean_distance(d2, count, 1)).any()
    rng = np.random.default_rng(8)
    D = np.sort(rng.uniform(0.0, 4.0, (300, 8)), axis=1)
    cnt = rng.integers(0, 16, 300).astype(np.int32)
    D[cnt[:, None] <= np.arange(8)[None, :]] = np.inf
    got = ops.knn_mean_distance(torch.from_numpy(D), torch.from_numpy(cnt), 8).numpy()
    want = kn.mean_distance_reference(D, cnt, 8)
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    assert fin.sum() > 100 and (np.abs(got[fin] - want[fin]) <= kn.mean_distance_bound(8) * want[fin]).all()
    for k in (0, 257, -1):
        with pytest.raises(ValueError, match="k must be"):
            ops.knn_mean_distance(d2, count, k)
    with pytest.raises(ValueError):
        ops.knn_mean_distance(d2, count, 4)                             # more slots than the answer holds
    with pytest.raises(ValueError):
        ops.knn_mean_distance(d2, count[:2], 3)
    with pytest.raises(TypeError):
        ops.knn_mean_distance(d2.float(), count, 3)
    with pytest.raises(TypeError):
        ops.knn_mean_distance(d2, count.long(), 3)
    with pytest.raises(TypeError):
        ops.knn_mean_distance(d2.numpy(), count, 3)


def test_drop_sparse_rows_argument_errors_need_no_device():
    from pointcloudhookup_amd import pipeline
    gf = dict(points=None)                                              # never looked at: the arguments come first
    for k in (0, 257, -8, 1.5):
        with pytest.raises(ValueError, match="k must be"):
            pipeline.drop_sparse_rows(gf, k=k)
    for radius in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            pipeline.drop_sparse_rows(gf, radius=radius)
    with pytest.raises(ValueError, match="std_ratio"):
        pipeline.drop_sparse_rows(gf, std_ratio=float("nan"))
    with pytest.raises(ValueError, match="kept no rows"):
        pipeline.drop_sparse_rows(dict(points=torch.empty((0, 3), dtype=torch.float32)))


def test_drop_sparse_from_env():
    from pointcloudhookup_amd.utils import tower_extraction as te
    assert te.drop_sparse_from_env(None) is None
    assert te.drop_sparse_from_env("") is None and te.drop_sparse_from_env("   ") is None
    assert te.drop_sparse_from_env("8,2,2") == dict(k=8, radius=2.0, std_ratio=2.0)
    got = te.drop_sparse_from_env(" 256 , 0.5, -1.5 ")
    assert got == dict(k=256, radius=0.5, std_ratio=-1.5) and isinstance(got["k"], int)
    for bad in ("8", "8,2", "8,2,2,1", "0,2,2", "257,2,2", "-1,2,2", "8.5,2,2", "8,0,2", "8,-1,2", "8,nan,2",
                "8,inf,2", "8,2,nan", "8,2,two", "a,b,c", ",,"):
        with pytest.raises(ValueError):
            te.drop_sparse_from_env(bad)
    assert te.DROP_SPARSE == te.drop_sparse_from_env(os.environ.get("PCH_DROP_SPARSE"))
    knob = te.drop_sparse_from_env("8,2,2")
    line = te.drop_sparse_line(dict(n_dropped=7, threshold=0.92851), 100, knob)
    assert "7/100" in line and "0.9285" in line and "\n" not in line


# ------------------------------------------------------------------ 6. signatures and the C ABI's names
def test_drop_sparse_is_off_by_default():
    from pointcloudhookup_amd import pipeline
    for f in (pipeline.cluster_points, pipeline.cluster_points_las):
        p = inspect.signature(f).parameters
        assert p["drop_sparse"].default is None and p["drop_linear"].default is None
    p = inspect.signature(pipeline.drop_sparse_rows).parameters
    assert [(n, p[n].default) for n in ("k", "radius", "std_ratio")] == [("k", 8), ("radius", 2.0), ("std_ratio", 2.0)]


def test_entry_points_are_exported_and_declared():
    from pointcloudhookup_amd import _lib
    header = open(os.path.join(ROOT, "include", "pch_hip.h"), encoding="utf-8").read()
    names = _lib.exported_symbols()
    for name in ("pch_dbscan_knn_ws_bytes", "pch_dbscan_knn_f32"):
        assert name in names
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+PCH_KNN_MAX_K\s+256\b", header)
    for word in ("out_rows", "(d2, row)", "GLOBAL row"):               # the rule stands in the header
        assert word in header
