"""pch_dbscan_kdist_f32 without a GPU: its all-pairs statement against live sklearn, the knee, and the argument errors
of ops.DbscanFit.kdist and pipeline.core_share that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import dbscan_cases as dc
import kdist_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _inputs(name):
    """(X, eps, min_samples, chunk, core | None)"""
    if name in dc.KDIST_CLOUDS:
        return dc.KDIST_CLOUDS[name](), (0.45 if name == "tight" else 4.0), 20, 0, None
    d = np.load(os.path.join(GOLD, f"dbscan_{name}.npz"))
    return d["X"], float(d["eps"]), int(d["min_samples"]), int(d["chunk"]), d["core"]


# ------------------------------------------------------------------ 1. the statement against sklearn
@pytest.mark.parametrize("name", ["towers5000", "towers30000_chunk10000", "local", "epsg", "tight"])
def test_reference_against_live_sklearn(name):
    """per chunk: sqrt(d2) is kneighbors' column k-1 bit for bit where finite, count is the length of radius_neighbors,
    and a live DBSCAN's core mask is d2 <= eps*eps at k = min_samples"""
    pytest.importorskip("sklearn")
    from sklearn.cluster import DBSCAN
    from sklearn.neighbors import NearestNeighbors
    X, eps, ms, chunk, gold_core = _inputs(name)
    n = len(X)
    cs = chunk if 0 < chunk < n else n
    qc = (np.arange(n) // cs).astype(np.int32) if cs < n else None
    ks = sorted({1, 2, 8, ms, ms + 1})
    d2, count = kc.kdist_reference(X, X, eps, ks, chunk, qc)
    assert d2.shape == (len(ks), n) and (d2[0] == 0.0).all()            # the row itself
    finite_share = np.isfinite(d2).mean(1)
    print(f"{name}: eps {eps}, finite share per k {dict(zip(ks, np.round(finite_share, 3)))}")
    core = np.zeros(n, dtype=bool)
    for s in range(0, n, cs):
        Xc = X[s:s + cs]
        nn = NearestNeighbors(algorithm="kd_tree").fit(Xc)
        dist, _ = nn.kneighbors(Xc, n_neighbors=max(ks))
        rad = nn.radius_neighbors(Xc, radius=eps, return_distance=False)
        np.testing.assert_array_equal(count[s:s + cs], np.array([len(r) for r in rad], dtype=np.int32))
        for a, k in enumerate(ks):
            mine = d2[a, s:s + cs]
            fin = np.isfinite(mine)
            np.testing.assert_array_equal(np.sqrt(mine[fin]).view(np.uint64), dist[fin, k - 1].view(np.uint64))
            assert (dist[~fin, k - 1] >= eps).all()
        core[s:s + cs][DBSCAN(eps=eps, min_samples=ms, algorithm="ball_tree").fit(Xc).core_sample_indices_] = True
    at_ms = d2[ks.index(ms)]
    np.testing.assert_array_equal(core, at_ms <= eps * eps)
    np.testing.assert_array_equal(core, count >= ms)
    if gold_core is not None:
        np.testing.assert_array_equal(core, gold_core.astype(bool))


def test_reference_edge_rules():
    """sub is a float32 subtraction; bad chunks, chunk indices out of range and non-finite queries give 0 and +inf; a
    chunk is its own fit; one rank and a list of ranks state the same"""
    import dbscan_assign_cases as ac
    X = dc.bridge_cloud(6000, 31)
    Q = ac.bridge_queries(X, 1.0)
    Q = np.vstack([Q[:-12:7], Q[-12:]])                                 # a seventh of them and the rows by hand
    d2, cnt = kc.kdist_reference(X, Q, 1.0, [1, 5, 40])
    assert np.isfinite(d2[0]).any() and np.isinf(d2[2]).any() and (d2[1:] >= d2[:-1]).all()
    one, cnt1 = kc.kdist_reference(X, Q, 1.0, 5)
    np.testing.assert_array_equal(one, d2[1])
    np.testing.assert_array_equal(cnt1, cnt)
    bad = ~np.isfinite(Q).all(1)
    assert bad.sum() == 3 and (cnt[bad] == 0).all() and np.isinf(d2[:, bad]).all()
    c = np.array([437000.0, 3139000.0, 80.0], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        raw = Q + c
        a = kc.kdist_reference(X, raw, 1.0, 5, sub=c)
        b = kc.kdist_reference(X, raw - c, 1.0, 5)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    qc = ac.mixed_chunks(len(Q), 3)
    got, gcnt = kc.kdist_reference(X, Q, 1.0, 3, 2000, qc)
    out = (qc < 0) | (qc > 2)
    assert out.any() and (gcnt[out] == 0).all() and np.isinf(got[out]).all() and np.isfinite(got).any()
    for k in range(3):
        sel = qc == k
        part = kc.kdist_reference(X[2000 * k:2000 * (k + 1)], Q[sel], 1.0, 3)
        np.testing.assert_array_equal(got[sel], part[0])
        np.testing.assert_array_equal(gcnt[sel], part[1])
    Xb = X.copy()
    Xb[3000, 1] = np.nan
    gb, gbc = kc.kdist_reference(Xb, Q, 1.0, 3, 2000, qc)
    assert (gbc[qc == 1] == 0).all() and np.isinf(gb[qc == 1]).all()
    np.testing.assert_array_equal(gb[qc != 1], got[qc != 1])


def test_big_cloud_is_beyond_an_on_chip_buffer():
    X, rows = kc.big_cloud()
    assert X.shape == (9000, 3) and len(np.unique(rows)) == 512
    d2, cnt = kc.kdist_reference(X, X[rows], kc.BIG_EPS, kc.BIG_KS)
    share = (cnt >= 5000).mean()
    print(f"big cloud: {share:.3f} of the queries have 5000 rows in reach, largest count {cnt.max()}")
    assert share >= 0.6
    assert np.isfinite(d2[kc.BIG_KS.index(4096)]).mean() >= 0.6


# ------------------------------------------------------------------ 2. the knee
def test_knee():
    from pointcloudhookup_amd import pipeline
    y = np.concatenate([np.linspace(1, 2, 900), np.linspace(2, 50, 100)])
    assert pipeline.kdistance_knee(y) == 2.0 and kc.knee_reference(y) == 2.0
    assert pipeline.kdistance_knee(np.full(10, 3.25)) == 3.25 and kc.knee_reference(np.full(10, 3.25)) == 3.25
    assert pipeline.kdistance_knee([1.0, 2.0]) is None and kc.knee_reference([1.0, 2.0]) is None
    assert pipeline.kdistance_knee([]) is None
    rng = np.random.default_rng(4)
    for m in (3, 4, 17, 1000):
        y = np.sort(rng.gamma(2.0, 1.5, m))
        assert pipeline.kdistance_knee(y) == kc.knee_reference(y)
    assert pipeline.kdistance_knee([0.0, 1.0, 2.0]) == 0.0             # on the chord everywhere: the first index


# ------------------------------------------------------------------ 3. argument errors that need no device
def test_kdist_argument_errors_need_no_device():
    from pointcloudhookup_amd import ops
    fit = ops.DbscanFit.__new__(ops.DbscanFit)                          # no fit is made: every call below raises first
    fit.n, fit.chunk_size, fit.device = 10, 0, torch.device("cpu")
    q = torch.zeros((10, 3), dtype=torch.float32)
    for k in (0, -3):
        with pytest.raises(ValueError, match="k must be"):
            fit.kdist(q, k)
    with pytest.raises(TypeError, match="CUDA/HIP"):
        fit.kdist(q, 1)
    with pytest.raises(TypeError):
        fit.kdist(q.double(), 1)
    with pytest.raises(TypeError):
        fit.kdist(q.numpy(), 1)
    with pytest.raises(ValueError, match="own"):
        fit.kdist(q, 1, chunk="mine")


def test_core_share_refuses_eps_beyond_the_profile():
    from pointcloudhookup_amd import pipeline
    prof = dict(k=4, eps_max=2.0, rows=np.arange(8), kdist=np.array([0.5, 1.0, 1.0, 1.5, 2.0]), truncated=3)
    assert pipeline.core_share(prof, 2.0) == 5 / 8
    assert pipeline.core_share(prof, 1.0) == 3 / 8
    assert pipeline.core_share(prof, 0.25) == 0.0
    with pytest.raises(ValueError, match="eps_max"):
        pipeline.core_share(prof, 2.0000001)


def test_entry_points_are_declared():
    from pointcloudhookup_amd import _lib
    header = open(os.path.join(ROOT, "include", "pch_hip.h")).read()
    for name in ("pch_dbscan_kdist_f32", "pch_dbscan_kdist_ws_bytes"):
        assert name in _lib.exported_symbols()
        assert re.search(r"\b%s\s*\(" % name, header), name
