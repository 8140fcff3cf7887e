"""The cluster merge on the CPU: the numpy statement (tests/merge_cases.py) against the procedure of the reference's
test/tttt.py:93-175 restated here - sklearn's KDTree.query_radius, union by cluster size, ids by first appearance -
the conditions of the end-to-end case, and the host side of the new C ABI group."""
import inspect
import os
import re

import numpy as np
import pytest

import merge_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script_map(C, sizes, r):
    """what the script does with centres C of clusters 0..K-1 of the given sizes, its new ids minus K"""
    from sklearn.neighbors import KDTree
    K = len(C)
    neighbours = KDTree(np.asarray(C)).query_radius(np.asarray(C), r=r)
    parent = list(range(K))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, near in enumerate(neighbours):
        for j in near:
            if i < j:
                a, b = find(i), find(int(j))
                if a != b:
                    if sizes[i] > sizes[j]:                # the sizes of the two clusters, not of the two sets
                        parent[b] = a
                    else:
                        parent[a] = b
    new, nxt = {}, K
    for i in range(K):
        if find(i) not in new:
            new[find(i)] = nxt
            nxt += 1
    return np.array([new[find(i)] - K for i in range(K)], dtype=np.int32), nxt - K


def _finite_sets():
    for K in mc.KS:
        if K:
            yield f"uniform{K}", mc.uniform_centers(K), 6.0
            yield f"lattice{K}", mc.lattice_centers(K), 6.0
            dup = mc.nan_dup_centers(K)
            dup[np.isnan(dup).any(axis=1)] = 1.0e4
            yield f"duplicates{K}", dup, 6.0
            yield f"duplicates{K}_r0", dup, 0.0
    yield "chain", mc.chain_centers(1), 6.0
    yield "two_chains", mc.chain_centers(2), 6.0


@pytest.mark.parametrize("name,C,r", [pytest.param(n, C, r, id=n) for n, C, r in _finite_sets()])
def test_statement_equals_kdtree_and_union_by_size(name, C, r):
    sizes = np.random.default_rng(len(C)).integers(1, 50, len(C))
    want, nwant = _script_map(C, sizes, r)
    got, ngot = mc.merge_map(C, r)
    np.testing.assert_array_equal(got, want)
    assert ngot == nwant and mc.map_is_ordered(got)


def test_the_sets_hold_what_they_are_for():
    hit = mc.links(mc.lattice_centers(65), 6.0)
    assert hit[0, 1] and hit[2, 3] and hit[8, 9] and hit[10, 11]          # distance exactly 6.0
    assert not hit[4, 5] and not hit[6, 7] and not hit[12, 13]            # one float32 step further
    d = mc.lattice_centers(1000).astype(np.float64)
    d2 = ((d[:, None] - d[None]) ** 2).sum(-1)
    assert (d2 == 36.0).sum() > 100 and (hit == hit.T).all()
    cmap, n = mc.merge_map(mc.chain_centers(1), 6.0)
    assert n == 1 and not cmap.any() and not mc.links(mc.chain_centers(1), 6.0)[0, 2]
    cmap, n = mc.merge_map(mc.chain_centers(2), 6.0)
    assert n == 2 and cmap[0::2].tolist() == [0] * 300 and cmap[1::2].tolist() == [1] * 300
    C = mc.nan_dup_centers(257)
    cmap, n = mc.merge_map(C, 0.0)
    nan = np.isnan(C).any(axis=1)
    assert nan.sum() > 30 and len(set(cmap[nan].tolist())) == nan.sum()    # a NaN centre is a component of its own
    same = (C[:, None, :] == C[None, :, :]).all(-1)
    assert n < 257 and((cmap[:, None] == cmap[None, :]) == (same | np.eye(257, dtype=bool))).all()
    for K in (257, 1000):
        P, lab = mc.clustered_cloud(K)
        assert 0 < mc.expected(P, lab, K)["nmerged"] < K
    assert mc.expected(*mc.clustered_cloud(257), 257)["nmerged"] < 256 <= mc.expected(*mc.clustered_cloud(1000), 1000)["nmerged"]


def test_centers_cloud_has_the_clusters_it_is_for():
    P, lab, K = mc.centers_cloud("zero")
    C, sizes = mc.centers(P, lab, K)
    assert len(P) == 120_000 and sizes.tolist() == mc.CENTER_SIZES + [0, 300, 300]
    assert np.isnan(C[10]).all() and np.isnan(C[11]).tolist() == [False, True, False] and C[12, 2] == np.inf
    assert np.isfinite(C[:10]).all() and (lab == -1).sum() > 60_000
    first = np.flatnonzero(lab == 9)
    assert (np.diff(first) > 1).any()                                      # interleaved: perm really gathers


def test_end_to_end_case_meets_its_conditions():
    """without the merge 6 clusters, with 6.0 exactly 4, the two towers that do not straddle keep their row sets"""
    from oracle import dbscan as odb
    from oracle import ground_filter as ogf
    raw, tower = mc.e2e_cloud()
    g = ogf.ground_filter(raw)
    assert not g["used_fallback"] and np.array_equal(g["keep"], tower >= 0)
    who = tower[g["keep"]]
    assert np.array_equal(who, np.repeat(np.arange(4), mc.E2E_TOWERS))
    labels = odb.dbscan_chunked(g["filtered"], mc.E2E["eps"], mc.E2E["min_points"], mc.E2E["chunk_size"], fit="sklearn")
    K = int(labels.max()) + 1
    assert K == 6
    for k, t in enumerate([0, 1, 1, 2, 3, 3]):
        assert (who[labels == k] == t).all()
    want = mc.expected(g["filtered"], labels, K, 6.0)
    assert want["nmerged"] == 4 and want["map"].tolist() == [0, 1, 1, 2, 3, 3]
    for k, t in ((0, 0), (3, 2)):
        np.testing.assert_array_equal(np.flatnonzero(labels == k), np.flatnonzero(want["labels"] == t))
    sizes, merged = want["sizes"], np.bincount(want["labels"][want["labels"] >= 0])
    assert merged[1] == sizes[1] + sizes[2] and merged[3] == sizes[4] + sizes[5] and min(sizes) >= 150


def test_symbols_are_declared_and_bound():
    from pointcloudhookup_amd import _lib
    header = open(os.path.join(ROOT, "include", "pch_hip.h"), encoding="utf-8").read()
    for name in ("pch_cluster_centers_f32", "pch_cluster_merge_ws_bytes", "pch_cluster_merge_f32"):
        assert name in _lib._SIGS and re.search(r"\b%s\(" % name, header)
    L = _lib.lib()
    sizes = [L.pch_cluster_merge_ws_bytes(k) for k in (0, 1, 2, 64, 65, 1000, 65536)]
    assert sizes[1] > 0 and sizes == sorted(sizes) and L.pch_cluster_merge_ws_bytes(-1) == 0


def test_drop_in_knob_parsing_and_pipeline_default():
    from pointcloudhookup_amd import pipeline
    from pointcloudhookup_amd.utils import tower_extraction as te
    assert te.merge_threshold_from_env(None) is None and te.merge_threshold_from_env("") is None
    assert te.merge_threshold_from_env("0") is None and te.merge_threshold_from_env("0.0") is None
    assert te.merge_threshold_from_env("6") == 6.0 and te.merge_threshold_from_env(" 7.5 ") == 7.5
    if "PCH_MERGE_THRESHOLD" not in os.environ:
        assert te.MERGE_THRESHOLD is None
    sig = inspect.signature(pipeline.cluster_points)
    assert sig.parameters["merge_threshold"].default is None
    assert list(inspect.signature(te.extract_towers).parameters) == [
        "input_las_path", "progress_callback", "log_callback", "eps", "min_points", "aspect_ratio_threshold",
        "min_height", "max_width", "min_width", "duplicate_threshold"]
